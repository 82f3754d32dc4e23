// Every launch that labels the [B][H][W] grid from low-resolution maps: the evaluators' arg-max (tools/evaluate_cityscapes.py:96-162,
// evaluate_simt: the main head's logits at two input scales, bilinearly upsampled with align_corners=True to the label resolution, SUMMED,
// arg-maxed; the reference does this on the CPU in numpy per image), the pseudo-label export, its class-balanced form, test-time augmentation
// and the online labels of the warm-up trainers.  They are ONE grid-stride sweep, one pixel per lane, composed of a SOURCE -- (arg-max,
// confidence) of one pixel, gathered from maps that stay L2-resident -- and a SINK, the output side.  A guarantee such as "the online labels
// are the export's labels bit for bit" holds because both launches instantiate the sweep with the same source.
#include "bilinear_taps.h"

struct ArgConf {
  int arg;             // first-index arg-max
  float conf;          // the maximum
};

// One pixel per lane, so that neighbouring lanes gather neighbouring taps (a version in which each thread labelled 4 consecutive pixels
// itself touched ~4x the cache lines per load instruction and ran 2.3-3.3x slower).  The trip count is uniform over the block: every lane
// of a wave reaches the sink's shuffles and ballots together.  The sink turns the (arg, conf) of pixel p into what it writes (its Item: a
// label, a histogram key) inside the bounds check, so that only the Item lives across it; for p >= P emit() gets a zeroed Item.
template <int BLOCK, class Source, class Sink>
__global__ __launch_bounds__(BLOCK) void label_sweep_kernel(Source src, Sink sink, int B, int H, int W) {
  __shared__ typename Sink::Shared sh;
  sink.template init<BLOCK>(sh);
  const long P = (long)B * H * W;
  for (long base = (long)blockIdx.x * BLOCK; base < P; base += (long)gridDim.x * BLOCK) {
    const long p = base + threadIdx.x;
    typename Sink::Item it = {};
    if (p < P) {
      const int x = (int)(p % W);
      const long t = p / W;
      it = sink.item(sh, src((int)(t / H), (int)(t % H), x));
    }
    sink.emit(sh, it, p, P);
  }
  sink.template flush<BLOCK>(sh);
}

// Launch shapes.  The int32 evaluation launches: 256 threads, no LDS.  The one-resample label family: the flush of the label counts is what
// a label launch adds to the gather; with 256-thread blocks and up to 2048 of them (41 k 64-bit atomics on 20 words) it cost 7-13 us at
// 1 x 1024 x 2048; 1024-thread blocks, at most 512 of them (the same 32 waves per CU), cut it to ~3 us (launch-shape sweep on MI355X,
// 138.6 us against 143.5 us of the int32 launch).  The two-resample family: the two-scale float4 gather holds ~220 VGPRs (2 waves per
// SIMD, as its int32 launch runs), which a 1024-thread block (128 VGPRs at most) would spill; at most 1024 blocks of 512 keeps the count
// flush at ~20 k atomics per frame.
constexpr int EV_BLOCK = 256, EV_MAX_GRID = 256 * 16;
constexpr int PL_BLOCK = 1024, PL_MAX_GRID = 512;
constexpr int PL2_BLOCK = 512, PL2_MAX_GRID = 1024;

template <int BLOCK, int MAX_GRID, class Source, class Sink>
static void launch_sweep(const Source& src, const Sink& sink, int B, int H, int W, simt_stream_t stream) {
  long grid = ((long)B * H * W + BLOCK - 1) / BLOCK;
  if (grid > MAX_GRID) grid = MAX_GRID;
  hipLaunchKernelGGL((label_sweep_kernel<BLOCK, Source, Sink>), dim3((unsigned)grid), dim3(BLOCK), 0, (hipStream_t)stream, src, sink, B, H, W);
}

// float4 gathers of 4 consecutive channels: ld % 4 == 0 on a 16-byte-aligned map (channels C..round_up(C, 4)-1 are read, lie inside ld, and
// are ignored)
static bool vec4_ok(const float* l, int ld) { return ld % 4 == 0 && ((uintptr_t)l & 15) == 0; }

// ================================================================ sources ==================================================================
// ---- one resample (DeepLab-v2, DeepLab-VGG16).  MODE 0: arg-max of up(la) + up(lb), the evaluator's label and mode 0 of the export.
// MODE 1: max / arg-max of up(la), probabilities: the confidence mode (the rule of trainV2_simt.py:353-359 with the high threshold only).
template <int MODE>
struct Resample1 {
  const float* la;     // [B][ha][wa][lda] logits (mode 0) or probabilities (mode 1), first C channels used
  const float* lb;     // [B][hb][wb][ldb] logits, scale B, or NULL (mode 1: always NULL)
  int ha, wa, lda, hb, wb, ldb, C;
  float sya, sxa, syb, sxb;

  __device__ __forceinline__ ArgConf operator()(int b, int y, int x) const {
    int a00, a01, a10, a11, b00 = 0, b01 = 0, b10 = 0, b11 = 0;
    float ay0, ay1, ax0, ax1, by0 = 0, by1 = 0, bx0 = 0, bx1 = 0;
    bil_taps(y, x, ha, wa, sya, sxa, a00, a01, a10, a11, ay0, ay1, ax0, ax1);
    const float* pa = la + (long)b * ha * wa * lda;
    const float* pb = nullptr;
    if (MODE == 0 && lb) {
      bil_taps(y, x, hb, wb, syb, sxb, b00, b01, b10, b11, by0, by1, bx0, bx1);
      pb = lb + (long)b * hb * wb * ldb;
    }
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      // same association as ATen: h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11); then numpy's a + b
      float v = ay0 * (ax0 * pa[(long)a00 * lda + c] + ax1 * pa[(long)a01 * lda + c]) +
                ay1 * (ax0 * pa[(long)a10 * lda + c] + ax1 * pa[(long)a11 * lda + c]);
      if (MODE == 0 && pb) {
        const float u = by0 * (bx0 * pb[(long)b00 * ldb + c] + bx1 * pb[(long)b01 * ldb + c]) +
                        by1 * (bx0 * pb[(long)b10 * ldb + c] + bx1 * pb[(long)b11 * ldb + c]);
        v = v + u;
      }
      if (v > best) { best = v; arg = c; }     // first index on ties, like np.argmax
    }
    return {arg, best};
  }
};

template <int MODE>
static Resample1<MODE> resample1(const float* la, int ha, int wa, int lda, const float* lb, int hb, int wb, int ldb, int H, int W, int C) {
  Resample1<MODE> s;
  s.la = la; s.lb = lb; s.ha = ha; s.wa = wa; s.lda = lda; s.hb = hb; s.wb = wb; s.ldb = ldb; s.C = C;
  s.sya = align_scale(ha, H); s.sxa = align_scale(wa, W);
  s.syb = lb ? align_scale(hb, H) : 0.f; s.sxb = lb ? align_scale(wb, W) : 0.f;
  return s;
}

// ---- two resamples: a model that upsamples INSIDE (DeepLabv3, model/deeplabv3.py:137), whose full-resolution output the reference
// resamples a second time (evaluate_cityscapes.py:108-133).  Per label pixel and scale: the align_corners=True taps of the label grid over a
// VIRTUAL [hi][wi] map (bil_taps' arithmetic), each of whose 4 samples is the align_corners=False value of the NHWC logits (up_taps, align
// = 0) -- 16 gathers per channel, nothing stored in between (the map would be 52 + 82 MB per frame at Q = 25).  V = 4: float4 gathers.
struct Up2Scale {
  const float* l;      // [B][h][w][ld] logits, first C channels used
  int h, w, ld, hi, wi;
  float osy, osx;      // outer: (hi-1)/(H-1), (wi-1)/(W-1)
  float isy, isx;      // inner: h/hi, w/wi
};

struct Up2Taps {
  int off[4][4];       // [virtual sample yi*2+xi][logit tap yj*2+xj] element offsets (B*h*w*ld < 2^31, checked on the host)
  float ly[2][2], lx[2][2];   // inner weights [virtual row / column][tap]
  float oy[2], ox[2];         // outer weights
};

// flip (test-time augmentation): the mirror applied to the virtual [hi][wi] map -- the outer (align_corners=True) columns vx become wi-1-vx
// before the inner (align_corners=False) taps are formed
__device__ __forceinline__ void up2_taps(const Up2Scale& s, int flip, int b, int y, int x, Up2Taps& t) {
  int vy[2], vx[2], iy[2][2], ix[2][2];
  up_taps(y, s.hi, s.osy, 1, vy[0], vy[1], t.oy[0], t.oy[1]);
  up_taps(x, s.wi, s.osx, 1, vx[0], vx[1], t.ox[0], t.ox[1]);
  if (flip) { vx[0] = s.wi - 1 - vx[0]; vx[1] = s.wi - 1 - vx[1]; }
  for (int i = 0; i < 2; ++i) {
    up_taps(vy[i], s.h, s.isy, 0, iy[i][0], iy[i][1], t.ly[i][0], t.ly[i][1]);
    up_taps(vx[i], s.w, s.isx, 0, ix[i][0], ix[i][1], t.lx[i][0], t.lx[i][1]);
  }
  const int base = b * s.h * s.w;
  for (int yi = 0; yi < 2; ++yi)
    for (int xi = 0; xi < 2; ++xi)
      for (int yj = 0; yj < 2; ++yj)
        for (int xj = 0; xj < 2; ++xj)
          t.off[yi * 2 + xi][yj * 2 + xj] = (base + iy[yi][yj] * s.w + ix[xi][xj]) * s.ld;
}

template <int V> struct VecF;
template <> struct VecF<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};
template <> struct VecF<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
};

// the 4 virtual samples [yi*2+xi] of up(l)[c0 .. c0+V-1] (the inner, align_corners=False level), in ATen's association:
// h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11)
template <int V>
__device__ __forceinline__ void up2_samples(const float* l, const Up2Taps& t, int c0, float (&vs)[4][V]) {
  for (int yi = 0; yi < 2; ++yi)
    for (int xi = 0; xi < 2; ++xi) {
      const int s = yi * 2 + xi;
      VecF<V> p00, p01, p10, p11;
      p00.load(l + t.off[s][0] + c0); p01.load(l + t.off[s][1] + c0);
      p10.load(l + t.off[s][2] + c0); p11.load(l + t.off[s][3] + c0);
      const float h0 = t.ly[yi][0], h1 = t.ly[yi][1], w0 = t.lx[xi][0], w1 = t.lx[xi][1];
      for (int k = 0; k < V; ++k) vs[s][k] = h0 * (w0 * p00.v[k] + w1 * p01.v[k]) + h1 * (w0 * p10.v[k] + w1 * p11.v[k]);
    }
}

// up(up(l))[c0 .. c0+V-1] at one pixel, in ATen's association at both levels
template <int V>
__device__ __forceinline__ void up2_value(const float* l, const Up2Taps& t, int c0, float (&out)[V]) {
  float vs[4][V];
  up2_samples<V>(l, t, c0, vs);
  for (int k = 0; k < V; ++k)
    out[k] = t.oy[0] * (t.ox[0] * vs[0][k] + t.ox[1] * vs[1][k]) + t.oy[1] * (t.ox[0] * vs[2][k] + t.ox[1] * vs[3][k]);
}

static void fill_up2(Up2Scale& s, const float* l, int h, int w, int ld, int hi, int wi, int H, int W) {
  s.l = l; s.h = h; s.w = w; s.ld = ld; s.hi = hi; s.wi = wi;
  s.osy = align_scale(hi, H);
  s.osx = align_scale(wi, W);
  s.isy = (float)h / (float)hi;
  s.isx = (float)w / (float)wi;
}

// MODE 0: the first-index arg-max of up(up(s[0])) (+ up(up(s[1])) with two scales): the evaluator's label, and mode 0 of the export
template <int V>
struct Up2Argmax {
  Up2Scale s[2];
  int nscales, C;

  __device__ __forceinline__ ArgConf operator()(int b, int y, int x) const {
    Up2Taps ta, tb;
    up2_taps(s[0], 0, b, y, x, ta);
    const bool two = nscales > 1;
    if (two) up2_taps(s[1], 0, b, y, x, tb);
    float best = -INFINITY;
    int arg = 0;
    for (int c0 = 0; c0 < C; c0 += V) {
      float va[V], vb[V];
      up2_value<V>(s[0].l, ta, c0, va);
      if (two) up2_value<V>(s[1].l, tb, c0, vb);
      for (int k = 0; k < V; ++k) {
        if (c0 + k >= C) break;
        const float v = two ? va[k] + vb[k] : va[k];
        if (v > best) { best = v; arg = c0 + k; }     // first index on ties, like np.argmax
      }
    }
    return {arg, best};
  }
};

template <int V>
static Up2Argmax<V> up2_argmax(const float* la, int ha, int wa, int lda, int hia, int wia, const float* lb, int hb, int wb, int ldb, int hib,
                               int wib, int H, int W, int C) {
  Up2Argmax<V> s;
  s.nscales = lb ? 2 : 1; s.C = C;
  fill_up2(s.s[0], la, ha, wa, lda, hia, wia, H, W);
  fill_up2(s.s[1], lb ? lb : la, lb ? hb : ha, lb ? wb : wa, lb ? ldb : lda, lb ? hib : hia, lb ? wib : wia, H, W);
  return s;
}

// MODE 1 (one scale): the confidence rule on the model's OUTPUT -- softmax at each of the 4 virtual samples (the input-size map), the
// probabilities resampled to the label pixel; their first-index arg-max and their maximum, the confidence.  The softmax is not separable
// from the inner resample, so the 4 samples' logits are re-gathered in three channel sweeps (max, sum of exps, probabilities + arg-max)
// instead of holding 4 x C values per lane; expf / fmaxf / 1/s as in softmax_rows_kernel.
template <int V>
struct Up2Confident {
  Up2Scale s;
  int C;

  __device__ __forceinline__ ArgConf operator()(int b, int y, int x) const {
    Up2Taps t;
    up2_taps(s, 0, b, y, x, t);
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, inv[4] = {0.f, 0.f, 0.f, 0.f};
    float vs[4][V];
    for (int c0 = 0; c0 < C; c0 += V) {
      up2_samples<V>(s.l, t, c0, vs);
      for (int k = 0; k < V; ++k) {
        if (c0 + k >= C) break;
        for (int i = 0; i < 4; ++i) mx[i] = fmaxf(mx[i], vs[i][k]);
      }
    }
    for (int c0 = 0; c0 < C; c0 += V) {
      up2_samples<V>(s.l, t, c0, vs);
      for (int k = 0; k < V; ++k) {
        if (c0 + k >= C) break;
        for (int i = 0; i < 4; ++i) inv[i] += expf(vs[i][k] - mx[i]);
      }
    }
    for (int i = 0; i < 4; ++i) inv[i] = 1.0f / inv[i];
    float best = -INFINITY;
    int arg = 0;
    for (int c0 = 0; c0 < C; c0 += V) {
      up2_samples<V>(s.l, t, c0, vs);
      for (int k = 0; k < V; ++k) {
        if (c0 + k >= C) break;
        float q[4];
        for (int i = 0; i < 4; ++i) q[i] = expf(vs[i][k] - mx[i]) * inv[i];
        const float v = t.oy[0] * (t.ox[0] * q[0] + t.ox[1] * q[1]) + t.oy[1] * (t.ox[0] * q[2] + t.ox[1] * q[3]);
        if (v > best) { best = v; arg = c0 + k; }     // first index on ties
      }
    }
    return {arg, best};
  }
};

template <int V>
static Up2Confident<V> up2_confident(const float* l, int h, int w, int ld, int hi, int wi, int H, int W, int C) {
  Up2Confident<V> s;
  fill_up2(s.s, l, h, w, ld, hi, wi, H, W);
  s.C = C;
  return s;
}

// ---- test-time augmentation: the label of up to SIMT_TTA_MAX maps, each of which may belong to the horizontally mirrored frame (the
// reference's offline tools import ttach, compute_ClassDistribution.py:6, compute_ConfusionMatrix.py:6, and never use it).  A term is one
// forward's low-res map; its value at a label pixel is the sources' value above -- bil_taps + ATen's association for the one-resample
// family (FAM 1), up2_taps / up2_value for a model that upsamples inside (FAM 2) -- read at mirrored COLUMN INDICES when the term is
// flipped: the weights are untouched, so a flipped term is bit for bit the plain term on the column-reversed map ("un-mirror the
// model's output, then resample").  Terms are added in term order (MODE 0: logits, arg-max of the sum; MODE 1: probabilities, the sum
// times 1/n).
// C is a run-time value up to 255 and the taps of 8 terms do not fit in registers, so the channels go in chunks of TTA_CH = 32 sums per
// lane (C = 19 / 22 / 25: one chunk), terms outermost inside a chunk: a term's taps are formed once per chunk.  Block sizes as the
// launches of the same family: FAM 1 PL_BLOCK (the chunk's 32 sums + one term's 4 float4 taps stay below the 128 VGPRs of a 1024-thread
// block), FAM 2 PL2_BLOCK (Up2Taps + 16 float4 gathers in flight on top of the sums).
constexpr int TTA_CH = 32;
struct TtaTerm {
  Up2Scale s;          // FAM 1: l, h, w, ld and osy / osx = (h-1)/(H-1), (w-1)/(W-1); FAM 2: as fill_up2 leaves it
  int flip;
};
struct TtaTerms {
  TtaTerm t[SIMT_TTA_MAX];
  int n, C;
  float inv_n;
};

// s[j] (+)= the term's value of channel c_lo + j, for the channels of the chunk below C (V = 4: up to the next multiple of 4, inside ld)
template <int V, bool FIRST>
__device__ __forceinline__ void tta_term1(const TtaTerm& tm, int b, int y, int x, int c_lo, int C, float (&s)[TTA_CH]) {
  const Up2Scale& g = tm.s;
  int o00, o01, o10, o11;
  float wy0, wy1, wx0, wx1;
  bil_taps(y, x, g.h, g.w, g.osy, g.osx, o00, o01, o10, o11, wy0, wy1, wx0, wx1);
  if (tm.flip) {       // column ix -> w-1-ix in all four taps; ix0 as bil_taps forms it
    int ix0 = (int)(g.osx * (float)x);
    if (ix0 > g.w - 1) ix0 = g.w - 1;
    const int ix1 = ix0 + (o01 - o00);
    const int d0 = g.w - 1 - 2 * ix0, d1 = g.w - 1 - 2 * ix1;
    o00 += d0; o10 += d0; o01 += d1; o11 += d1;
  }
  const float* p = g.l + (long)b * g.h * g.w * g.ld + c_lo;
  const float *p00 = p + (long)o00 * g.ld, *p01 = p + (long)o01 * g.ld, *p10 = p + (long)o10 * g.ld, *p11 = p + (long)o11 * g.ld;
#pragma unroll
  for (int j = 0; j < TTA_CH; j += V) {
    if (c_lo + j < C) {
      VecF<V> q00, q01, q10, q11;
      q00.load(p00 + j); q01.load(p01 + j); q10.load(p10 + j); q11.load(p11 + j);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        // same association as ATen (Resample1): h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11)
        const float v = wy0 * (wx0 * q00.v[k] + wx1 * q01.v[k]) + wy1 * (wx0 * q10.v[k] + wx1 * q11.v[k]);
        if (FIRST) s[j + k] = v; else s[j + k] = s[j + k] + v;
      }
    }
  }
}

template <int V, bool FIRST>
__device__ __forceinline__ void tta_term2(const TtaTerm& tm, int b, int y, int x, int c_lo, int C, float (&s)[TTA_CH]) {
  Up2Taps t;
  up2_taps(tm.s, tm.flip, b, y, x, t);
#pragma unroll
  for (int j = 0; j < TTA_CH; j += V) {
    if (c_lo + j < C) {
      float v[V];
      up2_value<V>(tm.s.l, t, c_lo + j, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (FIRST) s[j + k] = v[k]; else s[j + k] = s[j + k] + v[k];
      }
    }
  }
}

// the first-index arg-max and the maximum of the combined terms at one pixel
template <int FAM, int V, int MODE>
struct TtaSource : TtaTerms {
  __device__ __forceinline__ ArgConf operator()(int b, int y, int x) const {
    float best = -INFINITY;
    int arg = 0;
    for (int c_lo = 0; c_lo < C; c_lo += TTA_CH) {
      float s[TTA_CH];
      if (FAM == 1) tta_term1<V, true>(t[0], b, y, x, c_lo, C, s); else tta_term2<V, true>(t[0], b, y, x, c_lo, C, s);
      for (int i = 1; i < n; ++i) {
        if (FAM == 1) tta_term1<V, false>(t[i], b, y, x, c_lo, C, s); else tta_term2<V, false>(t[i], b, y, x, c_lo, C, s);
      }
#pragma unroll
      for (int j = 0; j < TTA_CH; ++j) {
        if (c_lo + j < C) {
          const float v = MODE == 1 ? s[j] * inv_n : s[j];
          if (v > best) { best = v; arg = c_lo + j; }     // first index on ties
        }
      }
    }
    return {arg, best};
  }
};

// ================================================================= sinks ===================================================================
// ---- int32 prediction: a plain store
struct PredSink {
  struct Shared {};
  typedef int Item;
  int* pred;           // [B][H][W] arg-max class
  template <int BLOCK> __device__ __forceinline__ void init(Shared&) const {}
  __device__ __forceinline__ Item item(const Shared&, ArgConf r) const { return r.arg; }
  __device__ __forceinline__ void emit(Shared&, Item arg, long p, long P) const {
    if (p < P) pred[p] = arg;
  }
  template <int BLOCK> __device__ __forceinline__ void flush(Shared&) const {}
};

// ---- labels (255 = ignore) together with the class counts of compute_ClassDistribution.py (bins 0..C-1, then the 255s).  Counts: LDS
// histogram per block, one global atomic per non-zero bin -- exact and order independent, like hist2d_u8_kernel.
template <int BLOCK>
__device__ __forceinline__ void pl_hist_init(unsigned int* sh, int nbins) {
  for (int i = threadIdx.x; i < nbins; i += BLOCK) sh[i] = 0u;
  __syncthreads();
}
// the first n labels packed in `word` (one per byte) into the LDS histogram: runs of equal labels are added once
__device__ __forceinline__ void pl_count(unsigned int word, int n, int C, unsigned int* sh) {
  int run_bin = 0, run_n = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned int l = (word >> (8 * i)) & 255u;
    const int bin = l == 255u ? C : (int)l;
    if (bin != run_bin && run_n) { atomicAdd(&sh[run_bin], (unsigned int)run_n); run_n = 0; }
    run_bin = bin;
    ++run_n;
  }
  atomicAdd(&sh[run_bin], (unsigned int)run_n);
}
// uint8 labels, a quarter of the int32 bytes.  Each quad of lanes = 4 consecutive pixels of the flattened [B][H][W] map (consecutive x; the
// quad runs on into the next row when W % 4 != 0): two lane shuffles pack the 4 labels into the quad leader, which writes one 32-bit store
// (byte stores for the last P % 4 pixels) and counts them.
__device__ __forceinline__ void pl_store(unsigned int lab, long p, long P, int C, unsigned char* out, unsigned int* sh) {
  const bool leader = (threadIdx.x & 3) == 0;
  unsigned int word = lab | (__shfl_down(lab, 1, 4) << 8);
  word |= __shfl_down(word, 2, 4) << 16;
  if (leader && p < P) {
    const int n = P - p < 4 ? (int)(P - p) : 4;
    if (n == 4) {
      *reinterpret_cast<unsigned int*>(out + p) = word;
    } else {
      for (int i = 0; i < n; ++i) out[p + i] = (unsigned char)(word >> (8 * i));
    }
    pl_count(word, n, C, sh);
  }
}
// the int64 labels the head kernels read (online labels, DESIGN 7.16: no uint8 map, no widening copy): a wave's 64 labels are one contiguous
// 512-byte store; the counts through the same quad shuffle
__device__ __forceinline__ void ol_store(unsigned int lab, long p, long P, int C, long long* label, unsigned int* sh) {
  unsigned int word = lab | (__shfl_down(lab, 1, 4) << 8);
  word |= __shfl_down(word, 2, 4) << 16;
  if (p < P) {
    label[p] = (long long)lab;
    if ((threadIdx.x & 3) == 0) pl_count(word, P - p < 4 ? (int)(P - p) : 4, C, sh);
  }
}
template <int BLOCK>
__device__ __forceinline__ void pl_hist_flush(const unsigned int* sh, int nbins, unsigned long long* counts) {
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += BLOCK)
    if (sh[i]) atomicAdd(&counts[i], (unsigned long long)sh[i]);
}

// where the labels go
struct U8Out {
  unsigned char* out;           // [B][H][W] labels, 4-byte aligned
  unsigned long long* counts;   // [C+1], accumulated
  __device__ __forceinline__ void store(unsigned int lab, long p, long P, int C, unsigned int* sh) const { pl_store(lab, p, P, C, out, sh); }
};
struct I64Out {
  long long* label;             // [B][H][W]
  unsigned long long* counts;   // [C+1], accumulated
  __device__ __forceinline__ void store(unsigned int lab, long p, long P, int C, unsigned int* sh) const { ol_store(lab, p, P, C, label, sh); }
};

// which pixels keep their arg-max (`thr`: the per-class thresholds in LDS, where the sink has them)
struct KeepAll {
  __device__ __forceinline__ unsigned int operator()(ArgConf r, const float*) const { return (unsigned int)r.arg; }
};
struct Strict {        // strictly greater (trainV2_simt.py:359); a NaN on either side: 255
  float threshold;
  __device__ __forceinline__ unsigned int operator()(ArgConf r, const float*) const { return (unsigned int)(!(r.conf > threshold) ? 255 : r.arg); }
};
struct PerClass {      // kept iff conf >= thr[arg]
  __device__ __forceinline__ unsigned int operator()(ArgConf r, const float* thr) const { return r.conf >= thr[r.arg] ? (unsigned int)r.arg : 255u; }
};
struct PerClassOrStrict {      // test-time augmentation, mode 1: the per-class rule where thresholds are given, else the strict one
  int strict;
  float threshold;
  __device__ __forceinline__ unsigned int operator()(ArgConf r, const float* thr) const {
    return strict ? Strict{threshold}(r, thr) : PerClass{}(r, thr);
  }
};

template <class Out, class Rule>
struct CountSink {
  typedef unsigned int Shared[256];
  typedef unsigned int Item;    // the label
  Out o;
  Rule rule;
  int C;
  template <int BLOCK> __device__ __forceinline__ void init(Shared& sh) const { pl_hist_init<BLOCK>(sh, C + 1); }
  __device__ __forceinline__ Item item(const Shared&, ArgConf r) const { return rule(r, nullptr); }
  static __device__ __forceinline__ unsigned int label(Item lab) { return lab; }
  __device__ __forceinline__ void emit(Shared& sh, Item lab, long p, long P) const { o.store(lab, p, P, C, sh); }
  template <int BLOCK> __device__ __forceinline__ void flush(Shared& sh) const { pl_hist_flush<BLOCK>(sh, C + 1, o.counts); }
};

// ---- class-balanced labels (CBST / the label generator of BDL): per class, the threshold is the confidence at a fixed rank among that
// class's own predictions, so the export needs the per-class distribution of the confidence over the whole data list.  The sink takes
// (arg, conf) and counts them into hist[arg][bin] (STATS; bin = floor(conf * 256) clamped to [0, 255]: the scaling by a power of two is
// exact, so the bin is a pure function of the float), labels with a per-class threshold (LABELS), or both.
//
// The histogram is the hot path: on real frames a large share of the pixels of a frame fall into ONE word (road at conf ~ 1), and one
// global word takes ~88 atomics / us.  So (1) the counters are private to the workgroup in LDS (C * 256 words, C <= 64), (2) equal keys
// are aggregated within the wave before the LDS atomic: up to CONF_AGG_ROUNDS times the first lane still to do broadcasts its key, the
// lanes holding that key are found with one ballot and the first lane adds their number -- a wave whose 64 lanes hit the hot bin
// issues one add; the lanes left after the rounds (keys spread over many bins: little contention) add 1 each -- and (3) only the
// non-zero bins are flushed, one 64-bit global atomic each.  Integer counts: exact and order independent.
//
// Over the two-resample gather the float4 launches hold 128-139 VGPRs, so the label and combined ones run 3 waves per SIMD where the
// strict-rule launch runs 4; a form that fit 124 had its 16-byte loads of the last sweep split into elements and ran 370 us against 319 us
// for this one and 317 us for the strict-rule launch: the gather is bound by its load instructions, not by occupancy.
constexpr int CONF_BINS = SIMT_CONF_BINS, CONF_MAX_C = 64, CONF_AGG_ROUNDS = 4;

__device__ __forceinline__ int conf_bin(float conf) {
  const float f = fminf(fmaxf(floorf(conf * (float)CONF_BINS), 0.f), (float)(CONF_BINS - 1));
  return (int)f;
}

// every lane of the wave calls this together
__device__ __forceinline__ void conf_hist_add(bool valid, unsigned int key, unsigned int* sh) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long todo = __ballot(valid);
  for (int r = 0; r < CONF_AGG_ROUNDS && todo; ++r) {
    const int leader = __ffsll(todo) - 1;
    const unsigned int k = (unsigned int)__builtin_amdgcn_readlane((int)key, leader);
    const unsigned long long m = __ballot(valid && key == k) & todo;
    if (lane == leader) atomicAdd(&sh[k], (unsigned int)__popcll(m));
    todo &= ~m;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&sh[key], 1u);
}

// the label counts and thresholds of the labels' side, and the confidence histogram
template <bool STATS>
struct ConfShared {
  unsigned int counts[256];
  float thr[256];
  unsigned int hist[STATS ? CONF_MAX_C * CONF_BINS : 1];
};

struct ConfOut : U8Out {        // (out and counts: with LABELS)
  unsigned long long* hist;     // [C][CONF_BINS], accumulated, or NULL
  float thr[255];               // per-class thresholds, kernel arguments
};
// class-balanced online labels: the thresholds are read from DEVICE memory at block start, so that the launch behind this one
// (class_thresholds_kernel) can move them without the host
struct OnlineCbOut : I64Out {
  unsigned long long* hist;     // [C][CONF_BINS], accumulated
  const float* thr;             // [C], device memory
};

template <bool STATS, bool LABELS, class Out, class Rule = PerClass>
struct ConfSink {
  typedef ConfShared<STATS> Shared;
  struct Item { unsigned int key, lab; };      // the histogram word (STATS) and the label (LABELS)
  Out o;
  Rule rule;
  int C;
  template <int BLOCK> __device__ __forceinline__ void init(Shared& sh) const {
    if (LABELS)
      for (int i = threadIdx.x; i < C; i += BLOCK) sh.thr[i] = o.thr[i];
    if (STATS)
      for (int i = threadIdx.x; i < C * CONF_BINS; i += BLOCK) sh.hist[i] = 0u;
    pl_hist_init<BLOCK>(sh.counts, C + 1);
  }
  __device__ __forceinline__ Item item(const Shared& sh, ArgConf r) const {
    Item it = {0u, 0u};
    if (STATS) it.key = (unsigned int)(r.arg * CONF_BINS + conf_bin(r.conf));
    if (LABELS) it.lab = rule(r, sh.thr);
    return it;
  }
  static __device__ __forceinline__ unsigned int label(const Item& it) { return it.lab; }
  __device__ __forceinline__ void emit(Shared& sh, Item it, long p, long P) const {
    if (STATS) conf_hist_add(p < P, it.key, sh.hist);
    if (LABELS) o.store(it.lab, p, P, C, sh.counts);
  }
  template <int BLOCK> __device__ __forceinline__ void flush(Shared& sh) const {
    if (LABELS) pl_hist_flush<BLOCK>(sh.counts, C + 1, o.counts);
    if (STATS) pl_hist_flush<BLOCK>(sh.hist, C * CONF_BINS, o.hist);
  }
};

// the checks of the class-balanced export's output side, and its arguments
static int conf_out_fill(ConfOut& o, int C, const float* thr, uint8_t* out, int64_t* counts, int64_t* hist) {
  SIMT_CHECK(out || hist);
  SIMT_CHECK(!out || (thr && counts && ((uintptr_t)out & 3) == 0));
  SIMT_CHECK(!hist || C <= CONF_MAX_C);
  o.out = out; o.counts = (unsigned long long*)counts; o.hist = (unsigned long long*)hist;
  for (int c = 0; c < 255; ++c) o.thr[c] = (out && c < C) ? thr[c] : 0.f;
  return SIMT_OK;
}

// the three (hist, out) combinations of a class-balanced uint8 launch
template <int BLOCK, int MAX_GRID, class Source, class Rule>
static void launch_conf(const Source& src, const ConfOut& o, Rule rule, int B, int H, int W, int C, simt_stream_t stream) {
  if (o.hist && o.out)
    launch_sweep<BLOCK, MAX_GRID>(src, ConfSink<true, true, ConfOut, Rule>{o, rule, C}, B, H, W, stream);
  else if (o.hist)
    launch_sweep<BLOCK, MAX_GRID>(src, ConfSink<true, false, ConfOut, Rule>{o, rule, C}, B, H, W, stream);
  else
    launch_sweep<BLOCK, MAX_GRID>(src, ConfSink<false, true, ConfOut, Rule>{o, rule, C}, B, H, W, stream);
}

// ---- test-time augmentation, mode 0: the int32 prediction and / or uint8 labels + counts
struct TtaArgmaxSink {
  typedef ConfShared<false> Shared;
  typedef int Item;
  int* pred;           // [B][H][W] or NULL
  U8Out o;             // out: [B][H][W] or NULL
  int C;
  template <int BLOCK> __device__ __forceinline__ void init(Shared& sh) const { pl_hist_init<BLOCK>(sh.counts, C + 1); }
  __device__ __forceinline__ Item item(const Shared&, ArgConf r) const { return r.arg; }
  __device__ __forceinline__ void emit(Shared& sh, Item arg, long p, long P) const {
    if (pred && p < P) pred[p] = arg;
    if (o.out) o.store((unsigned int)arg, p, P, C, sh.counts);
  }
  template <int BLOCK> __device__ __forceinline__ void flush(Shared& sh) const {
    if (o.out) pl_hist_flush<BLOCK>(sh.counts, C + 1, o.counts);
  }
};

// ---- class presence (ClassMix behind the teacher): a DECORATOR over a label sink.  Item, label rule, stores, counts and
// histogram are the inner sink's, untouched; on top, the sweep leaves the words simt_class_mix_u8 builds its paste mask from:
// part[b][g] = OR of 1u << l over the labels l < C of item b that workgroup g emitted (a 255 sets no bit; item-major, so that the mix reads
// an item's words as one contiguous run).  The sweep is flat over B*H*W and strides by the grid, so a workgroup meets several items: one
// LDS word per item (B <= SIMT_CLASS_MIX_MAX), OR-ed with LDS atomics -- once per wave where its 64 pixels lie in one item (an xor-shuffle
// OR first; every wave but the few that straddle an item's edge), once per lane with a bit otherwise.  The flush stores the workgroup's
// word of EVERY item, zeros included: every word of `part` is written by plain stores on every call -- no global atomics, nothing to
// zero, simt_label_presence's contract.  An OR: exact and order independent.  Nothing lives across the sweep's bounds check but the inner
// sink's Item.
template <class Inner>
struct PresenceSink {
  struct Shared {
    typename Inner::Shared in;
    unsigned int pres[SIMT_CLASS_MIX_MAX];
  };
  typedef typename Inner::Item Item;
  Inner in;
  unsigned int* part;  // [B][gridDim.x]
  int B;
  long HW;             // H * W: pixel p belongs to item p / HW
  template <int BLOCK> __device__ __forceinline__ void init(Shared& sh) const {
    if (threadIdx.x < SIMT_CLASS_MIX_MAX) sh.pres[threadIdx.x] = 0u;
    in.template init<BLOCK>(sh.in);                      // (ends with the barrier that also covers pres)
  }
  __device__ __forceinline__ Item item(const Shared& sh, ArgConf r) const { return in.item(sh.in, r); }
  __device__ __forceinline__ void emit(Shared& sh, Item it, long p, long P) const {
    in.emit(sh.in, it, p, P);
    const unsigned int lab = Inner::label(it);
    unsigned int bits = (p < P && lab < (unsigned int)in.C) ? 1u << lab : 0u;
    const int b = (int)((p < P ? p : P - 1) / HW);       // lanes past the end: the last item, and no bit
    const int b_first = __builtin_amdgcn_readfirstlane(b), b_last = __builtin_amdgcn_readlane(b, 63);
    if (b_first == b_last) {                             // wave-uniform: the 64 lanes' pixels are consecutive
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) bits |= (unsigned int)__shfl_xor((int)bits, o, 64);
      if ((threadIdx.x & 63) == 0 && bits) atomicOr(&sh.pres[b_first], bits);
    } else if (bits) {
      atomicOr(&sh.pres[b], bits);
    }
  }
  template <int BLOCK> __device__ __forceinline__ void flush(Shared& sh) const {
    in.template flush<BLOCK>(sh.in);
    __syncthreads();
    if ((int)threadIdx.x < B) part[(long)threadIdx.x * gridDim.x + blockIdx.x] = sh.pres[threadIdx.x];
  }
};

// class-balanced online labels as bytes: OnlineCbOut over the uint8 output
struct OnlineCbOut8 : U8Out {
  unsigned long long* hist;     // [C][CONF_BINS], accumulated
  const float* thr;             // [C], device memory
};

// ---- quality-weighted labels: the threshold no longer deletes a pixel, it only decides which count the pixel lands in.  The
// Item carries TWO labels: byte 0 the one that is written (Strict{-INFINITY}: the arg-max, 255 for a NaN confidence), byte 1 the one
// simt_online_label at the threshold would have written (Strict{threshold}), which is what is COUNTED -- counts[] therefore stays what that
// launch accumulates and `labelled` keeps its meaning.  pl_store / ol_store with the counted word packed beside the stored one.
__device__ __forceinline__ unsigned int quad_pack(unsigned int v) {
  unsigned int word = v | (__shfl_down(v, 1, 4) << 8);
  word |= __shfl_down(word, 2, 4) << 16;
  return word;
}
__device__ __forceinline__ void store_w(const U8Out& o, unsigned int lab, unsigned int key, long p, long P, int C, unsigned int* sh) {
  const unsigned int word = quad_pack(lab), kword = quad_pack(key);
  if ((threadIdx.x & 3) == 0 && p < P) {
    const int n = P - p < 4 ? (int)(P - p) : 4;
    if (n == 4) {
      *reinterpret_cast<unsigned int*>(o.out + p) = word;
    } else {
      for (int i = 0; i < n; ++i) o.out[p + i] = (unsigned char)(word >> (8 * i));
    }
    pl_count(kword, n, C, sh);
  }
}
__device__ __forceinline__ void store_w(const I64Out& o, unsigned int lab, unsigned int key, long p, long P, int C, unsigned int* sh) {
  const unsigned int kword = quad_pack(key);
  if (p < P) {
    o.label[p] = (long long)lab;
    if ((threadIdx.x & 3) == 0) pl_count(kword, P - p < 4 ? (int)(P - p) : 4, C, sh);
  }
}

template <class Out>
struct WeightedSink {
  typedef unsigned int Shared[256];
  typedef unsigned int Item;    // byte 0: the label written; byte 1: the label counted
  Out o;
  float threshold;
  int C;
  template <int BLOCK> __device__ __forceinline__ void init(Shared& sh) const { pl_hist_init<BLOCK>(sh, C + 1); }
  __device__ __forceinline__ Item item(const Shared&, ArgConf r) const {
    return Strict{-INFINITY}(r, nullptr) | (Strict{threshold}(r, nullptr) << 8);
  }
  static __device__ __forceinline__ unsigned int label(Item it) { return it & 255u; }
  static __device__ __forceinline__ bool confident(Item it) { return ((it >> 8) & 255u) != 255u; }
  __device__ __forceinline__ void emit(Shared& sh, Item it, long p, long P) const { store_w(o, it & 255u, (it >> 8) & 255u, p, P, C, sh); }
  template <int BLOCK> __device__ __forceinline__ void flush(Shared& sh) const { pl_hist_flush<BLOCK>(sh, C + 1, o.counts); }
};

// the per-item count of confident pixels: a DECORATOR in PresenceSink's pattern -- one LDS word per item, added to once per wave where the
// wave's 64 pixels lie in one item (a ballot's population count), once per confident lane otherwise; the flush stores the workgroup's word of
// EVERY item with a plain store: conf_part[b][g] is written on every call, no global atomics, nothing to zero.  Integer counts: exact and order
// independent.  It forwards label() and C, so that PresenceSink composes over it.
template <class Inner>
struct ConfPartSink {
  struct Shared {
    typename Inner::Shared in;
    unsigned int n[SIMT_CLASS_MIX_MAX];
  };
  typedef typename Inner::Item Item;
  Inner in;
  unsigned int* conf_part;      // [B][gridDim.x]
  int B;
  long HW;
  int C;
  template <int BLOCK> __device__ __forceinline__ void init(Shared& sh) const {
    if (threadIdx.x < SIMT_CLASS_MIX_MAX) sh.n[threadIdx.x] = 0u;
    in.template init<BLOCK>(sh.in);                      // (ends with the barrier that also covers n)
  }
  __device__ __forceinline__ Item item(const Shared& sh, ArgConf r) const { return in.item(sh.in, r); }
  static __device__ __forceinline__ unsigned int label(const Item& it) { return Inner::label(it); }
  __device__ __forceinline__ void emit(Shared& sh, Item it, long p, long P) const {
    in.emit(sh.in, it, p, P);
    const bool ok = p < P && Inner::confident(it);
    const int b = (int)((p < P ? p : P - 1) / HW);       // lanes past the end: the last item, and no count
    const int b_first = __builtin_amdgcn_readfirstlane(b), b_last = __builtin_amdgcn_readlane(b, 63);
    if (b_first == b_last) {
      const unsigned long long m = __ballot(ok);
      if ((threadIdx.x & 63) == 0 && m) atomicAdd(&sh.n[b_first], (unsigned int)__popcll(m));
    } else if (ok) {
      atomicAdd(&sh.n[b], 1u);
    }
  }
  template <int BLOCK> __device__ __forceinline__ void flush(Shared& sh) const {
    in.template flush<BLOCK>(sh.in);
    __syncthreads();
    if ((int)threadIdx.x < B) conf_part[(long)threadIdx.x * gridDim.x + blockIdx.x] = sh.n[threadIdx.x];
  }
};

// ============================================================== entry points ===============================================================
extern "C" int simt_upsample_sum_argmax(const float* la, int ha, int wa, int lda, const float* lb, int hb, int wb, int ldb,
                                        int B, int H, int W, int C, int32_t* pred, simt_stream_t stream) {
  SIMT_CHECK(la && pred && B > 0 && C > 0 && C <= lda && (!lb || C <= ldb));
  launch_sweep<EV_BLOCK, EV_MAX_GRID>(resample1<0>(la, ha, wa, lda, lb, hb, wb, ldb, H, W, C), PredSink{pred}, B, H, W, stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_upsample2_sum_argmax(const float* la, int ha, int wa, int lda, int hia, int wia, const float* lb, int hb, int wb,
                                         int ldb, int hib, int wib, int B, int H, int W, int C, int32_t* pred, simt_stream_t stream) {
  SIMT_CHECK(la && pred && B > 0 && H > 0 && W > 0 && C > 0 && C <= lda && ha > 0 && wa > 0 && hia > 0 && wia > 0);
  SIMT_CHECK(!lb || (C <= ldb && hb > 0 && wb > 0 && hib > 0 && wib > 0));
  SIMT_CHECK((long)B * ha * wa * lda < 2147483647L && (!lb || (long)B * hb * wb * ldb < 2147483647L));
  if (vec4_ok(la, lda) && (!lb || vec4_ok(lb, ldb)))
    launch_sweep<EV_BLOCK, EV_MAX_GRID>(up2_argmax<4>(la, ha, wa, lda, hia, wia, lb, hb, wb, ldb, hib, wib, H, W, C), PredSink{pred}, B, H, W, stream);
  else
    launch_sweep<EV_BLOCK, EV_MAX_GRID>(up2_argmax<1>(la, ha, wa, lda, hia, wia, lb, hb, wb, ldb, hib, wib, H, W, C), PredSink{pred}, B, H, W, stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- pseudo-label export (the commented-out save lines of evaluate_simt :150-156 / evaluate_warmup :214-219).  mode 0: the evaluator's
// arg-max as uint8; mode 1: the arg-max of the probabilities where their maximum > threshold, 255 elsewhere.
extern "C" int simt_pseudo_label_u8(const float* la, int ha, int wa, int lda, const float* lb, int hb, int wb, int ldb, int B, int H,
                                    int W, int C, int mode, float threshold, uint8_t* out, int64_t* counts, simt_stream_t stream) {
  SIMT_CHECK(la && out && counts && B > 0 && H > 0 && W > 0 && ha > 0 && wa > 0 && C > 0 && C <= 255 && C <= lda);
  SIMT_CHECK((mode == 0 && (!lb || (C <= ldb && hb > 0 && wb > 0))) || (mode == 1 && !lb));
  SIMT_CHECK(((uintptr_t)out & 3) == 0);
  const U8Out o{out, (unsigned long long*)counts};
  if (mode == 0)
    launch_sweep<PL_BLOCK, PL_MAX_GRID>(resample1<0>(la, ha, wa, lda, lb, hb, wb, ldb, H, W, C), CountSink<U8Out, KeepAll>{o, {}, C}, B, H, W, stream);
  else
    launch_sweep<PL_BLOCK, PL_MAX_GRID>(resample1<1>(la, ha, wa, lda, lb, hb, wb, ldb, H, W, C), CountSink<U8Out, Strict>{o, {threshold}, C}, B, H, W, stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_pseudo_label2_u8(const float* la, int ha, int wa, int lda, int hia, int wia, const float* lb, int hb, int wb, int ldb,
                                     int hib, int wib, int B, int H, int W, int C, int mode, float threshold, uint8_t* out, int64_t* counts,
                                     simt_stream_t stream) {
  SIMT_CHECK(la && out && counts && B > 0 && H > 0 && W > 0 && C > 0 && C <= 255 && C <= lda && ha > 0 && wa > 0 && hia > 0 && wia > 0);
  SIMT_CHECK((mode == 0 && (!lb || (C <= ldb && hb > 0 && wb > 0 && hib > 0 && wib > 0))) || (mode == 1 && !lb));
  SIMT_CHECK((long)B * ha * wa * lda < 2147483647L && (!lb || (long)B * hb * wb * ldb < 2147483647L));
  SIMT_CHECK(((uintptr_t)out & 3) == 0);
  const U8Out o{out, (unsigned long long*)counts};
  const CountSink<U8Out, KeepAll> all{o, {}, C};
  const CountSink<U8Out, Strict> strict{o, {threshold}, C};
  const bool vec = vec4_ok(la, lda) && (!lb || vec4_ok(lb, ldb));
  if (mode == 0 && vec)
    launch_sweep<PL2_BLOCK, PL2_MAX_GRID>(up2_argmax<4>(la, ha, wa, lda, hia, wia, lb, hb, wb, ldb, hib, wib, H, W, C), all, B, H, W, stream);
  else if (mode == 0)
    launch_sweep<PL2_BLOCK, PL2_MAX_GRID>(up2_argmax<1>(la, ha, wa, lda, hia, wia, lb, hb, wb, ldb, hib, wib, H, W, C), all, B, H, W, stream);
  else if (vec)
    launch_sweep<PL2_BLOCK, PL2_MAX_GRID>(up2_confident<4>(la, ha, wa, lda, hia, wia, H, W, C), strict, B, H, W, stream);
  else
    launch_sweep<PL2_BLOCK, PL2_MAX_GRID>(up2_confident<1>(la, ha, wa, lda, hia, wia, H, W, C), strict, B, H, W, stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_pseudo_conf_u8(const float* la, int ha, int wa, int lda, int B, int H, int W, int C, const float* thr, uint8_t* out,
                                   int64_t* counts, int64_t* hist, simt_stream_t stream) {
  SIMT_CHECK(la && B > 0 && H > 0 && W > 0 && ha > 0 && wa > 0 && C > 0 && C <= 255 && C <= lda);
  ConfOut o;
  if (int rc = conf_out_fill(o, C, thr, out, counts, hist)) return rc;
  launch_conf<PL_BLOCK, PL_MAX_GRID>(resample1<1>(la, ha, wa, lda, nullptr, 0, 0, 0, H, W, C), o, PerClass{}, B, H, W, C, stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_pseudo_conf2_u8(const float* la, int ha, int wa, int lda, int hia, int wia, int B, int H, int W, int C,
                                    const float* thr, uint8_t* out, int64_t* counts, int64_t* hist, simt_stream_t stream) {
  SIMT_CHECK(la && B > 0 && H > 0 && W > 0 && C > 0 && C <= 255 && C <= lda && ha > 0 && wa > 0 && hia > 0 && wia > 0);
  SIMT_CHECK((long)B * ha * wa * lda < 2147483647L);
  ConfOut o;
  if (int rc = conf_out_fill(o, C, thr, out, counts, hist)) return rc;
  if (vec4_ok(la, lda))
    launch_conf<PL2_BLOCK, PL2_MAX_GRID>(up2_confident<4>(la, ha, wa, lda, hia, wia, H, W, C), o, PerClass{}, B, H, W, C, stream);
  else
    launch_conf<PL2_BLOCK, PL2_MAX_GRID>(up2_confident<1>(la, ha, wa, lda, hia, wia, H, W, C), o, PerClass{}, B, H, W, C, stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- online labels: the warm-up trainers' teacher labels every batch on the device: the sources and the rule of the export's
// confidence mode, written as int64.  Family 0: Resample1<1>.  Family 1: Up2Confident with a virtual map of the label's own size (hia = H,
// wia = W): its outer taps then have weights exactly 1 and 0, but a one-sample shortcut is NOT bit-equal (0 * NaN of a neighbouring sample
// is NaN there, and H == 1 gives scale 0), so the four-sample source is used as it is.
template <class Sink>
static int launch_online(const float* fix, int B, int h, int w, int ld, int H, int W, int C, int family, const Sink& sink, simt_stream_t stream) {
  if (family == 0) {
    launch_sweep<PL_BLOCK, PL_MAX_GRID>(resample1<1>(fix, h, w, ld, nullptr, 0, 0, 0, H, W, C), sink, B, H, W, stream);
  } else {
    SIMT_CHECK((long)B * h * w * ld < 2147483647L);          // the taps' element offsets are 32-bit (Up2Taps)
    if (vec4_ok(fix, ld))
      launch_sweep<PL2_BLOCK, PL2_MAX_GRID>(up2_confident<4>(fix, h, w, ld, H, W, H, W, C), sink, B, H, W, stream);
    else
      launch_sweep<PL2_BLOCK, PL2_MAX_GRID>(up2_confident<1>(fix, h, w, ld, H, W, H, W, C), sink, B, H, W, stream);
  }
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_online_label(const simt_online_label_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->fix && d->label && d->counts);
  SIMT_CHECK(d->B > 0 && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C <= 255 && d->C <= d->ld);
  SIMT_CHECK(d->family == 0 || d->family == 1);
  SIMT_CHECK(((uintptr_t)d->label & 7) == 0);
  const CountSink<I64Out, Strict> sink{{(long long*)d->label, (unsigned long long*)d->counts}, {d->threshold}, d->C};
  return launch_online(d->fix, d->B, d->h, d->w, d->ld, d->H, d->W, d->C, d->family, sink, stream);
}

// class-balanced online labels: the combined class-balanced sink (STATS and LABELS) over the int64 output
extern "C" int simt_online_label_cb(const simt_online_label_cb_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->fix && d->label && d->counts && d->hist && d->thr);
  SIMT_CHECK(d->B > 0 && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C <= CONF_MAX_C && d->C <= d->ld);
  SIMT_CHECK(d->family == 0 || d->family == 1);
  SIMT_CHECK(((uintptr_t)d->label & 7) == 0 && ((uintptr_t)d->hist & 7) == 0 && ((uintptr_t)d->thr & 3) == 0);
  OnlineCbOut o;
  o.label = (long long*)d->label; o.counts = (unsigned long long*)d->counts; o.hist = (unsigned long long*)d->hist; o.thr = d->thr;
  const ConfSink<true, true, OnlineCbOut> sink{o, {}, d->C};
  return launch_online(d->fix, d->B, d->h, d->w, d->ld, d->H, d->W, d->C, d->family, sink, stream);
}

// ---- online labels for the mix behind the teacher: the two launches above with the label as a BYTE (U8Out: the export's
// store) and the presence words on top (PresenceSink).  Sources, rule, counts, hist and thr are the parents'.
template <class D>
static int online_u8_checks(const D* d) {
  SIMT_CHECK(d && d->fix && d->lab8 && d->counts && d->part);
  SIMT_CHECK(d->B > 0 && d->B <= SIMT_CLASS_MIX_MAX && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0);
  SIMT_CHECK(d->C > 0 && d->C <= SIMT_CLASS_MIX_CLASSES && d->C <= d->ld);
  SIMT_CHECK(d->family == 0 || d->family == 1);
  SIMT_CHECK((long)d->H * d->W < (1L << 31));
  SIMT_CHECK(((uintptr_t)d->lab8 & 15) == 0 && ((uintptr_t)d->counts & 7) == 0 && ((uintptr_t)d->part & 3) == 0);
  return SIMT_OK;
}

extern "C" int simt_online_label_parts(const simt_online_label_u8_desc* d) {
  if (!d || d->B <= 0 || d->H <= 0 || d->W <= 0 || (d->family != 0 && d->family != 1)) return -1;
  const long P = (long)d->B * d->H * d->W;
  const long block = d->family ? PL2_BLOCK : PL_BLOCK, max_grid = d->family ? PL2_MAX_GRID : PL_MAX_GRID;      // launch_sweep's clamp
  const long grid = (P + block - 1) / block;
  return (int)(grid > max_grid ? max_grid : grid);
}

extern "C" int simt_online_label_u8(const simt_online_label_u8_desc* d, simt_stream_t stream) {
  if (int rc = online_u8_checks(d)) return rc;
  const CountSink<U8Out, Strict> inner{{d->lab8, (unsigned long long*)d->counts}, {d->threshold}, d->C};
  const PresenceSink<CountSink<U8Out, Strict>> sink{inner, d->part, d->B, (long)d->H * d->W};
  return launch_online(d->fix, d->B, d->h, d->w, d->ld, d->H, d->W, d->C, d->family, sink, stream);
}

extern "C" int simt_online_label_cb_u8(const simt_online_label_cb_u8_desc* d, simt_stream_t stream) {
  if (int rc = online_u8_checks(d)) return rc;
  SIMT_CHECK(d->hist && d->thr && ((uintptr_t)d->hist & 7) == 0 && ((uintptr_t)d->thr & 3) == 0);
  OnlineCbOut8 o;
  o.out = d->lab8; o.counts = (unsigned long long*)d->counts; o.hist = (unsigned long long*)d->hist; o.thr = d->thr;
  const ConfSink<true, true, OnlineCbOut8> inner{o, {}, d->C};
  const PresenceSink<ConfSink<true, true, OnlineCbOut8>> sink{inner, d->part, d->B, (long)d->H * d->W};
  return launch_online(d->fix, d->B, d->h, d->w, d->ld, d->H, d->W, d->C, d->family, sink, stream);
}

// ---- quality-weighted online labels: every pixel keeps its arg-max, the threshold decides the counts and the per-item
// number of confident pixels simt_label_quality turns into the weights.  Sources and families are launch_online's.
template <class D>
static int online_w_checks(const D* d, bool u8) {
  SIMT_CHECK(d && d->fix && d->counts && d->conf_part);
  SIMT_CHECK(d->B > 0 && d->B <= SIMT_CLASS_MIX_MAX && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0);
  SIMT_CHECK(d->C > 0 && d->C <= (u8 ? SIMT_CLASS_MIX_CLASSES : 255) && d->C <= d->ld);
  SIMT_CHECK(d->family == 0 || d->family == 1);
  SIMT_CHECK((long)d->H * d->W < (1L << 31));
  SIMT_CHECK(((uintptr_t)d->counts & 7) == 0 && ((uintptr_t)d->conf_part & 3) == 0);
  return SIMT_OK;
}

extern "C" int simt_online_label_w(const simt_online_label_w_desc* d, simt_stream_t stream) {
  if (int rc = online_w_checks(d, false)) return rc;
  SIMT_CHECK(d->label && ((uintptr_t)d->label & 7) == 0);
  const WeightedSink<I64Out> inner{{(long long*)d->label, (unsigned long long*)d->counts}, d->threshold, d->C};
  const ConfPartSink<WeightedSink<I64Out>> sink{inner, d->conf_part, d->B, (long)d->H * d->W, d->C};
  return launch_online(d->fix, d->B, d->h, d->w, d->ld, d->H, d->W, d->C, d->family, sink, stream);
}

extern "C" int simt_online_label_w_u8(const simt_online_label_w_u8_desc* d, simt_stream_t stream) {
  if (int rc = online_w_checks(d, true)) return rc;
  SIMT_CHECK(d->lab8 && d->part && ((uintptr_t)d->lab8 & 15) == 0 && ((uintptr_t)d->part & 3) == 0);
  const WeightedSink<U8Out> inner{{d->lab8, (unsigned long long*)d->counts}, d->threshold, d->C};
  const ConfPartSink<WeightedSink<U8Out>> mid{inner, d->conf_part, d->B, (long)d->H * d->W, d->C};
  const PresenceSink<ConfPartSink<WeightedSink<U8Out>>> sink{mid, d->part, d->B, (long)d->H * d->W};
  return launch_online(d->fix, d->B, d->h, d->w, d->ld, d->H, d->W, d->C, d->family, sink, stream);
}

// The weights: q[b] = the share of confident pixels, of item b (mode 0, "item") or of the whole micro-batch (mode 1, "batch": DACS's scalar,
// written to every entry).  ONE workgroup; wave v sums the rows of items v, v + LQ_BLOCK / 64, ... as 64-bit integers (lanes stride the row,
// six shuffle steps), the sums meet in LDS, and thread b forms its quotient: one conversion of each integer to double (exact below 2^53),
// one division, one rounding to float -- np.float32(np.float64(n) / np.float64(N)).  No atomics.
constexpr int LQ_BLOCK = 256;

__global__ __launch_bounds__(LQ_BLOCK) void label_quality_kernel(const unsigned int* __restrict__ conf_part, float* __restrict__ q, int B,
                                                                 int rows, long HW, int mode) {
  __shared__ unsigned long long n[SIMT_CLASS_MIX_MAX];
  const int lane = (int)(threadIdx.x & 63);
  for (int b = (int)(threadIdx.x >> 6); b < B; b += LQ_BLOCK / 64) {          // uniform over the wave
    unsigned long long s = 0ull;
    for (int g = lane; g < rows; g += 64) s += (unsigned long long)conf_part[(long)b * rows + g];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) n[b] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < B) {
    unsigned long long num = n[threadIdx.x];
    long den = HW;
    if (mode == 1) {
      num = 0ull;
      for (int b = 0; b < B; ++b) num += n[b];
      den = (long)B * HW;
    }
    q[threadIdx.x] = (float)((double)num / (double)den);
  }
}

extern "C" int simt_label_quality(const simt_label_quality_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->conf_part && d->q && ((uintptr_t)d->conf_part & 3) == 0 && ((uintptr_t)d->q & 3) == 0);
  SIMT_CHECK(d->B > 0 && d->B <= SIMT_CLASS_MIX_MAX && d->H > 0 && d->W > 0 && (long)d->H * d->W < (1L << 31));
  SIMT_CHECK(d->rows >= 1 && d->rows <= SIMT_ONLINE_LABEL_MAX_PARTS);
  SIMT_CHECK(d->mode == 0 || d->mode == 1);
  hipLaunchKernelGGL(label_quality_kernel, dim3(1), dim3(LQ_BLOCK), 0, (hipStream_t)stream, d->conf_part, d->q, d->B, d->rows,
                     (long)d->H * d->W, d->mode);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// The thresholds' side: class_thresholds() of tools/make_pseudo_labels.py on the device, the fold into thr, and the histogram's reset.  ONE
// workgroup of CT_BLOCK / 64 waves; wave v takes classes v, v + CT_BLOCK / 64, ...  Lane l holds bins 4l .. 4l+3 of the class's row (the
// row is 64 lanes x 4 bins = CONF_BINS), an inclusive prefix sum of the lanes' 64-bit totals runs over the wave (6 shuffle steps), the
// first lane whose inclusive sum exceeds k is found with one ballot, and that lane walks its 4 bins.  Integer arithmetic throughout; the
// only floating point is (double)n * drop (n < 2^53: exact conversion, one rounding, then rint: half to even -- np.round of the same
// product) and the three fp32 operations of the fold.  The lane then zeroes its 4 bins.  No LDS, no atomics.
constexpr int CT_BLOCK = 256;
static_assert(CONF_BINS == 64 * 4, "class_thresholds_kernel: one wave holds one row, four bins per lane");

struct ClassThrArgs {
  unsigned long long* hist;
  float* thr;
  float* t_out;
  double drop;
  int C;
  float cap, omd;
};

__global__ __launch_bounds__(CT_BLOCK) void class_thresholds_kernel(ClassThrArgs a) {
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  for (int c = (int)(threadIdx.x >> 6); c < a.C; c += CT_BLOCK / 64) {      // uniform over the wave
    unsigned long long* row = a.hist + (long)c * CONF_BINS + 4 * lane;
    const unsigned long long h0 = row[0], h1 = row[1], h2 = row[2], h3 = row[3];
    const unsigned long long mine = (h0 + h1) + (h2 + h3);
    unsigned long long incl = mine;
    for (int s = 1; s < 64; s <<= 1) {
      const unsigned long long up = __shfl_up(incl, s, 64);
      if (lane >= s) incl += up;
    }
    const long long n = (long long)__shfl(incl, 63, 64);
    row[0] = 0ull; row[1] = 0ull; row[2] = 0ull; row[3] = 0ull;
    float t = 0.f;
    if (n > 0) {
      long long k = (long long)rint((double)n * a.drop);
      if (k > n - 1) k = n - 1;
      const unsigned long long over = __ballot(incl > (unsigned long long)k);      // never empty: lane 63 holds n > k
      const int first = __ffsll(over) - 1;
      const unsigned long long before = incl - mine;      // the exclusive prefix
      const int j = before + h0 > (unsigned long long)k ? 0 : before + h0 + h1 > (unsigned long long)k ? 1 :
                    before + h0 + h1 + h2 > (unsigned long long)k ? 2 : 3;
      const int b = __shfl(4 * lane + j, first, 64);
      t = fminf((float)b / (float)CONF_BINS, a.cap);
      if (lane == 0) {
        const float old = a.thr[c];
        const float diff = t - old;
        const float step = a.omd * diff;
        a.thr[c] = old + step;
      }
    }
    if (lane == 0 && a.t_out) a.t_out[c] = t;
  }
}

extern "C" int simt_class_thresholds(const simt_class_thresholds_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->hist && d->thr && d->C > 0 && d->C <= CONF_MAX_C);
  SIMT_CHECK(((uintptr_t)d->hist & 7) == 0 && ((uintptr_t)d->thr & 3) == 0 && ((uintptr_t)d->t_out & 3) == 0);
  SIMT_CHECK(d->drop >= 0.0 && d->drop < 1.0 && d->omd > 0.0f && d->omd <= 1.0f && d->cap == d->cap);      // (a NaN fails every comparison)
  ClassThrArgs a;
  a.hist = (unsigned long long*)d->hist; a.thr = d->thr; a.t_out = d->t_out;
  a.drop = d->drop; a.C = d->C; a.cap = d->cap; a.omd = d->omd;
  hipLaunchKernelGGL(class_thresholds_kernel, dim3(1), dim3(CT_BLOCK), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- test-time augmentation.  Mode 0: the arg-max of the summed logits -> pred and / or out + counts.  Mode 1 (one-resample family only):
// the averaged probabilities -> labels (strict rule where no thr is given, else per class), the confidence histogram, or both.
template <int FAM, int V>
static void launch_tta(const simt_tta_desc* d, const TtaTerms& terms, const ConfOut& o, simt_stream_t stream) {
  constexpr int BLOCK = FAM == 1 ? PL_BLOCK : PL2_BLOCK, MAX_GRID = FAM == 1 ? PL_MAX_GRID : PL2_MAX_GRID;
  if (d->mode == 0)
    launch_sweep<BLOCK, MAX_GRID>(TtaSource<FAM, V, 0>{terms}, TtaArgmaxSink{d->pred, o, d->C}, d->B, d->H, d->W, stream);
  if constexpr (FAM == 1) {
    if (d->mode == 1)
      launch_conf<BLOCK, MAX_GRID>(TtaSource<1, V, 1>{terms}, o, PerClassOrStrict{d->thr ? 0 : 1, d->threshold}, d->B, d->H, d->W, d->C, stream);
  }
}

extern "C" int simt_tta_label(const simt_tta_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->n >= 1 && d->n <= SIMT_TTA_MAX);
  SIMT_CHECK(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C <= 255);
  SIMT_CHECK(d->mode == 0 || d->mode == 1);
  const bool two = d->t[0].hi > 0;
  bool vec = true;
  for (int i = 0; i < d->n; ++i) {
    const simt_tta_term& t = d->t[i];
    SIMT_CHECK(t.l && t.h > 0 && t.w > 0 && d->C <= t.ld);
    SIMT_CHECK(two ? (t.hi > 0 && t.wi > 0) : (t.hi == 0 && t.wi == 0));          // one family per call
    SIMT_CHECK((long)d->B * t.h * t.w * t.ld < 2147483647L);
    vec = vec && vec4_ok(t.l, t.ld);
  }
  SIMT_CHECK(!(d->mode == 1 && two));                                           // mode 1 of the two-resample family is not built
  SIMT_CHECK(!(d->mode == 1 && d->pred));
  SIMT_CHECK(!d->out || (d->counts && ((uintptr_t)d->out & 3) == 0));
  SIMT_CHECK(d->mode == 0 ? (d->pred || d->out) && !d->hist && !d->thr : (d->out || d->hist));   // something to write; thr / hist are mode 1's
  SIMT_CHECK(!d->hist || d->C <= CONF_MAX_C);
  TtaTerms a;
  for (int i = 0; i < SIMT_TTA_MAX; ++i) {
    const simt_tta_term& t = d->t[i < d->n ? i : 0];
    if (two) {
      fill_up2(a.t[i].s, t.l, t.h, t.w, t.ld, t.hi, t.wi, d->H, d->W);
    } else {
      Up2Scale& s = a.t[i].s;
      s.l = t.l; s.h = t.h; s.w = t.w; s.ld = t.ld; s.hi = 0; s.wi = 0; s.isy = 0.f; s.isx = 0.f;
      s.osy = align_scale(t.h, d->H);
      s.osx = align_scale(t.w, d->W);
    }
    a.t[i].flip = t.flip ? 1 : 0;
  }
  a.n = d->n; a.C = d->C;
  a.inv_n = 1.0f / (float)d->n;
  ConfOut o;
  o.out = d->out; o.counts = (unsigned long long*)d->counts; o.hist = (unsigned long long*)d->hist;
  for (int c = 0; c < 255; ++c) o.thr[c] = (d->thr && c < d->C) ? d->thr[c] : 0.f;
  if (two) { if (vec) launch_tta<2, 4>(d, a, o, stream); else launch_tta<2, 1>(d, a, o, stream); }
  else     { if (vec) launch_tta<1, 4>(d, a, o, stream); else launch_tta<1, 1>(d, a, o, stream); }
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
