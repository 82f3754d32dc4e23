// Evaluation path of the reference (tools/evaluate_cityscapes.py:96-162, evaluate_simt): logits of the main head at two
// input scales are bilinearly upsampled (align_corners=True) to the label resolution, SUMMED, arg-maxed, and scored with
// a confusion histogram (fast_hist :81-83) -> per-class IoU / mIoU (:86-87).  The reference does the sum / argmax /
// bincount on the CPU in numpy per image; here one fused kernel gathers the 4 taps of both low-res maps (L2-resident),
// and the histogram is integer atomics (exact, order-independent).
#include "common.h"

struct EvalArgs {
  const float* la;     // [B][ha][wa][lda] logits, scale A (first C channels used)
  const float* lb;     // [B][hb][wb][ldb] logits, scale B, or NULL
  int* pred;           // [B][H][W] arg-max class
  int B, ha, wa, lda, hb, wb, ldb, H, W, C;
  float sya, sxa, syb, sxb;
};

__device__ __forceinline__ void bil_taps(int y, int x, int h, int w, float sy, float sx, int& o00, int& o01, int& o10, int& o11,
                                         float& wy0, float& wy1, float& wx0, float& wx1) {
  // ATen upsample_bilinear2d, align_corners=True: src = scale * dst, scale = (in-1)/(out-1)
  const float fy = sy * (float)y, fx = sx * (float)x;
  int iy0 = (int)fy, ix0 = (int)fx;
  if (iy0 > h - 1) iy0 = h - 1;
  if (ix0 > w - 1) ix0 = w - 1;
  const int iy1 = iy0 + (iy0 < h - 1 ? 1 : 0), ix1 = ix0 + (ix0 < w - 1 ? 1 : 0);
  wy1 = fy - (float)iy0; wy0 = 1.f - wy1;
  wx1 = fx - (float)ix0; wx0 = 1.f - wx1;
  o00 = iy0 * w + ix0; o01 = iy0 * w + ix1; o10 = iy1 * w + ix0; o11 = iy1 * w + ix1;
}

__global__ __launch_bounds__(256) void upsample_sum_argmax_kernel(EvalArgs a) {
  const long P = (long)a.B * a.H * a.W;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long)gridDim.x * blockDim.x) {
    const int x = (int)(p % a.W);
    const long t = p / a.W;
    const int y = (int)(t % a.H);
    const int b = (int)(t / a.H);
    int a00, a01, a10, a11, b00 = 0, b01 = 0, b10 = 0, b11 = 0;
    float ay0, ay1, ax0, ax1, by0 = 0, by1 = 0, bx0 = 0, bx1 = 0;
    bil_taps(y, x, a.ha, a.wa, a.sya, a.sxa, a00, a01, a10, a11, ay0, ay1, ax0, ax1);
    const float* pa = a.la + (long)b * a.ha * a.wa * a.lda;
    const float* pb = nullptr;
    if (a.lb) {
      bil_taps(y, x, a.hb, a.wb, a.syb, a.sxb, b00, b01, b10, b11, by0, by1, bx0, bx1);
      pb = a.lb + (long)b * a.hb * a.wb * a.ldb;
    }
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < a.C; ++c) {
      // same association as ATen: h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11); then numpy's a + b
      float v = ay0 * (ax0 * pa[(long)a00 * a.lda + c] + ax1 * pa[(long)a01 * a.lda + c]) +
                ay1 * (ax0 * pa[(long)a10 * a.lda + c] + ax1 * pa[(long)a11 * a.lda + c]);
      if (pb) {
        const float u = by0 * (bx0 * pb[(long)b00 * a.ldb + c] + bx1 * pb[(long)b01 * a.ldb + c]) +
                        by1 * (bx0 * pb[(long)b10 * a.ldb + c] + bx1 * pb[(long)b11 * a.ldb + c]);
        v = v + u;
      }
      if (v > best) { best = v; arg = c; }     // first index on ties, like np.argmax
    }
    a.pred[p] = arg;
  }
}

extern "C" int simt_upsample_sum_argmax(const float* la, int ha, int wa, int lda, const float* lb, int hb, int wb, int ldb,
                                        int B, int H, int W, int C, int32_t* pred, simt_stream_t stream) {
  SIMT_CHECK(la && pred && B > 0 && C > 0 && C <= lda && (!lb || C <= ldb));
  EvalArgs a;
  a.la = la; a.lb = lb; a.pred = pred; a.B = B; a.ha = ha; a.wa = wa; a.lda = lda; a.hb = hb; a.wb = wb; a.ldb = ldb;
  a.H = H; a.W = W; a.C = C;
  a.sya = H > 1 ? (float)(ha - 1) / (float)(H - 1) : 0.f;
  a.sxa = W > 1 ? (float)(wa - 1) / (float)(W - 1) : 0.f;
  a.syb = (lb && H > 1) ? (float)(hb - 1) / (float)(H - 1) : 0.f;
  a.sxb = (lb && W > 1) ? (float)(wb - 1) / (float)(W - 1) : 0.f;
  long P = (long)B * H * W;
  long grid = (P + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(upsample_sum_argmax_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- pseudo-label export (the commented-out save lines of evaluate_simt :150-156 / evaluate_warmup :214-219; the confidence rule of
// trainV2_simt.py:353-359 with the high threshold only).  Same gather as upsample_sum_argmax_kernel, written as uint8 (a quarter of the
// int32 bytes) together with the class counts of compute_ClassDistribution.py (bins 0..C-1, then the 255s).
struct PseudoArgs {
  const float* la;     // [B][ha][wa][lda] logits (mode 0) or probabilities (mode 1), first C channels used
  const float* lb;     // [B][hb][wb][ldb] logits, scale B, or NULL (mode 1: always NULL)
  unsigned char* out;  // [B][H][W] labels, 4-byte aligned
  unsigned long long* counts;   // [C+1], accumulated
  int B, ha, wa, lda, hb, wb, ldb, H, W, C;
  float sya, sxa, syb, sxb, threshold;
};

// MODE 0: arg-max of up(la) + up(lb) -- the arithmetic of upsample_sum_argmax_kernel, statement for statement, so the labels are its
// labels bit for bit.  MODE 1: max / arg-max of up(la); the caller keeps the arg-max where max > threshold (255 elsewhere).  `conf` is
// the maximum: the confidence of mode 1, which the class-balanced kernels below bin and threshold per class -- one function, so their
// (arg, conf) are the old kernel's bit for bit.
struct ArgConf {
  int arg;             // first-index arg-max
  float conf;          // the maximum
};

template <int MODE>
__device__ __forceinline__ ArgConf pseudo_pixel(const PseudoArgs& a, int b, int y, int x) {
  int a00, a01, a10, a11, b00 = 0, b01 = 0, b10 = 0, b11 = 0;
  float ay0, ay1, ax0, ax1, by0 = 0, by1 = 0, bx0 = 0, bx1 = 0;
  bil_taps(y, x, a.ha, a.wa, a.sya, a.sxa, a00, a01, a10, a11, ay0, ay1, ax0, ax1);
  const float* pa = a.la + (long)b * a.ha * a.wa * a.lda;
  const float* pb = nullptr;
  if (MODE == 0 && a.lb) {
    bil_taps(y, x, a.hb, a.wb, a.syb, a.sxb, b00, b01, b10, b11, by0, by1, bx0, bx1);
    pb = a.lb + (long)b * a.hb * a.wb * a.ldb;
  }
  float best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < a.C; ++c) {
    float v = ay0 * (ax0 * pa[(long)a00 * a.lda + c] + ax1 * pa[(long)a01 * a.lda + c]) +
              ay1 * (ax0 * pa[(long)a10 * a.lda + c] + ax1 * pa[(long)a11 * a.lda + c]);
    if (MODE == 0 && pb) {
      const float u = by0 * (bx0 * pb[(long)b00 * a.ldb + c] + bx1 * pb[(long)b01 * a.ldb + c]) +
                      by1 * (bx0 * pb[(long)b10 * a.ldb + c] + bx1 * pb[(long)b11 * a.ldb + c]);
      v = v + u;
    }
    if (v > best) { best = v; arg = c; }     // first index on ties
  }
  return {arg, best};
}

// One pixel per lane, so that neighbouring lanes gather neighbouring taps exactly as upsample_sum_argmax_kernel does (a version in which
// each thread labelled 4 consecutive pixels itself touched ~4x the cache lines per load instruction and ran 2.3-3.3x slower than that
// kernel).  Each quad of lanes = 4 consecutive pixels of the flattened [B][H][W] map (consecutive x; the quad runs on into the next row
// when W % 4 != 0): two lane shuffles pack the 4 labels into the quad leader, which writes one 32-bit store (byte stores for the last
// P % 4 pixels).  Counts: LDS histogram per block (the leader adds runs of equal labels once), one global atomic per non-zero bin --
// exact and order independent, like hist2d_u8_kernel.  The flush is what this kernel adds to the gather: with 256-thread blocks and up to
// 2048 of them (41 k 64-bit atomics on 20 words) it cost 7-13 us at 1 x 1024 x 2048; 1024-thread blocks, at most 512 of them (the
// same 32 waves per CU), cut it to ~3 us (launch-shape sweep on MI355X, 138.6 us against 143.5 us of upsample_sum_argmax_kernel).
constexpr int PL_BLOCK = 1024, PL_MAX_GRID = 512;

// The output side of the pseudo-label kernels.  Every lane of the block calls pl_store once per grid-stride step (the loop bound is
// uniform over the block: every lane of a wave reaches the shuffles together) with the label of pixel p (anything for p >= P).
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
template <int BLOCK>
__device__ __forceinline__ void pl_hist_flush(const unsigned int* sh, int nbins, unsigned long long* counts) {
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += BLOCK)
    if (sh[i]) atomicAdd(&counts[i], (unsigned long long)sh[i]);
}

// ---- class-balanced pseudo labels (CBST / the label generator of BDL): per class, the threshold is the confidence at a fixed rank among
// that class's own predictions, so the export needs the per-class distribution of the confidence over the whole data list.  The kernels
// below take (arg, conf) from the functions of the confidence mode and either count them into hist[arg][bin] (bin = floor(conf * 256)
// clamped to [0, 255]: the scaling by a power of two is exact, so the bin is a pure function of the float), label with a per-class
// threshold (kept iff conf >= thr[arg]; the output side is pl_store / pl_hist_flush), or both.
//
// The histogram is the hot path: on real frames a large share of the pixels of a frame fall into ONE word (road at conf ~ 1), and one
// global word takes ~88 atomics / us.  So (1) the counters are private to the workgroup in LDS (C * 256 words, C <= 64), (2) equal keys
// are aggregated within the wave before the LDS atomic: up to CONF_AGG_ROUNDS times the first lane still to do broadcasts its key, the
// lanes holding that key are found with one ballot and the first lane adds their number -- a wave whose 64 lanes hit the hot bin
// issues one add; the lanes left after the rounds (keys spread over many bins: little contention) add 1 each -- and (3) only the
// non-zero bins are flushed, one 64-bit global atomic each.  Integer counts: exact and order independent.
constexpr int CONF_BINS = SIMT_CONF_BINS, CONF_MAX_C = 64, CONF_AGG_ROUNDS = 4;

struct ConfOut {
  unsigned char* out;           // [B][H][W] labels, 4-byte aligned, or NULL
  unsigned long long* counts;   // [C+1], accumulated (with out)
  unsigned long long* hist;     // [C][CONF_BINS], accumulated, or NULL
  float thr[255];               // per-class thresholds (with out)
};

__device__ __forceinline__ int conf_bin(float conf) {
  const float f = fminf(fmaxf(floorf(conf * (float)CONF_BINS), 0.f), (float)(CONF_BINS - 1));
  return (int)f;
}

// every lane of the wave calls this together (the callers' loop bounds are uniform over the block)
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

// LDS of the class-balanced kernels: the label counts and thresholds of pl_store's side, and the confidence histogram
template <bool STATS>
struct ConfShared {
  unsigned int counts[256];
  float thr[256];
  unsigned int hist[STATS ? CONF_MAX_C * CONF_BINS : 1];
};

template <int BLOCK, bool STATS, bool LABELS>
__device__ __forceinline__ void conf_init(ConfShared<STATS>& sh, const ConfOut& o, int C) {
  if (LABELS)
    for (int i = threadIdx.x; i < C; i += BLOCK) sh.thr[i] = o.thr[i];
  if (STATS)
    for (int i = threadIdx.x; i < C * CONF_BINS; i += BLOCK) sh.hist[i] = 0u;
  pl_hist_init<BLOCK>(sh.counts, C + 1);
}
// one grid-stride step: every lane of the block calls conf_emit with the key / label conf_pixel gave for pixel p (anything for p >= P)
template <bool STATS, bool LABELS>
__device__ __forceinline__ void conf_pixel(const ConfShared<STATS>& sh, ArgConf r, unsigned int& key, unsigned int& lab) {
  if (STATS) key = (unsigned int)(r.arg * CONF_BINS + conf_bin(r.conf));
  if (LABELS) lab = r.conf >= sh.thr[r.arg] ? (unsigned int)r.arg : 255u;
}
template <bool STATS, bool LABELS>
__device__ __forceinline__ void conf_emit(ConfShared<STATS>& sh, const ConfOut& o, unsigned int key, unsigned int lab, long p, long P, int C) {
  if (STATS) conf_hist_add(p < P, key, sh.hist);
  if (LABELS) pl_store(lab, p, P, C, o.out, sh.counts);
}
template <int BLOCK, bool STATS, bool LABELS>
__device__ __forceinline__ void conf_flush(const ConfShared<STATS>& sh, const ConfOut& o, int C) {
  if (LABELS) {
    pl_hist_flush<BLOCK>(sh.counts, C + 1, o.counts);
    if (STATS) pl_hist_flush<BLOCK>(sh.hist, C * CONF_BINS, o.hist);
  } else {
    pl_hist_flush<BLOCK>(sh.hist, C * CONF_BINS, o.hist);
  }
}
// the checks of the output side, and its arguments
static int conf_out_fill(ConfOut& o, int C, const float* thr, uint8_t* out, int64_t* counts, int64_t* hist) {
  SIMT_CHECK(out || hist);
  SIMT_CHECK(!out || (thr && counts && ((uintptr_t)out & 3) == 0));
  SIMT_CHECK(!hist || C <= CONF_MAX_C);
  o.out = out; o.counts = (unsigned long long*)counts; o.hist = (unsigned long long*)hist;
  for (int c = 0; c < 255; ++c) o.thr[c] = (out && c < C) ? thr[c] : 0.f;
  return SIMT_OK;
}

template <int MODE>
__global__ __launch_bounds__(PL_BLOCK) void pseudo_label_u8_kernel(PseudoArgs a) {
  __shared__ unsigned int sh[256];
  pl_hist_init<PL_BLOCK>(sh, a.C + 1);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * PL_BLOCK; base < P; base += (long)gridDim.x * PL_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      const ArgConf r = pseudo_pixel<MODE>(a, (int)(t / a.H), (int)(t % a.H), x);
      lab = (unsigned int)(MODE == 1 && !(r.conf > a.threshold) ? 255 : r.arg);   // strictly greater (:359)
    }
    pl_store(lab, p, P, a.C, a.out, sh);
  }
  pl_hist_flush<PL_BLOCK>(sh, a.C + 1, a.counts);
}

extern "C" int simt_pseudo_label_u8(const float* la, int ha, int wa, int lda, const float* lb, int hb, int wb, int ldb, int B, int H,
                                    int W, int C, int mode, float threshold, uint8_t* out, int64_t* counts, simt_stream_t stream) {
  SIMT_CHECK(la && out && counts && B > 0 && H > 0 && W > 0 && ha > 0 && wa > 0 && C > 0 && C <= 255 && C <= lda);
  SIMT_CHECK((mode == 0 && (!lb || (C <= ldb && hb > 0 && wb > 0))) || (mode == 1 && !lb));
  SIMT_CHECK(((uintptr_t)out & 3) == 0);
  PseudoArgs a;
  a.la = la; a.lb = lb; a.out = out; a.counts = (unsigned long long*)counts;
  a.B = B; a.ha = ha; a.wa = wa; a.lda = lda; a.hb = hb; a.wb = wb; a.ldb = ldb; a.H = H; a.W = W; a.C = C;
  a.sya = H > 1 ? (float)(ha - 1) / (float)(H - 1) : 0.f;
  a.sxa = W > 1 ? (float)(wa - 1) / (float)(W - 1) : 0.f;
  a.syb = (lb && H > 1) ? (float)(hb - 1) / (float)(H - 1) : 0.f;
  a.sxb = (lb && W > 1) ? (float)(wb - 1) / (float)(W - 1) : 0.f;
  a.threshold = threshold;
  const long P = (long)B * H * W;
  long grid = (P + PL_BLOCK - 1) / PL_BLOCK;
  if (grid > PL_MAX_GRID) grid = PL_MAX_GRID;
  if (mode == 0)
    hipLaunchKernelGGL(pseudo_label_u8_kernel<0>, dim3((unsigned)grid), dim3(PL_BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(pseudo_label_u8_kernel<1>, dim3((unsigned)grid), dim3(PL_BLOCK), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

struct PseudoConfArgs {
  PseudoArgs g;        // la, the geometry and C of mode 1 (lb, out, counts, threshold unused)
  ConfOut o;
};

template <bool STATS, bool LABELS>
__global__ __launch_bounds__(PL_BLOCK) void pseudo_conf_u8_kernel(PseudoConfArgs a) {
  __shared__ ConfShared<STATS> sh;
  conf_init<PL_BLOCK, STATS, LABELS>(sh, a.o, a.g.C);
  const long P = (long)a.g.B * a.g.H * a.g.W;
  for (long base = (long)blockIdx.x * PL_BLOCK; base < P; base += (long)gridDim.x * PL_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int key = 0u, lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.g.W);
      const long t = p / a.g.W;
      conf_pixel<STATS, LABELS>(sh, pseudo_pixel<1>(a.g, (int)(t / a.g.H), (int)(t % a.g.H), x), key, lab);
    }
    conf_emit<STATS, LABELS>(sh, a.o, key, lab, p, P, a.g.C);
  }
  conf_flush<PL_BLOCK, STATS, LABELS>(sh, a.o, a.g.C);
}

extern "C" int simt_pseudo_conf_u8(const float* la, int ha, int wa, int lda, int B, int H, int W, int C, const float* thr, uint8_t* out,
                                   int64_t* counts, int64_t* hist, simt_stream_t stream) {
  SIMT_CHECK(la && B > 0 && H > 0 && W > 0 && ha > 0 && wa > 0 && C > 0 && C <= 255 && C <= lda);
  PseudoConfArgs a;
  if (int rc = conf_out_fill(a.o, C, thr, out, counts, hist)) return rc;
  PseudoArgs& g = a.g;
  g.la = la; g.lb = nullptr; g.out = nullptr; g.counts = nullptr;
  g.B = B; g.ha = ha; g.wa = wa; g.lda = lda; g.hb = 0; g.wb = 0; g.ldb = 0; g.H = H; g.W = W; g.C = C;
  g.sya = H > 1 ? (float)(ha - 1) / (float)(H - 1) : 0.f;
  g.sxa = W > 1 ? (float)(wa - 1) / (float)(W - 1) : 0.f;
  g.syb = 0.f; g.sxb = 0.f; g.threshold = 0.f;
  const long P = (long)B * H * W;
  long grid = (P + PL_BLOCK - 1) / PL_BLOCK;
  if (grid > PL_MAX_GRID) grid = PL_MAX_GRID;
  const dim3 gr((unsigned)grid), blk(PL_BLOCK);
  if (hist && out)
    hipLaunchKernelGGL((pseudo_conf_u8_kernel<true, true>), gr, blk, 0, (hipStream_t)stream, a);
  else if (hist)
    hipLaunchKernelGGL((pseudo_conf_u8_kernel<true, false>), gr, blk, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((pseudo_conf_u8_kernel<false, true>), gr, blk, 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// hist[n*gt + pred] += 1 for 0 <= gt < n   (fast_hist: labels outside [0, n) -- the 255 "ignore" id -- are skipped)
__global__ __launch_bounds__(256) void confusion_hist_kernel(const int64_t* gt, const int32_t* pred, long P, int n,
                                                             unsigned long long* hist) {
  __shared__ unsigned int sh[32 * 32];
  const int nn = n * n;
  for (int i = threadIdx.x; i < nn; i += 256) sh[i] = 0u;
  __syncthreads();
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long)gridDim.x * blockDim.x) {
    const long long g = gt[p];
    const int q = pred[p];
    if (g >= 0 && g < n && q >= 0 && q < n) atomicAdd(&sh[(int)g * n + q], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nn; i += 256)
    if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}

extern "C" int simt_confusion_hist(const int64_t* gt, const int32_t* pred, long P, int n, int64_t* hist,
                                   simt_stream_t stream) {
  SIMT_CHECK(gt && pred && hist && n > 0 && n <= 32);
  long grid = (P + 255) / 256;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(confusion_hist_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, gt, pred, P, n,
                     (unsigned long long*)hist);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- F.interpolate(mode='bilinear') of NHWC low-res maps to an NCHW fp32 tensor and its adjoint.
// model/deeplabv3.py:137 upsamples the logits INSIDE the model with the default align_corners=False
// (src = (dst + 0.5) * in/out - 0.5, clamped at 0); align_corners=True is the interp_target flavour of trainV2_simt.py:301.
struct UpArgs {
  const float* src;   // [B][h][w][lds]
  float* dst;         // [B][C][H][W]
  int B, h, w, lds, C, H, W, align;
  float sy, sx;
};
__device__ __forceinline__ void up_taps(int d, int in, float scale, int align, int& i0, int& i1, float& l0, float& l1) {
  float f = align ? scale * (float)d : fmaxf(((float)d + 0.5f) * scale - 0.5f, 0.f);
  i0 = (int)f;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = f - (float)i0;
  l0 = 1.f - l1;
}
__global__ __launch_bounds__(256) void upsample_nchw_kernel(UpArgs a) {
  const long total = (long)a.B * a.C * a.H * a.W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % a.W);
    long t = i / a.W;
    const int y = (int)(t % a.H); t /= a.H;
    const int c = (int)(t % a.C);
    const int b = (int)(t / a.C);
    int y0, y1, x0, x1; float wy0, wy1, wx0, wx1;
    up_taps(y, a.h, a.sy, a.align, y0, y1, wy0, wy1);
    up_taps(x, a.w, a.sx, a.align, x0, x1, wx0, wx1);
    const float* p = a.src + (long)b * a.h * a.w * a.lds + c;
    a.dst[i] = wy0 * (wx0 * p[((long)y0 * a.w + x0) * a.lds] + wx1 * p[((long)y0 * a.w + x1) * a.lds]) +
               wy1 * (wx0 * p[((long)y1 * a.w + x0) * a.lds] + wx1 * p[((long)y1 * a.w + x1) * a.lds]);
  }
}
// adjoint: dsrc[b][yl][xl][c] = sum over (y, x) of w(y,yl) * w(x,xl) * ddst[b][c][y][x]   (gather form, deterministic).
// Separable: pass 1 folds x (tmp[b][c][y][xl] = sum_x w(x,xl) ddst[b][c][y][x]), pass 2 folds y -- the one-pass version
// evaluated ~2 700 weight pairs per low-res element (0.67 ms at 4 x 25 x 512 x 1024).
__device__ __forceinline__ void up_range(int l, int in, int out, float scale, int& lo, int& hi) {
  if (scale > 0.f) {
    const float r = 1.f / scale;
    lo = (int)floorf(((float)l - 1.f) * r) - 2;
    hi = (int)ceilf(((float)l + 2.f) * r) + 2;
  } else { lo = 0; hi = out - 1; }
  lo = max(lo, 0); hi = min(hi, out - 1);
}
__global__ __launch_bounds__(256) void upsample_bwd_x_kernel(const float* ddst, float* tmp, UpArgs a) {
  const long total = (long)a.B * a.C * a.H * a.w;          // tmp[b][c][y][xl]
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xl = (int)(i % a.w);
    const long row = i / a.w;                              // (b*C + c)*H + y
    int xlo, xhi;
    up_range(xl, a.w, a.W, a.sx, xlo, xhi);
    const float* g = ddst + row * a.W;
    float s = 0.f;
    for (int x = xlo; x <= xhi; ++x) {
      int x0, x1; float wx0, wx1;
      up_taps(x, a.w, a.sx, a.align, x0, x1, wx0, wx1);
      const float wx = (x0 == xl ? wx0 : 0.f) + (x1 == xl ? wx1 : 0.f);
      s += wx * g[x];
    }
    tmp[i] = s;
  }
}
template <typename T>
__global__ __launch_bounds__(256) void upsample_bwd_y_kernel(const float* tmp, T* dsrc, UpArgs a) {
  const long total = (long)a.B * a.h * a.w * a.C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % a.C);
    long t = i / a.C;
    const int xl = (int)(t % a.w); t /= a.w;
    const int yl = (int)(t % a.h);
    const int b = (int)(t / a.h);
    int ylo, yhi;
    up_range(yl, a.h, a.H, a.sy, ylo, yhi);
    const float* g = tmp + ((long)(b * a.C + c) * a.H) * a.w + xl;
    float s = 0.f;
    for (int y = ylo; y <= yhi; ++y) {
      int y0, y1; float wy0, wy1;
      up_taps(y, a.h, a.sy, a.align, y0, y1, wy0, wy1);
      const float wy = (y0 == yl ? wy0 : 0.f) + (y1 == yl ? wy1 : 0.f);
      s += wy * g[(long)y * a.w];
    }
    Elem<T>::st(dsrc + ((long)(b * a.h + yl) * a.w + xl) * a.lds + c, s);
  }
}
static void fill_up(UpArgs& a, int B, int h, int w, int lds, int C, int H, int W, int align) {
  a.B = B; a.h = h; a.w = w; a.lds = lds; a.C = C; a.H = H; a.W = W; a.align = align;
  if (align) {
    a.sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    a.sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
  } else {
    a.sy = (float)h / (float)H;
    a.sx = (float)w / (float)W;
  }
}
extern "C" int simt_upsample_nchw(const float* src, int B, int h, int w, int lds, int C, int H, int W, int align_corners, float* dst,
                                  simt_stream_t stream) {
  SIMT_CHECK(src && dst && C <= lds);
  UpArgs a; a.src = src; a.dst = dst;
  fill_up(a, B, h, w, lds, C, H, W, align_corners);
  long total = (long)B * C * H * W, grid = (total + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(upsample_nchw_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
// tmp: caller-owned scratch of B*C*H*w floats for the separable adjoint (allocated with the plan's other buffers: no allocation on
// the launch path, nothing shared between plans / streams / devices)
extern "C" int simt_upsample_nchw_bwd(const float* ddst, int B, int h, int w, int lds, int C, int H, int W, int align_corners,
                                      void* dsrc, int dtype, float* tmp, simt_stream_t stream) {
  SIMT_CHECK(ddst && dsrc && tmp && C <= lds);
  UpArgs a; a.src = nullptr; a.dst = nullptr;
  fill_up(a, B, h, w, lds, C, H, W, align_corners);
  float* g_upbwd_tmp = tmp;
  long t1 = (long)B * C * H * w, g1 = (t1 + 255) / 256;
  if (g1 > 256 * 32) g1 = 256 * 32;
  hipLaunchKernelGGL(upsample_bwd_x_kernel, dim3((unsigned)g1), dim3(256), 0, (hipStream_t)stream, ddst, g_upbwd_tmp, a);
  SIMT_LAUNCH_CHECK();
  long total = (long)B * h * w * C, grid = (total + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  if (dtype == SIMT_BF16)
    hipLaunchKernelGGL(upsample_bwd_y_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g_upbwd_tmp, (bf16_t*)dsrc, a);
  else
    hipLaunchKernelGGL(upsample_bwd_y_kernel<float>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g_upbwd_tmp, (float*)dsrc, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- evaluation of a model that upsamples INSIDE (DeepLabv3, model/deeplabv3.py:137): the reference resamples its full-resolution
// output a second time (evaluate_cityscapes.py:108-133).  Per label pixel and scale: the align_corners=True taps of the label grid over a
// VIRTUAL [Hi][Wi] map (bil_taps' arithmetic), each of whose 4 samples is the align_corners=False value of the NHWC logits (up_taps, align
// = 0) -- 16 gathers per channel, nothing stored in between (the map would be 52 + 82 MB per frame at Q = 25).  Both scales summed, then
// the first-index arg-max, like upsample_sum_argmax_kernel.  V = 4: float4 gathers of 4 consecutive channels (ld % 4 == 0, 16-byte
// aligned maps; channels C..round_up(C, 4)-1 are read, lie inside ld, and are ignored).
struct Up2Scale {
  const float* l;      // [B][h][w][ld] logits, first C channels used
  int h, w, ld, hi, wi;
  float osy, osx;      // outer: (hi-1)/(H-1), (wi-1)/(W-1)
  float isy, isx;      // inner: h/hi, w/wi
};
struct Up2Args {
  Up2Scale s[2];
  int nscales;
  int* pred;
  int B, H, W, C;
};

struct Up2Taps {
  int off[4][4];       // [virtual sample yi*2+xi][logit tap yj*2+xj] element offsets (B*h*w*ld < 2^31, checked on the host)
  float ly[2][2], lx[2][2];   // inner weights [virtual row / column][tap]
  float oy[2], ox[2];         // outer weights
};

__device__ __forceinline__ void up2_taps(const Up2Scale& s, int b, int y, int x, Up2Taps& t) {
  int vy[2], vx[2], iy[2][2], ix[2][2];
  up_taps(y, s.hi, s.osy, 1, vy[0], vy[1], t.oy[0], t.oy[1]);
  up_taps(x, s.wi, s.osx, 1, vx[0], vx[1], t.ox[0], t.ox[1]);
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

// the first-index arg-max of up(up(s[0])) (+ up(up(s[1])) with two scales) at one pixel: the evaluator's label, and mode 0 of the
// pseudo-label export (one function, so the two agree bit for bit)
template <int V>
__device__ __forceinline__ int up2_argmax(const Up2Scale (&s)[2], int nscales, int C, int b, int y, int x) {
  Up2Taps ta, tb;
  up2_taps(s[0], b, y, x, ta);
  const bool two = nscales > 1;
  if (two) up2_taps(s[1], b, y, x, tb);
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
  return arg;
}

template <int V>
__global__ __launch_bounds__(256) void upsample2_sum_argmax_kernel(Up2Args a) {
  const long P = (long)a.B * a.H * a.W;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long)gridDim.x * blockDim.x) {
    const int x = (int)(p % a.W);
    const long t = p / a.W;
    const int y = (int)(t % a.H);
    const int b = (int)(t / a.H);
    a.pred[p] = up2_argmax<V>(a.s, a.nscales, a.C, b, y, x);
  }
}

static void fill_up2(Up2Scale& s, const float* l, int h, int w, int ld, int hi, int wi, int H, int W) {
  s.l = l; s.h = h; s.w = w; s.ld = ld; s.hi = hi; s.wi = wi;
  s.osy = H > 1 ? (float)(hi - 1) / (float)(H - 1) : 0.f;
  s.osx = W > 1 ? (float)(wi - 1) / (float)(W - 1) : 0.f;
  s.isy = (float)h / (float)hi;
  s.isx = (float)w / (float)wi;
}

extern "C" int simt_upsample2_sum_argmax(const float* la, int ha, int wa, int lda, int hia, int wia, const float* lb, int hb, int wb,
                                         int ldb, int hib, int wib, int B, int H, int W, int C, int32_t* pred, simt_stream_t stream) {
  SIMT_CHECK(la && pred && B > 0 && H > 0 && W > 0 && C > 0 && C <= lda && ha > 0 && wa > 0 && hia > 0 && wia > 0);
  SIMT_CHECK(!lb || (C <= ldb && hb > 0 && wb > 0 && hib > 0 && wib > 0));
  SIMT_CHECK((long)B * ha * wa * lda < 2147483647L && (!lb || (long)B * hb * wb * ldb < 2147483647L));
  Up2Args a;
  a.nscales = lb ? 2 : 1;
  fill_up2(a.s[0], la, ha, wa, lda, hia, wia, H, W);
  fill_up2(a.s[1], lb ? lb : la, lb ? hb : ha, lb ? wb : wa, lb ? ldb : lda, lb ? hib : hia, lb ? wib : wia, H, W);
  a.pred = pred; a.B = B; a.H = H; a.W = W; a.C = C;
  const bool vec = lda % 4 == 0 && ((uintptr_t)la & 15) == 0 && (!lb || (ldb % 4 == 0 && ((uintptr_t)lb & 15) == 0));
  long P = (long)B * H * W;
  long grid = (P + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  if (vec)
    hipLaunchKernelGGL(upsample2_sum_argmax_kernel<4>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(upsample2_sum_argmax_kernel<1>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- pseudo-label export of a model that upsamples inside (DeepLabv3): the gather of upsample2_sum_argmax_kernel with the output side of
// pseudo_label_u8_kernel.  MODE 0: up2_argmax, as uint8.  MODE 1 (one scale): the confidence rule on the model's OUTPUT -- softmax at
// each of the 4 virtual samples (the input-size map), the probabilities resampled to the label pixel, arg-max where max > threshold.  The
// softmax is not separable from the inner resample, so the 4 samples' logits are re-gathered in three channel sweeps (max, sum of
// exps, probabilities + arg-max) instead of holding 4 x C values per lane; expf / fmaxf / 1/s as in softmax_rows_kernel.
struct Pseudo2Args {
  Up2Scale s[2];
  int nscales;
  unsigned char* out;           // [B][H][W], 4-byte aligned
  unsigned long long* counts;   // [C+1], accumulated
  int B, H, W, C;
  float threshold;
};

// PAIR: -> the first-index arg-max of the resampled probabilities and their maximum, the confidence, for the class-balanced kernels below
// (one function, so the two agree bit for bit; `threshold` unused)
template <int V, bool PAIR = false>
__device__ __forceinline__ auto up2_confident(const Up2Scale& s, int C, float threshold, int b, int y, int x) {
  Up2Taps t;
  up2_taps(s, b, y, x, t);
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
  if constexpr (PAIR)
    return ArgConf{arg, best};
  else
    return best > threshold ? arg : 255;             // strictly greater (trainV2_simt.py:359)
}

// 512-thread blocks: the two-scale float4 gather holds ~220 VGPRs (2 waves per SIMD, as upsample2_sum_argmax_kernel runs), which a
// 1024-thread block (128 VGPRs at most) would spill; at most 1024 of them keeps the count flush at ~20 k atomics per frame.
constexpr int PL2_BLOCK = 512, PL2_MAX_GRID = 1024;
template <int MODE, int V>
__global__ __launch_bounds__(PL2_BLOCK) void pseudo_label2_u8_kernel(Pseudo2Args a) {
  __shared__ unsigned int sh[256];
  pl_hist_init<PL2_BLOCK>(sh, a.C + 1);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * PL2_BLOCK; base < P; base += (long)gridDim.x * PL2_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      const int y = (int)(t % a.H), b = (int)(t / a.H);
      lab = (unsigned int)(MODE == 0 ? up2_argmax<V>(a.s, a.nscales, a.C, b, y, x) : up2_confident<V>(a.s[0], a.C, a.threshold, b, y, x));
    }
    pl_store(lab, p, P, a.C, a.out, sh);
  }
  pl_hist_flush<PL2_BLOCK>(sh, a.C + 1, a.counts);
}

extern "C" int simt_pseudo_label2_u8(const float* la, int ha, int wa, int lda, int hia, int wia, const float* lb, int hb, int wb, int ldb,
                                     int hib, int wib, int B, int H, int W, int C, int mode, float threshold, uint8_t* out, int64_t* counts,
                                     simt_stream_t stream) {
  SIMT_CHECK(la && out && counts && B > 0 && H > 0 && W > 0 && C > 0 && C <= 255 && C <= lda && ha > 0 && wa > 0 && hia > 0 && wia > 0);
  SIMT_CHECK((mode == 0 && (!lb || (C <= ldb && hb > 0 && wb > 0 && hib > 0 && wib > 0))) || (mode == 1 && !lb));
  SIMT_CHECK((long)B * ha * wa * lda < 2147483647L && (!lb || (long)B * hb * wb * ldb < 2147483647L));
  SIMT_CHECK(((uintptr_t)out & 3) == 0);
  Pseudo2Args a;
  a.nscales = lb ? 2 : 1;
  fill_up2(a.s[0], la, ha, wa, lda, hia, wia, H, W);
  fill_up2(a.s[1], lb ? lb : la, lb ? hb : ha, lb ? wb : wa, lb ? ldb : lda, lb ? hib : hia, lb ? wib : wia, H, W);
  a.out = out; a.counts = (unsigned long long*)counts;
  a.B = B; a.H = H; a.W = W; a.C = C; a.threshold = threshold;
  const bool vec = lda % 4 == 0 && ((uintptr_t)la & 15) == 0 && (!lb || (ldb % 4 == 0 && ((uintptr_t)lb & 15) == 0));
  const long P = (long)B * H * W;
  long grid = (P + PL2_BLOCK - 1) / PL2_BLOCK;
  if (grid > PL2_MAX_GRID) grid = PL2_MAX_GRID;
  const dim3 g((unsigned)grid), blk(PL2_BLOCK);
  if (mode == 0 && vec)
    hipLaunchKernelGGL((pseudo_label2_u8_kernel<0, 4>), g, blk, 0, (hipStream_t)stream, a);
  else if (mode == 0)
    hipLaunchKernelGGL((pseudo_label2_u8_kernel<0, 1>), g, blk, 0, (hipStream_t)stream, a);
  else if (vec)
    hipLaunchKernelGGL((pseudo_label2_u8_kernel<1, 4>), g, blk, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((pseudo_label2_u8_kernel<1, 1>), g, blk, 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- online labels: the warm-up trainers' teacher labels every batch on the device.  The label rule of the export kernels'
// confidence mode, through the SAME device functions (pseudo_pixel<1> / up2_confident: (arg, conf) are theirs bit for bit), written as the
// int64 label the head kernels read -- no uint8 map, no widening copy.  FAM 0: pseudo_label_u8_kernel<1>.  FAM 1: pseudo_label2_u8_kernel<1>
// with a virtual map of the label's own size (hia = H, wia = W): its outer taps then have weights exactly 1 and 0, but a one-sample
// shortcut is NOT bit-equal (0 * NaN of a neighbouring sample is NaN there, and H == 1 gives scale 0), so the four-sample function is called
// as it is.  One pixel per lane, as above: a wave's 64 labels are one contiguous 512-byte store.  Counts: the quad shuffle of pl_store packs
// 4 labels into the quad leader, which adds runs of equal labels to the LDS histogram once (pl_count); pl_hist_flush as above.
struct Online2Args {
  Up2Scale s;
  int B, H, W, C;
  float threshold;
};

__device__ __forceinline__ void ol_store(unsigned int lab, long p, long P, int C, long long* label, unsigned int* sh) {
  unsigned int word = lab | (__shfl_down(lab, 1, 4) << 8);
  word |= __shfl_down(word, 2, 4) << 16;
  if (p < P) {
    label[p] = (long long)lab;
    if ((threadIdx.x & 3) == 0) pl_count(word, P - p < 4 ? (int)(P - p) : 4, C, sh);
  }
}

__global__ __launch_bounds__(PL_BLOCK) void online_label_kernel(PseudoArgs a, long long* label) {
  __shared__ unsigned int sh[256];
  pl_hist_init<PL_BLOCK>(sh, a.C + 1);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * PL_BLOCK; base < P; base += (long)gridDim.x * PL_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      const ArgConf r = pseudo_pixel<1>(a, (int)(t / a.H), (int)(t % a.H), x);
      lab = (unsigned int)(!(r.conf > a.threshold) ? 255 : r.arg);   // strictly greater (:359); a NaN on either side: 255
    }
    ol_store(lab, p, P, a.C, label, sh);
  }
  pl_hist_flush<PL_BLOCK>(sh, a.C + 1, a.counts);
}

template <int V>
__global__ __launch_bounds__(PL2_BLOCK) void online_label2_kernel(Online2Args a, long long* label, unsigned long long* counts) {
  __shared__ unsigned int sh[256];
  pl_hist_init<PL2_BLOCK>(sh, a.C + 1);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * PL2_BLOCK; base < P; base += (long)gridDim.x * PL2_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      lab = (unsigned int)up2_confident<V>(a.s, a.C, a.threshold, (int)(t / a.H), (int)(t % a.H), x);
    }
    ol_store(lab, p, P, a.C, label, sh);
  }
  pl_hist_flush<PL2_BLOCK>(sh, a.C + 1, counts);
}

extern "C" int simt_online_label(const simt_online_label_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->fix && d->label && d->counts);
  SIMT_CHECK(d->B > 0 && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C <= 255 && d->C <= d->ld);
  SIMT_CHECK(d->family == 0 || d->family == 1);
  SIMT_CHECK(((uintptr_t)d->label & 7) == 0);
  const int B = d->B, h = d->h, w = d->w, ld = d->ld, H = d->H, W = d->W;
  const long P = (long)B * H * W;
  if (d->family == 0) {
    PseudoArgs a;
    a.la = d->fix; a.lb = nullptr; a.out = nullptr; a.counts = (unsigned long long*)d->counts;
    a.B = B; a.ha = h; a.wa = w; a.lda = ld; a.hb = 0; a.wb = 0; a.ldb = 0; a.H = H; a.W = W; a.C = d->C;
    a.sya = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    a.sxa = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    a.syb = 0.f; a.sxb = 0.f;
    a.threshold = d->threshold;
    long grid = (P + PL_BLOCK - 1) / PL_BLOCK;
    if (grid > PL_MAX_GRID) grid = PL_MAX_GRID;
    hipLaunchKernelGGL(online_label_kernel, dim3((unsigned)grid), dim3(PL_BLOCK), 0, (hipStream_t)stream, a, (long long*)d->label);
  } else {
    SIMT_CHECK((long)B * h * w * ld < 2147483647L);          // the taps' element offsets are 32-bit (Up2Taps)
    Online2Args a;
    fill_up2(a.s, d->fix, h, w, ld, H, W, H, W);
    a.B = B; a.H = H; a.W = W; a.C = d->C; a.threshold = d->threshold;
    long grid = (P + PL2_BLOCK - 1) / PL2_BLOCK;
    if (grid > PL2_MAX_GRID) grid = PL2_MAX_GRID;
    const dim3 g((unsigned)grid), blk(PL2_BLOCK);
    if (ld % 4 == 0 && ((uintptr_t)d->fix & 15) == 0)
      hipLaunchKernelGGL(online_label2_kernel<4>, g, blk, 0, (hipStream_t)stream, a, (long long*)d->label, (unsigned long long*)d->counts);
    else
      hipLaunchKernelGGL(online_label2_kernel<1>, g, blk, 0, (hipStream_t)stream, a, (long long*)d->label, (unsigned long long*)d->counts);
  }
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// the class-balanced kernels over the gather of mode 1 above (up2_confident<V, true>): same block size and grid cap, for the same reasons.
// The float4 kernels hold 128-139 VGPRs, so the label and combined ones run 3 waves per SIMD where pseudo_label2_u8_kernel<1, 4> (121)
// runs 4; a form of the label kernel that fit 124 had its 16-byte loads of the last sweep split into elements and ran 370 us against
// 319 us for this one and 317 us for that kernel: the gather is bound by its load instructions, not by occupancy.
struct PseudoConf2Args {
  Up2Scale s;
  int B, H, W, C;
  ConfOut o;
};

template <bool STATS, bool LABELS, int V>
__global__ __launch_bounds__(PL2_BLOCK) void pseudo_conf2_u8_kernel(PseudoConf2Args a) {
  __shared__ ConfShared<STATS> sh;
  conf_init<PL2_BLOCK, STATS, LABELS>(sh, a.o, a.C);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * PL2_BLOCK; base < P; base += (long)gridDim.x * PL2_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int key = 0u, lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      conf_pixel<STATS, LABELS>(sh, up2_confident<V, true>(a.s, a.C, 0.f, (int)(t / a.H), (int)(t % a.H), x), key, lab);
    }
    conf_emit<STATS, LABELS>(sh, a.o, key, lab, p, P, a.C);
  }
  conf_flush<PL2_BLOCK, STATS, LABELS>(sh, a.o, a.C);
}

template <int V>
static void launch_conf2(const PseudoConf2Args& a, dim3 g, hipStream_t stream) {
  const dim3 blk(PL2_BLOCK);
  if (a.o.hist && a.o.out)
    hipLaunchKernelGGL((pseudo_conf2_u8_kernel<true, true, V>), g, blk, 0, stream, a);
  else if (a.o.hist)
    hipLaunchKernelGGL((pseudo_conf2_u8_kernel<true, false, V>), g, blk, 0, stream, a);
  else
    hipLaunchKernelGGL((pseudo_conf2_u8_kernel<false, true, V>), g, blk, 0, stream, a);
}

extern "C" int simt_pseudo_conf2_u8(const float* la, int ha, int wa, int lda, int hia, int wia, int B, int H, int W, int C,
                                    const float* thr, uint8_t* out, int64_t* counts, int64_t* hist, simt_stream_t stream) {
  SIMT_CHECK(la && B > 0 && H > 0 && W > 0 && C > 0 && C <= 255 && C <= lda && ha > 0 && wa > 0 && hia > 0 && wia > 0);
  SIMT_CHECK((long)B * ha * wa * lda < 2147483647L);
  PseudoConf2Args a;
  if (int rc = conf_out_fill(a.o, C, thr, out, counts, hist)) return rc;
  fill_up2(a.s, la, ha, wa, lda, hia, wia, H, W);
  a.B = B; a.H = H; a.W = W; a.C = C;
  const long P = (long)B * H * W;
  long grid = (P + PL2_BLOCK - 1) / PL2_BLOCK;
  if (grid > PL2_MAX_GRID) grid = PL2_MAX_GRID;
  if (lda % 4 == 0 && ((uintptr_t)la & 15) == 0)
    launch_conf2<4>(a, dim3((unsigned)grid), (hipStream_t)stream);
  else
    launch_conf2<1>(a, dim3((unsigned)grid), (hipStream_t)stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- class-balanced online labels: the combined kernels above (STATS and LABELS) with the output side of the online-label
// kernels -- int64 labels through ol_store -- and the thresholds read from DEVICE memory into ConfShared::thr at block start, so that the
// launch behind this one (class_thresholds_kernel) can move them without the host.  Every device function is the export kernels' own:
// (arg, conf), the bin, the rule (kept iff conf >= thr[arg]), the in-wave key aggregation and the flushes are theirs bit for bit.  Families, block
// sizes and grid caps: those of simt_online_label.
struct OnlineCbOut {
  long long* label;             // [B][H][W]
  unsigned long long* counts;   // [C+1], accumulated
  unsigned long long* hist;     // [C][CONF_BINS], accumulated
  const float* thr;             // [C], device memory
};

template <int BLOCK>
__device__ __forceinline__ void ol_cb_init(ConfShared<true>& sh, const OnlineCbOut& o, int C) {
  for (int i = threadIdx.x; i < C; i += BLOCK) sh.thr[i] = o.thr[i];
  for (int i = threadIdx.x; i < C * CONF_BINS; i += BLOCK) sh.hist[i] = 0u;
  pl_hist_init<BLOCK>(sh.counts, C + 1);
}
template <int BLOCK>
__device__ __forceinline__ void ol_cb_flush(const ConfShared<true>& sh, const OnlineCbOut& o, int C) {
  pl_hist_flush<BLOCK>(sh.counts, C + 1, o.counts);
  pl_hist_flush<BLOCK>(sh.hist, C * CONF_BINS, o.hist);
}

__global__ __launch_bounds__(PL_BLOCK) void online_label_cb_kernel(PseudoArgs a, OnlineCbOut o) {
  __shared__ ConfShared<true> sh;
  ol_cb_init<PL_BLOCK>(sh, o, a.C);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * PL_BLOCK; base < P; base += (long)gridDim.x * PL_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int key = 0u, lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      conf_pixel<true, true>(sh, pseudo_pixel<1>(a, (int)(t / a.H), (int)(t % a.H), x), key, lab);
    }
    conf_hist_add(p < P, key, sh.hist);
    ol_store(lab, p, P, a.C, o.label, sh.counts);
  }
  ol_cb_flush<PL_BLOCK>(sh, o, a.C);
}

template <int V>
__global__ __launch_bounds__(PL2_BLOCK) void online_label2_cb_kernel(Online2Args a, OnlineCbOut o) {
  __shared__ ConfShared<true> sh;
  ol_cb_init<PL2_BLOCK>(sh, o, a.C);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * PL2_BLOCK; base < P; base += (long)gridDim.x * PL2_BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int key = 0u, lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      conf_pixel<true, true>(sh, up2_confident<V, true>(a.s, a.C, 0.f, (int)(t / a.H), (int)(t % a.H), x), key, lab);
    }
    conf_hist_add(p < P, key, sh.hist);
    ol_store(lab, p, P, a.C, o.label, sh.counts);
  }
  ol_cb_flush<PL2_BLOCK>(sh, o, a.C);
}

extern "C" int simt_online_label_cb(const simt_online_label_cb_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->fix && d->label && d->counts && d->hist && d->thr);
  SIMT_CHECK(d->B > 0 && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C <= CONF_MAX_C && d->C <= d->ld);
  SIMT_CHECK(d->family == 0 || d->family == 1);
  SIMT_CHECK(((uintptr_t)d->label & 7) == 0 && ((uintptr_t)d->hist & 7) == 0 && ((uintptr_t)d->thr & 3) == 0);
  const int B = d->B, h = d->h, w = d->w, ld = d->ld, H = d->H, W = d->W;
  const long P = (long)B * H * W;
  OnlineCbOut o;
  o.label = (long long*)d->label; o.counts = (unsigned long long*)d->counts; o.hist = (unsigned long long*)d->hist; o.thr = d->thr;
  if (d->family == 0) {
    PseudoArgs a;
    a.la = d->fix; a.lb = nullptr; a.out = nullptr; a.counts = nullptr;
    a.B = B; a.ha = h; a.wa = w; a.lda = ld; a.hb = 0; a.wb = 0; a.ldb = 0; a.H = H; a.W = W; a.C = d->C;
    a.sya = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    a.sxa = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    a.syb = 0.f; a.sxb = 0.f; a.threshold = 0.f;
    long grid = (P + PL_BLOCK - 1) / PL_BLOCK;
    if (grid > PL_MAX_GRID) grid = PL_MAX_GRID;
    hipLaunchKernelGGL(online_label_cb_kernel, dim3((unsigned)grid), dim3(PL_BLOCK), 0, (hipStream_t)stream, a, o);
  } else {
    SIMT_CHECK((long)B * h * w * ld < 2147483647L);          // the taps' element offsets are 32-bit (Up2Taps)
    Online2Args a;
    fill_up2(a.s, d->fix, h, w, ld, H, W, H, W);
    a.B = B; a.H = H; a.W = W; a.C = d->C; a.threshold = 0.f;
    long grid = (P + PL2_BLOCK - 1) / PL2_BLOCK;
    if (grid > PL2_MAX_GRID) grid = PL2_MAX_GRID;
    const dim3 g((unsigned)grid), blk(PL2_BLOCK);
    if (ld % 4 == 0 && ((uintptr_t)d->fix & 15) == 0)
      hipLaunchKernelGGL(online_label2_cb_kernel<4>, g, blk, 0, (hipStream_t)stream, a, o);
    else
      hipLaunchKernelGGL(online_label2_cb_kernel<1>, g, blk, 0, (hipStream_t)stream, a, o);
  }
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

// ---- test-time augmentation: the label of up to SIMT_TTA_MAX maps, each of which may belong to the horizontally mirrored frame (the
// reference's offline tools import ttach, compute_ClassDistribution.py:6, compute_ConfusionMatrix.py:6, and never use it).  A term is one
// forward's low-res map; its value at a label pixel is the old kernels' value -- bil_taps + ATen's association for the one-resample
// family (FAM 1), up2_taps / up2_value for a model that upsamples inside (FAM 2) -- read at mirrored COLUMN INDICES when the term is
// flipped: the weights are untouched, so a flipped term is bit for bit the plain term on the column-reversed map ("un-mirror the
// model's output, then resample").  Terms are added in term order (mode 0: logits, arg-max of the sum; mode 1: probabilities, the sum
// times 1/n, then the rules of pseudo_label_u8_kernel<1> / pseudo_conf_u8_kernel).
// C is a run-time value up to 255 and the taps of 8 terms do not fit in registers, so the channels go in chunks of TTA_CH = 32 sums per
// lane (C = 19 / 22 / 25: one chunk), terms outermost inside a chunk: a term's taps are formed once per chunk.  The output side is
// pl_store / conf_emit as they are.
constexpr int TTA_CH = 32;
struct TtaTerm {
  Up2Scale s;          // FAM 1: l, h, w, ld and osy / osx = (h-1)/(H-1), (w-1)/(W-1); FAM 2: as fill_up2 leaves it
  int flip;
};
struct TtaArgs {
  TtaTerm t[SIMT_TTA_MAX];
  int n, B, H, W, C;
  int strict;          // mode 1 labels: 1 = keep where conf > threshold (no thr given), 0 = where conf >= thr[arg]
  float inv_n, threshold;
  int* pred;           // mode 0: [B][H][W] or NULL
  ConfOut o;
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
        // same association as ATen (upsample_sum_argmax_kernel): h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11)
        const float v = wy0 * (wx0 * q00.v[k] + wx1 * q01.v[k]) + wy1 * (wx0 * q10.v[k] + wx1 * q11.v[k]);
        if (FIRST) s[j + k] = v; else s[j + k] = s[j + k] + v;
      }
    }
  }
}

// up2_taps with the mirror applied to the virtual [hi][wi] map: the outer (align_corners=True) columns vx become wi-1-vx before the inner
// (align_corners=False) taps are formed
__device__ __forceinline__ void tta_up2_taps(const Up2Scale& s, int flip, int b, int y, int x, Up2Taps& t) {
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

template <int V, bool FIRST>
__device__ __forceinline__ void tta_term2(const TtaTerm& tm, int b, int y, int x, int c_lo, int C, float (&s)[TTA_CH]) {
  Up2Taps t;
  tta_up2_taps(tm.s, tm.flip, b, y, x, t);
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
__device__ __forceinline__ ArgConf tta_pixel(const TtaArgs& a, int b, int y, int x) {
  float best = -INFINITY;
  int arg = 0;
  for (int c_lo = 0; c_lo < a.C; c_lo += TTA_CH) {
    float s[TTA_CH];
    if (FAM == 1) tta_term1<V, true>(a.t[0], b, y, x, c_lo, a.C, s); else tta_term2<V, true>(a.t[0], b, y, x, c_lo, a.C, s);
    for (int t = 1; t < a.n; ++t) {
      if (FAM == 1) tta_term1<V, false>(a.t[t], b, y, x, c_lo, a.C, s); else tta_term2<V, false>(a.t[t], b, y, x, c_lo, a.C, s);
    }
#pragma unroll
    for (int j = 0; j < TTA_CH; ++j) {
      if (c_lo + j < a.C) {
        const float v = MODE == 1 ? s[j] * a.inv_n : s[j];
        if (v > best) { best = v; arg = c_lo + j; }     // first index on ties
      }
    }
  }
  return {arg, best};
}

// KIND 0: mode 0 (pred and / or out + counts).  Mode 1: 1 labels, 2 confidence histogram, 3 both.  Block sizes as the kernels of the same
// family: FAM 1 PL_BLOCK (the chunk's 32 sums + one term's 4 float4 taps stay below the 128 VGPRs of a 1024-thread block), FAM 2 PL2_BLOCK
// (Up2Taps + 16 float4 gathers in flight on top of the sums).
template <int FAM, int V, int KIND>
__global__ __launch_bounds__(FAM == 1 ? PL_BLOCK : PL2_BLOCK) void tta_label_kernel(TtaArgs a) {
  constexpr int BLOCK = FAM == 1 ? PL_BLOCK : PL2_BLOCK;
  constexpr bool STATS = KIND >= 2, LABELS = KIND == 1 || KIND == 3;
  __shared__ ConfShared<STATS> sh;
  conf_init<BLOCK, STATS, LABELS>(sh, a.o, a.C);
  const long P = (long)a.B * a.H * a.W;
  for (long base = (long)blockIdx.x * BLOCK; base < P; base += (long)gridDim.x * BLOCK) {
    const long p = base + threadIdx.x;
    unsigned int key = 0u, lab = 0u;
    if (p < P) {
      const int x = (int)(p % a.W);
      const long t = p / a.W;
      const ArgConf r = tta_pixel<FAM, V, KIND ? 1 : 0>(a, (int)(t / a.H), (int)(t % a.H), x);
      if (KIND == 0) {
        lab = (unsigned int)r.arg;
        if (a.pred) a.pred[p] = r.arg;
      } else {
        conf_pixel<STATS, LABELS>(sh, r, key, lab);                      // the bin, and the per-class rule: conf >= thr[arg]
        if (LABELS && a.strict) lab = (unsigned int)(!(r.conf > a.threshold) ? 255 : r.arg);     // the rule of pseudo_label_u8_kernel<1>
      }
    }
    if (KIND == 0) {
      if (a.o.out) pl_store(lab, p, P, a.C, a.o.out, sh.counts);
    } else {
      conf_emit<STATS, LABELS>(sh, a.o, key, lab, p, P, a.C);
    }
  }
  if (KIND == 0) {
    if (a.o.out) pl_hist_flush<BLOCK>(sh.counts, a.C + 1, a.o.counts);
  } else {
    conf_flush<BLOCK, STATS, LABELS>(sh, a.o, a.C);
  }
}

template <int FAM, int V>
static void launch_tta(const TtaArgs& a, int kind, hipStream_t stream) {
  constexpr int BLOCK = FAM == 1 ? PL_BLOCK : PL2_BLOCK, MAX_GRID = FAM == 1 ? PL_MAX_GRID : PL2_MAX_GRID;
  const long P = (long)a.B * a.H * a.W;
  long grid = (P + BLOCK - 1) / BLOCK;
  if (grid > MAX_GRID) grid = MAX_GRID;
  const dim3 g((unsigned)grid), blk(BLOCK);
  if (kind == 0) hipLaunchKernelGGL((tta_label_kernel<FAM, V, 0>), g, blk, 0, stream, a);
  if constexpr (FAM == 1) {
    if (kind == 1) hipLaunchKernelGGL((tta_label_kernel<1, V, 1>), g, blk, 0, stream, a);
    if (kind == 2) hipLaunchKernelGGL((tta_label_kernel<1, V, 2>), g, blk, 0, stream, a);
    if (kind == 3) hipLaunchKernelGGL((tta_label_kernel<1, V, 3>), g, blk, 0, stream, a);
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
    vec = vec && t.ld % 4 == 0 && ((uintptr_t)t.l & 15) == 0;
  }
  SIMT_CHECK(!(d->mode == 1 && two));                                           // mode 1 of the two-resample family is not built
  SIMT_CHECK(!(d->mode == 1 && d->pred));
  SIMT_CHECK(!d->out || (d->counts && ((uintptr_t)d->out & 3) == 0));
  SIMT_CHECK(d->mode == 0 ? (d->pred || d->out) && !d->hist && !d->thr : (d->out || d->hist));   // something to write; thr / hist are mode 1's
  SIMT_CHECK(!d->hist || d->C <= CONF_MAX_C);
  TtaArgs a;
  for (int i = 0; i < SIMT_TTA_MAX; ++i) {
    const simt_tta_term& t = d->t[i < d->n ? i : 0];
    if (two) {
      fill_up2(a.t[i].s, t.l, t.h, t.w, t.ld, t.hi, t.wi, d->H, d->W);
    } else {
      Up2Scale& s = a.t[i].s;
      s.l = t.l; s.h = t.h; s.w = t.w; s.ld = t.ld; s.hi = 0; s.wi = 0; s.isy = 0.f; s.isx = 0.f;
      s.osy = d->H > 1 ? (float)(t.h - 1) / (float)(d->H - 1) : 0.f;
      s.osx = d->W > 1 ? (float)(t.w - 1) / (float)(d->W - 1) : 0.f;
    }
    a.t[i].flip = t.flip ? 1 : 0;
  }
  a.n = d->n; a.B = d->B; a.H = d->H; a.W = d->W; a.C = d->C;
  a.strict = d->thr ? 0 : 1;
  a.inv_n = 1.0f / (float)d->n;
  a.threshold = d->threshold;
  a.pred = d->pred;
  a.o.out = d->out; a.o.counts = (unsigned long long*)d->counts; a.o.hist = (unsigned long long*)d->hist;
  for (int c = 0; c < 255; ++c) a.o.thr[c] = (d->thr && c < d->C) ? d->thr[c] : 0.f;
  const int kind = d->mode == 0 ? 0 : (d->out ? 1 : 0) + (d->hist ? 2 : 0);
  const hipStream_t st = (hipStream_t)stream;
  if (two) { if (vec) launch_tta<2, 4>(a, kind, st); else launch_tta<2, 1>(a, kind, st); }
  else     { if (vec) launch_tta<1, 4>(a, kind, st); else launch_tta<1, 1>(a, kind, st); }
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- offline NTM utilities (tools/compute_ClassDistribution.py:49-51,66-86; tools/compute_ConfusionMatrix.py:54-56,68-98) ----------
// hist[na_idx * nb + b] += 1 over uint8 label images: a = row class (optional 256-entry LUT = label_mapping; NULL a -> row 0, i.e. the
// 1-D class histogram of compute_CD), b = column class.  Entries with a (after the LUT) >= na or b >= nb are skipped: 255 = ignore.
// Integer atomics -> exact and order independent; LDS histogram per block (na * nb <= 2048), one global atomic per non-zero bin.
__global__ __launch_bounds__(256) void hist2d_u8_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, long P,
                                                        int na, int nb, const unsigned char* __restrict__ lut,
                                                        unsigned long long* __restrict__ hist) {
  __shared__ unsigned int sh[2048];
  __shared__ unsigned char sl[256];
  const int nn = na * nb;
  for (int i = threadIdx.x; i < nn; i += 256) sh[i] = 0u;
  sl[threadIdx.x] = lut ? lut[threadIdx.x] : (unsigned char)threadIdx.x;
  __syncthreads();
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long)gridDim.x * blockDim.x) {
    const int r = a ? (int)sl[a[p]] : 0;
    const int c = (int)b[p];
    if (r < na && c < nb) atomicAdd(&sh[r * nb + c], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nn; i += 256)
    if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}

extern "C" int simt_hist2d_u8(const unsigned char* a, const unsigned char* b, long P, int na, int nb, const unsigned char* lut,
                              int64_t* hist, simt_stream_t stream) {
  SIMT_CHECK(b && hist && P >= 0 && na >= 1 && nb >= 1 && na * nb <= 2048 && (a || na == 1));
  if (P == 0) return SIMT_OK;
  long grid = (P + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(hist2d_u8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, b, P, na, nb, lut,
                     (unsigned long long*)hist);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
