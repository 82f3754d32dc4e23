// Prototype contrastive loss on the student's layer-4 features (SePiCo, Xie et al., TPAMI'23; the second half of ProDA; contract in
// include/simt_hip.h): four streaming launches between the student's forward and its backward, over the prototypes of 7.26.
//   cell_labels_kernel          grid ceil(B*h*w / 32), 256 lanes: feat_dist_mask_kernel's walk (a wave owns 8 consecutive cells, the window read
//                               64 pixels at a time, one compare + ballot per class, lane c keeps count_c) over ALL classes c < C; the class that
//                               fills the window to min_ratio becomes the cell's byte label.  part[g]: the workgroup's cells of a seen class.
//   proto_contrast_prep_kernel  ONE workgroup of 1024 lanes: wave w normalises the prototype rows w, w + 16, ... (the norm lane-local in element
//                               order, then the xor butterfly) into phat [Cpad][D], zero rows for classes that are unseen, zero, not finite or
//                               padding; then the seen word, and N = the cells whose label is a seen class (integers: any order), into hdr.
//   proto_contrast_kernel<T, NT>  grid min(ceil(M / 32), 4096), 64 lanes: a wave owns tiles of 32 consecutive cells.  Lane l: cell r = l & 31, half
//                               hf = l >> 5.  Sweep 1: S^T [class][cell] = phat x f^T on mfma_f32_32x32x2f32, K = D: both operands are 8 consecutive
//                               channels of the lane's row at k0 + 8 hf, the next step's loads in flight behind the 8 (16) MFMAs of this one.  The
//                               accumulator puts the cell on the lane and 16 classes per tile in its registers (the other 16 in lane l ^ 32): the
//                               softmax is register-local plus one xor-32 exchange.  Sweep 2: the accumulator registers, now a_c, ARE the B operand of
//                               G^T [channel][cell] = phat^T x a^T, K = Cpad (k-steps whose two classes are both unseen are skipped); the A rows are
//                               permuted so that a lane ends with 16 consecutive channels of its cell: the fhat correction reads f a second time in
//                               16-byte loads and the row leaves in 16-byte stores.  A tile without a valid cell: zeros stored, nothing loaded.
//   proto_contrast_finalize_kernel  one wave: the partials in double in index order, three floats.
// No atomics, no scratch.  LDS: cell labels 4 words, prep 83 words, the rest none.  NT = 1: C <= 32, NT = 2: C <= 64; any D % 8 == 0 up to 4096.
// Traffic at M = 37 636, D = 2048, C = 19, bf16: f read twice and seed written once (3 x 154 MB); phat (256 KB, L2-resident) read twice per tile.
#include "common.h"

#define CL_WAVES 4
#define CL_CELLS_PER_WAVE 8
#define PC_MAX_WG 4096
#define PC_PREP_LANES 1024
#define PC_PREP_WAVES 16

typedef __attribute__((ext_vector_type(16))) float f32x16;

__global__ __launch_bounds__(256) void cell_labels_kernel(const simt_cell_labels_desc d, const int cells) {
  __shared__ int wsum[CL_WAVES];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int first = ((int)blockIdx.x * CL_WAVES + wv) * CL_CELLS_PER_WAVE;
  const int hw = d.h * d.w, C = d.C;
  const uint64_t seen_set = __ballot(lane < C && (d.n == nullptr || d.n[lane] > 0));
  int nseen = 0;
  for (int k = 0; k < CL_CELLS_PER_WAVE; ++k) {
    const int cell = first + k;
    if (cell >= cells) break;                            // (wave-uniform)
    const int b = cell / hw, ij = cell - b * hw, i = ij / d.w, j = ij - i * d.w;
    const int r0 = (int)(((long)i * d.H) / d.h), r1 = (int)(((long)(i + 1) * d.H) / d.h);
    const int c0 = (int)(((long)j * d.W) / d.w), c1 = (int)(((long)(j + 1) * d.W) / d.w);
    const int ww = c1 - c0, n = (r1 - r0) * ww;          // >= 1: h <= H and w <= W
    const int64_t* base = d.label + ((long)b * d.H + r0) * d.W + c0;
    int cnt = 0;                                         // lane c: the pixels of class c
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int t = t0 + lane;
      int64_t lab = -1;                                  // matches no class
      if (t < n) {
        const int rr = t / ww;
        lab = base[(long)rr * d.W + (t - rr * ww)];
      }
      for (int c = 0; c < C; ++c) {                      // (scalar loop: C is a kernel argument)
        const int m = __popcll(__ballot(lab == (int64_t)c));
        if (lane == c) cnt += m;
      }
    }
    const float bar = d.min_ratio * (float)n;
    const uint64_t hit = __ballot(lane < C && (float)cnt >= bar);
    const int cls = hit ? (int)__builtin_ctzll(hit) : 255;
    if (lane == 0) d.lab[cell] = (uint8_t)cls;
    nseen += (cls < C && ((seen_set >> cls) & 1ull) != 0ull) ? 1 : 0;
  }
  if (lane == 0) wsum[wv] = nseen;
  __syncthreads();
  if (threadIdx.x == 0) d.part[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

static __host__ __device__ __forceinline__ int pc_cpad(int C) { return C <= 32 ? 32 : 64; }

__global__ __launch_bounds__(PC_PREP_LANES) void proto_contrast_prep_kernel(const simt_proto_contrast_desc d) {
  __shared__ int flag[64];
  __shared__ int wcnt[PC_PREP_WAVES];
  __shared__ uint32_t word[3];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int C = d.C, D = d.D, chunks = D >> 3, Cpad = pc_cpad(C);
  for (int c = wv; c < Cpad; c += PC_PREP_WAVES) {       // (c is wave-uniform)
    float* po = d.phat + (long)c * D;
    bool good = false;
    float ne = 0.f;
    if (c < C && d.n[c] > 0) {
      const float* pe = d.eta + (long)c * D;
      float ss = 0.f;
      for (int k = lane; k < chunks; k += 64) {
        float v[8];
        load8(pe + 8 * k, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += v[e] * v[e];
      }
      ne = sqrtf(wave_sum(ss));
      good = ne > 0.f && ne < INFINITY;                  // (a NaN fails the first)
      if (good) {
        for (int k = lane; k < chunks; k += 64) {
          float v[8];
          load8(pe + 8 * k, v);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = v[e] / ne;
          store8(po + 8 * k, v);
        }
      }
    }
    if (!good) {
      const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int k = lane; k < chunks; k += 64) store8(po + 8 * k, z);
    }
    if (lane == 0) flag[c] = good ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0ull;
    for (int c = 0; c < C; ++c) s |= flag[c] ? (1ull << c) : 0ull;
    word[2] = (uint32_t)__popcll(s);
    if (__popcll(s) < 2) s = 0ull;                       // fewer than two seen classes: no cell is valid, the term is 0
    word[0] = (uint32_t)s;
    word[1] = (uint32_t)(s >> 32);
  }
  __syncthreads();
  const uint64_t seen = (uint64_t)word[0] | ((uint64_t)word[1] << 32);
  int cnt = 0;
  for (long m = threadIdx.x; m < d.M; m += PC_PREP_LANES) {
    const int y = (int)d.lab[m];
    cnt += (y < C && ((seen >> y) & 1ull) != 0ull) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) wcnt[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int N = 0;
    for (int w = 0; w < PC_PREP_WAVES; ++w) N += wcnt[w];
    d.hdr[0] = word[0];
    d.hdr[1] = word[1];
    d.hdr[2] = (uint32_t)N;
    d.hdr[3] = word[2];
  }
}

// the class of accumulator register q of tile t in lane half hf (the 32x32 C/D map: row = (q & 3) + 8 (q >> 2) + 4 hf)
#define PC_CLASS(t, q, hf) (32 * (t) + ((q) & 3) + 8 * ((q) >> 2) + 4 * (hf))

template <typename T> static __device__ __forceinline__ void pc_zero8(T* p);
template <> __device__ __forceinline__ void pc_zero8<bf16_t>(bf16_t* p) { *(uint4*)p = make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ void pc_zero8<float>(float* p) {
  *(uint4*)p = make_uint4(0u, 0u, 0u, 0u);
  *(uint4*)(p + 4) = make_uint4(0u, 0u, 0u, 0u);
}

template <typename T, int NT>
__global__ __launch_bounds__(64) void proto_contrast_kernel(const simt_proto_contrast_desc d) {
  const int lane = threadIdx.x;
  const int r = lane & 31, hf = lane >> 5;
  const int C = d.C, D = d.D, chunks = D >> 3;
  const uint64_t seen = (uint64_t)d.hdr[0] | ((uint64_t)d.hdr[1] << 32);
  const int N = (int)d.hdr[2];
  const float per_cell = N > 0 ? d.lam_g / (float)N : 0.f;
  const long tiles = (d.M + 31) >> 5;
  const float* phat = d.phat;
  // sweep 2's A row r is channel d0 + pcol: a lane's 16 accumulator registers then hold the channels d0 + 16 hf .. d0 + 16 hf + 15 in order
  const int pcol = 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3);
  float acc = 0.f;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (wave-uniform)
    const long m = tile * 32 + r;
    const bool in = m < d.M;
    const int y = in ? (int)d.lab[m] : 255;
    const bool valid = N > 0 && y < C && ((seen >> y) & 1ull) != 0ull;
    if (__ballot(valid) == 0ull) {                       // no valid cell: zeros, nothing loaded (lanes over the columns: whole rows per store)
      for (int rr = 0; rr < 32; ++rr) {
        const long m2 = tile * 32 + rr;
        if (m2 >= d.M) break;
        T* so = (T*)d.seed + m2 * D;
        for (int k = lane; k < chunks; k += 64) pc_zero8<T>(so + 8 * k);
      }
      if (in && hf == 0) d.d[m] = 0.f;
      continue;
    }
    const T* pf = (const T*)d.fs + (valid ? m : 0) * D;  // read only where `valid`
    // ---- sweep 1: logits, K = D, 16 channels per step (8 per lane half)
    f32x16 S[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) S[t][q] = 0.f;
    float ss = 0.f;
    Raw8<T> fa;
    Raw8<float> pa[NT];
    {
      const int kk = 8 * hf;
      if (valid && kk < D) raw8_load(pf + kk, fa);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (kk < D) raw8_load(phat + (long)(32 * t + r) * D + kk, pa[t]);
    }
    for (int k0 = 0; k0 < D; k0 += 16) {
      const int kk = k0 + 8 * hf, kn = kk + 16;
      float a[8], p[NT][8];
      if (valid && kk < D) {
        raw8_unpack(fa, a);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (kk < D) {
          raw8_unpack(pa[t], p[t]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) p[t][e] = 0.f;
        }
      }
      if (valid && kn < D) raw8_load(pf + kn, fa);       // the next step's loads, in flight behind this step's MFMAs
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (kn < D) raw8_load(phat + (long)(32 * t + r) * D + kn, pa[t]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ss += a[e] * a[e];
#pragma unroll
        for (int t = 0; t < NT; ++t) S[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[t][e], a[e], S[t], 0, 0, 0);
      }
    }
    const float nf = sqrtf(ss + __shfl_xor(ss, 32, 64));
    const bool ok = valid && nf > 0.f && nf < INFINITY;  // (a NaN fails the first) a degenerate row: loss 0, a +0 row, counted in N
    // ---- softmax over the seen classes: 16 NT of them in this lane's registers, the others in lane ^ 32
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = PC_CLASS(t, q, hf);
        const float cosv = S[t][q] / nf;
        S[t][q] = cosv;
        if (((seen >> c) & 1ull) != 0ull) mx = fmaxf(mx, cosv / d.temp);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f, sy = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = PC_CLASS(t, q, hf);
        if (((seen >> c) & 1ull) != 0ull) {
          const float s = S[t][q] / d.temp;
          se += expf(s - mx);
          if (c == y) sy += s;
        }
      }
    se += __shfl_xor(se, 32, 64);
    sy += __shfl_xor(sy, 32, 64);
    const float lse = mx + logf(se);
    const float loss = ok ? lse - sy : 0.f;
    float dot = 0.f;                                     // sum_c a_c cos_c
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = PC_CLASS(t, q, hf);
        float av = 0.f;
        if (ok && ((seen >> c) & 1ull) != 0ull) {
          av = expf(S[t][q] / d.temp - lse) - (c == y ? 1.f : 0.f);
          dot += av * S[t][q];
        }
        S[t][q] = av;                                    // from here on the registers hold a_c: sweep 2's B operand
      }
    dot += __shfl_xor(dot, 32, 64);
    const float coef = ok ? per_cell / (d.temp * nf) : 0.f;
    const float wf = ok ? dot / nf : 0.f;                // (sum_c a_c cos_c) * fhat = wf * f
    if (in && hf == 0) d.d[m] = loss;
    acc += wave_sum((in && hf == 0) ? loss : 0.f);
    // ---- sweep 2: the gradient block, 32 channels per step, K = Cpad
    T* so = (T*)d.seed + m * D;
    for (int d0 = 0; d0 < D; d0 += 32) {
      f32x16 G;
#pragma unroll
      for (int q = 0; q < 16; ++q) G[q] = 0.f;
      const int col = d0 + pcol;
      const bool cin = col < D;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int c0 = PC_CLASS(t, q, 0);              // the k-step's two classes: c0 (half 0) and c0 + 4 (half 1)
          if (((seen >> c0) & 0x11ull) == 0ull) continue;      // (wave-uniform) both unseen: their a_c are 0
          const float pv = cin ? phat[(long)(c0 + 4 * hf) * D + col] : 0.f;
          G = __builtin_amdgcn_mfma_f32_32x32x2f32(pv, S[t][q], G, 0, 0, 0);
        }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cb = d0 + 16 * hf + 8 * j;
        if (!in || cb >= D) continue;
        float v[8];
        if (ok) {
          float fv[8];
          load8(pf + cb, fv);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = coef * (G[8 * j + e] - wf * fv[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
        store8(so + cb, v);
      }
    }
  }
  if (lane == 0) d.part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(64) void proto_contrast_finalize_kernel(const simt_proto_contrast_desc d, const int nparts) {
  const int lane = threadIdx.x;
  const int N = (int)d.hdr[2];
  double S = 0.0;
  for (int p0 = 0; p0 < nparts; p0 += 64) {
    const double v = p0 + lane < nparts ? (double)d.part[p0 + lane] : 0.0;
    for (int j = 0; j < 64; ++j) S += __shfl(v, j, 64);      // index order; the tail adds +0.0
  }
  if (lane == 0) {
    const double mean = N > 0 ? S / (double)N : 0.0;
    d.out[0] = N > 0 ? (float)(d.lambda * mean) : 0.f;
    d.out[1] = (float)mean;
    d.out[2] = (float)N;
  }
}

extern "C" int simt_cell_labels_parts(int B, int h, int w) {
  if (B < 1 || h < 1 || w < 1 || (long)B * h * w >= (1L << 31)) return 0;
  const long cells = (long)B * h * w, per = CL_WAVES * CL_CELLS_PER_WAVE;
  return (int)((cells + per - 1) / per);
}

extern "C" int simt_proto_contrast_parts(long M) {
  if (M < 1 || M >= (1L << 31)) return 0;
  const long t = (M + 31) >> 5;
  return (int)(t < PC_MAX_WG ? t : PC_MAX_WG);
}

extern "C" long simt_proto_contrast_phat_floats(int C, int D) {
  if (C < 2 || C > SIMT_PROTO_MAX_CLASSES || D < 8 || D > SIMT_PROTO_MAX_DIM || (D & 7) != 0) return 0;
  return (long)pc_cpad(C) * D;
}

extern "C" int simt_cell_labels(const simt_cell_labels_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->label && d->lab && d->part);
  SIMT_CHECK(d->B >= 1 && d->H >= 1 && d->W >= 1 && d->h >= 1 && d->w >= 1);
  SIMT_CHECK(d->h <= d->H && d->w <= d->W);
  SIMT_CHECK(d->C >= 2 && d->C <= SIMT_PROTO_MAX_CLASSES);
  SIMT_CHECK(d->min_ratio > 0.5f && d->min_ratio <= 1.0f);      // (a NaN fails both)
  SIMT_CHECK((long)d->H * d->W < (1L << 31) && (long)d->B * d->h * d->w < (1L << 31));
  SIMT_CHECK(((uintptr_t)d->label & 7) == 0 && ((uintptr_t)d->part & 3) == 0 && ((uintptr_t)d->n & 3) == 0);
  const int cells = d->B * d->h * d->w;
  const int grid = simt_cell_labels_parts(d->B, d->h, d->w);
  hipLaunchKernelGGL(cell_labels_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *d, cells);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

static int pc_check(const simt_proto_contrast_desc* d) {
  SIMT_CHECK(d && d->fs && d->lab && d->eta && d->n && d->phat && d->hdr && d->seed && d->d && d->part && d->out);
  SIMT_CHECK(d->M >= 1 && d->M < (1L << 31));
  SIMT_CHECK(d->C >= 2 && d->C <= SIMT_PROTO_MAX_CLASSES);
  SIMT_CHECK(d->D >= 8 && d->D <= SIMT_PROTO_MAX_DIM && (d->D & 7) == 0);
  SIMT_CHECK(d->dtype == SIMT_F32 || d->dtype == SIMT_BF16);
  SIMT_CHECK(d->temp > 0.f && d->temp <= 3.4028234e38f);      // (a NaN fails the first)
  SIMT_CHECK(d->lam_g == d->lam_g && d->lambda == d->lambda);      // not NaN
  SIMT_CHECK(((uintptr_t)d->fs & 15) == 0 && ((uintptr_t)d->seed & 15) == 0 && ((uintptr_t)d->eta & 15) == 0 && ((uintptr_t)d->phat & 15) == 0);
  SIMT_CHECK(((uintptr_t)d->n & 3) == 0 && ((uintptr_t)d->hdr & 3) == 0 && ((uintptr_t)d->d & 3) == 0 && ((uintptr_t)d->part & 3) == 0 &&
             ((uintptr_t)d->out & 3) == 0);
  return SIMT_OK;
}

extern "C" int simt_proto_contrast_prep(const simt_proto_contrast_desc* d, simt_stream_t stream) {
  const int rc = pc_check(d);
  if (rc != SIMT_OK) return rc;
  hipLaunchKernelGGL(proto_contrast_prep_kernel, dim3(1), dim3(PC_PREP_LANES), 0, (hipStream_t)stream, *d);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_proto_contrast(const simt_proto_contrast_desc* d, simt_stream_t stream) {
  const int rc = pc_check(d);
  if (rc != SIMT_OK) return rc;
  const dim3 grid((unsigned)simt_proto_contrast_parts(d->M));
  const bool one = d->C <= 32;
  if (d->dtype == SIMT_BF16) {
    if (one) hipLaunchKernelGGL((proto_contrast_kernel<bf16_t, 1>), grid, dim3(64), 0, (hipStream_t)stream, *d);
    else hipLaunchKernelGGL((proto_contrast_kernel<bf16_t, 2>), grid, dim3(64), 0, (hipStream_t)stream, *d);
  } else {
    if (one) hipLaunchKernelGGL((proto_contrast_kernel<float, 1>), grid, dim3(64), 0, (hipStream_t)stream, *d);
    else hipLaunchKernelGGL((proto_contrast_kernel<float, 2>), grid, dim3(64), 0, (hipStream_t)stream, *d);
  }
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_proto_contrast_finalize(const simt_proto_contrast_desc* d, simt_stream_t stream) {
  const int rc = pc_check(d);
  if (rc != SIMT_OK) return rc;
  hipLaunchKernelGGL(proto_contrast_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *d, simt_proto_contrast_parts(d->M));
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
