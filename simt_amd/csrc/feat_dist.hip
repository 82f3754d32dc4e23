// DAFormer's thing-class ImageNet feature distance (Hoyer et al., CVPR'22; contract in include/simt_hip.h): three streaming
// launches between the student's forward and its backward.
//   feat_dist_mask_kernel      grid ceil(B*h*w / 32), 256 lanes: a wave owns 8 consecutive feature cells, one after the other.  The label window
//                              of a cell is read 64 pixels at a time (one int64 per lane; any window size); per candidate class of the thing set
//                              ONE wave-wide compare + ballot, the count kept by the lane whose id is the class -- 64 counters without an array.
//                              mask[cell] by lane 0; the workgroup's number of kept cells by one plain store (4 ints of LDS join the waves).
//                              Label-bound: 8 bytes per pixel, every pixel read once.
//   feat_dist_kernel<T, REG>   grid min(ceil(M / 4), 1024), 256 lanes: wave g of the launch owns rows g, g + waves, ...  Every wave re-sums the
//                              mask launch's partials (integers: any order gives N).  A row that is not kept: C zeros stored, nothing loaded.
//                              A kept row: both feature rows in 16-byte loads, all in flight together (REG: C <= 2048, 8 * 4 elements per lane
//                              stay in registers between the sum and the store; else the row is read a second time, from L2), the squared
//                              differences summed lane-locally in element order and across the wave by the xor butterfly (a fixed order:
//                              a launch repeats bit for bit), d = sqrtf(s), seed = ((lam_g / N) / d) * diff.  d[m] by lane 0; the workgroup's
//                              sum of d by one plain store.
//   feat_dist_finalize_kernel  one wave: N, then the partials in double in index order (64 loaded at a time, added lane by lane), three floats.
// No atomics, no scratch; LDS: 4 words per workgroup for the two per-workgroup partials.
// Byte floor: mask 8*B*H*W read; main pass M*C*esz written + 2*C*esz read per kept row.
#include "common.h"

#define FD_WAVES 4
#define FD_CELLS_PER_WAVE 8
#define FD_MAX_WG 1024
#define FD_REG_CHUNKS 4          // 16-byte (bf16) / 32-byte (fp32) chunks of 8 elements a lane keeps: 64 * 4 * 8 = 2048 channels

__global__ __launch_bounds__(256) void feat_dist_mask_kernel(const simt_feat_dist_mask_desc d, const int cells) {
  __shared__ int wsum[FD_WAVES];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int first = ((int)blockIdx.x * FD_WAVES + wv) * FD_CELLS_PER_WAVE;
  const int hw = d.h * d.w;
  int nkept = 0;
  for (int k = 0; k < FD_CELLS_PER_WAVE; ++k) {
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
      uint64_t set = d.classes;
      while (set) {                                      // (scalar loop: the set is a kernel argument)
        const int c = __builtin_ctzll(set);
        set &= set - 1;
        const int m = __popcll(__ballot(lab == (int64_t)c));
        if (lane == c) cnt += m;
      }
    }
    const float bar = d.min_ratio * (float)n;
    const bool ok = ((d.classes >> lane) & 1ull) != 0ull && (float)cnt >= bar;
    const bool kept = __ballot(ok) != 0ull;
    if (lane == 0) d.mask[cell] = kept ? 1 : 0;
    nkept += kept ? 1 : 0;
  }
  if (lane == 0) wsum[wv] = nkept;
  __syncthreads();
  if (threadIdx.x == 0) d.part[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

static __device__ __forceinline__ int fd_kept_cells(const simt_feat_dist_desc& d, const int lane) {
  int n = 0;
  for (int p = lane; p < d.n_kept_part; p += 64) n += d.kept_part[p];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  return n;
}

template <typename T> static __device__ __forceinline__ void fd_zero8(T* p);
template <> __device__ __forceinline__ void fd_zero8<bf16_t>(bf16_t* p) { *(uint4*)p = make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ void fd_zero8<float>(float* p) {
  *(uint4*)p = make_uint4(0u, 0u, 0u, 0u);
  *(uint4*)(p + 4) = make_uint4(0u, 0u, 0u, 0u);
}

template <typename T, bool REG>
__global__ __launch_bounds__(256) void feat_dist_kernel(const simt_feat_dist_desc d) {
  __shared__ float wsum[FD_WAVES];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int N = fd_kept_cells(d, lane);
  const float per_cell = N > 0 ? d.lam_g / (float)N : 0.f;
  const int C = d.C, chunks = C >> 3;
  const long waves = (long)gridDim.x * FD_WAVES;
  float acc = 0.f;
  for (long m = (long)blockIdx.x * FD_WAVES + wv; m < d.M; m += waves) {      // (m is wave-uniform)
    T* so = (T*)d.seed + m * C;
    if (d.mask[m] == 0) {                                // neither feature row is read
      for (int k = lane; k < chunks; k += 64) fd_zero8<T>(so + 8 * k);
      if (lane == 0) d.d[m] = 0.f;
      continue;
    }
    const T* ps = (const T*)d.fs + m * C;
    const T* pi = (const T*)d.fi + m * C;
    float s = 0.f;
    if (REG) {
      Raw8<T> ra[FD_REG_CHUNKS], rb[FD_REG_CHUNKS];
#pragma unroll
      for (int q = 0; q < FD_REG_CHUNKS; ++q) {
        const int k = lane + 64 * q;
        if (k < chunks) {
          raw8_load(ps + 8 * k, ra[q]);
          raw8_load(pi + 8 * k, rb[q]);
        }
      }
      float df[FD_REG_CHUNKS][8];
#pragma unroll
      for (int q = 0; q < FD_REG_CHUNKS; ++q) {
        const int k = lane + 64 * q;
        if (k < chunks) {
          float a[8], b[8];
          raw8_unpack(ra[q], a);
          raw8_unpack(rb[q], b);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            df[q][e] = a[e] - b[e];
            s += df[q][e] * df[q][e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) df[q][e] = 0.f;
        }
      }
      s = wave_sum(s);
      const float dist = sqrtf(s);
      const bool pos = dist > 0.f;
      const float coef = pos ? per_cell / dist : 0.f;
#pragma unroll
      for (int q = 0; q < FD_REG_CHUNKS; ++q) {
        const int k = lane + 64 * q;
        if (k < chunks) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = pos ? coef * df[q][e] : 0.f;
          store8(so + 8 * k, v);
        }
      }
      if (lane == 0) d.d[m] = dist;
      acc += dist;
    } else {
      for (int k = lane; k < chunks; k += 64) {
        float a[8], b[8];
        load8(ps + 8 * k, a);
        load8(pi + 8 * k, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = a[e] - b[e];
          s += t * t;
        }
      }
      s = wave_sum(s);
      const float dist = sqrtf(s);
      const bool pos = dist > 0.f;
      const float coef = pos ? per_cell / dist : 0.f;
      for (int k = lane; k < chunks; k += 64) {          // the row again (from L2)
        float a[8], b[8], v[8];
        load8(ps + 8 * k, a);
        load8(pi + 8 * k, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = pos ? coef * (a[e] - b[e]) : 0.f;
        store8(so + 8 * k, v);
      }
      if (lane == 0) d.d[m] = dist;
      acc += dist;
    }
  }
  if (lane == 0) wsum[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) d.part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(64) void feat_dist_finalize_kernel(const simt_feat_dist_desc d, const int nparts) {
  const int lane = threadIdx.x;
  const int N = fd_kept_cells(d, lane);
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

extern "C" int simt_feat_dist_mask_parts(int B, int h, int w) {
  if (B < 1 || h < 1 || w < 1 || (long)B * h * w >= (1L << 31)) return 0;
  const long cells = (long)B * h * w, per = FD_WAVES * FD_CELLS_PER_WAVE;
  return (int)((cells + per - 1) / per);
}

extern "C" int simt_feat_dist_parts(long M) {
  if (M < 1) return 0;
  const long g = (M + FD_WAVES - 1) / FD_WAVES;
  return (int)(g < FD_MAX_WG ? g : FD_MAX_WG);
}

extern "C" int simt_feat_dist_mask(const simt_feat_dist_mask_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->label && d->mask && d->part);
  SIMT_CHECK(d->B >= 1 && d->H >= 1 && d->W >= 1 && d->h >= 1 && d->w >= 1);
  SIMT_CHECK(d->h <= d->H && d->w <= d->W);
  SIMT_CHECK(d->min_ratio > 0.5f && d->min_ratio <= 1.0f);      // (a NaN fails both)
  SIMT_CHECK((long)d->H * d->W < (1L << 31) && (long)d->B * d->h * d->w < (1L << 31));
  SIMT_CHECK(((uintptr_t)d->label & 7) == 0 && ((uintptr_t)d->part & 3) == 0);
  const int cells = d->B * d->h * d->w;
  const int grid = simt_feat_dist_mask_parts(d->B, d->h, d->w);
  hipLaunchKernelGGL(feat_dist_mask_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *d, cells);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

static int fd_check(const simt_feat_dist_desc* d) {
  SIMT_CHECK(d && d->fs && d->fi && d->mask && d->kept_part && d->seed && d->d && d->part && d->out);
  SIMT_CHECK(d->M >= 1 && d->M < (1L << 31) && d->C >= 8 && (d->C & 7) == 0 && d->ld == d->C);
  SIMT_CHECK(d->dtype == SIMT_F32 || d->dtype == SIMT_BF16);
  SIMT_CHECK(d->n_kept_part >= 1);
  SIMT_CHECK(((uintptr_t)d->fs & 15) == 0 && ((uintptr_t)d->fi & 15) == 0 && ((uintptr_t)d->seed & 15) == 0);
  SIMT_CHECK(((uintptr_t)d->kept_part & 3) == 0 && ((uintptr_t)d->d & 3) == 0 && ((uintptr_t)d->part & 3) == 0 && ((uintptr_t)d->out & 3) == 0);
  SIMT_CHECK(d->lam_g == d->lam_g && d->lambda == d->lambda);      // not NaN
  return SIMT_OK;
}

extern "C" int simt_feat_dist(const simt_feat_dist_desc* d, simt_stream_t stream) {
  const int rc = fd_check(d);
  if (rc != SIMT_OK) return rc;
  const dim3 grid((unsigned)simt_feat_dist_parts(d->M));
  const bool reg = d->C <= 64 * FD_REG_CHUNKS * 8;
  if (d->dtype == SIMT_BF16) {
    if (reg) hipLaunchKernelGGL((feat_dist_kernel<bf16_t, true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
    else hipLaunchKernelGGL((feat_dist_kernel<bf16_t, false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  } else {
    if (reg) hipLaunchKernelGGL((feat_dist_kernel<float, true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
    else hipLaunchKernelGGL((feat_dist_kernel<float, false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  }
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_feat_dist_finalize(const simt_feat_dist_desc* d, simt_stream_t stream) {
  const int rc = fd_check(d);
  if (rc != SIMT_OK) return rc;
  hipLaunchKernelGGL(feat_dist_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *d, simt_feat_dist_parts(d->M));
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
