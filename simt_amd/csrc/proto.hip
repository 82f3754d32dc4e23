// ProDA's prototype weights on the teacher's output (Zhang et al., CVPR'21; contract in include/simt_hip.h): three streaming launches
// behind the teacher's forward, in front of the label launch.
//   proto_rectify_kernel<T, R, REG>  grid simt_proto_parts(M), 256 lanes: wave g of the launch owns the row groups g, g + waves, ... of R
//                              consecutive cells (R = 2).  REG (D <= 2048): the R feature rows stay in registers as loaded
//                              (16 / 32 bytes per lane and chunk); else they are read again per class, from L2.  Per SEEN class (a scalar
//                              loop over the ballot of n > 0) the prototype row is read once for the R cells: the squared differences summed
//                              lane-locally in element order and across the wave by the xor butterfly; lane c keeps d_c -- C <= 64 distances
//                              without an array.  The rest is one value per lane: min, weights, the renormalising sum (butterfly), arg-max by
//                              ballot.  lab[m] by lane 0; the workgroup's number of moved cells by one plain store (4 ints of LDS).
//   proto_acc_kernel<T, V>     grid (ceil(M / 256), ceil(D / (256 V))), 256 lanes: a workgroup owns 256 consecutive cells and a slab of
//                              256 V channels; thread t owns V columns of an LDS [C][256 V] array (V = 4 / 2 / 1 for C <= 16 / 32 / 64: at most
//                              64 KB), so nothing is shared and nothing synchronises.  The cell's label is a scalar: 8 cells' loads in
//                              flight, then 8 read-add-writes of the thread's own columns, in cell order.  The array goes to the workspace
//                              by plain stores; the slab-0 workgroup also counts the part's cells per class.
//   proto_update_kernel        grid C, 256 lanes: class c's partial sums in part order, four channels per thread at a time; the moving
//                              average; n[c] by thread 0 behind a barrier (every thread has read it).
// No atomics, no scratch.  Byte floor: F read twice (rectify, accumulate), P read and out written once, the workspace written and read once.
#include "common.h"

#define PR_WAVES 4
#define PR_MAX_WG 2048
#define PR_ROWS 2                // cells a wave works on together: one read of a prototype row serves both
#define PR_GROUP 8               // cells per workgroup and sweep: 4 waves x PR_ROWS
#define PR_REG_CHUNKS 4          // 64 * 4 * 8 = 2048 channels in registers
#define PA_CELLS 256             // cells per accumulate part
#define PA_BATCH 8               // loads in flight per thread

static __device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
static __device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// the first index of the maximum of the lanes < C, a NaN counting as -inf (all NaN: 0); mx: that maximum
static __device__ __forceinline__ int first_argmax(const float v, const bool in, float& mx) {
  const float u = (in && v == v) ? v : -INFINITY;
  mx = wave_max(u);
  const uint64_t hit = __ballot(in && u == mx);
  return hit ? (int)__builtin_ctzll(hit) : 0;
}

template <typename T, int R, bool REG>
__global__ __launch_bounds__(256) void proto_rectify_kernel(const simt_proto_rectify_desc d) {
  __shared__ int wsum[PR_WAVES];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int C = d.C, D = d.D, chunks = D >> 3;
  const bool in = lane < C;
  const bool seen = in && d.n[lane] > 0;
  const uint64_t seen_set = __ballot(seen);
  const long groups = (d.M + R - 1) / R;
  const long waves = (long)gridDim.x * PR_WAVES;
  const T* F = (const T*)d.F;
  int moved = 0;
  for (long g = (long)blockIdx.x * PR_WAVES + wv; g < groups; g += waves) {      // (g is wave-uniform)
    const long m0 = g * R;
    float dist[R];
#pragma unroll
    for (int r = 0; r < R; ++r) dist[r] = 0.f;
    if (REG) {
      Raw8<T> raw[R][PR_REG_CHUNKS];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const long m = m0 + r < d.M ? m0 + r : d.M - 1;      // a row past the end: the last row again, its result is dropped
#pragma unroll
        for (int q = 0; q < PR_REG_CHUNKS; ++q) {
          const int k = lane + 64 * q;
          if (k < chunks) raw8_load(F + m * d.ldF + 8 * k, raw[r][q]);
        }
      }
      uint64_t set = seen_set;
      while (set) {                                        // (scalar loop: the set is wave-uniform)
        const int c = __builtin_ctzll(set);
        set &= set - 1;
        const float* pe = d.eta + (long)c * D;
        float s[R];
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] = 0.f;
#pragma unroll
        for (int q = 0; q < PR_REG_CHUNKS; ++q) {
          const int k = lane + 64 * q;
          if (k < chunks) {
            float ev[8];
            load8(pe + 8 * k, ev);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              float a[8];
              raw8_unpack(raw[r][q], a);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float t = a[e] - ev[e];
                s[r] += t * t;
              }
            }
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float dd = sqrtf(wave_sum(s[r]));
          if (lane == c) dist[r] = dd;
        }
      }
    } else {
      uint64_t set = seen_set;
      while (set) {
        const int c = __builtin_ctzll(set);
        set &= set - 1;
        const float* pe = d.eta + (long)c * D;
        float s[R];
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] = 0.f;
        for (int k = lane; k < chunks; k += 64) {
          float ev[8];
          load8(pe + 8 * k, ev);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const long m = m0 + r < d.M ? m0 + r : d.M - 1;
            float a[8];
            load8(F + m * d.ldF + 8 * k, a);                // the row again (from L2)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float t = a[e] - ev[e];
              s[r] += t * t;
            }
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float dd = sqrtf(wave_sum(s[r]));
          if (lane == c) dist[r] = dd;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long m = m0 + r;
      if (m >= d.M) break;                                 // (wave-uniform)
      const float* pp = d.P + m * d.ldp;
      float* po = d.out + m * d.ldp;
      const float p = in ? pp[lane] : 0.f;
      float o = p;
      if (seen_set) {
        const float dmin = wave_min(seen ? dist[r] : INFINITY);      // fminf: a NaN loses to a number
        const float dc = seen ? dist[r] : dmin;            // an unseen class: the distance of the nearest seen one
        const float z = -(dc - dmin) / d.temp;
        if (d.family == 0) {
          const float w = in ? expf(z) * p : 0.f;
          o = w / wave_sum(w);
        } else {
          o = p + z;
        }
      }
      if (in) po[lane] = o;
      for (int col = C + lane; col < d.ldp; col += 64) po[col] = pp[col];
      float mx, mp;
      const int arg = first_argmax(o, in, mx);
      const int argp = first_argmax(p, in, mp);
      float conf = mx;
      if (d.family != 0) conf = 1.f / wave_sum(in ? expf(o - mx) : 0.f);
      const bool bad = __ballot(in && o != o) != 0ull;
      if (lane == 0) d.lab[m] = (!bad && conf > d.thr) ? (uint8_t)arg : (uint8_t)255;
      moved += arg != argp ? 1 : 0;
    }
  }
  if (lane == 0) wsum[wv] = moved;
  __syncthreads();
  if (threadIdx.x == 0) d.changed_part[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

template <typename T, int V> static __device__ __forceinline__ void pa_load(const T* p, float* v);
template <> __device__ __forceinline__ void pa_load<float, 1>(const float* p, float* v) { v[0] = *p; }
template <> __device__ __forceinline__ void pa_load<float, 2>(const float* p, float* v) { const float2 a = *(const float2*)p; v[0] = a.x; v[1] = a.y; }
template <> __device__ __forceinline__ void pa_load<float, 4>(const float* p, float* v) {
  const float4 a = *(const float4*)p;
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
template <> __device__ __forceinline__ void pa_load<bf16_t, 1>(const bf16_t* p, float* v) { v[0] = bf2f(*p); }
template <> __device__ __forceinline__ void pa_load<bf16_t, 2>(const bf16_t* p, float* v) {
  const uint32_t a = *(const uint32_t*)p;
  v[0] = __uint_as_float(a << 16); v[1] = __uint_as_float(a & 0xffff0000u);
}
template <> __device__ __forceinline__ void pa_load<bf16_t, 4>(const bf16_t* p, float* v) {
  const uint2 a = *(const uint2*)p;
  v[0] = __uint_as_float(a.x << 16); v[1] = __uint_as_float(a.x & 0xffff0000u);
  v[2] = __uint_as_float(a.y << 16); v[3] = __uint_as_float(a.y & 0xffff0000u);
}

template <typename T, int V>
__global__ __launch_bounds__(256) void proto_acc_kernel(const simt_proto_acc_desc d, const int parts) {
  extern __shared__ float acc[];                           // [C][256 * V]: thread t owns columns t * V .. t * V + V - 1
  const int t = threadIdx.x, W = 256 * V, C = d.C;
  const int part = blockIdx.x;
  const int k0 = (int)blockIdx.y * W + t * V;
  const bool live = k0 < d.D;                              // D % 8 == 0 and V divides 8: a live thread's V columns all lie below D
  float* mine = acc + t * V;
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int v = 0; v < V; ++v) mine[c * W + v] = 0.f;
  }
  const long m0 = (long)part * PA_CELLS;
  const long m1 = m0 + PA_CELLS < d.M ? m0 + PA_CELLS : d.M;
  const T* F = (const T*)d.F + k0;
  for (long m = m0; m < m1; m += PA_BATCH) {
    int cc[PA_BATCH];
    float val[PA_BATCH][V];
#pragma unroll
    for (int j = 0; j < PA_BATCH; ++j) {
      cc[j] = m + j < m1 ? __builtin_amdgcn_readfirstlane((int)d.lab[m + j]) : 255;      // (a scalar: the address is uniform)
      if (cc[j] < C && live) pa_load<T, V>(F + (m + j) * d.ldF, val[j]);
    }
#pragma unroll
    for (int j = 0; j < PA_BATCH; ++j) {                   // in cell order
      if (cc[j] < C && live) {
        float* a = mine + cc[j] * W;
#pragma unroll
        for (int v = 0; v < V; ++v) a[v] += val[j][v];
      }
    }
  }
  if (live) {
    float* ws = d.ws + (long)part * C * d.D + k0;
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int v = 0; v < V; ++v) ws[(long)c * d.D + v] = mine[c * W + v];
    }
  }
  if (blockIdx.y == 0 && t < C) {
    int cnt = 0;
    for (long m = m0; m < m1; ++m) cnt += (int)d.lab[m] == t ? 1 : 0;
    ((int32_t*)(d.ws + (long)parts * C * d.D))[(long)part * C + t] = cnt;
  }
}

__global__ __launch_bounds__(256) void proto_update_kernel(const simt_proto_update_desc d, const int parts, const float omm) {
  const int c = blockIdx.x, t = threadIdx.x, C = d.C, D = d.D;
  const int n0 = d.n[c];
  const int32_t* pc = (const int32_t*)(d.ws + (long)parts * C * D) + c;
  int cnt = 0;
  for (int p = 0; p < parts; ++p) cnt += pc[(long)p * C];
  __syncthreads();                                         // every thread holds n[c]: thread 0 may write it
  if (cnt == 0) return;                                    // (uniform) the class is absent from the batch: nothing is touched
  const float fc = (float)cnt;
  const float a = fmaxf(omm, 1.f / (float)(n0 + 1));
  for (int k = 4 * t; k < D; k += 1024) {
    const float* ps = d.ws + (long)c * D + k;
    float4 S = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = 0; p < parts; ++p) {                      // part order
      const float4 v = *(const float4*)(ps + (long)p * C * D);
      S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
    }
    float* pe = d.eta + (long)c * D + k;
    float4 e = *(const float4*)pe;
    const float4 mean = make_float4(S.x / fc, S.y / fc, S.z / fc, S.w / fc);
    if (n0 > 0) {
      e.x = __fmaf_rn(a, mean.x - e.x, e.x); e.y = __fmaf_rn(a, mean.y - e.y, e.y);
      e.z = __fmaf_rn(a, mean.z - e.z, e.z); e.w = __fmaf_rn(a, mean.w - e.w, e.w);
    } else {
      e = mean;
    }
    *(float4*)pe = e;
  }
  if (t == 0) d.n[c] = n0 + 1;
}

static int pa_parts(long M) { return (int)((M + PA_CELLS - 1) / PA_CELLS); }
static bool pr_geometry(long M, int C, int D) {
  return M >= 1 && M < (1L << 31) && C >= 2 && C <= SIMT_PROTO_MAX_CLASSES && D >= 8 && D <= SIMT_PROTO_MAX_DIM && (D & 7) == 0;
}

extern "C" int simt_proto_parts(long M) {
  if (M < 1 || M >= (1L << 31)) return 0;
  const long g = (M + PR_GROUP - 1) / PR_GROUP;
  return (int)(g < PR_MAX_WG ? g : PR_MAX_WG);
}

extern "C" long simt_proto_ws_floats(long M, int C, int D) {
  if (!pr_geometry(M, C, D)) return 0;
  return (long)pa_parts(M) * C * ((long)D + 1);
}

extern "C" int simt_proto_rectify(const simt_proto_rectify_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->F && d->P && d->out && d->eta && d->n && d->lab && d->changed_part);
  SIMT_CHECK(pr_geometry(d->M, d->C, d->D));
  SIMT_CHECK(d->dtype == SIMT_F32 || d->dtype == SIMT_BF16);
  SIMT_CHECK(d->ldF >= d->D && (d->ldF & 7) == 0 && d->ldp >= d->C);
  SIMT_CHECK(d->family == 0 || d->family == 1);
  SIMT_CHECK(d->temp > 0.f && d->temp <= 3.4028234e38f);      // (a NaN fails the first)
  SIMT_CHECK(d->thr == d->thr);
  SIMT_CHECK(((uintptr_t)d->F & 15) == 0 && ((uintptr_t)d->eta & 15) == 0);
  SIMT_CHECK(((uintptr_t)d->P & 3) == 0 && ((uintptr_t)d->out & 3) == 0 && ((uintptr_t)d->n & 3) == 0 && ((uintptr_t)d->changed_part & 3) == 0);
  const dim3 grid((unsigned)simt_proto_parts(d->M));
  const bool reg = d->D <= 64 * PR_REG_CHUNKS * 8;
  if (d->dtype == SIMT_BF16) {
    if (reg) hipLaunchKernelGGL((proto_rectify_kernel<bf16_t, PR_ROWS, true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
    else hipLaunchKernelGGL((proto_rectify_kernel<bf16_t, PR_ROWS, false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  } else {
    if (reg) hipLaunchKernelGGL((proto_rectify_kernel<float, PR_ROWS, true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
    else hipLaunchKernelGGL((proto_rectify_kernel<float, PR_ROWS, false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  }
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

template <typename T>
static void pa_launch(const simt_proto_acc_desc* d, hipStream_t stream) {
  const int parts = pa_parts(d->M);
  const int V = d->C <= 16 ? 4 : d->C <= 32 ? 2 : 1;
  const dim3 grid((unsigned)parts, (unsigned)((d->D + 256 * V - 1) / (256 * V)));
  const size_t lds = (size_t)d->C * 256 * V * sizeof(float);      // <= 64 KB
  if (V == 4) hipLaunchKernelGGL((proto_acc_kernel<T, 4>), grid, dim3(256), lds, stream, *d, parts);
  else if (V == 2) hipLaunchKernelGGL((proto_acc_kernel<T, 2>), grid, dim3(256), lds, stream, *d, parts);
  else hipLaunchKernelGGL((proto_acc_kernel<T, 1>), grid, dim3(256), lds, stream, *d, parts);
}

extern "C" int simt_proto_accumulate(const simt_proto_acc_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->F && d->lab && d->ws);
  SIMT_CHECK(pr_geometry(d->M, d->C, d->D));
  SIMT_CHECK(d->dtype == SIMT_F32 || d->dtype == SIMT_BF16);
  SIMT_CHECK(d->ldF >= d->D && (d->ldF & 7) == 0);
  SIMT_CHECK(((uintptr_t)d->F & 15) == 0 && ((uintptr_t)d->ws & 15) == 0);
  if (d->dtype == SIMT_BF16) pa_launch<bf16_t>(d, (hipStream_t)stream);
  else pa_launch<float>(d, (hipStream_t)stream);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_proto_update(const simt_proto_update_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->ws && d->eta && d->n);
  SIMT_CHECK(pr_geometry(d->M, d->C, d->D));
  SIMT_CHECK(d->momentum >= 0.0 && d->momentum < 1.0);      // (a NaN fails both)
  SIMT_CHECK(((uintptr_t)d->ws & 15) == 0 && ((uintptr_t)d->eta & 15) == 0 && ((uintptr_t)d->n & 3) == 0);
  hipLaunchKernelGGL(proto_update_kernel, dim3((unsigned)d->C), dim3(256), 0, (hipStream_t)stream, *d, pa_parts(d->M),
                     (float)(1.0 - d->momentum));
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
