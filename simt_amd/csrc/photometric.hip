// Photometric augmentation of a finished batch (simt_amd/data/photometric.py): colour jitter (brightness, contrast, saturation + hue as one
// matrix), then a separable radius-5 Gaussian blur, per item, to the arithmetic contract of include/simt_hip.h: IEEE float32,
// every multiply and add rounded on its own, in the order written -- so a numpy restatement gives the same bits.  Contraction into FMA is
// switched off for this whole file (the pragma below); no fast-math, no reciprocal, no division on the device.
//   grey_mean_kernel    grid (PARTS, B), in the style of label_presence_kernel (csrc/class_mix.hip): workgroup (g, b) sums
//                       q = rint(65536 * grey) over its strided share of item b in 64-bit integers (exact, order-free), reduces over the
//                       wave by shuffles and over the waves through LDS, and lane 0 stores ONE uint64, part[b][g] -- every word is
//                       written on every call: no atomics, nothing to zero.  An item without jitter stores 0 and reads nothing.
//   photometric_kernel  grid (tiles, B): 256 lanes own a 16 x 64 output tile, lane t the 4 pixels (row t / 16, columns 4 * (t % 16) ...).
//                       Three workgroup-uniform paths per item:
//                         neither flag  the tile is copied as integer words;
//                         jitter only   pointwise from registers: no halo, no LDS;
//                         blur          the tile + its 5-pixel halo (26 x 74, coordinates reflected at the frame's edges) is normalised and
//                                       jittered from global memory into LDS (all three planes: the matrix needs them together), the
//                                       horizontal pass runs LDS -> LDS (26 x 64), the vertical pass out of LDS into registers.
//                       Every wave first sums the item's 64 partial words to get the grey mean m (jitter only).  The jittered frame and
//                       the half-blurred frame never exist in HBM.
// LDS: 3 * 26 * 74 * 4 = 23 088 bytes (jittered tile + halo) + 3 * 26 * 64 * 4 = 19 968 (after the horizontal pass) = 43 056 of 65 536.
// Byte floor: 12 bytes read + 12 written per pixel; the grey mean reads 12 more on jittered items.  The halo re-reads 26 * 74 / (16 * 64) =
// 1.88x the tile's pixels on blurred items, mostly from L2.
#include "common.h"

#pragma clang fp contract(off)

#define PH_PARTS SIMT_PHOTOMETRIC_PARTS
#define PH_TH 16
#define PH_TW 64
#define PH_R 5
#define PH_AH (PH_TH + 2 * PH_R)
#define PH_AW (PH_TW + 2 * PH_R)

static constexpr float PH_C255 = (float)(1.0 / 255.0);
static constexpr float PH_WG0 = 0.114f, PH_WG1 = 0.587f, PH_WG2 = 0.299f;

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float normalise(float x, float mean) { return clamp01((x + mean) * PH_C255); }
__device__ __forceinline__ float back(float v, float mean) { return v * 255.0f - mean; }
__device__ __forceinline__ float grey(float v0, float v1, float v2) { return (PH_WG0 * v0 + PH_WG1 * v1) + PH_WG2 * v2; }

// q of one pixel: normalise, brightness, grey, 16 fractional bits with ties to even (v_rndne_f32).  0 <= grey <= 1 + a few ulps.
__device__ __forceinline__ unsigned long long grey_q(float x0, float x1, float x2, float mean0, float mean1, float mean2, float fb) {
  const float v0 = clamp01(fb * normalise(x0, mean0)), v1 = clamp01(fb * normalise(x1, mean1)), v2 = clamp01(fb * normalise(x2, mean2));
  return (unsigned long long)(uint32_t)rintf(grey(v0, v1, v2) * 65536.0f);
}

template <bool VEC>
__global__ __launch_bounds__(256) void grey_mean_kernel(const simt_photometric_desc d) {
  const int b = blockIdx.y;
  unsigned long long* out = d.part + (long)b * PH_PARTS + blockIdx.x;
  if (!d.jit[b]) {                                           // workgroup-uniform: nothing is read
    if (threadIdx.x == 0) *out = 0ull;
    return;
  }
  const long HW = (long)d.h * d.w;
  const float* __restrict__ x0 = d.x + (long)b * 3 * HW;
  const float* __restrict__ x1 = x0 + HW;
  const float* __restrict__ x2 = x1 + HW;
  const float mean0 = d.mean[0], mean1 = d.mean[1], mean2 = d.mean[2], fb = d.fb[b];
  const long nquad = HW >> 2;
  const long last = (HW & 3) ? nquad : nquad - 1;            // lane index `nquad` takes the tail, when there is one
  unsigned long long s = 0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q <= last; q += (long)PH_PARTS * 256) {
    if (q < nquad) {
      const long p = q << 2;
      float a[4], g[4], r[4];
      if (VEC) {
        const float4 u = *(const float4*)(x0 + p), v = *(const float4*)(x1 + p), t = *(const float4*)(x2 + p);
        a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w;
        g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = x0[p + e]; g[e] = x1[p + e]; r[e] = x2[p + e]; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) s += grey_q(a[e], g[e], r[e], mean0, mean1, mean2, fb);
    } else {
      for (long p = nquad << 2; p < HW; ++p) s += grey_q(x0[p], x1[p], x2[p], mean0, mean1, mean2, fb);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ unsigned long long wave_sum64[4];
  if ((threadIdx.x & 63) == 0) wave_sum64[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (wave_sum64[0] + wave_sum64[1]) + (wave_sum64[2] + wave_sum64[3]);
}

// m of item i, the same value in every lane: the 64 partial words summed exactly (one word per lane), then ONE float64 product and ONE
// rounding to float32.  S < 2^47 (q <= 65537, h * w < 2^31), so the conversion to float64 is exact.
__device__ __forceinline__ float grey_mean(const simt_photometric_desc& d, int i) {
  unsigned long long s = d.part[(long)i * PH_PARTS + (threadIdx.x & 63)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return (float)((double)s * d.inv);
}

struct Jitter {
  float fb, fc, t;          // t = omfc * m
  float a[9];
};

__device__ __forceinline__ void jitter_pixel(const Jitter& j, float& v0, float& v1, float& v2) {
  v0 = clamp01(j.fb * v0); v1 = clamp01(j.fb * v1); v2 = clamp01(j.fb * v2);
  v0 = clamp01(j.fc * v0 + j.t); v1 = clamp01(j.fc * v1 + j.t); v2 = clamp01(j.fc * v2 + j.t);
  const float n0 = clamp01((j.a[0] * v0 + j.a[1] * v1) + j.a[2] * v2);
  const float n1 = clamp01((j.a[3] * v0 + j.a[4] * v1) + j.a[5] * v2);
  const float n2 = clamp01((j.a[6] * v0 + j.a[7] * v1) + j.a[8] * v2);
  v0 = n0; v1 = n1; v2 = n2;
}

// -k -> k, n-1+k -> n-1-k for the 5 pixels beyond either edge (n >= 6); a coordinate further out belongs to a part of the tile past the
// frame, whose results are never stored: it is clamped into the frame so that the load stays inside.
__device__ __forceinline__ int reflect(int v, int n) {
  v = v < 0 ? -v : v;
  v = v > n - 1 ? 2 * (n - 1) - v : v;
  return v < 0 ? 0 : v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void photometric_kernel(const simt_photometric_desc d) {
  const int i = blockIdx.y;
  const int jit = d.jit[i], blur = d.blur[i];
  const int h = d.h, w = d.w;
  const long HW = (long)h * w;
  const int ntx = (w + PH_TW - 1) / PH_TW;
  const int ty0 = ((int)blockIdx.x / ntx) * PH_TH, tx0 = ((int)blockIdx.x % ntx) * PH_TW;
  const float* __restrict__ xi = d.x + (long)i * 3 * HW;
  float* __restrict__ xo = d.x_out + (long)i * 3 * HW;
  const int tid = threadIdx.x;
  const int r = tid >> 4, c4 = (tid & 15) << 2;
  const int y = ty0 + r, x = tx0 + c4;                       // this lane's pixels: (y, x .. x + 3)
  const long o = (long)y * w + x;
  const bool live = y < h && x < w;                          // (VEC: w % 4 == 0, so x < w means x + 3 < w)

  if (!jit && !blur) {                                       // a straight copy of the tile, as integer words (workgroup-uniform branch)
    if (live) {
      const uint32_t* __restrict__ wi = (const uint32_t*)xi;
      uint32_t* __restrict__ wo = (uint32_t*)xo;
      if (VEC) {
#pragma unroll
        for (int p = 0; p < 3; ++p) *(uint4*)(wo + p * HW + o) = *(const uint4*)(wi + p * HW + o);
      } else {
        for (int e = 0; e < 4 && x + e < w; ++e)
#pragma unroll
          for (int p = 0; p < 3; ++p) wo[p * HW + o + e] = wi[p * HW + o + e];
      }
    }
    return;
  }

  const float mean[3] = {d.mean[0], d.mean[1], d.mean[2]};
  Jitter j;
  if (jit) {
    j.fb = d.fb[i];
    j.fc = d.fc[i];
    j.t = d.omfc[i] * grey_mean(d, i);
#pragma unroll
    for (int k = 0; k < 9; ++k) j.a[k] = d.A[i][k];
  }
  float v[3][4];                                             // this lane's results, in [0, 1]

  if (!blur) {                                               // pointwise: no halo, no LDS
    if (!live) return;
    if (VEC) {
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const float4 u = *(const float4*)(xi + p * HW + o);
        v[p][0] = u.x; v[p][1] = u.y; v[p][2] = u.z; v[p][3] = u.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int p = 0; p < 3; ++p) v[p][e] = x + e < w ? xi[p * HW + o + e] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int p = 0; p < 3; ++p) v[p][e] = normalise(v[p][e], mean[p]);
      jitter_pixel(j, v[0][e], v[1][e], v[2][e]);
    }
  } else {
    __shared__ float sA[3][PH_AH][PH_AW];                                  // normalised + jittered tile and halo
    __shared__ __attribute__((aligned(16))) float sB[3][PH_AH][PH_TW];     // after the horizontal pass
    const float k0 = d.wk[i][0], k1 = d.wk[i][1], k2 = d.wk[i][2], k3 = d.wk[i][3], k4 = d.wk[i][4], k5 = d.wk[i][5];
    for (int idx = tid; idx < PH_AH * PH_AW; idx += 256) {
      const int rr = idx / PH_AW, cc = idx - rr * PH_AW;
      const long g = (long)reflect(ty0 - PH_R + rr, h) * w + reflect(tx0 - PH_R + cc, w);
      float v0 = normalise(xi[g], mean[0]), v1 = normalise(xi[HW + g], mean[1]), v2 = normalise(xi[2 * HW + g], mean[2]);
      if (jit) jitter_pixel(j, v0, v1, v2);
      sA[0][rr][cc] = v0; sA[1][rr][cc] = v1; sA[2][rr][cc] = v2;
    }
    __syncthreads();
    // horizontal pass: one (plane, row, quad of columns) per lane and turn -- 14 values in, 4 out
    for (int idx = tid; idx < 3 * PH_AH * (PH_TW / 4); idx += 256) {
      const int q = idx & 15, pr = idx >> 4;
      const int p = pr / PH_AH, rr = pr - p * PH_AH;
      float a[4 + 2 * PH_R];
#pragma unroll
      for (int n = 0; n < 4 + 2 * PH_R; ++n) a[n] = sA[p][rr][4 * q + n];
      float4 out;
      float* oe = (float*)&out;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float acc = k0 * a[e + 5];
        acc = acc + k1 * (a[e + 4] + a[e + 6]);
        acc = acc + k2 * (a[e + 3] + a[e + 7]);
        acc = acc + k3 * (a[e + 2] + a[e + 8]);
        acc = acc + k4 * (a[e + 1] + a[e + 9]);
        acc = acc + k5 * (a[e + 0] + a[e + 10]);
        oe[e] = acc;
      }
      *(float4*)&sB[p][rr][4 * q] = out;
    }
    __syncthreads();
    if (!live) return;
    // vertical pass: this lane's 4 columns of output row r = rows r .. r + 10 of sB
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      float4 rows[2 * PH_R + 1];
#pragma unroll
      for (int n = 0; n < 2 * PH_R + 1; ++n) rows[n] = *(const float4*)&sB[p][r + n][c4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#define PH_AT(n) (((const float*)&rows[n])[e])
        float acc = k0 * PH_AT(5);
        acc = acc + k1 * (PH_AT(4) + PH_AT(6));
        acc = acc + k2 * (PH_AT(3) + PH_AT(7));
        acc = acc + k3 * (PH_AT(2) + PH_AT(8));
        acc = acc + k4 * (PH_AT(1) + PH_AT(9));
        acc = acc + k5 * (PH_AT(0) + PH_AT(10));
#undef PH_AT
        v[p][e] = clamp01(acc);
      }
    }
  }

  if (VEC) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
      *(float4*)(xo + p * HW + o) = make_float4(back(v[p][0], mean[p]), back(v[p][1], mean[p]), back(v[p][2], mean[p]), back(v[p][3], mean[p]));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x + e < w) {
#pragma unroll
        for (int p = 0; p < 3; ++p) xo[p * HW + o + e] = back(v[p][e], mean[p]);
      }
  }
}

static int photometric_check(const simt_photometric_desc* d) {
  SIMT_CHECK(d && d->x && d->x_out && d->part);
  SIMT_CHECK(((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->x_out & 15) == 0 && ((uintptr_t)d->part & 7) == 0);
  SIMT_CHECK((const void*)d->x != (const void*)d->x_out);
  SIMT_CHECK(d->B > 0 && d->B <= SIMT_PHOTOMETRIC_MAX && d->h >= 6 && d->w >= 6);
  SIMT_CHECK((long)d->h * d->w < (1L << 31));
  return SIMT_OK;
}

extern "C" int simt_grey_mean_parts(const simt_photometric_desc* d, simt_stream_t stream) {
  const int rc = photometric_check(d);
  if (rc != SIMT_OK) return rc;
  const dim3 grid(SIMT_PHOTOMETRIC_PARTS, (unsigned)d->B);
  if ((((long)d->h * d->w) & 3) == 0)
    hipLaunchKernelGGL((grey_mean_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else
    hipLaunchKernelGGL((grey_mean_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_photometric(const simt_photometric_desc* d, simt_stream_t stream) {
  const int rc = photometric_check(d);
  if (rc != SIMT_OK) return rc;
  const long tiles = (long)((d->w + PH_TW - 1) / PH_TW) * ((d->h + PH_TH - 1) / PH_TH);
  const dim3 grid((unsigned)tiles, (unsigned)d->B);
  if ((d->w & 3) == 0)
    hipLaunchKernelGGL((photometric_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else
    hipLaunchKernelGGL((photometric_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
