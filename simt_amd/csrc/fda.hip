// FDA, Fourier low-band style transfer of the source batch (simt_amd/data/fda.py), to the contract of include/simt_hip.h: the
// amplitude of the (2b+1)^2 lowest frequencies of every source plane is replaced by the paired target plane's, the phase is kept.  Only those
// frequencies change, so the output is the source plus a band-limited trigonometric polynomial: no FFT, no complex image.  With R = 3 B h flat
// pixel rows (xs and xt are [R][w] matrices), nv = b + 1 and nu = 2b + 1, four launches:
//   fda_rows_kernel    G[set][r][v] = sum_y (x[r][y] + mean) e^{-2 pi i v y / w}, set = source | target.  A [R][w] x [w][nv] product with the
//                      twiddle matrix: grid (R / 64, nv / 8, 2); a workgroup stages 64 rows x 128 columns in LDS (16-byte loads where w % 4 ==
//                      0), lane = row, the four waves split the tile's columns; the twiddles of a (column, v) pair are staged once per tile in
//                      LDS from the host's table -- indexed by the integer (v y) mod w, advanced tile to tile by an add and a compare -- and
//                      read as wave-uniform broadcasts.  8 complex accumulators per lane; the waves' sums meet in LDS.
//   fda_swap_kernel    F(u, v) = sum_x G[x][v] e^{-2 pi i u x / h} for both sets, then D = (|F_T| p - F_S) * wt_v / (h w).  grid (nu, 3 B): tiny.
//   fda_cols_kernel    E[r][v] = sum_u D(u, v) e^{+2 pi i u x / h}: one lane per (x, v).
//   fda_apply_kernel   x_out[r][y] = xs[r][y] + sum_v Re(E[r][v] e^{+2 pi i v y / w}).  A lane owns 4 columns and holds their twiddles for 8
//                      frequencies in registers; a wave walks 8 rows, E[r][*] is wave-uniform.  b >= 8: further passes add onto x_out.
// Partial results are plain stores into the workspace, G | E | D; every word read is written by the same call.  No atomics, no scratch.
// Byte floor: xs is read twice, xt once, x_out written once: 16 bytes per pixel and plane.
#include "common.h"

#define FD_TR 64                 // rows of a row-pass tile (lane = row)
#define FD_TC 128                // columns of a row-pass tile (32 per wave)
#define FD_VC 8                  // frequencies v per pass
#define FD_LD (FD_TC + 1)        // odd row pitch: lanes of a wave read one column of 64 rows without a bank conflict
#define FD_AR 32                 // rows of an apply workgroup (8 per wave)

__device__ __forceinline__ float fda_mean(const simt_fda_desc& d, long r) {
  const int c = (int)((r / d.h) % 3);
  return c == 0 ? d.mean[0] : c == 1 ? d.mean[1] : d.mean[2];
}

template <bool VEC>
__global__ __launch_bounds__(256) void fda_rows_kernel(const simt_fda_desc d) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = d.w, nv = d.b + 1;
  const long R = 3L * d.B * d.h;
  const long r0 = (long)blockIdx.x * FD_TR;
  const int v0 = blockIdx.y * FD_VC;
  const float* __restrict__ x = blockIdx.z ? d.xt : d.xs;
  float2* __restrict__ G = (float2*)d.work + (long)blockIdx.z * R * nv;
  const float2* __restrict__ tw = (const float2*)d.tw_w;
  __shared__ __attribute__((aligned(16))) float sV[FD_TR * FD_LD];
  __shared__ __attribute__((aligned(16))) float2 sT[FD_TC][FD_VC];

  // tile loads: lane -> row (tid >> 5) + 8 i, columns 4 (tid & 31) ..
  const int lr = tid >> 5, lc = (tid & 31) << 2;
  float mean_i[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) mean_i[i] = r0 + lr + 8 * i < R ? fda_mean(d, r0 + lr + 8 * i) : 0.0f;
  // twiddle staging: lane -> frequency v0 + (tid & 7), columns (tid >> 3) + 32 i of the tile
  const int tv = tid & 7, tj = tid >> 3;
  uint32_t idx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) idx[i] = ((uint32_t)(v0 + tv) * (uint32_t)(tj + 32 * i)) % (uint32_t)w;
  const uint32_t step = ((uint32_t)(v0 + tv) * (uint32_t)FD_TC) % (uint32_t)w;

  float re[FD_VC], im[FD_VC];
#pragma unroll
  for (int q = 0; q < FD_VC; ++q) re[q] = im[q] = 0.0f;

  for (int k0 = 0; k0 < w; k0 += FD_TC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sT[tj + 32 * i][tv] = tw[idx[i]];
      idx[i] += step;
      if (idx[i] >= (uint32_t)w) idx[i] -= (uint32_t)w;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long r = r0 + lr + 8 * i;
      const int c = k0 + lc;
      float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (r < R && c < w) {
        const float* __restrict__ p = x + r * w + c;
        if (VEC) {                                            // w % 4 == 0: c < w means c + 3 < w, and the quad is 16-byte aligned
          const float4 u = *(const float4*)p;
          a[0] = u.x + mean_i[i]; a[1] = u.y + mean_i[i]; a[2] = u.z + mean_i[i]; a[3] = u.w + mean_i[i];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < w) a[e] = p[e] + mean_i[i];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) sV[(lr + 8 * i) * FD_LD + lc + e] = a[e];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < 32; ++j) {
      const float val = sV[lane * FD_LD + 32 * wave + j];
      const float4* __restrict__ t4 = (const float4*)&sT[32 * wave + j][0];      // wave-uniform: broadcast reads
#pragma unroll
      for (int q2 = 0; q2 < FD_VC / 2; ++q2) {
        const float4 t = t4[q2];
        re[2 * q2] = fmaf(val, t.x, re[2 * q2]);
        im[2 * q2] = fmaf(-val, t.y, im[2 * q2]);
        re[2 * q2 + 1] = fmaf(val, t.z, re[2 * q2 + 1]);
        im[2 * q2 + 1] = fmaf(-val, t.w, im[2 * q2 + 1]);
      }
    }
    __syncthreads();
  }

  float2* red = (float2*)sV;                                 // [4 waves][FD_VC][64 rows]: 32 768 of sV's 33 024 bytes
#pragma unroll
  for (int q = 0; q < FD_VC; ++q) red[(wave * FD_VC + q) * 64 + lane] = make_float2(re[q], im[q]);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = 2 * wave + k, v = v0 + q;
    const float2 a0 = red[(0 * FD_VC + q) * 64 + lane], a1 = red[(1 * FD_VC + q) * 64 + lane];
    const float2 a2 = red[(2 * FD_VC + q) * 64 + lane], a3 = red[(3 * FD_VC + q) * 64 + lane];
    if (r0 + lane < R && v < nv) G[(r0 + lane) * nv + v] = make_float2((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y));
  }
}

__global__ __launch_bounds__(256) void fda_swap_kernel(const simt_fda_desc d, float scale) {
  const int tid = threadIdx.x;
  const int h = d.h, b = d.b, nv = b + 1, nu = 2 * b + 1;
  const long R = 3L * d.B * h;
  const int p = blockIdx.y, ui = blockIdx.x;
  const uint32_t um = ui < b ? (uint32_t)(h - b + ui) : (uint32_t)(ui - b);      // u = ui - b, mod h
  const int parts = 256 / nv;                                // >= 3 (nv <= 65): the rows x are dealt out to `parts` lanes per v
  const int part = tid / nv, v = tid - part * nv;
  const float2* __restrict__ GS = (const float2*)d.work + (long)p * h * nv;
  const float2* __restrict__ GT = GS + R * nv;
  const float2* __restrict__ tw = (const float2*)d.tw_h;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);          // (F_S, F_T) of this lane's rows
  if (part < parts) {
    uint32_t idx = (uint32_t)(((unsigned long long)um * (unsigned)part) % (unsigned)h);
    const uint32_t step = (uint32_t)(((unsigned long long)um * (unsigned)parts) % (unsigned)h);
    for (int x = part; x < h; x += parts) {
      const float2 t = tw[idx], s = GS[(long)x * nv + v], g = GT[(long)x * nv + v];
      acc.x = fmaf(s.x, t.x, fmaf(s.y, t.y, acc.x));         // (a + i b)(c - i s) = (a c + b s) + i (b c - a s)
      acc.y = fmaf(s.y, t.x, fmaf(-s.x, t.y, acc.y));
      acc.z = fmaf(g.x, t.x, fmaf(g.y, t.y, acc.z));
      acc.w = fmaf(g.y, t.x, fmaf(-g.x, t.y, acc.w));
      idx += step;
      if (idx >= (uint32_t)h) idx -= (uint32_t)h;
    }
  }
  __shared__ float4 sR[256];
  sR[tid] = acc;
  __syncthreads();
  if (tid < nv) {                                            // part 0 of every v
    float4 f = sR[tid];
    for (int k = 1; k < parts; ++k) {
      const float4 o = sR[k * nv + tid];
      f.x += o.x; f.y += o.y; f.z += o.z; f.w += o.w;
    }
    const float aS = sqrtf(f.x * f.x + f.y * f.y), aT = sqrtf(f.z * f.z + f.w * f.w);
    const float px = aS > 0.0f ? f.x / aS : 1.0f, py = aS > 0.0f ? f.y / aS : 0.0f;
    const float wt = tid == 0 ? scale : 2.0f * scale;        // v = 0 once, v > 0 for itself and its Hermitian twin
    float2* __restrict__ D = (float2*)d.work + 3 * R * nv;
    D[((long)p * nu + ui) * nv + tid] = make_float2((aT * px - f.x) * wt, (aT * py - f.y) * wt);
  }
}

__global__ __launch_bounds__(256) void fda_cols_kernel(const simt_fda_desc d) {
  const int h = d.h, b = d.b, nv = b + 1, nu = 2 * b + 1;
  const long R = 3L * d.B * h;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)h * nv) return;
  const int x = (int)(i / nv), v = (int)(i - (long)x * nv), p = blockIdx.y;
  const float2* __restrict__ D = (const float2*)d.work + 3 * R * nv + (long)p * nu * nv;
  const float2* __restrict__ tw = (const float2*)d.tw_h;
  float2* __restrict__ E = (float2*)d.work + 2 * R * nv;
  uint32_t idx = (uint32_t)(((unsigned long long)((h - b) % h) * (unsigned)x) % (unsigned)h);      // u = -b
  float er = 0.0f, ei = 0.0f;
  for (int ui = 0; ui < nu; ++ui) {
    const float2 t = tw[idx], dv = D[(long)ui * nv + v];
    er = fmaf(dv.x, t.x, fmaf(-dv.y, t.y, er));              // (a + i b)(c + i s) = (a c - b s) + i (a s + b c)
    ei = fmaf(dv.x, t.y, fmaf(dv.y, t.x, ei));
    idx += (uint32_t)x;
    if (idx >= (uint32_t)h) idx -= (uint32_t)h;
  }
  E[((long)p * h + x) * nv + v] = make_float2(er, ei);
}

template <bool VEC>
__global__ __launch_bounds__(256) void fda_apply_kernel(const simt_fda_desc d, int strips) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w = d.w, nv = d.b + 1;
  const long R = 3L * d.B * d.h;
  const int strip = (int)(blockIdx.x % (unsigned)strips);
  const long rb = (long)(blockIdx.x / (unsigned)strips) * FD_AR;
  const int y0 = strip * 256 + 4 * lane;
  if (y0 >= w) return;
  const float2* __restrict__ tw = (const float2*)d.tw_w;
  const float2* __restrict__ E = (const float2*)d.work + 2 * R * nv;
  for (int v0 = 0; v0 < nv; v0 += FD_VC) {
    const float* src = v0 == 0 ? d.xs : d.x_out;             // a later pass adds onto what this lane stored in the pass before
    float c[4][FD_VC], s[4][FD_VC];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t y = (uint32_t)min(y0 + e, w - 1);
      uint32_t idx = v0 == 0 ? 0u : (uint32_t)(((unsigned long long)v0 * y) % (unsigned)w);
#pragma unroll
      for (int q = 0; q < FD_VC; ++q) {
        const float2 t = tw[idx];
        c[e][q] = t.x; s[e][q] = t.y;
        idx += y;
        if (idx >= (uint32_t)w) idx -= (uint32_t)w;
      }
    }
    for (int k = 0; k < FD_AR / 4; ++k) {
      const long r = rb + wave + 4 * k;
      if (r >= R) break;
      float er[FD_VC], ei[FD_VC];
#pragma unroll
      for (int q = 0; q < FD_VC; ++q) {
        const float2 ev = v0 + q < nv ? E[r * nv + v0 + q] : make_float2(0.0f, 0.0f);      // wave-uniform
        er[q] = ev.x; ei[q] = ev.y;
      }
      const long o = r * w + y0;
      float a[4];
      if (VEC) {
        const float4 u = *(const float4*)(src + o);
        a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = y0 + e < w ? src[o + e] : 0.0f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < FD_VC; ++q) acc = fmaf(er[q], c[e][q], fmaf(-ei[q], s[e][q], acc));
        a[e] += acc;
      }
      if (VEC) {
        *(float4*)(d.x_out + o) = make_float4(a[0], a[1], a[2], a[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (y0 + e < w) d.x_out[o + e] = a[e];
      }
    }
  }
}

static bool fda_geometry_ok(long B, long h, long w, long b) {
  return B >= 1 && B <= SIMT_FDA_MAX_ITEMS && h >= 1 && w >= 1 && b >= 0 && b <= SIMT_FDA_MAX_BAND && 2 * b + 1 <= (h < w ? h : w) &&
         h * w < (1L << 31) && 3 * B * h < (1L << 31);
}

extern "C" long simt_fda_workspace_bytes(int B, int h, int w, int b) {
  if (!fda_geometry_ok(B, h, w, b)) return 0;
  const long R = 3L * B * h, nv = b + 1, nu = 2 * b + 1;
  return (long)sizeof(float2) * (3 * R * nv + 3L * B * nu * nv);       // G[2][R][nv] | E[R][nv] | D[3 B][nu][nv]
}

extern "C" int simt_fda_transfer(const simt_fda_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->xs && d->xt && d->x_out && d->tw_h && d->tw_w && d->work);
  SIMT_CHECK((((uintptr_t)d->xs | (uintptr_t)d->xt | (uintptr_t)d->x_out | (uintptr_t)d->work) & 15) == 0);
  SIMT_CHECK((((uintptr_t)d->tw_h | (uintptr_t)d->tw_w) & 7) == 0);
  SIMT_CHECK(fda_geometry_ok(d->B, d->h, d->w, d->b));
  const uintptr_t n = (uintptr_t)d->B * 3 * d->h * d->w * sizeof(float), xo = (uintptr_t)d->x_out;
  SIMT_CHECK(xo + n <= (uintptr_t)d->xs || (uintptr_t)d->xs + n <= xo);
  SIMT_CHECK(xo + n <= (uintptr_t)d->xt || (uintptr_t)d->xt + n <= xo);
  const long R = 3L * d->B * d->h;
  const int nv = d->b + 1, nu = 2 * d->b + 1;
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = (d->w & 3) == 0;
  const dim3 grows((unsigned)((R + FD_TR - 1) / FD_TR), (unsigned)((nv + FD_VC - 1) / FD_VC), 2);
  if (vec) hipLaunchKernelGGL((fda_rows_kernel<true>), grows, dim3(256), 0, st, *d);
  else     hipLaunchKernelGGL((fda_rows_kernel<false>), grows, dim3(256), 0, st, *d);
  SIMT_LAUNCH_CHECK();
  const float scale = (float)(1.0 / ((double)d->h * (double)d->w));
  hipLaunchKernelGGL(fda_swap_kernel, dim3((unsigned)nu, (unsigned)(3 * d->B)), dim3(256), 0, st, *d, scale);
  SIMT_LAUNCH_CHECK();
  hipLaunchKernelGGL(fda_cols_kernel, dim3((unsigned)(((long)d->h * nv + 255) / 256), (unsigned)(3 * d->B)), dim3(256), 0, st, *d);
  SIMT_LAUNCH_CHECK();
  const int strips = (d->w + 255) / 256;
  const dim3 gapply((unsigned)(((R + FD_AR - 1) / FD_AR) * strips));
  if (vec) hipLaunchKernelGGL((fda_apply_kernel<true>), gapply, dim3(256), 0, st, *d, strips);
  else     hipLaunchKernelGGL((fda_apply_kernel<false>), gapply, dim3(256), 0, st, *d, strips);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
