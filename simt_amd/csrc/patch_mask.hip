// MIC patch masking (Hoyer et al., CVPR'23) of a finished batch (simt_amd/data/patch_mask.py): the square patches the row words name become
// +0.0f -- the mean colour of a batch that holds colour - mean -- in all three planes.  Pure selection, like mix_sweep_kernel: a kept value
// travels as an integer word.  One streaming kernel, descriptor by value in the kernel-argument segment:
//   patch_mask_kernel<VEC, INPLACE>   grid (ceil(h / 4), B), 256 lanes: wave v of workgroup (g, i) owns pixel row y = 4 g + v of item i in all
//                                     three planes.  Its patch row y / patch is wave-uniform, so the mask word rows[i][y / patch] is ONE scalar
//                                     load from the kernel arguments; a lane only shifts it by its column's patch.
//   VEC      w % 4 == 0 and patch % 4 == 0: 4 consecutive pixels per lane, 16-byte loads and stores (rows start on 16-byte boundaries, a quad
//            lies in one patch); otherwise one pixel per lane, dwords, consecutive lanes on consecutive words.
//   INPLACE  x_out == x: blanked words are stored, nothing is loaded, a wave whose row has no blanked patch leaves at once.
// Byte floor with R the blanked share: in place R * 12*B*h*w (stores only), out of place (2 - R) * 12*B*h*w (the blanked patches are not read).
// At 768 x 768 a wave moves 9 KB out of place, the grid is 192 x B workgroups: 3 waves per SIMD at B = 4, one round of the chip.
#include "common.h"

template <bool VEC, bool INPLACE>
__global__ __launch_bounds__(256) void patch_mask_kernel(const simt_patch_mask_desc d) {
  const int i = blockIdx.y;
  const int y = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (y >= d.h) return;                                  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int P = d.patch, w = d.w;
  const uint32_t word = d.rows[i][y / P];               // scalar: i and y are wave-uniform
  if (INPLACE) {
    const int gw = (w - 1) / P + 1;
    if ((word & (gw >= 32 ? 0xffffffffu : ((1u << gw) - 1u))) == 0u) return;
  }
  const long HW = (long)d.h * w;
  const long row = (long)i * 3 * HW + (long)y * w;
  const uint32_t* xi = (const uint32_t*)d.x + row;
  uint32_t* xo = (uint32_t*)d.x_out + row;
  constexpr int N = VEC ? 4 : 1;
  for (int x = lane * N; x < w; x += 64 * N) {
    const bool m = (word >> (x / P)) & 1u;               // x / P < gw <= 32
    if (INPLACE) {
      if (m) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          if (VEC) *(uint4*)(xo + p * HW + x) = make_uint4(0u, 0u, 0u, 0u);
          else xo[p * HW + x] = 0u;
        }
      }
    } else if (VEC) {                                    // the three planes' loads are in flight together; a blanked quad loads nothing
      uint4 v[3] = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
      if (!m) {
#pragma unroll
        for (int p = 0; p < 3; ++p) v[p] = *(const uint4*)(xi + p * HW + x);
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) *(uint4*)(xo + p * HW + x) = v[p];
    } else {
      uint32_t v[3] = {0u, 0u, 0u};
      if (!m) {
#pragma unroll
        for (int p = 0; p < 3; ++p) v[p] = xi[p * HW + x];
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) xo[p * HW + x] = v[p];
    }
  }
}

extern "C" int simt_patch_mask(const simt_patch_mask_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->x && d->x_out);
  SIMT_CHECK(d->B >= 1 && d->B <= SIMT_PATCH_MASK_MAX && d->h >= 1 && d->w >= 1 && d->patch >= 1);
  const long gh = ((long)d->h + d->patch - 1) / d->patch, gw = ((long)d->w + d->patch - 1) / d->patch;
  SIMT_CHECK(gh <= SIMT_PATCH_MASK_GRID && gw <= SIMT_PATCH_MASK_GRID);
  const long HW = (long)d->h * d->w;
  SIMT_CHECK(HW < (1L << 31));
  const uintptr_t a = (uintptr_t)d->x, b = (uintptr_t)d->x_out, bytes = (uintptr_t)d->B * 3 * (uintptr_t)HW * 4;
  SIMT_CHECK((a & 15) == 0 && (b & 15) == 0);
  const bool inplace = a == b;
  SIMT_CHECK(inplace || a + bytes <= b || b + bytes <= a);
  const bool vec = (d->w & 3) == 0 && (d->patch & 3) == 0;
  const dim3 grid((unsigned)(((long)d->h + 3) / 4), (unsigned)d->B);
  if (vec && inplace)
    hipLaunchKernelGGL((patch_mask_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else if (vec)
    hipLaunchKernelGGL((patch_mask_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else if (inplace)
    hipLaunchKernelGGL((patch_mask_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else
    hipLaunchKernelGGL((patch_mask_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
