// Random scale + crop on the device (simt_amd/data/scale_crop.py): item b of a batch is the w x h window at (ox, oy) of
// S = Image.resize((ws, hs), BICUBIC) of its source frame (label: NEAREST), 0 / 255 where the window leaves S, then BGR - mean, CHW, int64
// labels and the reference's mirror rule -- in ONE launch per batch, straight from the decoded uint8 frames (upload buffers or dataset-cache
// slots) to the network's input.  S is never stored: scaling the whole frame and cutting a window afterwards would compute up to 2.25x the
// pixels the window keeps (s = 1.5) and cost two more HBM round trips per item.
//
// Bit-exactness.  Pillow's 8-bit resampler is two integer passes, horizontal first, each rounded to uint8 with
// clip8(((1 << 21) + sum) >> 22) (csrc/input_prep.hip).  A workgroup owns a TH x TW = 16 x 64 tile of the output:
//   1. the horizontal pass for the tile's columns and for exactly the source rows its output rows read,
//      bounds_y[first].lo ... bounds_y[last].lo + n (bounds are monotone), into LDS as uint8 [row][channel][TW];
//   2. the vertical pass out of LDS: a lane owns 4 consecutive columns of one row and reads one dword per channel and tap;
//   3. minus mean, the three planes and the labels, 16 bytes per store where w % 4 == 0.
// Same tables (simt_amd/data/resample.py), same order, same intermediate: the bytes are Pillow's.
// LDS: max_rows * 192 bytes of pixels + the tile's coefficients (64 * ksize_x + 16 * ksize_y dwords): 1024 x 2048 -> 512 x 256 (s = 0.5 at
// the 1024 x 512 crop, ksize 17 on both axes) reads at most 76 rows per tile = 14.3 KB + 5.3 KB, eight workgroups per CU.
// The descriptor arrives in the kernel-argument segment; everything indexed by the item (blockIdx.z) is wave-uniform: scalar loads.
#include <stdio.h>

#include "common.h"

#define SC_TH SIMT_SCALE_CROP_TILE_H
#define SC_TW SIMT_SCALE_CROP_TILE_W
#define SC_PRECISION 22

typedef __attribute__((ext_vector_type(2))) long long sc_i64x2;

__device__ __forceinline__ int sc_clip8(int acc) {
  const int v = acc >> SC_PRECISION;                     // arithmetic shift, then clip8
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// WIN_: empty for simt_scale_crop (name and code as before the flavour existed); {true} for simt_scale_crop_win (csrc/rare_crop.hip), whose
// block-uniform choice and origin are three words of device memory, win[b][0..2], clamped so that whatever they hold no table is read out
// of range: the choice to n_choices - 1, the origin to its choice's origin range (the range max_rows was computed over).
template <bool VEC, bool... WIN_>
__global__ __launch_bounds__(256) void scale_crop_kernel(const simt_scale_crop_desc d, int ksx_max, const int32_t* __restrict__ win) {
  constexpr bool WIN = (false || ... || WIN_);
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_smem[];
  const int b = blockIdx.z, tid = threadIdx.x;
  int ci = d.choice[b];
  if (WIN) ci = (int)min((unsigned)__builtin_amdgcn_readfirstlane(win[4 * b]), (unsigned)(d.n_choices - 1));
  const int ws = d.c[ci].ws, hs = d.c[ci].hs, ksx = d.c[ci].ksx, ksy = d.c[ci].ksy;
  const int32_t* __restrict__ T = d.tables;
  const int32_t* __restrict__ bx = T + d.c[ci].bounds_x;
  const int32_t* __restrict__ kx = T + d.c[ci].coef_x;
  const int32_t* __restrict__ by = T + d.c[ci].bounds_y;
  const int32_t* __restrict__ ky = T + d.c[ci].coef_y;
  const unsigned char* __restrict__ img = d.img[b];
  const int w = d.w, h = d.h, Ws = d.Ws, max_rows = d.max_rows;
  int ox = d.ox[b], oy = d.oy[b];
  if (WIN) {
    ox = min(max(__builtin_amdgcn_readfirstlane(win[4 * b + 1]), min(0, ws - w)), max(0, ws - w));
    oy = min(max(__builtin_amdgcn_readfirstlane(win[4 * b + 2]), min(0, hs - h)), max(0, hs - h));
  }
  const int mirror = d.mirror[b];
  const int x0 = blockIdx.x * SC_TW, y0 = blockIdx.y * SC_TH;
  // the rows [sy_lo, sy_hi) and columns [sx_lo, sx_hi) of S this tile shows
  const int sy_lo = max(0, y0 + oy), sy_hi = min(hs, min(y0 + SC_TH, h) + oy);
  const int sx_lo = max(0, x0 + ox), sx_hi = min(ws, min(x0 + SC_TW, w) + ox);
  unsigned char* pix = sc_smem;                                    // [max_rows][3][SC_TW] u8: the horizontal pass's output
  int* kxs = (int*)(sc_smem + (size_t)max_rows * 3 * SC_TW);       // [SC_TW][ksx]: ksx is odd, a wave's 64 columns hit 64 banks
  int* kys = kxs + SC_TW * ksx_max;                                // [SC_TH][ksy]
  const bool any = sy_lo < sy_hi && sx_lo < sx_hi;                 // block-uniform: the barriers below are too
  int r0 = 0;
  if (any) {
    r0 = by[2 * sy_lo];
    const int nrows = min(by[2 * (sy_hi - 1)] + by[2 * (sy_hi - 1) + 1] - r0, max_rows);
    const long gx = (long)(x0 + ox) * ksx, nx = (long)ws * ksx;
    for (int i = tid; i < SC_TW * ksx; i += 256) kxs[i] = (gx + i >= 0 && gx + i < nx) ? kx[gx + i] : 0;
    const long gy = (long)(y0 + oy) * ksy, ny = (long)hs * ksy;
    for (int i = tid; i < SC_TH * ksy; i += 256) kys[i] = (gy + i >= 0 && gy + i < ny) ? ky[gy + i] : 0;
    __syncthreads();
    // 1. horizontal pass: a lane owns one column, a wave every fourth row
    const int j = tid & 63, sx = x0 + j + ox;
    if (sx >= sx_lo && sx < sx_hi) {
      const int lo = bx[2 * sx], n = bx[2 * sx + 1];
      const int* kc = kxs + j * ksx;
      for (int rr = tid >> 6; rr < nrows; rr += 4) {
        const unsigned char* p = img + ((long)(r0 + rr) * Ws + lo) * 3;
        int a0 = 1 << (SC_PRECISION - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t, p += 3) {
          const int kv = kc[t];
          a0 += (int)p[0] * kv;
          a1 += (int)p[1] * kv;
          a2 += (int)p[2] * kv;
        }
        unsigned char* q = pix + rr * 3 * SC_TW + j;
        q[0] = (unsigned char)sc_clip8(a0);
        q[SC_TW] = (unsigned char)sc_clip8(a1);
        q[2 * SC_TW] = (unsigned char)sc_clip8(a2);
      }
    }
    __syncthreads();
  }
  // 2. vertical pass: a lane owns 4 consecutive columns of one row
  const int i = tid >> 4, q4 = (tid & 15) * 4;
  const int y = y0 + i, x = x0 + q4;
  if (y >= h || x >= w) return;
  const int sy = y + oy;
  const bool row_in = sy >= 0 && sy < hs;
  int a0[4], a1[4], a2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a0[k] = a1[k] = a2[k] = 1 << (SC_PRECISION - 1);
  if (any && row_in) {
    const int lo = by[2 * sy] - r0, n = by[2 * sy + 1];
    const int* kc = kys + i * ksy;
    const unsigned char* p = pix + lo * 3 * SC_TW + q4;
    for (int t = 0; t < n; ++t, p += 3 * SC_TW) {
      const int kv = kc[t];
      const uint32_t u0 = *(const uint32_t*)p, u1 = *(const uint32_t*)(p + SC_TW), u2 = *(const uint32_t*)(p + 2 * SC_TW);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a0[k] += (int)((u0 >> (8 * k)) & 255u) * kv;
        a1[k] += (int)((u1 >> (8 * k)) & 255u) * kv;
        a2[k] += (int)((u2 >> (8 * k)) & 255u) * kv;
      }
    }
  }
  // 3. planes: plane 0 = B - mean0, mirrored: R (the reference's channel-axis flip); 0.0f outside S
  const float m0 = d.mean[0], m1 = d.mean[1], m2 = d.mean[2];
  float v0[4], v1[4], v2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int sx = x + k + ox;
    const bool in = row_in && sx >= 0 && sx < ws;
    const float r = (float)sc_clip8(a0[k]), g = (float)sc_clip8(a1[k]), bl = (float)sc_clip8(a2[k]);
    v0[k] = in ? (mirror ? r : bl) - m0 : 0.0f;
    v1[k] = in ? g - m1 : 0.0f;
    v2[k] = in ? (mirror ? bl : r) - m2 : 0.0f;
  }
  const long HW = (long)h * w;
  const long o = (long)y * w + x;
  float* __restrict__ xo = d.x + (long)b * 3 * HW + o;
  if (VEC) {
    *(float4*)xo = make_float4(v0[0], v0[1], v0[2], v0[3]);
    *(float4*)(xo + HW) = make_float4(v1[0], v1[1], v1[2], v1[3]);
    *(float4*)(xo + 2 * HW) = make_float4(v2[0], v2[1], v2[2], v2[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < w) {
        xo[k] = v0[k];
        xo[HW + k] = v1[k];
        xo[2 * HW + k] = v2[k];
      }
  }
  if (d.lab_out) {
    const unsigned char* __restrict__ lab = d.lab[b];
    const int32_t* __restrict__ xtab = T + d.c[ci].xtab;
    const long lrow = row_in ? (long)T[d.c[ci].ytab + sy] * Ws : 0;
    long long l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xw = mirror ? w - 1 - (x + k) : x + k;      // only the label is reversed along x
      const int sx = xw + ox;
      const bool in = row_in && xw >= 0 && sx >= 0 && sx < ws;
      l[k] = in ? (long long)lab[lrow + xtab[sx]] : 255ll;
    }
    long long* __restrict__ lo = d.lab_out + (long)b * HW + o;
    if (VEC) {
      sc_i64x2 u = {l[0], l[1]}, v = {l[2], l[3]};
      *(sc_i64x2*)lo = u;
      *(sc_i64x2*)(lo + 2) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < w) lo[k] = l[k];
    }
  }
}

// Validates everything the kernel indexes with: sizes, the choices' table extents against n_tables, the per-item choice.
static bool sc_valid(const simt_scale_crop_desc* d) {
  if (!d || !d->x || !d->tables || d->B <= 0 || d->B > SIMT_SCALE_CROP_MAX) return false;
  if (d->Hs <= 0 || d->Ws <= 0 || d->h <= 0 || d->w <= 0 || d->max_rows <= 0 || d->max_rows > d->Hs) return false;
  if ((long)d->Hs * d->Ws * 3 >= (1L << 31) || (long)d->h * d->w >= (1L << 31)) return false;
  if (d->n_choices <= 0 || d->n_choices > SIMT_SCALE_CROP_CHOICES || d->n_tables <= 0) return false;
  for (int c = 0; c < d->n_choices; ++c) {
    const simt_scale_crop_choice& k = d->c[c];
    if (k.ws <= 0 || k.hs <= 0 || k.ksx <= 0 || k.ksy <= 0 || k.ws > (1 << 20) || k.hs > (1 << 20) || k.ksx > 4096 || k.ksy > 4096) return false;
    const long n = d->n_tables;
    if (k.bounds_x < 0 || k.bounds_x + 2L * k.ws > n || k.coef_x < 0 || k.coef_x + (long)k.ws * k.ksx > n) return false;
    if (k.bounds_y < 0 || k.bounds_y + 2L * k.hs > n || k.coef_y < 0 || k.coef_y + (long)k.hs * k.ksy > n) return false;
    if (d->lab_out && (k.xtab < 0 || k.xtab + (long)k.ws > n || k.ytab < 0 || k.ytab + (long)k.hs > n)) return false;
  }
  for (int b = 0; b < d->B; ++b) {
    if (!d->img[b] || (d->lab_out && !d->lab[b]) || d->choice[b] >= d->n_choices) return false;
    if (d->ox[b] < -(1 << 20) || d->ox[b] > (1 << 20) || d->oy[b] < -(1 << 20) || d->oy[b] > (1 << 20)) return false;
  }
  return true;
}

static void sc_ksize_max(const simt_scale_crop_desc* d, int* ksx, int* ksy) {
  *ksx = *ksy = 0;
  for (int c = 0; c < d->n_choices; ++c) {
    if (d->c[c].ksx > *ksx) *ksx = d->c[c].ksx;
    if (d->c[c].ksy > *ksy) *ksy = d->c[c].ksy;
  }
}

extern "C" long simt_scale_crop_lds_bytes(const simt_scale_crop_desc* d) {
  if (!sc_valid(d)) return -1;
  int ksx, ksy;
  sc_ksize_max(d, &ksx, &ksy);
  return (long)d->max_rows * 3 * SC_TW + ((long)SC_TW * ksx + (long)SC_TH * ksy) * 4;
}

// The launch of both flavours: win NULL is simt_scale_crop, else simt_scale_crop_win (csrc/rare_crop.hip builds `d` from its descriptor).
int simt_scale_crop_launch(const simt_scale_crop_desc* d, const int32_t* win, simt_stream_t stream) {
  SIMT_CHECK(sc_valid(d));
  const bool vec = (d->w & 3) == 0;
  SIMT_CHECK(!vec || (((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->lab_out & 15) == 0));
  int ksx, ksy;
  sc_ksize_max(d, &ksx, &ksy);
  const long lds = simt_scale_crop_lds_bytes(d);
  if (lds > SIMT_SCALE_CROP_LDS_MAX) {
    char msg[200];
    snprintf(msg, sizeof(msg), "scale-crop geometry %d x %d -> crop %d x %d needs %ld bytes of LDS (%d source rows per tile, ksize %d / %d), "
             "the limit is %d", d->Ws, d->Hs, d->w, d->h, lds, d->max_rows, ksx, ksy, SIMT_SCALE_CROP_LDS_MAX);
    simt_set_error(__FILE__, __LINE__, msg);
    return SIMT_ERR_INVALID;
  }
  const dim3 grid((unsigned)((d->w + SC_TW - 1) / SC_TW), (unsigned)((d->h + SC_TH - 1) / SC_TH), (unsigned)d->B);
  SIMT_CHECK(grid.y <= 65535);
  const int32_t* none = nullptr;
  if (win && vec)
    hipLaunchKernelGGL((scale_crop_kernel<true, true>), grid, dim3(256), (size_t)lds, (hipStream_t)stream, *d, ksx, win);
  else if (win)
    hipLaunchKernelGGL((scale_crop_kernel<false, true>), grid, dim3(256), (size_t)lds, (hipStream_t)stream, *d, ksx, win);
  else if (vec)
    hipLaunchKernelGGL((scale_crop_kernel<true>), grid, dim3(256), (size_t)lds, (hipStream_t)stream, *d, ksx, none);
  else
    hipLaunchKernelGGL((scale_crop_kernel<false>), grid, dim3(256), (size_t)lds, (hipStream_t)stream, *d, ksx, none);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_scale_crop(const simt_scale_crop_desc* d, simt_stream_t stream) { return simt_scale_crop_launch(d, nullptr, stream); }
