// The tap arithmetic of ATen's upsample_bilinear2d, shared by the resampling kernels (eval_metric.hip) and the label sweep (label_sweep.hip).
#pragma once
#include "common.h"

// one axis: align_corners=True is src = scale * dst with scale = (in-1)/(out-1) (the interp_target flavour of trainV2_simt.py:301); the
// default align_corners=False is src = (dst + 0.5) * in/out - 0.5, clamped at 0 (model/deeplabv3.py:137)
__device__ __forceinline__ void up_taps(int d, int in, float scale, int align, int& i0, int& i1, float& l0, float& l1) {
  float f = align ? scale * (float)d : fmaxf(((float)d + 0.5f) * scale - 0.5f, 0.f);
  i0 = (int)f;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = f - (float)i0;
  l0 = 1.f - l1;
}

// both axes, align_corners=True: the 4 pixel offsets into an [h][w] map and their weights
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

// the align_corners=True scale of one axis, as the host hands it to the kernels
static inline float align_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
