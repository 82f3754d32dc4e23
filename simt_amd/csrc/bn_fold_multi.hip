// Every eval-mode BatchNorm fold of a plan in ONE launch (simt_amd/ema_teacher.py): the table-driven form of simt_bn_fold
// (bn_pool.hip), for a frozen plan whose weights move.  Held bit for bit to that kernel (include/simt_hip.h, simt_bn_fold_desc): the
// arithmetic below is bn_fold_kernel's source expression, and this file is compiled with the flags of bn_pool.hip and, like it, WITHOUT a
// floating-point contraction pragma -- the compiler's choice for `beta - rm * sc` (one fused multiply-add under the default setting) is
// the same in both.  Do not add `#pragma clang fp contract` here unless bn_pool.hip gets the same one.
//   bn_fold_multi_kernel  one workgroup of 256 lanes per chunk: (segment, chunk index) pairs as in simt_sgd_multi / simt_ema_multi; lane t
//                         serves channels index * chunk + t, + 256, ... of its segment.  16 bytes read and 8 written per channel, nothing
//                         read twice: no LDS, no atomics, no scratch; plain loads and plain stores.
#include "common.h"

struct BnFoldArgs {
  const simt_bn_fold_seg* segs;
  const int* chunks;  // [nchunks][2] = (segment, first channel / chunk)
  int nsegs, chunk;
  float eps;
};

__global__ __launch_bounds__(256) void bn_fold_multi_kernel(BnFoldArgs a) {
  const int si = a.chunks[2 * blockIdx.x];
  if ((unsigned)si >= (unsigned)a.nsegs) return;      // (a table that names no segment writes nothing)
  const simt_bn_fold_seg s = a.segs[si];
  const long long c0 = (long long)a.chunks[2 * blockIdx.x + 1] * a.chunk;
  for (int i = threadIdx.x; i < a.chunk; i += 256) {
    const long long c = c0 + i;
    if (c < 0 || c >= s.C) return;
    float sc = s.gamma[c] / sqrtf(s.running_var[c] + a.eps);
    s.scale[c] = sc;
    s.shift[c] = s.beta[c] - s.running_mean[c] * sc;
  }
}

extern "C" int simt_bn_fold_multi(const simt_bn_fold_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->segs && d->segs_host && d->chunks);
  SIMT_CHECK(d->nsegs > 0 && d->nchunks > 0 && d->chunk > 0);
  for (int i = 0; i < d->nsegs; ++i) {
    const simt_bn_fold_seg& s = d->segs_host[i];
    SIMT_CHECK(s.C > 0);
    SIMT_CHECK(s.gamma && s.beta && s.running_mean && s.running_var && s.scale && s.shift);
  }
  BnFoldArgs a;
  a.segs = d->segs; a.chunks = (const int*)d->chunks; a.nsegs = d->nsegs; a.chunk = d->chunk; a.eps = d->eps;
  hipLaunchKernelGGL(bn_fold_multi_kernel, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
