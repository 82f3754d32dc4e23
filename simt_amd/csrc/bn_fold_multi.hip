// Every eval-mode BatchNorm fold of a plan in ONE launch (simt_amd/ema_teacher.py): the table-driven form of simt_bn_fold
// (bn_pool.hip), for a frozen plan whose weights move.  Held bit for bit to that kernel (include/simt_hip.h, simt_bn_fold_desc): the
// arithmetic below is bn_fold_kernel's source expression, and this file is compiled with the flags of bn_pool.hip and, like it, WITHOUT a
// floating-point contraction pragma -- the compiler's choice for `beta - rm * sc` (one fused multiply-add under the default setting) is
// the same in both.  Do not add `#pragma clang fp contract` here unless bn_pool.hip gets the same one.
//   bn_fold_multi_kernel  the sweep of multi_sweep.h without a 16-byte path: lane t serves channels index * chunk + t, + 256, ... of its
//                         segment.  16 bytes read and 8 written per channel, nothing read twice: no LDS, no atomics, no scratch; plain loads
//                         and plain stores.
#include "multi_sweep.h"

static_assert(sizeof(simt_bn_fold_seg) == 56, "simt_bn_fold_desc.segs");

struct BnFoldArgs {
  MultiTable<simt_bn_fold_seg> t;
  int nsegs;
  float eps;
};

struct BnFoldOp {
  typedef simt_bn_fold_seg Seg;
  static constexpr bool VECTOR = false;
  template <class T> struct Vals { T gamma, beta, rm, rv, sc, sh; };
  float eps;
  Seg s; long long c0;      // the segment and the chunk's first channel: set by bind()
  __device__ __forceinline__ long long count(const Seg& seg) const { return seg.C; }
  __device__ __forceinline__ void bind(const Seg& seg, long long start) { s = seg; c0 = start; }
  template <class T> __device__ __forceinline__ Vals<T> load(int i) const {
    return {s.gamma[c0 + i], s.beta[c0 + i], s.running_mean[c0 + i], s.running_var[c0 + i], 0.f, 0.f};
  }
  __device__ __forceinline__ void update(Vals<float>& v) const {
    float sc = v.gamma / sqrtf(v.rv + eps);
    v.sc = sc;
    v.sh = v.beta - v.rm * sc;
  }
  template <class T> __device__ __forceinline__ void store(int i, const Vals<T>& v) const {
    const long long c = c0 + i;
    s.scale[c] = v.sc;
    s.shift[c] = v.sh;
  }
};

__global__ __launch_bounds__(256) void bn_fold_multi_kernel(BnFoldArgs a) {
  if ((unsigned)a.t.chunks[2 * blockIdx.x] >= (unsigned)a.nsegs) return;      // (a table that names no segment writes nothing)
  multi_sweep<1>(a.t, BnFoldOp{a.eps});
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
  a.t = {d->segs, (const int*)d->chunks, d->nchunks, d->chunk, nullptr};
  a.nsegs = d->nsegs; a.eps = d->eps;
  hipLaunchKernelGGL(bn_fold_multi_kernel, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
