// Fused multi-tensor SGD (momentum, weight decay) with the reference's duplicate-parameter semantics.
//
// Replaces torch.optim.SGD(model.optim_parameters(args)).step() (tools/trainV2_simt.py:296-297,434).  The reference's
// parameter generator lists every layer3/layer4 tensor 3-4 times (model/deeplab_multi.py:211-217) and
// the optimiser it ran (single-tensor loop, foreach=False) applies the update once PER LISTING, sequentially, sharing one
// momentum buffer.  Here the `mult` listings of an element are replayed in registers, so the whole 43 M-parameter
// update is ONE launch instead of ~3000.
#include "multi_sweep.h"

// One 256-lane workgroup per (segment, chunk) entry: the sweep of multi_sweep.h, 16-byte loads and stores where p, g and buf are all aligned
// at the chunk's start.  16 bytes per element (3 loads, 2 stores; the first step does not load buf, a launch without momentum never stores it).
struct SgdSeg { float* p; const float* g; float* buf; long long n; int mult, group; };
static_assert(sizeof(SgdSeg) == 40, "simt_sgd_desc.segs");

struct SgdArgs {
  MultiTable<SgdSeg> t;
  float lr[4], wd[4];
  float momentum, dampening;
  int first_step;
};

struct SgdOp {
  typedef SgdSeg Seg;
  static constexpr bool VECTOR = true;
  template <class T> struct Vals { T p, g, buf; };
  const SgdArgs& a;
  float* p; const float* g; float* buf; float lr, wd; int mult;      // of the chunk: set by bind()
  __device__ __forceinline__ long long count(const Seg& s) const { return s.n; }
  __device__ __forceinline__ void bind(const Seg& s, long long start) {
    p = s.p + start; g = s.g + start; buf = s.buf + start;
    lr = a.lr[s.group]; wd = a.wd[s.group]; mult = s.mult;
  }
  __device__ __forceinline__ bool aligned() const { return (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) == 0; }
  template <class T> __device__ __forceinline__ Vals<T> load(int i) const {
    return {*(const T*)(p + i), *(const T*)(g + i), a.first_step ? multi_zero<T>() : *(const T*)(buf + i)};
  }
  // ONE update for both widths: the aligned and the unaligned run store the same bits
  __device__ __forceinline__ void upd(float& p, float g, float& buf) const {
    for (int r = 0; r < mult; ++r) {
      float d = wd != 0.f ? g + wd * p : g;
      if (a.momentum != 0.f) {
        buf = a.first_step ? d : a.momentum * buf + (1.f - a.dampening) * d;
        d = buf;
      }
      p = p - lr * d;
    }
  }
  __device__ __forceinline__ void update(Vals<float>& v) const { upd(v.p, v.g, v.buf); }
  __device__ __forceinline__ void update(Vals<float4>& v) const {
    upd(v.p.x, v.g.x, v.buf.x); upd(v.p.y, v.g.y, v.buf.y); upd(v.p.z, v.g.z, v.buf.z); upd(v.p.w, v.g.w, v.buf.w);
  }
  template <class T> __device__ __forceinline__ void store(int i, const Vals<T>& v) const {
    *(T*)(p + i) = v.p;
    if (a.momentum != 0.f) *(T*)(buf + i) = v.buf;
  }
};

__global__ __launch_bounds__(256) void sgd_multi_kernel(SgdArgs a) { multi_sweep<1>(a.t, SgdOp{a}); }

extern "C" int simt_sgd_multi(const simt_sgd_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->segs && d->chunks && d->nchunks > 0 && d->chunk > 0);
  SgdArgs a;
  a.t = {(const SgdSeg*)d->segs, (const int*)d->chunks, d->nchunks, d->chunk, (const unsigned long long*)d->skip_if};
  for (int i = 0; i < 4; ++i) { a.lr[i] = d->lr[i]; a.wd[i] = d->wd[i]; }
  a.momentum = d->momentum; a.dampening = d->dampening; a.first_step = d->first_step;
  hipLaunchKernelGGL(sgd_multi_kernel, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// Multi-tensor AdamW (decoupled weight decay), torch.optim.AdamW's single-tensor order, every tensor listed ONCE.
// The same sweep: 28 bytes per element (4 loads, 3 stores; the first step loads neither moment), no LDS, no atomics.
// step_size = lr / (1 - beta1^t), decay = 1 - lr * wd and bc2s = sqrt(1 - beta2^t) are formed by the caller in double and rounded once, as
// simt_adam_step_guarded does (ntm.hip).
struct AdamwSeg { float* p; const float* g; float* m; float* v; long long n; int group, pad; };
static_assert(sizeof(AdamwSeg) == 48, "simt_adamw_desc.segs");

struct AdamwArgs {
  MultiTable<AdamwSeg> t;
  float step_size[4], decay[4];
  float beta2, omb1, omb2, bc2s, eps;
  int first_step;
};

struct AdamwOp {
  typedef AdamwSeg Seg;
  static constexpr bool VECTOR = true;
  template <class T> struct Vals { T p, g, m, v; };
  const AdamwArgs& a;
  float* p; const float* g; float* m; float* v; float step_size, decay;      // of the chunk: set by bind()
  __device__ __forceinline__ long long count(const Seg& s) const { return s.n; }
  __device__ __forceinline__ void bind(const Seg& s, long long start) {
    p = s.p + start; g = s.g + start; m = s.m + start; v = s.v + start;
    step_size = a.step_size[s.group]; decay = a.decay[s.group];
  }
  __device__ __forceinline__ bool aligned() const { return (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0; }
  template <class T> __device__ __forceinline__ Vals<T> load(int i) const {
    Vals<T> r = {*(const T*)(p + i), *(const T*)(g + i), multi_zero<T>(), multi_zero<T>()};
    if (!a.first_step) {      // the first step creates the moments: whatever the buffers hold is not read
      r.m = *(const T*)(m + i);
      r.v = *(const T*)(v + i);
    }
    return r;
  }
  // ONE update for both widths: the aligned and the unaligned run store the same bits
  __device__ __forceinline__ void upd(float& p, float g, float& m, float& v) const {
    p = p * decay;
    // omb2 * g * g is formed in front of the branch: contraction is on in this file, and with both products inside `else` the compiler
    // may fuse either one into the sum -- it then chose differently per float4 lane.  From here only v * beta2 can fuse, the form the
    // kernel has always stored: fma(v, beta2, round(omb2 * g * g))  (tests/test_gpu_multi_chunk.py holds the two widths to one another)
    const float gg = a.omb2 * g * g;
    if (a.first_step) {
      m = g * a.omb1;
      v = gg;
    } else {
      m = m + (g - m) * a.omb1;
      v = v * a.beta2 + gg;
    }
    const float den = sqrtf(v) / a.bc2s + a.eps;
    p = p - step_size * (m / den);
  }
  __device__ __forceinline__ void update(Vals<float>& r) const { upd(r.p, r.g, r.m, r.v); }
  __device__ __forceinline__ void update(Vals<float4>& r) const {
    upd(r.p.x, r.g.x, r.m.x, r.v.x); upd(r.p.y, r.g.y, r.m.y, r.v.y); upd(r.p.z, r.g.z, r.m.z, r.v.z); upd(r.p.w, r.g.w, r.m.w, r.v.w);
  }
  template <class T> __device__ __forceinline__ void store(int i, const Vals<T>& r) const {
    *(T*)(p + i) = r.p; *(T*)(m + i) = r.m; *(T*)(v + i) = r.v;
  }
};

__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamwArgs a) { multi_sweep<1>(a.t, AdamwOp{a}); }

extern "C" int simt_adamw_multi(const simt_adamw_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->segs && d->chunks && d->nchunks > 0 && d->chunk > 0);
  SIMT_CHECK(d->beta1 >= 0.f && d->beta1 < 1.f && d->beta2 >= 0.f && d->beta2 < 1.f && d->eps > 0.f && __builtin_isfinite(d->eps));
  SIMT_CHECK(__builtin_isfinite(d->omb1) && __builtin_isfinite(d->omb2) && __builtin_isfinite(d->bc2s) && d->bc2s > 0.f);
  for (int i = 0; i < 4; ++i) SIMT_CHECK(__builtin_isfinite(d->step_size[i]) && __builtin_isfinite(d->decay[i]));
  AdamwArgs a;
  a.t = {(const AdamwSeg*)d->segs, (const int*)d->chunks, d->nchunks, d->chunk, (const unsigned long long*)d->skip_if};
  for (int i = 0; i < 4; ++i) { a.step_size[i] = d->step_size[i]; a.decay[i] = d->decay[i]; }
  a.beta2 = d->beta2; a.omb1 = d->omb1; a.omb2 = d->omb2; a.bc2s = d->bc2s; a.eps = d->eps;
  a.first_step = d->first_step;
  hipLaunchKernelGGL(adamw_multi_kernel, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// dst[i] (+)= src[i]   (tiny fp32 vectors: the bias of the fused ASPP GEMM is the sum of its branches' biases,
// model/deeplab_multi.py:115-119)
__global__ void vec_acc_kernel(float* dst, const float* src, int n, int accumulate) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = accumulate ? dst[i] + src[i] : src[i];
}
extern "C" int simt_vec_acc(float* dst, const float* src, int n, int accumulate, simt_stream_t stream) {
  SIMT_CHECK(dst && src && n > 0);
  hipLaunchKernelGGL(vec_acc_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, dst, src, n, accumulate);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
