// Exponential moving average of the weights (simt_amd/ema.py): the shadow model e follows the live tensors w,
//   e <- e + omd * (w - e),
// over a segment table, ONE launch per optimiser step.  Held bit for bit to the arithmetic contract of include/simt_hip.h (simt_ema_desc):
// IEEE float32, subtract, multiply and add each rounded on its own in that order, gradual underflow honoured, no FMA (the pragma below);
// omd == 1 copies 32-bit words.  tests/_ema_ref.py restates it in numpy.
//   ema_multi_kernel<COPY>  the sweep of multi_sweep.h at UNROLL = 2: where w and e are both 16-byte aligned at the chunk's start each lane issues
//                           TWO float4 loads of w and two of e before the first use and stores two float4 of e.  COPY (omd == 1) does not read e.
// Pure streaming: 8 bytes read + 4 written per element (4 + 4 for COPY), nothing is read twice: no LDS, no atomics, no scratch.  Plain loads
// and plain stores, the policies of sgd_multi_kernel beside which it is measured (DESIGN 7.12 says why not non-temporal).
#include "multi_sweep.h"

#pragma clang fp contract(off)

struct EmaSeg { const float* w; float* e; long long n; };
static_assert(sizeof(EmaSeg) == 24, "simt_ema_desc.segs");

struct EmaArgs {
  MultiTable<EmaSeg> t;
  float omd;
};

template <bool COPY>
__device__ __forceinline__ float ema1(float w, float e, float omd) {
  if (COPY) return w;                  // a register move: the word as loaded
  const float t = w - e;
  const float u = omd * t;
  return e + u;
}
template <bool COPY>
__device__ __forceinline__ float4 ema4(const float4& w, const float4& e, float omd) {
  return make_float4(ema1<COPY>(w.x, e.x, omd), ema1<COPY>(w.y, e.y, omd), ema1<COPY>(w.z, e.z, omd), ema1<COPY>(w.w, e.w, omd));
}

template <bool COPY>
struct EmaOp {
  typedef EmaSeg Seg;
  static constexpr bool VECTOR = true;
  template <class T> struct Vals { T w, e; };
  float omd;
  const float* w; float* e;      // of the chunk: set by bind()
  __device__ __forceinline__ long long count(const Seg& s) const { return s.n; }
  __device__ __forceinline__ void bind(const Seg& s, long long start) { w = s.w + start; e = s.e + start; }
  __device__ __forceinline__ bool aligned() const { return (((uintptr_t)w | (uintptr_t)e) & 15) == 0; }
  template <class T> __device__ __forceinline__ Vals<T> load(int i) const {
    return {*(const T*)(w + i), COPY ? multi_zero<T>() : *(const T*)(e + i)};
  }
  __device__ __forceinline__ void update(Vals<float>& v) const { v.e = ema1<COPY>(v.w, v.e, omd); }
  __device__ __forceinline__ void update(Vals<float4>& v) const { v.e = ema4<COPY>(v.w, v.e, omd); }
  template <class T> __device__ __forceinline__ void store(int i, const Vals<T>& v) const { *(T*)(e + i) = v.e; }
};

template <bool COPY>
__global__ __launch_bounds__(256) void ema_multi_kernel(EmaArgs a) { multi_sweep<2>(a.t, EmaOp<COPY>{a.omd}); }

extern "C" int simt_ema_multi(const simt_ema_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->segs && d->chunks && d->nchunks > 0 && d->chunk > 0);
  SIMT_CHECK(d->omd > 0.0f && d->omd <= 1.0f);      // (a NaN fails both comparisons)
  EmaArgs a;
  a.t = {(const EmaSeg*)d->segs, (const int*)d->chunks, d->nchunks, d->chunk, (const unsigned long long*)d->skip_if};
  a.omd = d->omd;
  if (d->omd == 1.0f)
    hipLaunchKernelGGL(ema_multi_kernel<true>, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ema_multi_kernel<false>, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
