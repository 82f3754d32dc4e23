// Exponential moving average of the weights (simt_amd/ema.py): the shadow model e follows the live tensors w,
//   e <- e + omd * (w - e),
// over a segment table, ONE launch per optimiser step.  Held bit for bit to the arithmetic contract of include/simt_hip.h (simt_ema_desc):
// IEEE float32, subtract, multiply and add each rounded on its own in that order, gradual underflow honoured, no FMA (the pragma below);
// omd == 1 copies 32-bit words.  tests/_ema_ref.py restates it in numpy.
//   ema_multi_kernel<COPY>  one workgroup of 256 lanes per chunk (the table of simt_sgd_multi: (segment, chunk index) pairs).  Where w and e
//                           are both 16-byte aligned at the chunk's start each lane issues TWO float4 loads of w and two of e (512 elements
//                           apart in the chunk's quads) before the first use and stores two float4 of e; one more quad for an odd count, then
//                           dwords for the tail and for a chunk that starts unaligned.  COPY (omd == 1) does not read e.
// Pure streaming: 8 bytes read + 4 written per element (4 + 4 for COPY), nothing is read twice: no LDS, no atomics, no scratch.  Plain loads
// and plain stores, the policies of sgd_multi_kernel beside which it is measured (DESIGN 7.12 says why not non-temporal).
#include "common.h"

#pragma clang fp contract(off)

struct EmaSeg {
  const float* w;
  float* e;
  long long n;
};

struct EmaArgs {
  const EmaSeg* segs;
  const int* chunks;  // [nchunks][2] = (segment, first element / chunk)
  int nchunks, chunk;
  float omd;
  const unsigned long long* skip_if;   // simt_ema_desc.skip_if: the launch changes nothing while this device word is non-zero
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
__global__ __launch_bounds__(256) void ema_multi_kernel(EmaArgs a) {
  const int ch = blockIdx.x;
  // a fused-BatchNorm launch of this step bailed out (conv2_epilogue.h): the optimisers skipped their updates, the shadow skips this one
  if (a.skip_if && __hip_atomic_load(a.skip_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) return;
  const EmaSeg s = a.segs[a.chunks[2 * ch]];
  const long long start = (long long)a.chunks[2 * ch + 1] * a.chunk;
  if (start >= s.n) return;
  const int n = (int)(s.n - start < (long long)a.chunk ? s.n - start : (long long)a.chunk);
  const float* w = s.w + start;
  float* e = s.e + start;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  int i0 = 0;
  if ((((uintptr_t)w | (uintptr_t)e) & 15) == 0) {
    const int n4 = n >> 2;
    const float4* w4 = (const float4*)w;
    float4* e4 = (float4*)e;
    int q = threadIdx.x;
    for (; q + 256 < n4; q += 512) {
      const float4 wa = w4[q], wb = w4[q + 256];
      const float4 ea = COPY ? z : e4[q], eb = COPY ? z : e4[q + 256];
      e4[q] = ema4<COPY>(wa, ea, a.omd);
      e4[q + 256] = ema4<COPY>(wb, eb, a.omd);
    }
    if (q < n4) {
      const float4 wa = w4[q];
      const float4 ea = COPY ? z : e4[q];
      e4[q] = ema4<COPY>(wa, ea, a.omd);
    }
    i0 = n4 << 2;
  }
  for (int i = i0 + threadIdx.x; i < n; i += 256) e[i] = ema1<COPY>(w[i], COPY ? 0.f : e[i], a.omd);
}

extern "C" int simt_ema_multi(const simt_ema_desc* d, simt_stream_t stream) {
  SIMT_CHECK(d && d->segs && d->chunks && d->nchunks > 0 && d->chunk > 0);
  SIMT_CHECK(d->omd > 0.0f && d->omd <= 1.0f);      // (a NaN fails both comparisons)
  EmaArgs a;
  a.segs = (const EmaSeg*)d->segs; a.chunks = (const int*)d->chunks; a.nchunks = d->nchunks; a.chunk = d->chunk;
  a.omd = d->omd;
  a.skip_if = (const unsigned long long*)d->skip_if;
  if (d->omd == 1.0f)
    hipLaunchKernelGGL(ema_multi_kernel<true>, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ema_multi_kernel<false>, dim3(d->nchunks), dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}
