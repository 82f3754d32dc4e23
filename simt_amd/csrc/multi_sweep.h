// The chunk sweep of the multi-tensor launches: simt_sgd_multi and simt_adamw_multi (optim.hip), simt_ema_multi (ema.hip) and
// simt_bn_fold_multi (bn_fold_multi.hip).  A launch walks a table of (segment, chunk index) pairs, one workgroup of 256 lanes per pair
// (simt_amd/multi_tensor.py builds the table).  What a workgroup does with its pair is written here ONCE: the `skip_if` early-out, the
// segment fetch, the clamp to the segment's end, the 16-byte path where the op's pointers allow it, and the dword tail.  What the launch
// computes is its Op; the sweep does no floating-point arithmetic: an op's bits are decided in its own file, under its contraction setting.
// An Op supplies
//   Seg                      its segment record (one element of the device table);
//   count(s)                 the segment's length in elements;
//   bind(s, start)           take the segment's pointers, advanced to the chunk's first element, and its per-segment constants;
//   VECTOR, aligned()        VECTOR = false: the op has no 16-byte path.  Otherwise aligned(): are ALL its pointers 16-byte aligned at the
//                            chunk's start?  (A flat gradient buffer packs tensors back to back, and a chunk size need not be a multiple of 4.)
//   load<T>(i), update(v), store<T>(i, v)
//                            T = float4 (i a multiple of 4) and T = float: element(s) i.. of the chunk.  Both widths must store the same bits.
// UNROLL = 2 issues the loads of two quads, 256 quads = 1024 elements apart, before the first use, then one more quad for an odd count: the
// loop shape measured for the EMA.  UNROLL = 1 is the plain loop.
#pragma once
#include "common.h"

template <class Seg>
struct MultiTable {
  const Seg* segs;
  const int* chunks;  // [nchunks][2] = (segment, chunk index inside the segment)
  int nchunks, chunk;
  const unsigned long long* skip_if;   // optional: the launch changes nothing while this device word is non-zero
};

template <class T> __device__ __forceinline__ T multi_zero();
template <> __device__ __forceinline__ float multi_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 multi_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// (`t` by value: taken by reference, the kernel's argument block stays a private copy until after the pass that proves the segment's pointers
// global, and every access becomes a flat_ one)
template <int UNROLL, class Op>
__device__ __forceinline__ void multi_sweep(const MultiTable<typename Op::Seg> t, Op op) {
  static_assert(UNROLL == 1 || UNROLL == 2, "one quad per trip, or a pair");
  // a fused-BatchNorm launch of this step bailed out (its polling timed out: conv2_epilogue.h): nothing of this step is applied
  if (t.skip_if && __hip_atomic_load(t.skip_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) return;
  const typename Op::Seg s = t.segs[t.chunks[2 * blockIdx.x]];
  const long long start = (long long)t.chunks[2 * blockIdx.x + 1] * t.chunk, left = op.count(s) - start;
  if (start < 0 || left <= 0) return;
  const int n = (int)(left < (long long)t.chunk ? left : (long long)t.chunk);
  op.bind(s, start);
  int i0 = 0;
  if constexpr (Op::VECTOR) {
    if (op.aligned()) {
      const int n4 = n >> 2;
      auto put = [&](int q, auto&& v) { op.update(v); op.template store<float4>(q << 2, v); };
      int q = threadIdx.x;
      for (; q + 256 * (UNROLL - 1) < n4; q += 256 * UNROLL) {
        auto a = op.template load<float4>(q << 2);
        if constexpr (UNROLL == 1) put(q, a);
        else { auto b = op.template load<float4>((q + 256) << 2); put(q, a); put(q + 256, b); }
      }
      if (UNROLL == 2 && q < n4) put(q, op.template load<float4>(q << 2));
      i0 = n4 << 2;
    }
  }
  for (int i = i0 + threadIdx.x; i < n; i += 256) {
    auto v = op.template load<float>(i);
    op.update(v);
    op.template store<float>(i, v);
  }
}
