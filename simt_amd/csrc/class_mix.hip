// ClassMix (Olsson et al., WACV'21) on a finished batch (simt_amd/data/class_mix.py): item i receives, from its partner j, the pixels
// -- labels included -- of half of the classes that occur in lab[j].  Pure selection: no arithmetic touches a value.  Two streaming
// kernels in the style of cache_gather_kernel (csrc/dataset_cache.hip): descriptor by value in the kernel-argument segment, 4 consecutive
// pixels per lane, flat over h*w, 16-byte loads and stores when h*w % 4 == 0 (every plane and label row then starts on a 16-byte
// boundary), dwords / qwords otherwise, one lane takes the h*w % 4 tail.
//   label_presence_kernel  grid (PARTS, B): workgroup (g, b) ORs 1u << l over its strided share of item b's valid labels and lane 0
//                          stores ONE word, part[b][g] -- every word is written on every call: no atomics, nothing to zero.
//   class_mix_kernel       grid (quads / 256, B): every wave builds the paste mask S_j from the partner's PARTS words and the item's
//                          rank permutation (a few dozen instructions, no LDS, no barrier), then selects quad by quad.
// Byte floor per pixel: the mix writes 12 + 8 bytes and reads at least 8 (lab[j]) + 12 (one image), plus 8 more (lab[i]) where the pixel
// is not pasted: 40-48 bytes, 94-113 MB at B = 4, 768 x 768.  Presence reads 8 bytes per pixel: 19 MB there.  A quad whose four pixels
// agree loads one source only, so the floor is what the kernel moves except on class boundaries.
#include "common.h"

typedef __attribute__((ext_vector_type(2))) long long i64x2;

__device__ __forceinline__ uint32_t label_bit(long long l, int C) { return (l >= 0 && l < C) ? (1u << (int)l) : 0u; }

template <bool VEC>
__global__ __launch_bounds__(256) void label_presence_kernel(const long long* __restrict__ lab, long HW, int C, uint32_t* __restrict__ part) {
  const int b = blockIdx.y;
  const long long* __restrict__ l = lab + (long)b * HW;
  const long nquad = HW >> 2;
  const long last = (HW & 3) ? nquad : nquad - 1;          // lane index `nquad` takes the tail, when there is one
  uint32_t bits = 0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q <= last; q += (long)SIMT_CLASS_MIX_PARTS * 256) {
    if (q < nquad) {
      const long p = q << 2;
      long long v0, v1, v2, v3;
      if (VEC) {
        const i64x2 u = *(const i64x2*)(l + p), v = *(const i64x2*)(l + p + 2);
        v0 = u.x; v1 = u.y; v2 = v.x; v3 = v.y;
      } else {
        v0 = l[p]; v1 = l[p + 1]; v2 = l[p + 2]; v3 = l[p + 3];
      }
      bits |= label_bit(v0, C) | label_bit(v1, C) | label_bit(v2, C) | label_bit(v3, C);
    } else {
      for (long p = nquad << 2; p < HW; ++p) bits |= label_bit(l[p], C);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, o, 64);
  __shared__ uint32_t wave_bits[4];
  if ((threadIdx.x & 63) == 0) wave_bits[threadIdx.x >> 6] = bits;
  __syncthreads();
  if (threadIdx.x == 0) part[b * SIMT_CLASS_MIX_PARTS + blockIdx.x] = wave_bits[0] | wave_bits[1] | wave_bits[2] | wave_bits[3];
}

extern "C" int simt_label_presence(const long long* lab, int B, long hw, int n_classes, uint32_t* part, simt_stream_t stream) {
  SIMT_CHECK(lab && part && ((uintptr_t)lab & 15) == 0 && ((uintptr_t)part & 3) == 0);
  SIMT_CHECK(B > 0 && B <= SIMT_CLASS_MIX_MAX && hw > 0 && hw < (1L << 31));
  SIMT_CHECK(n_classes >= 1 && n_classes <= SIMT_CLASS_MIX_CLASSES);
  const dim3 grid(SIMT_CLASS_MIX_PARTS, (unsigned)B);
  if ((hw & 3) == 0)
    hipLaunchKernelGGL((label_presence_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, lab, hw, n_classes, part);
  else
    hipLaunchKernelGGL((label_presence_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, lab, hw, n_classes, part);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// The paste mask of item i, the same word in every lane.  Lane r < C plays RANK r: a wave-uniform walk over the classes (rank[i][c] is a
// scalar load from the kernel arguments) tells it which class holds its rank; the ballot of "my class is present" then is the present
// classes in rank order, and the class of rank r is chosen when fewer than k present ones rank below it.
// `present`: this lane's share of the partner's presence words (the OR over the wave is the partner's classes); `row`: rank[i], 32 bytes
// at a 4-byte boundary of the descriptor: 8 scalar dwords.
__device__ __forceinline__ uint32_t paste_mask_of(uint32_t present, const uint32_t* row, int C) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) present |= (uint32_t)__shfl_xor((int)present, o, 64);
  present &= C >= 32 ? 0xffffffffu : ((1u << C) - 1u);
  const int k = (__popc(present) + 1) >> 1;
  int cls = -1;
#pragma unroll
  for (int c = 0; c < SIMT_CLASS_MIX_CLASSES; ++c)
    if (c < C && (int)((row[c >> 2] >> (8 * (c & 3))) & 255u) == lane) cls = c;
  const bool here = cls >= 0 && ((present >> cls) & 1u);
  const unsigned long long order = __ballot(here);                       // bit r: the class of rank r is present
  const int below = __popcll(order & ((1ull << lane) - 1ull));
  uint32_t mask = (here && below < k) ? (1u << cls) : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mask |= (uint32_t)__shfl_xor((int)mask, o, 64);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)mask);
}

__device__ __forceinline__ uint32_t paste_mask(const simt_class_mix_desc& d, int i, int j) {
  return paste_mask_of(d.part[j * SIMT_CLASS_MIX_PARTS + (threadIdx.x & 63)], (const uint32_t*)d.rank[i], d.n_classes);   // PARTS = 64 = one word per lane
}

__device__ __forceinline__ bool pasted(long long l, int C, uint32_t mask) { return l >= 0 && l < C && ((mask >> (int)l) & 1u); }

// One lane: pixels p .. p+3 of item i = blockIdx.y.  lab[j] is read always (when apply[i]); a quad whose four decisions agree reads one
// source only, a mixed quad reads both and selects.  Values travel as integer words.
// ITEMS_: empty for simt_class_mix (name and code as before the flavour existed); {true} for simt_class_mix_items, which also writes the item
// each pixel came from, item_out[i][p] = m ? j : i -- one byte per pixel on top of the 40-48: a quad's four bytes leave as one dword when
// VEC (h*w % 4 == 0 and a 4-byte aligned base: every item's row then starts on a dword), as bytes in the unaligned flavour and the tail.
template <bool VEC, bool... ITEMS_>
__global__ __launch_bounds__(256) void class_mix_kernel(const simt_class_mix_desc d, uint8_t* __restrict__ item_out) {
  constexpr bool ITEMS = (false || ... || ITEMS_);
  const int i = blockIdx.y;
  const int apply = d.apply[i];
  const int j = d.partner[i];
  const int C = d.n_classes;
  const long HW = (long)d.h * d.w;
  const long nquad = HW >> 2;
  const uint32_t* __restrict__ xi = (const uint32_t*)d.x + (long)i * 3 * HW;
  const long long* __restrict__ li = d.lab + (long)i * HW;
  uint32_t* __restrict__ xo = (uint32_t*)d.x_out + (long)i * 3 * HW;
  long long* __restrict__ lo = d.lab_out + (long)i * HW;
  uint8_t* __restrict__ io = ITEMS ? item_out + (long)i * HW : nullptr;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (!apply) {                                          // a straight copy of item i (wave-uniform branch): the partner is not read
    if (q < nquad) {
      const long p = q << 2;
      if (VEC) {
        *(i64x2*)(lo + p) = *(const i64x2*)(li + p);
        *(i64x2*)(lo + p + 2) = *(const i64x2*)(li + p + 2);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) *(uint4*)(xo + ch * HW + p) = *(const uint4*)(xi + ch * HW + p);
        if (ITEMS) *(uint32_t*)(io + p) = (uint32_t)i * 0x01010101u;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lo[p + e] = li[p + e];
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) xo[ch * HW + p + e] = xi[ch * HW + p + e];
          if (ITEMS) io[p + e] = (uint8_t)i;
        }
      }
    } else if (q == nquad) {
      for (long p = nquad << 2; p < HW; ++p) {
        lo[p] = li[p];
        for (int ch = 0; ch < 3; ++ch) xo[ch * HW + p] = xi[ch * HW + p];
        if (ITEMS) io[p] = (uint8_t)i;
      }
    }
    return;
  }
  const uint32_t mask = paste_mask(d, i, j);
  const uint32_t* __restrict__ xj = (const uint32_t*)d.x + (long)j * 3 * HW;
  const long long* __restrict__ lj = d.lab + (long)j * HW;
  if (q < nquad) {
    const long p = q << 2;
    long long a[4];                                      // the partner's labels, then the output's
    if (VEC) {
      const i64x2 u = *(const i64x2*)(lj + p), v = *(const i64x2*)(lj + p + 2);
      a[0] = u.x; a[1] = u.y; a[2] = v.x; a[3] = v.y;
    } else {
      a[0] = lj[p]; a[1] = lj[p + 1]; a[2] = lj[p + 2]; a[3] = lj[p + 3];
    }
    const bool m0 = pasted(a[0], C, mask), m1 = pasted(a[1], C, mask), m2 = pasted(a[2], C, mask), m3 = pasted(a[3], C, mask);
    const bool all = m0 && m1 && m2 && m3, none = !(m0 || m1 || m2 || m3);
    if (!all) {
      long long o0, o1, o2, o3;
      if (VEC) {
        const i64x2 u = *(const i64x2*)(li + p), v = *(const i64x2*)(li + p + 2);
        o0 = u.x; o1 = u.y; o2 = v.x; o3 = v.y;
      } else {
        o0 = li[p]; o1 = li[p + 1]; o2 = li[p + 2]; o3 = li[p + 3];
      }
      a[0] = m0 ? a[0] : o0; a[1] = m1 ? a[1] : o1; a[2] = m2 ? a[2] : o2; a[3] = m3 ? a[3] : o3;
    }
    if (VEC) {
      const i64x2 u = {a[0], a[1]}, v = {a[2], a[3]};
      *(i64x2*)(lo + p) = u;
      *(i64x2*)(lo + p + 2) = v;
    } else {
      lo[p] = a[0]; lo[p + 1] = a[1]; lo[p + 2] = a[2]; lo[p + 3] = a[3];
    }
    if (ITEMS) {
      const uint32_t b0 = m0 ? j : i, b1 = m1 ? j : i, b2 = m2 ? j : i, b3 = m3 ? j : i;
      if (VEC) {
        *(uint32_t*)(io + p) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
      } else {
        io[p] = (uint8_t)b0; io[p + 1] = (uint8_t)b1; io[p + 2] = (uint8_t)b2; io[p + 3] = (uint8_t)b3;
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const long o = ch * HW + p;
      uint4 r;
      if (VEC) {
        if (all) {
          r = *(const uint4*)(xj + o);
        } else if (none) {
          r = *(const uint4*)(xi + o);
        } else {
          const uint4 s = *(const uint4*)(xj + o), t = *(const uint4*)(xi + o);
          r = make_uint4(m0 ? s.x : t.x, m1 ? s.y : t.y, m2 ? s.z : t.z, m3 ? s.w : t.w);
        }
        *(uint4*)(xo + o) = r;
      } else {
        r.x = m0 ? xj[o] : xi[o];
        r.y = m1 ? xj[o + 1] : xi[o + 1];
        r.z = m2 ? xj[o + 2] : xi[o + 2];
        r.w = m3 ? xj[o + 3] : xi[o + 3];
        xo[o] = r.x; xo[o + 1] = r.y; xo[o + 2] = r.z; xo[o + 3] = r.w;
      }
    }
  } else if (q == nquad) {                               // scalar tail: h*w % 4 pixels
    for (long p = nquad << 2; p < HW; ++p) {
      const long long l = lj[p];
      const bool m = pasted(l, C, mask);
      lo[p] = m ? l : li[p];
      for (int ch = 0; ch < 3; ++ch) xo[ch * HW + p] = m ? xj[ch * HW + p] : xi[ch * HW + p];
      if (ITEMS) io[p] = (uint8_t)(m ? j : i);
    }
  }
}

static int class_mix_launch(const simt_class_mix_desc* d, uint8_t* item_out, bool items, simt_stream_t stream) {
  SIMT_CHECK(d && d->x && d->lab && d->x_out && d->lab_out && d->part);
  SIMT_CHECK(!items || (item_out && ((uintptr_t)item_out & 3) == 0));
  SIMT_CHECK(((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->lab & 15) == 0 && ((uintptr_t)d->x_out & 15) == 0 && ((uintptr_t)d->lab_out & 15) == 0);
  SIMT_CHECK(((uintptr_t)d->part & 3) == 0 && (const void*)d->x != (const void*)d->x_out && (const void*)d->lab != (const void*)d->lab_out);
  SIMT_CHECK(d->B > 0 && d->B <= SIMT_CLASS_MIX_MAX && d->h > 0 && d->w > 0);
  SIMT_CHECK(d->n_classes >= 1 && d->n_classes <= SIMT_CLASS_MIX_CLASSES);
  const long HW = (long)d->h * d->w;
  SIMT_CHECK(HW < (1L << 31));
  for (int b = 0; b < d->B; ++b) {
    SIMT_CHECK(d->partner[b] < d->B);
    for (int c = 0; c < d->n_classes; ++c) SIMT_CHECK(d->rank[b][c] < d->n_classes);
  }
  const long lanes = (HW >> 2) + ((HW & 3) ? 1 : 0);
  const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)d->B);
  const bool vec = (HW & 3) == 0;
  if (vec && !items)
    hipLaunchKernelGGL((class_mix_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, *d, (uint8_t*)nullptr);
  else if (!items)
    hipLaunchKernelGGL((class_mix_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, *d, (uint8_t*)nullptr);
  else if (vec)
    hipLaunchKernelGGL((class_mix_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, *d, item_out);
  else
    hipLaunchKernelGGL((class_mix_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, *d, item_out);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_class_mix(const simt_class_mix_desc* d, simt_stream_t stream) { return class_mix_launch(d, nullptr, false, stream); }

// simt_class_mix plus the item map (the weak-view teacher gathers its predictions through it): x_out / lab_out bit for bit as above.
extern "C" int simt_class_mix_items(const simt_class_mix_desc* d, uint8_t* item_out, simt_stream_t stream) {
  return class_mix_launch(d, item_out, true, stream);
}

// ---- simt_class_mix_u8: the mix BEHIND a teacher, inside the warm-up trainers.  simt_class_mix's selection over BYTE
// labels (simt_online_label_u8's lab8) and that launch's presence words (part[b][g], `rows` of them per item), written straight into the
// buffers the student's forward and the head kernels read: x_out fp32, lab_out int64.  Byte floor per pixel: 12 + 8 written, 12 + 1-2
// read = 33-34, against 40-48 of simt_class_mix, 8 of simt_label_presence and 24 + 16 of the copies into the trainer's buffers.
// A lane takes MIX8_QPT quads, 256 * 4 pixels apart (every access of a wave stays one contiguous run), so the wave's paste mask -- the OR
// of the partner's row of `part`, rows / 64 contiguous loads per lane from L2, then paste_mask_of: no LDS, no barrier -- is paid once per
// 512 pixels.  Measured on MI355X (profiles/online_mix.txt): 2 quads per lane over item-major words 17.8 / 16.7 us (B = 4 768 x 768 / B = 8
// 512 x 512); 1 quad 21.8 / 16.6; 4 quads 20.4 / 19.4 (too few waves); the words workgroup-major ([g][b]: a wave's loads B * 4 bytes apart)
// 20.4 / 19.6 at 4 quads, 22.0 / 19.9 at 1.  The quad's four labels are ONE dword when h * w % 4 == 0; a quad whose four decisions agree
// reads one image source.
constexpr int MIX8_QPT = 2;

__device__ __forceinline__ bool pasted8(uint32_t l, int C, uint32_t mask) { return l < (uint32_t)C && ((mask >> (l & 31u)) & 1u); }

template <bool VEC>
__device__ __forceinline__ uint32_t load_labels4(const uint8_t* __restrict__ l, long p) {
  if (VEC) return *(const uint32_t*)(l + p);
  return (uint32_t)l[p] | ((uint32_t)l[p + 1] << 8) | ((uint32_t)l[p + 2] << 16) | ((uint32_t)l[p + 3] << 24);
}

// ItemOut: empty for simt_class_mix_u8 (name, arguments and code as before the flavour existed); {uint8_t*} for simt_class_mix_u8_items,
// which also writes the item each pixel came from (class_mix_kernel's item_out: one dword per quad when VEC, bytes otherwise and in the tail).
__device__ __forceinline__ uint8_t* first_item_out() { return nullptr; }
__device__ __forceinline__ uint8_t* first_item_out(uint8_t* p) { return p; }

template <bool VEC, class... ItemOut>
__global__ __launch_bounds__(256) void class_mix_u8_kernel(const simt_class_mix_u8_desc d, ItemOut... item_out) {
  constexpr bool ITEMS = sizeof...(ItemOut) > 0;
  const int i = blockIdx.y;
  const int apply = d.apply[i];
  const int C = d.n_classes;
  const long HW = (long)d.h * d.w;
  const long nquad = HW >> 2;
  const uint32_t* __restrict__ xi = (const uint32_t*)d.x + (long)i * 3 * HW;
  const uint8_t* __restrict__ li = d.lab8 + (long)i * HW;
  uint32_t* __restrict__ xo = (uint32_t*)d.x_out + (long)i * 3 * HW;
  long long* __restrict__ lo = d.lab_out + (long)i * HW;
  // apply[i] == 0 (wave-uniform): mask 0 over the item's own labels -- an image copy and a widening copy, the partner is not read
  const uint32_t* __restrict__ xj = xi;
  const uint8_t* __restrict__ lj = li;
  uint32_t mask = 0u;
  uint8_t* __restrict__ io = ITEMS ? first_item_out(item_out...) + (long)i * HW : nullptr;
  const uint32_t jj = apply ? d.partner[i] : (uint32_t)i;      // (ITEMS: the item a pasted pixel came from)
  if (apply) {
    const int j = d.partner[i];
    uint32_t present = 0u;
    for (int g = threadIdx.x & 63; g < d.rows; g += 64) present |= d.part[(long)j * d.rows + g];
    mask = paste_mask_of(present, (const uint32_t*)d.rank[i], C);
    xj = (const uint32_t*)d.x + (long)j * 3 * HW;
    lj = d.lab8 + (long)j * HW;
  }
  for (int r = 0; r < MIX8_QPT; ++r) {
    const long q = ((long)blockIdx.x * MIX8_QPT + r) * 256 + threadIdx.x;
    if (q < nquad) {
      const long p = q << 2;
      uint32_t a = load_labels4<VEC>(lj, p);             // the partner's four labels, then the output's
      const bool m0 = pasted8(a & 255u, C, mask), m1 = pasted8((a >> 8) & 255u, C, mask), m2 = pasted8((a >> 16) & 255u, C, mask),
                 m3 = pasted8(a >> 24, C, mask);
      const bool all = m0 && m1 && m2 && m3, none = !(m0 || m1 || m2 || m3);
      if (apply && !all) {
        const uint32_t sel = (m0 ? 0xffu : 0u) | (m1 ? 0xff00u : 0u) | (m2 ? 0xff0000u : 0u) | (m3 ? 0xff000000u : 0u);
        a = (a & sel) | (load_labels4<VEC>(li, p) & ~sel);
      }
      if (VEC) {
        const i64x2 u = {(long long)(a & 255u), (long long)((a >> 8) & 255u)}, v = {(long long)((a >> 16) & 255u), (long long)(a >> 24)};
        *(i64x2*)(lo + p) = u;
        *(i64x2*)(lo + p + 2) = v;
      } else {
        lo[p] = (long long)(a & 255u); lo[p + 1] = (long long)((a >> 8) & 255u);
        lo[p + 2] = (long long)((a >> 16) & 255u); lo[p + 3] = (long long)(a >> 24);
      }
      if (ITEMS) {
        const uint32_t b0 = m0 ? jj : (uint32_t)i, b1 = m1 ? jj : (uint32_t)i, b2 = m2 ? jj : (uint32_t)i, b3 = m3 ? jj : (uint32_t)i;
        if (VEC) {
          *(uint32_t*)(io + p) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        } else {
          io[p] = (uint8_t)b0; io[p + 1] = (uint8_t)b1; io[p + 2] = (uint8_t)b2; io[p + 3] = (uint8_t)b3;
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const long o = ch * HW + p;
        if (VEC) {
          uint4 v;
          if (all) {
            v = *(const uint4*)(xj + o);
          } else if (none) {
            v = *(const uint4*)(xi + o);
          } else {
            const uint4 s = *(const uint4*)(xj + o), t = *(const uint4*)(xi + o);
            v = make_uint4(m0 ? s.x : t.x, m1 ? s.y : t.y, m2 ? s.z : t.z, m3 ? s.w : t.w);
          }
          *(uint4*)(xo + o) = v;
        } else {
          const uint32_t v0 = m0 ? xj[o] : xi[o], v1 = m1 ? xj[o + 1] : xi[o + 1], v2 = m2 ? xj[o + 2] : xi[o + 2],
                         v3 = m3 ? xj[o + 3] : xi[o + 3];
          xo[o] = v0; xo[o + 1] = v1; xo[o + 2] = v2; xo[o + 3] = v3;
        }
      }
    } else if (q == nquad) {                             // scalar tail: h*w % 4 pixels
      for (long p = nquad << 2; p < HW; ++p) {
        const uint32_t l = lj[p];
        const bool m = pasted8(l, C, mask);
        lo[p] = (long long)(m ? l : (uint32_t)li[p]);
        for (int ch = 0; ch < 3; ++ch) xo[ch * HW + p] = m ? xj[ch * HW + p] : xi[ch * HW + p];
        if (ITEMS) io[p] = (uint8_t)(m ? jj : (uint32_t)i);
      }
    }
  }
}

static int class_mix_u8_launch(const simt_class_mix_u8_desc* d, uint8_t* item_out, bool items, simt_stream_t stream) {
  SIMT_CHECK(d && d->x && d->lab8 && d->x_out && d->lab_out && d->part);
  SIMT_CHECK(!items || (item_out && ((uintptr_t)item_out & 3) == 0));
  SIMT_CHECK(((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->lab8 & 15) == 0 && ((uintptr_t)d->x_out & 15) == 0 && ((uintptr_t)d->lab_out & 15) == 0);
  SIMT_CHECK(((uintptr_t)d->part & 3) == 0);
  SIMT_CHECK(d->B >= 2 && d->B <= SIMT_CLASS_MIX_MAX && d->h > 0 && d->w > 0);
  SIMT_CHECK(d->n_classes >= 1 && d->n_classes <= SIMT_CLASS_MIX_CLASSES);
  SIMT_CHECK(d->rows >= 1 && d->rows <= SIMT_ONLINE_LABEL_MAX_PARTS);
  const long HW = (long)d->h * d->w;
  SIMT_CHECK(HW < (1L << 31));
  const uintptr_t x0 = (uintptr_t)d->x, y0 = (uintptr_t)d->x_out, xbytes = (uintptr_t)d->B * 3 * HW * sizeof(float);
  SIMT_CHECK(x0 + xbytes <= y0 || y0 + xbytes <= x0);    // x_out does not overlap x: item i reads its partner's image
  for (int b = 0; b < d->B; ++b) {
    SIMT_CHECK(d->partner[b] < d->B);
    for (int c = 0; c < d->n_classes; ++c) SIMT_CHECK(d->rank[b][c] < d->n_classes);
  }
  const long lanes = (HW >> 2) + ((HW & 3) ? 1 : 0);
  const dim3 grid((unsigned)((lanes + 256 * MIX8_QPT - 1) / (256 * MIX8_QPT)), (unsigned)d->B);
  const bool vec = (HW & 3) == 0;
  if (vec && !items)
    hipLaunchKernelGGL((class_mix_u8_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else if (!items)
    hipLaunchKernelGGL((class_mix_u8_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else if (vec)
    hipLaunchKernelGGL((class_mix_u8_kernel<true, uint8_t*>), grid, dim3(256), 0, (hipStream_t)stream, *d, item_out);
  else
    hipLaunchKernelGGL((class_mix_u8_kernel<false, uint8_t*>), grid, dim3(256), 0, (hipStream_t)stream, *d, item_out);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_class_mix_u8(const simt_class_mix_u8_desc* d, simt_stream_t stream) { return class_mix_u8_launch(d, nullptr, false, stream); }

// simt_class_mix_u8 plus the item map (the weighted head reads a pasted pixel's weight from its partner's entry): x_out /
// lab_out bit for bit as above -- same grid, same paste mask.
extern "C" int simt_class_mix_u8_items(const simt_class_mix_u8_desc* d, uint8_t* item_out, simt_stream_t stream) {
  return class_mix_u8_launch(d, item_out, true, stream);
}

// ---- simt_source_mix: the cross-domain mix of DACS, behind a teacher and beside a labelled source batch.  class_mix_u8_kernel's
// shape -- MIX8_QPT quads per lane 256 * 4 pixels apart, the paste mask once per wave, a quad whose four decisions agree reads one image --
// with the pasted side a SOURCE item: its image xs[i], its ground truth labs[i] as int64 (what the loader hands out: there is no byte copy
// of it) and its presence words from simt_label_presence, SIMT_CLASS_MIX_PARTS = 64 of them: one contiguous word per lane, no loop.  The
// decision needs the quad's four source labels (32 bytes); the target's label dword is read only where a pixel is not pasted.  Byte floor per
// pixel: 12 + 8 written, 12 + 8 read, + 1 where not pasted = 40-41; the item map adds one.  apply[i] == 0 (workgroup-uniform): mask 0 and no
// source pointer is dereferenced.
template <bool VEC, class... ItemOut>
__global__ __launch_bounds__(256) void source_mix_kernel(const simt_source_mix_desc d, ItemOut... item_out) {
  constexpr bool ITEMS = sizeof...(ItemOut) > 0;
  const int i = blockIdx.y;
  const int apply = d.apply[i];
  const int C = d.n_classes;
  const long HW = (long)d.h * d.w;
  const long nquad = HW >> 2;
  const uint32_t* __restrict__ xs = (const uint32_t*)d.xs + (long)i * 3 * HW;
  const uint32_t* __restrict__ xt = (const uint32_t*)d.xt + (long)i * 3 * HW;
  const long long* __restrict__ ls = d.labs + (long)i * HW;
  const uint8_t* __restrict__ lt = d.lab8 + (long)i * HW;
  uint32_t* __restrict__ xo = (uint32_t*)d.x_out + (long)i * 3 * HW;
  long long* __restrict__ lo = d.lab_out + (long)i * HW;
  uint8_t* __restrict__ io = ITEMS ? first_item_out(item_out...) + (long)i * HW : nullptr;
  const uint32_t ti = (uint32_t)i, si = (uint32_t)(d.B + i);      // (ITEMS: the table entries of a target and of a pasted pixel; B + i <= 63)
  uint32_t mask = 0u;
  if (apply) mask = paste_mask_of(d.part_s[i * SIMT_CLASS_MIX_PARTS + (threadIdx.x & 63)], (const uint32_t*)d.rank[i], C);
  for (int r = 0; r < MIX8_QPT; ++r) {
    const long q = ((long)blockIdx.x * MIX8_QPT + r) * 256 + threadIdx.x;
    if (q < nquad) {
      const long p = q << 2;
      long long a[4] = {0, 0, 0, 0};                     // the source's four labels, then the output's
      bool m0 = false, m1 = false, m2 = false, m3 = false;
      if (apply) {
        if (VEC) {
          const i64x2 u = *(const i64x2*)(ls + p), v = *(const i64x2*)(ls + p + 2);
          a[0] = u.x; a[1] = u.y; a[2] = v.x; a[3] = v.y;
        } else {
          a[0] = ls[p]; a[1] = ls[p + 1]; a[2] = ls[p + 2]; a[3] = ls[p + 3];
        }
        m0 = pasted(a[0], C, mask); m1 = pasted(a[1], C, mask); m2 = pasted(a[2], C, mask); m3 = pasted(a[3], C, mask);
      }
      const bool all = m0 && m1 && m2 && m3, none = !(m0 || m1 || m2 || m3);
      if (!all) {
        const uint32_t t = load_labels4<VEC>(lt, p);
        a[0] = m0 ? a[0] : (long long)(t & 255u); a[1] = m1 ? a[1] : (long long)((t >> 8) & 255u);
        a[2] = m2 ? a[2] : (long long)((t >> 16) & 255u); a[3] = m3 ? a[3] : (long long)(t >> 24);
      }
      if (VEC) {
        const i64x2 u = {a[0], a[1]}, v = {a[2], a[3]};
        *(i64x2*)(lo + p) = u;
        *(i64x2*)(lo + p + 2) = v;
      } else {
        lo[p] = a[0]; lo[p + 1] = a[1]; lo[p + 2] = a[2]; lo[p + 3] = a[3];
      }
      if (ITEMS) {
        const uint32_t b0 = m0 ? si : ti, b1 = m1 ? si : ti, b2 = m2 ? si : ti, b3 = m3 ? si : ti;
        if (VEC) {
          *(uint32_t*)(io + p) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        } else {
          io[p] = (uint8_t)b0; io[p + 1] = (uint8_t)b1; io[p + 2] = (uint8_t)b2; io[p + 3] = (uint8_t)b3;
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const long o = ch * HW + p;
        if (VEC) {
          uint4 v;
          if (all) {
            v = *(const uint4*)(xs + o);
          } else if (none) {
            v = *(const uint4*)(xt + o);
          } else {
            const uint4 s = *(const uint4*)(xs + o), t = *(const uint4*)(xt + o);
            v = make_uint4(m0 ? s.x : t.x, m1 ? s.y : t.y, m2 ? s.z : t.z, m3 ? s.w : t.w);
          }
          *(uint4*)(xo + o) = v;
        } else if (none) {                               // (also apply[i] == 0: the source is not read)
          const uint32_t v0 = xt[o], v1 = xt[o + 1], v2 = xt[o + 2], v3 = xt[o + 3];
          xo[o] = v0; xo[o + 1] = v1; xo[o + 2] = v2; xo[o + 3] = v3;
        } else {
          const uint32_t v0 = m0 ? xs[o] : xt[o], v1 = m1 ? xs[o + 1] : xt[o + 1], v2 = m2 ? xs[o + 2] : xt[o + 2],
                         v3 = m3 ? xs[o + 3] : xt[o + 3];
          xo[o] = v0; xo[o + 1] = v1; xo[o + 2] = v2; xo[o + 3] = v3;
        }
      }
    } else if (q == nquad) {                             // scalar tail: h*w % 4 pixels
      for (long p = nquad << 2; p < HW; ++p) {
        const long long l = apply ? ls[p] : 255;
        const bool m = pasted(l, C, mask);
        lo[p] = m ? l : (long long)lt[p];
        for (int ch = 0; ch < 3; ++ch) xo[ch * HW + p] = m ? xs[ch * HW + p] : xt[ch * HW + p];
        if (ITEMS) io[p] = (uint8_t)(m ? si : ti);
      }
    }
  }
}

static bool ranges_overlap(const void* a, const void* b, uintptr_t bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return !(a0 + bytes <= b0 || b0 + bytes <= a0);
}

static int source_mix_launch(const simt_source_mix_desc* d, uint8_t* item_out, bool items, simt_stream_t stream) {
  SIMT_CHECK(d && d->xs && d->labs && d->part_s && d->xt && d->lab8 && d->x_out && d->lab_out);
  SIMT_CHECK(!items || (item_out && ((uintptr_t)item_out & 3) == 0));
  SIMT_CHECK(((uintptr_t)d->xs & 15) == 0 && ((uintptr_t)d->labs & 15) == 0 && ((uintptr_t)d->xt & 15) == 0 && ((uintptr_t)d->lab8 & 15) == 0);
  SIMT_CHECK(((uintptr_t)d->x_out & 15) == 0 && ((uintptr_t)d->lab_out & 15) == 0 && ((uintptr_t)d->part_s & 3) == 0);
  SIMT_CHECK(d->B >= 1 && d->B <= SIMT_CLASS_MIX_MAX && d->h > 0 && d->w > 0);
  SIMT_CHECK(d->n_classes >= 1 && d->n_classes <= SIMT_CLASS_MIX_CLASSES);
  const long HW = (long)d->h * d->w;
  SIMT_CHECK(HW < (1L << 31));
  const uintptr_t xbytes = (uintptr_t)d->B * 3 * HW * sizeof(float), lbytes = (uintptr_t)d->B * HW * sizeof(long long);
  SIMT_CHECK(!ranges_overlap(d->x_out, d->xs, xbytes) && !ranges_overlap(d->x_out, d->xt, xbytes));      // a lane's stores may land in front of
  SIMT_CHECK(!ranges_overlap(d->lab_out, d->labs, lbytes));                                              // another lane's loads
  for (int b = 0; b < d->B; ++b)
    for (int c = 0; c < d->n_classes; ++c) SIMT_CHECK(d->rank[b][c] < d->n_classes);
  const long lanes = (HW >> 2) + ((HW & 3) ? 1 : 0);
  const dim3 grid((unsigned)((lanes + 256 * MIX8_QPT - 1) / (256 * MIX8_QPT)), (unsigned)d->B);
  const bool vec = (HW & 3) == 0;
  if (vec && !items)
    hipLaunchKernelGGL((source_mix_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else if (!items)
    hipLaunchKernelGGL((source_mix_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, *d);
  else if (vec)
    hipLaunchKernelGGL((source_mix_kernel<true, uint8_t*>), grid, dim3(256), 0, (hipStream_t)stream, *d, item_out);
  else
    hipLaunchKernelGGL((source_mix_kernel<false, uint8_t*>), grid, dim3(256), 0, (hipStream_t)stream, *d, item_out);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_source_mix(const simt_source_mix_desc* d, simt_stream_t stream) { return source_mix_launch(d, nullptr, false, stream); }

// simt_source_mix plus the item map: a pasted pixel reads entry B + i of the head's [2B] weight table (1.0), a target pixel entry i (q).
extern "C" int simt_source_mix_items(const simt_source_mix_desc* d, uint8_t* item_out, simt_stream_t stream) {
  return source_mix_launch(d, item_out, true, stream);
}
