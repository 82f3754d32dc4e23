// ClassMix (Olsson et al., WACV'21) on a finished batch (simt_amd/data/class_mix.py) and its descendants behind a teacher:
// item i receives, from a PASTED side, the pixels -- labels included -- of half of the classes that occur in that side's labels.  Pure
// selection: no arithmetic touches a value.  Streaming kernels in the style of cache_gather_kernel (csrc/dataset_cache.hip): arguments by
// value in the kernel-argument segment, 4 consecutive pixels (a quad) per lane, flat over h*w, 16-byte loads and stores when h*w % 4 == 0
// (every plane and label row then starts on a 16-byte boundary), dwords / qwords otherwise, one lane takes the h*w % 4 tail.
//   label_presence_kernel  grid (PARTS, B): workgroup (g, b) ORs 1u << l over its strided share of item b's valid labels and lane 0
//                          stores ONE word, part[b][g] -- every word is written on every call: no atomics, nothing to zero.
//   mix_sweep_kernel       grid (quads / (256 * QPT), B): every wave builds the paste mask from the pasted side's presence words and the
//                          item's rank permutation (a few dozen instructions, no LDS, no barrier), then selects quad by quad: the pasted
//                          side's four labels decide, the kept side's are read only where a pixel is not pasted, and a quad whose four
//                          decisions agree loads one image only -- so the byte floors below are what a launch moves except on class
//                          boundaries.  Its compile-time axes, and what the six entry points make of them:
//                            Paste / Keep  the label width of either side: Lab64x4 (int64, two 16-byte loads per quad) or Lab8x4 (bytes, one dword);
//                                          Paste also says how many presence words an item has: they come from the launch that made its labels
//                            QPT           quads per lane, 256 * 4 pixels apart (every access of a wave stays one contiguous run)
//                            ITEMS         also store the item each pixel came from, one byte per pixel (+0.4..0.7 us; a launch without
//                                          the map pays no pointer test per quad)
//                            VEC           h*w % 4 == 0
//                          Everything else is set-up in MixArgs: which batch and item the pasted side is, which byte marks a pasted pixel.
//                          A further mixing launch is a further set of these, not a further kernel.
// Byte floors per pixel (12 + 8 written by every launch):
//   simt_class_mix     <1, int64, int64>  reads 8 (lab[j]) + 12 (one image), + 8 (lab[i]) where not pasted: 40-48, 94-113 MB at B = 4,
//                                         768 x 768.  simt_label_presence in front of it reads 8: 19 MB there.
//   simt_class_mix_u8  <2, bytes, bytes>  reads 12 + 1-2 = 33-34, against 40-48 above, 8 of the presence launch and 24 + 16 of the copies
//                                         into the trainer's buffers.
//   simt_source_mix    <2, int64, bytes>  reads 12 + 8 (the decision needs the source's four labels), + 1 where not pasted: 40-41.
//   The _items flavour of each adds one byte.
#include "common.h"
#include <stddef.h>
#include <string.h>

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

// ================================================================ the mix sweep ============================================================
// A quad's four labels, as one side stores them (T) and as the sweep handles one of them (V).  WORDS: the presence words per item of the
// launch that made such labels -- simt_label_presence's 64, one per lane, or 0: the online label launch's MixArgs::words, strided by 64.
struct Lab64x4 {
  typedef long long T;
  typedef long long V;
  static constexpr int WORDS = SIMT_CLASS_MIX_PARTS;
  long long v[4];
  template <bool VEC>
  static __device__ __forceinline__ Lab64x4 load(const long long* __restrict__ l, long p) {
    if (VEC) {
      const i64x2 u = *(const i64x2*)(l + p), v = *(const i64x2*)(l + p + 2);
      return {{u.x, u.y, v.x, v.y}};
    }
    return {{l[p], l[p + 1], l[p + 2], l[p + 3]}};
  }
  __device__ __forceinline__ long long operator[](int e) const { return v[e]; }
};

struct Lab8x4 {
  typedef uint8_t T;
  typedef uint32_t V;
  static constexpr int WORDS = 0;
  uint32_t w;                                            // ONE dword when VEC
  template <bool VEC>
  static __device__ __forceinline__ Lab8x4 load(const uint8_t* __restrict__ l, long p) {
    if (VEC) return {*(const uint32_t*)(l + p)};
    return {(uint32_t)l[p] | ((uint32_t)l[p + 1] << 8) | ((uint32_t)l[p + 2] << 16) | ((uint32_t)l[p + 3] << 24)};
  }
  __device__ __forceinline__ uint32_t operator[](int e) const { return (w >> (8 * e)) & 255u; }
};

__device__ __forceinline__ bool pasted(long long l, int C, uint32_t mask) { return l >= 0 && l < C && ((mask >> (int)l) & 1u); }
__device__ __forceinline__ bool pasted(uint32_t l, int C, uint32_t mask) { return l < (uint32_t)C && ((mask >> (l & 31u)) & 1u); }

// The output's four labels: the pasted side's where m, the kept side's elsewhere.  Two byte sides stay one packed dword until the store.
__device__ __forceinline__ Lab8x4 select4(Lab8x4 s, Lab8x4 k, bool m0, bool m1, bool m2, bool m3) {
  const uint32_t sel = (m0 ? 0xffu : 0u) | (m1 ? 0xff00u : 0u) | (m2 ? 0xff0000u : 0u) | (m3 ? 0xff000000u : 0u);
  return {(s.w & sel) | (k.w & ~sel)};
}
template <class Paste, class Keep>
__device__ __forceinline__ Lab64x4 select4(Paste s, Keep k, bool m0, bool m1, bool m2, bool m3) {
  return {{m0 ? (long long)s[0] : (long long)k[0], m1 ? (long long)s[1] : (long long)k[1], m2 ? (long long)s[2] : (long long)k[2],
           m3 ? (long long)s[3] : (long long)k[3]}};
}
__device__ __forceinline__ Lab64x4 widened(Lab64x4 a) { return a; }
__device__ __forceinline__ Lab64x4 widened(Lab8x4 a) { return {{(long long)a[0], (long long)a[1], (long long)a[2], (long long)a[3]}}; }

// What a launch is made of beyond its template axes.  Item i keeps its own pixels (x_keep[i], lab_keep[i]) and is pasted from item
// paste[i] of x_paste / lab_paste: partner[i] of the same batch, or item i of a second one; MIX_NONE where apply[i] == 0 -- ONE byte, so
// that a wave's presence words are two dependent loads away, not three.  `rank` sits at a 4-byte boundary: paste_mask_of reads a row as
// scalar dwords.
constexpr int MIX_NONE = 255;
struct MixArgs {
  const uint32_t* x_keep;      // [B][3][h][w] words
  const uint32_t* x_paste;
  const void* lab_keep;        // [B][h][w] Keep::T
  const void* lab_paste;       // [B][h][w] Paste::T
  const uint32_t* part;        // [B][Paste::WORDS or words]: the presence words of lab_paste
  uint32_t* x_out;
  long long* lab_out;
  uint8_t* item_out;           // ITEMS: [B][h][w] bytes, i where the pixel is kept, paste_entry + paste[i] where it is pasted
  int32_t h, w, n_classes, words, paste_entry;
  uint8_t paste[SIMT_CLASS_MIX_MAX];
  uint8_t rank[SIMT_CLASS_MIX_MAX][SIMT_CLASS_MIX_CLASSES];
};
static_assert(offsetof(MixArgs, rank) % 4 == 0, "paste_mask_of reads rank[i] as dwords");

// One lane: pixels p .. p+3 of item i = blockIdx.y, QPT times.  Values travel as integer words.  apply[i] == 0 (workgroup-uniform) is mask 0
// over the item's own data -- its labels once, its image once, out-of-range int64 labels verbatim -- and dereferences no pointer of the
// pasted side.  With ITEMS a quad's four bytes leave as one dword when VEC (a 4-byte aligned base: every item's row then starts on a dword).
template <bool VEC, bool ITEMS, int QPT, class Paste, class Keep>
__global__ __launch_bounds__(256) void mix_sweep_kernel(const MixArgs a) {
  const int i = blockIdx.y;
  const int j = a.paste[i];
  const bool apply = j != MIX_NONE;
  const int C = a.n_classes;
  const long HW = (long)a.h * a.w;
  const long nquad = HW >> 2;
  const uint32_t* __restrict__ xi = a.x_keep + (long)i * 3 * HW;
  const typename Keep::T* __restrict__ li = (const typename Keep::T*)a.lab_keep + (long)i * HW;
  uint32_t* __restrict__ xo = a.x_out + (long)i * 3 * HW;
  long long* __restrict__ lo = a.lab_out + (long)i * HW;
  uint8_t* __restrict__ io = ITEMS ? a.item_out + (long)i * HW : nullptr;
  const uint32_t bi = (uint32_t)i, bj = (uint32_t)(a.paste_entry + j);
  const uint32_t* __restrict__ xj = xi;
  const typename Paste::T* __restrict__ lj = nullptr;
  uint32_t mask = 0u;
  if (apply) {
    const int words = Paste::WORDS ? Paste::WORDS : a.words;
    uint32_t present = 0u;                               // words / 64 contiguous loads per lane from L2
    for (int g = threadIdx.x & 63; g < words; g += 64) present |= a.part[(long)j * words + g];
    mask = paste_mask_of(present, (const uint32_t*)a.rank[i], C);
    xj = a.x_paste + (long)j * 3 * HW;
    lj = (const typename Paste::T*)a.lab_paste + (long)j * HW;
  }
  for (int r = 0; r < QPT; ++r) {
    const long q = ((long)blockIdx.x * QPT + r) * 256 + threadIdx.x;
    if (q < nquad) {
      const long p = q << 2;
      Paste s = {};
      bool m0 = false, m1 = false, m2 = false, m3 = false;
      if (apply) {
        s = Paste::template load<VEC>(lj, p);
        m0 = pasted(s[0], C, mask); m1 = pasted(s[1], C, mask); m2 = pasted(s[2], C, mask); m3 = pasted(s[3], C, mask);
      }
      const bool all = m0 && m1 && m2 && m3, none = !(m0 || m1 || m2 || m3);
      Keep k = {};
      if (!all) k = Keep::template load<VEC>(li, p);
      const Lab64x4 o = widened(select4(s, k, m0, m1, m2, m3));
      if (VEC) {
        const i64x2 u = {o.v[0], o.v[1]}, v = {o.v[2], o.v[3]};
        *(i64x2*)(lo + p) = u;
        *(i64x2*)(lo + p + 2) = v;
      } else {
        lo[p] = o.v[0]; lo[p + 1] = o.v[1]; lo[p + 2] = o.v[2]; lo[p + 3] = o.v[3];
      }
      if (ITEMS) {
        const uint32_t b0 = m0 ? bj : bi, b1 = m1 ? bj : bi, b2 = m2 ? bj : bi, b3 = m3 ? bj : bi;
        if (VEC) {
          *(uint32_t*)(io + p) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        } else {
          io[p] = (uint8_t)b0; io[p + 1] = (uint8_t)b1; io[p + 2] = (uint8_t)b2; io[p + 3] = (uint8_t)b3;
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const long c = ch * HW + p;
        if (VEC) {
          uint4 v;
          if (all) {
            v = *(const uint4*)(xj + c);
          } else if (none) {
            v = *(const uint4*)(xi + c);
          } else {
            const uint4 s4 = *(const uint4*)(xj + c), t4 = *(const uint4*)(xi + c);
            v = make_uint4(m0 ? s4.x : t4.x, m1 ? s4.y : t4.y, m2 ? s4.z : t4.z, m3 ? s4.w : t4.w);
          }
          *(uint4*)(xo + c) = v;
        } else {
          const uint32_t v0 = m0 ? xj[c] : xi[c], v1 = m1 ? xj[c + 1] : xi[c + 1], v2 = m2 ? xj[c + 2] : xi[c + 2],
                         v3 = m3 ? xj[c + 3] : xi[c + 3];
          xo[c] = v0; xo[c + 1] = v1; xo[c + 2] = v2; xo[c + 3] = v3;
        }
      }
    } else if (q == nquad) {                             // scalar tail: h*w % 4 pixels
      for (long p = nquad << 2; p < HW; ++p) {
        typename Paste::V l = 0;
        bool m = false;
        if (apply) {
          l = lj[p];
          m = pasted(l, C, mask);
        }
        lo[p] = m ? (long long)l : (long long)li[p];
        for (int ch = 0; ch < 3; ++ch) xo[ch * HW + p] = m ? xj[ch * HW + p] : xi[ch * HW + p];
        if (ITEMS) io[p] = (uint8_t)(m ? bj : bi);
      }
    }
  }
}

static bool ranges_overlap(const void* a, const void* b, uintptr_t bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return !(a0 + bytes <= b0 || b0 + bytes <= a0);
}

// The tables of a public descriptor.  partner NULL: item i of the second batch.  false: a partner outside the batch.
static bool mix_tables(MixArgs& a, int B, const uint8_t* partner, const uint8_t* apply, const uint8_t (*rank)[SIMT_CLASS_MIX_CLASSES]) {
  for (int b = 0; b < B && b < SIMT_CLASS_MIX_MAX; ++b) {
    const int j = partner ? partner[b] : b;
    if (j >= B) return false;
    a.paste[b] = apply[b] ? (uint8_t)j : (uint8_t)MIX_NONE;
  }
  memcpy(a.rank, rank, sizeof a.rank);
  return true;
}

// The checks every entry point shares, and the launch.
template <int QPT, class Paste, class Keep>
static int mix_launch(const MixArgs& a, int B, bool items, simt_stream_t stream) {
  SIMT_CHECK(a.x_keep && a.x_paste && a.lab_keep && a.lab_paste && a.part && a.x_out && a.lab_out);
  SIMT_CHECK(!items || (a.item_out && ((uintptr_t)a.item_out & 3) == 0));
  SIMT_CHECK((((uintptr_t)a.x_keep | (uintptr_t)a.x_paste | (uintptr_t)a.lab_keep | (uintptr_t)a.lab_paste) & 15) == 0);
  SIMT_CHECK((((uintptr_t)a.x_out | (uintptr_t)a.lab_out) & 15) == 0 && ((uintptr_t)a.part & 3) == 0);
  SIMT_CHECK(B >= 1 && B <= SIMT_CLASS_MIX_MAX && a.h > 0 && a.w > 0);
  SIMT_CHECK(a.n_classes >= 1 && a.n_classes <= SIMT_CLASS_MIX_CLASSES);
  const long HW = (long)a.h * a.w;
  SIMT_CHECK(HW < (1L << 31));
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < a.n_classes; ++c) SIMT_CHECK(a.rank[b][c] < a.n_classes);
  const long lanes = (HW >> 2) + ((HW & 3) ? 1 : 0);
  const dim3 grid((unsigned)((lanes + 256 * QPT - 1) / (256 * QPT)), (unsigned)B);
  const bool vec = (HW & 3) == 0;
  if (vec && !items)
    hipLaunchKernelGGL((mix_sweep_kernel<true, false, QPT, Paste, Keep>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (!items)
    hipLaunchKernelGGL((mix_sweep_kernel<false, false, QPT, Paste, Keep>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (vec)
    hipLaunchKernelGGL((mix_sweep_kernel<true, true, QPT, Paste, Keep>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((mix_sweep_kernel<false, true, QPT, Paste, Keep>), grid, dim3(256), 0, (hipStream_t)stream, a);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

// ---- simt_class_mix: both sides one batch of int64 labels, simt_label_presence's SIMT_CLASS_MIX_PARTS = 64 words per item (one per lane).
static int class_mix(const simt_class_mix_desc* d, uint8_t* item_out, bool items, simt_stream_t stream) {
  SIMT_CHECK(d && (const void*)d->x != (const void*)d->x_out && (const void*)d->lab != (const void*)d->lab_out);
  MixArgs a = {};
  a.x_keep = a.x_paste = (const uint32_t*)d->x;
  a.lab_keep = a.lab_paste = d->lab;
  a.part = d->part;
  a.x_out = (uint32_t*)d->x_out; a.lab_out = d->lab_out; a.item_out = item_out;
  a.h = d->h; a.w = d->w; a.n_classes = d->n_classes;
  SIMT_CHECK(mix_tables(a, d->B, d->partner, d->apply, d->rank));
  return mix_launch<1, Lab64x4, Lab64x4>(a, d->B, items, stream);
}

extern "C" int simt_class_mix(const simt_class_mix_desc* d, simt_stream_t stream) { return class_mix(d, nullptr, false, stream); }

// simt_class_mix plus the item map (the weak-view teacher gathers its predictions through it): x_out / lab_out bit for bit as above.
extern "C" int simt_class_mix_items(const simt_class_mix_desc* d, uint8_t* item_out, simt_stream_t stream) {
  return class_mix(d, item_out, true, stream);
}

// ---- simt_class_mix_u8: the mix BEHIND a teacher, inside the warm-up trainers.  simt_class_mix's selection over BYTE
// labels (simt_online_label_u8's lab8) and that launch's presence words (part[b][g], `rows` of them per item), written straight into the
// buffers the student's forward and the head kernels read: x_out fp32, lab_out int64.
// A lane takes MIX8_QPT quads, so the wave's paste mask is paid once per 512 pixels.  Measured on MI355X (profiles/online_mix.txt): 2 quads
// per lane over item-major words 17.8 / 16.7 us (B = 4 768 x 768 / B = 8 512 x 512); 1 quad 21.8 / 16.6; 4 quads 20.4 / 19.4 (too few
// waves); the words workgroup-major ([g][b]: a wave's loads B * 4 bytes apart) 20.4 / 19.6 at 4 quads, 22.0 / 19.9 at 1.
constexpr int MIX8_QPT = 2;

static int class_mix_u8(const simt_class_mix_u8_desc* d, uint8_t* item_out, bool items, simt_stream_t stream) {
  SIMT_CHECK(d && d->B >= 2 && d->rows >= 1 && d->rows <= SIMT_ONLINE_LABEL_MAX_PARTS);
  SIMT_CHECK(!ranges_overlap(d->x, d->x_out, (uintptr_t)d->B * 3 * d->h * d->w * sizeof(float)));      // item i reads its partner's image
  MixArgs a = {};
  a.x_keep = a.x_paste = (const uint32_t*)d->x;
  a.lab_keep = a.lab_paste = d->lab8;
  a.part = d->part; a.words = d->rows;
  a.x_out = (uint32_t*)d->x_out; a.lab_out = d->lab_out; a.item_out = item_out;
  a.h = d->h; a.w = d->w; a.n_classes = d->n_classes;
  SIMT_CHECK(mix_tables(a, d->B, d->partner, d->apply, d->rank));
  return mix_launch<MIX8_QPT, Lab8x4, Lab8x4>(a, d->B, items, stream);
}

extern "C" int simt_class_mix_u8(const simt_class_mix_u8_desc* d, simt_stream_t stream) { return class_mix_u8(d, nullptr, false, stream); }

// simt_class_mix_u8 plus the item map (the weighted head reads a pasted pixel's weight from its partner's entry): x_out /
// lab_out bit for bit as above -- same grid, same paste mask.
extern "C" int simt_class_mix_u8_items(const simt_class_mix_u8_desc* d, uint8_t* item_out, simt_stream_t stream) {
  return class_mix_u8(d, item_out, true, stream);
}

// ---- simt_source_mix: the cross-domain mix of DACS, behind a teacher and beside a labelled source batch.  simt_class_mix_u8's
// launch shape with the pasted side SOURCE item i: its image xs[i], its ground truth labs[i] as int64 (what the loader hands out: there is
// no byte copy of it) and its presence words from simt_label_presence.
static int source_mix(const simt_source_mix_desc* d, uint8_t* item_out, bool items, simt_stream_t stream) {
  SIMT_CHECK(d);
  const uintptr_t px = (uintptr_t)d->B * d->h * d->w;
  SIMT_CHECK(!ranges_overlap(d->x_out, d->xs, px * 3 * sizeof(float)) && !ranges_overlap(d->x_out, d->xt, px * 3 * sizeof(float)));
  SIMT_CHECK(!ranges_overlap(d->lab_out, d->labs, px * sizeof(long long)));     // a lane's stores may land in front of another lane's loads
  MixArgs a = {};
  a.x_keep = (const uint32_t*)d->xt; a.x_paste = (const uint32_t*)d->xs;
  a.lab_keep = d->lab8; a.lab_paste = d->labs;
  a.part = d->part_s;
  a.x_out = (uint32_t*)d->x_out; a.lab_out = d->lab_out; a.item_out = item_out;
  a.h = d->h; a.w = d->w; a.n_classes = d->n_classes;
  a.paste_entry = d->B;                                  // entry B + i of the head's [2B] weight table (<= 63)
  SIMT_CHECK(mix_tables(a, d->B, nullptr, d->apply, d->rank));
  return mix_launch<MIX8_QPT, Lab64x4, Lab8x4>(a, d->B, items, stream);
}

extern "C" int simt_source_mix(const simt_source_mix_desc* d, simt_stream_t stream) { return source_mix(d, nullptr, false, stream); }

// simt_source_mix plus the item map: a pasted pixel reads entry B + i of the head's [2B] weight table (1.0), a target pixel entry i (q).
extern "C" int simt_source_mix_items(const simt_source_mix_desc* d, uint8_t* item_out, simt_stream_t stream) {
  return source_mix(d, item_out, true, stream);
}
