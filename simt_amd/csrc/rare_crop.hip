// Rare-class crops (simt_amd/data/rare_class.py): DAFormer re-draws the random crop until it holds enough pixels of the
// sampled class.  The host draws K candidate windows per item; the counts, the pick and the crop run on one stream, and the pick reaches
// the crop launch through device memory (`win`): nothing is read back.
//   rare_crop_counts_kernel  grid (PARTS, K, B): workgroup (g, k, b) counts the pixels of class cls[b] that candidate k's window shows in
//                            the rows y = 4 * g + wave (mod 4 * PARTS); a wave owns a row -- ytab[y + oy] and the row's base are scalar --
//                            and a lane every 64th column: xtab is read coalesced, the label byte is a gather out of a frame that stays
//                            in L2 over the K windows.  Lane 0 stores ONE word, parts[b][k][g]: no atomics, nothing to zero.
//   rare_crop_pick_kernel    grid (B), one wave: lane k < K sums candidate k's PARTS words; a ballot finds the first that passes.
// The crop is scale_crop_kernel's WIN flavour (csrc/scale_crop.hip).
#include "common.h"

#define RC_PARTS SIMT_RARE_CROP_PARTS
#define RC_CANDS SIMT_RARE_CROP_CANDS

static_assert(sizeof(simt_rare_crop_desc) <= 4096, "the descriptor travels in the 4 KB kernel-argument segment");

int simt_scale_crop_launch(const simt_scale_crop_desc* d, const int32_t* win, simt_stream_t stream);   // csrc/scale_crop.hip

__global__ __launch_bounds__(256) void rare_crop_counts_kernel(const simt_rare_crop_desc d) {
  const int g = blockIdx.x, k = blockIdx.y, b = blockIdx.z;
  const int c = d.cls[b];
  int32_t* __restrict__ out = d.parts + ((long)b * d.K + k) * RC_PARTS + g;
  if (c == 255) {                                        // block-uniform
    if (threadIdx.x == 0) *out = 0;
    return;
  }
  const int ci = d.cand_choice[b][k], ox = d.cand_ox[b][k], oy = d.cand_oy[b][k];
  const int ws = d.c[ci].ws, hs = d.c[ci].hs, w = d.w, h = d.h;
  const int32_t* __restrict__ xtab = d.tables + d.c[ci].xtab;
  const int32_t* __restrict__ ytab = d.tables + d.c[ci].ytab;
  const unsigned char* __restrict__ lab = d.lab[b];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the rows [ya, yb) and columns [xa, xb) of the window that lie inside the scaled frame
  const int ya = max(0, -oy), yb = min(h, hs - oy), xa = max(0, -ox), xb = min(w, ws - ox);
  int n = 0;
  for (int y = 4 * g + wave; y < yb; y += 4 * RC_PARTS) {
    if (y < ya) continue;
    const unsigned char* __restrict__ row = lab + (long)ytab[y + oy] * d.Ws;
    for (int x = xa + lane; x < xb; x += 64) n += row[xtab[x + ox]] == c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  __shared__ int wave_n[4];
  if (lane == 0) wave_n[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) *out = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ __launch_bounds__(64) void rare_crop_pick_kernel(const simt_rare_crop_desc d) {
  const int b = blockIdx.x, lane = threadIdx.x, K = d.K;
  int n = 0;
  if (lane < K) {
    const int32_t* __restrict__ p = d.parts + ((long)b * K + lane) * RC_PARTS;
#pragma unroll
    for (int g = 0; g < RC_PARTS; ++g) n += p[g];
  }
  const unsigned long long pass = __ballot(lane < K && n > d.min_count);
  int ks = pass ? __ffsll((long long)pass) - 1 : K - 1;
  if (d.cls[b] == 255) ks = 0;
  ks = __builtin_amdgcn_readfirstlane(ks);
  const int count = __shfl(n, ks, 64);
  if (lane == 0) *(int4*)(d.win + 4 * b) = make_int4((int)d.cand_choice[b][ks], d.cand_ox[b][ks], d.cand_oy[b][ks], count);
}

// The scale-crop descriptor of the same batch (choice 0 at origin 0 for every item: the WIN flavour reads neither).
static void rc_scale_crop_desc(const simt_rare_crop_desc* d, simt_scale_crop_desc* s) {
  *s = simt_scale_crop_desc{};
  for (int b = 0; b < d->B; ++b) {
    s->img[b] = d->img[b];
    s->lab[b] = d->lab[b];
    s->mirror[b] = d->mirror[b];
  }
  for (int c = 0; c < SIMT_SCALE_CROP_CHOICES; ++c) s->c[c] = d->c[c];
  s->tables = d->tables, s->x = d->x, s->lab_out = d->lab_out;
  s->B = d->B, s->Hs = d->Hs, s->Ws = d->Ws, s->h = d->h, s->w = d->w, s->n_choices = d->n_choices, s->max_rows = d->max_rows;
  s->n_tables = d->n_tables;
  for (int i = 0; i < 3; ++i) s->mean[i] = d->mean[i];
}

// Everything simt_scale_crop validates (through simt_scale_crop_lds_bytes, on the descriptor above) and what the three launches add.
static bool rc_valid(const simt_rare_crop_desc* d, simt_scale_crop_desc* s) {
  if (!d || d->B <= 0 || d->B > SIMT_RARE_CROP_MAX) return false;
  rc_scale_crop_desc(d, s);
  const long lds = simt_scale_crop_lds_bytes(s);
  if (lds < 0 || lds > SIMT_SCALE_CROP_LDS_MAX) return false;
  if ((d->w & 3) == 0 && ((((uintptr_t)d->x) & 15) != 0 || (((uintptr_t)d->lab_out) & 15) != 0)) return false;
  if (d->K < 1 || d->K > RC_CANDS || d->min_count < 0) return false;
  if (!d->parts || ((uintptr_t)d->parts & 3) != 0 || !d->win || ((uintptr_t)d->win & 15) != 0) return false;
  for (int c = 0; c < d->n_choices; ++c) {               // the label tables, whether or not lab_out is given: the counts read them
    const simt_scale_crop_choice& k = d->c[c];
    if (k.xtab < 0 || k.xtab + (long)k.ws > d->n_tables || k.ytab < 0 || k.ytab + (long)k.hs > d->n_tables) return false;
  }
  for (int b = 0; b < d->B; ++b) {
    if (!d->lab[b]) return false;
    for (int k = 0; k < d->K; ++k) {
      const int ci = d->cand_choice[b][k];
      if (ci >= d->n_choices) return false;
      const int dx = d->c[ci].ws - d->w, dy = d->c[ci].hs - d->h, ox = d->cand_ox[b][k], oy = d->cand_oy[b][k];
      if (ox < (dx < 0 ? dx : 0) || ox > (dx > 0 ? dx : 0) || oy < (dy < 0 ? dy : 0) || oy > (dy > 0 ? dy : 0)) return false;
    }
  }
  return true;
}

extern "C" int simt_rare_crop_counts(const simt_rare_crop_desc* d, simt_stream_t stream) {
  simt_scale_crop_desc s;
  SIMT_CHECK(rc_valid(d, &s));
  hipLaunchKernelGGL(rare_crop_counts_kernel, dim3(RC_PARTS, (unsigned)d->K, (unsigned)d->B), dim3(256), 0, (hipStream_t)stream, *d);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_rare_crop_pick(const simt_rare_crop_desc* d, simt_stream_t stream) {
  simt_scale_crop_desc s;
  SIMT_CHECK(rc_valid(d, &s));
  hipLaunchKernelGGL(rare_crop_pick_kernel, dim3((unsigned)d->B), dim3(64), 0, (hipStream_t)stream, *d);
  SIMT_LAUNCH_CHECK();
  return SIMT_OK;
}

extern "C" int simt_scale_crop_win(const simt_rare_crop_desc* d, simt_stream_t stream) {
  simt_scale_crop_desc s;
  SIMT_CHECK(rc_valid(d, &s));
  return simt_scale_crop_launch(&s, d->win, stream);
}
