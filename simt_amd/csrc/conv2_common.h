// Declarations shared by the bf16 throughput conv kernels (conv_igemm2.hip, conv1x1_stream.hip).
#pragma once
#include "common.h"

struct Conv2KArgs {
  const char* x;
  const char* w;
  const char* wf;                      // unused (always NULL: the weights-direct form was removed); kept for the kernel-argument layout
  int nt16;                            // unused (Npad / 16); kept for the kernel-argument layout
  bf16_t* y;
  const float* bias;
  const bf16_t* res;
  const bf16_t* mask;
  const unsigned char* res_bits;
  const bf16_t* bnr_y;                 // fused first pass of the BatchNorm backward (simt_conv_desc.bnr_*)
  const float *bnr_mean, *bnr_rstd, *bnr_scale, *bnr_shift;
  const unsigned char* bnr_bits;
  float* bnr_part;
  int bnr_mode, bnr_ld;
  float* stats;
  const char* zero;
  int H, W, Ho, Wo, Cout, Nstore, ldy, ldr, stride, ntaps, relu, M;
  int kc_per_tap, pix_bytes, wrow_bytes, ldm;
  int ntiles_n, ntiles_m;
  int out_f32;     // 1: y is fp32 and is stored straight from the accumulators (no bias/residual/ReLU/stats)
  int rows;        // pixels per tile (<= BM)
  int nblk128;     // stats slots allocated by the caller: ceil(M/128) >= ntiles_m
  float rcp_hw, rcp_wo;   // 1 / (Ho*Wo), 1 / Wo for fast_divmod (exact below 2^24 pixels)
  int toff[SIMT_MAX_TAPS];   // (dy*W + dx) * pix_bytes: 32-bit so that the uniform per-stage lookup is an s_load_dword
                             // (a 16-bit table compiles to global_load_sshort, whose vmcnt(0) drains the glds ring)
  short dy[SIMT_MAX_TAPS], dx[SIMT_MAX_TAPS];
  // fused train-mode BatchNorm (simt_fbn_desc; kernels instantiated with FBN = 1 only)
  int fbn_mode, fbn_ldo;
  bf16_t* fbn_out;
  unsigned long long* fbn_bar;         // [SIMT_FBN_BAR_WORDS] ticket counters
  unsigned long long* fbn_err;         // sticky error word (simt_fbn_desc.err or work[SIMT_FBN_ERR_WORD]): set by a poller that timed out
  unsigned long long *fbn_cgran, *fbn_slots;   // [2][Cout] constants granules; [ntiles_m][2 | 3][Cout] tile-sum granules
  const float *fbn_gamma, *fbn_beta;
  float *fbn_rmean, *fbn_rvar;
  float fbn_momentum, fbn_eps;
  float *fbn_mean, *fbn_rstd, *fbn_scale, *fbn_shift, *fbn_coef, *fbn_dgamma, *fbn_dbeta;
  // BatchNorm + ReLU of the input in the operand path (simt_conv_desc.in_*; conv1x1_rows_kernel FL_STATS_INBN only)
  const float *in_scale, *in_shift;
  bf16_t* in_out;
};

template <int N> __device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 16, "unsupported vmcnt");
#define SIMT_VMCNT_CASE(K) else if constexpr (N == K) asm volatile("s_waitcnt vmcnt(" #K ")" ::: "memory")
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  SIMT_VMCNT_CASE(1); SIMT_VMCNT_CASE(2); SIMT_VMCNT_CASE(3); SIMT_VMCNT_CASE(4); SIMT_VMCNT_CASE(5); SIMT_VMCNT_CASE(6);
  SIMT_VMCNT_CASE(7); SIMT_VMCNT_CASE(8); SIMT_VMCNT_CASE(9); SIMT_VMCNT_CASE(10); SIMT_VMCNT_CASE(11); SIMT_VMCNT_CASE(12);
  SIMT_VMCNT_CASE(13); SIMT_VMCNT_CASE(14); SIMT_VMCNT_CASE(15); SIMT_VMCNT_CASE(16);
#undef SIMT_VMCNT_CASE
}

