/* simt_hip.h -- C ABI of libsimt_hip.so, the gfx950 (MI355X) implementation of SimT's per-iteration hot path.
 *
 * The reference (CityU-AIM-Group/SimT) has no FFI layer: its hot path is a chain of torch ops called from
 * Python (tools/trainV2_simt.py:326-436 through model/deeplab_multi.py and utils/loss.py).  Each entry point
 * below replaces the torch op(s) cited next to it.  Conventions:
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (borrowed for the call),
 *     except descriptors, which are host structs read during the call;
 *   - `stream` is a hipStream_t; kernels are enqueued there and the call never synchronises;
 *   - activations are NHWC ([B][H][W][C], C contiguous), dtype SIMT_BF16 or SIMT_F32 (fp32 = parity mode);
 *   - master weights / gradients are fp32 in PyTorch OIHW layout (the reference's state_dict contract);
 *   - return value: SIMT_OK or an error code; simt_last_error() gives the text (mirrors the reference's
 *     assert-style failures, utils/loss.py:22-27).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 */
#ifndef SIMT_HIP_H
#define SIMT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* simt_stream_t; /* hipStream_t */

enum { SIMT_OK = 0, SIMT_ERR_INVALID = 1, SIMT_ERR_LAUNCH = 2 };
enum { SIMT_F32 = 0, SIMT_BF16 = 1 };
#define SIMT_MAX_TAPS 36

const char* simt_last_error(void);
/* Device-scope events for ordering two HIP streams of ONE device (the launch lists of simt_amd/engine.py): like hipEventCreateWithFlags /
 * hipEventRecord / hipStreamWaitEvent (which torch.cuda.Event wraps), but recorded with a device-scope release instead of the default
 * system-scope fence -- the host never inspects them.  Replaces torch.cuda.Event().record() / stream.wait_event().  `scope`:
 *   0  hipEventDisableTiming | hipEventReleaseToDevice      the DOCUMENTED device-scope release (default of the launch lists since ABI 2)
 *   1  hipEventDisableTiming                                system-scope release (what torch.cuda.Event does)
 *   2  hipEventDisableTiming | hipEventDisableSystemFence   no release at the marker at all: ordering rests on the producing kernels' own
 *      end-of-kernel agent-scope release (round 5's form; explicit opt-in, SIMT_EVENT_SCOPE=2) */
int simt_event_create(void** ev, int scope);
int simt_event_destroy(void* ev);
int simt_event_record(void* ev, simt_stream_t stream);
int simt_stream_wait_event(simt_stream_t stream, void* ev);
/* 2 since round 6: simt_sgd_desc.skip_if, simt_fbn_desc.err, simt_ntm_inner_desc.skip_if (trailing pointers the library dereferences),
 * simt_adam_step_guarded, simt_event_create's scope values, simt_conv_desc.cu_budget / in_scale / in_shift / in_out.  A caller built against an older header passes
 * shorter structs: check the version before the first call (simt_amd/_lib.py does). */
#define SIMT_ABI_VERSION 2
int simt_abi_version(void);

/* ---- convolution: fprop / dgrad (implicit GEMM, MFMA) --------------------------------------------------
 * y[m][n] = act( sum_{tap,ci} x[pixel(m)*stride + (dy,dx)[tap]][ci] * w[n][tap*Cin+ci] + bias[n] + res[m][n] )
 * replaces nn.Conv2d forward (model/deeplab_multi.py:62,68,73,110,127,156; Classifier_Module.forward :115-119 is
 * ONE call with the taps of both live dilations) and, with the dgrad-packed weight and negated taps, its dgrad.
 * stats (optional): [ceil(M/128)][2][Cout] per-tile sum / sum-of-squares of the fp32 results (BatchNorm batch stats). */
typedef struct {
  const void* x;       /* [B][H][W][Cin] dtype_in */
  const void* w;       /* [Npad][ntaps*Cin] dtype_in, K contiguous (simt_pack_weight) */
  void* y;             /* [B*Ho*Wo][ldy] dtype_out */
  const float* bias;   /* [Cout] or NULL */
  const void* res;     /* [B*Ho*Wo][ldr] dtype_in, added before the activation, or NULL */
  float* stats;        /* or NULL */
  int32_t B, H, W, Cin, Ho, Wo, Cout;
  int32_t Npad;        /* rows of w, multiple of tile_n */
  int32_t Nstore;      /* columns written, multiple of 8, <= ldy */
  int32_t ldy, ldr, stride, ntaps, relu;
  int32_t dtype_in, dtype_out, tile_n; /* tile_n in {128,64,32}; bf16 -> bf16 also 256 */
  int16_t dy[SIMT_MAX_TAPS], dx[SIMT_MAX_TAPS];
  const void* mask;    /* [B*Ho*Wo][ldm] dtype_in or NULL: the result is zeroed where mask <= 0 (ReLU backward of the layer
                        * whose output this gradient belongs to; used by the BN-free VGG trunk, model/deeplab_vgg.py) */
  int32_t ldm;
  const unsigned char* res_bits; /* or NULL: res[m][n] only counts where bit (n & 7) of res_bits[(m*ldr + n) / 8] is set -- the
                                  * identity-shortcut gradient dz * (z > 0) of a residual block (model/deeplab_multi.py:97-100)
                                  * taken straight from dz and the bit mask of simt_bn_apply_bits, never materialised */
  /* Fused first pass of the BatchNorm backward (bf16 v2 kernel only; bnr_mode 0 = off).  When this launch PRODUCES the
   * gradient dz of a BatchNorm-ed activation (it is the dgrad of the conv that consumed relu(bn(y)), or the dx of the next
   * block), the epilogue also accumulates, on the values it stores, S1 = sum g and S2 = sum g*xhat with
   * g = dz * mask, xhat = (y - mean) * rstd -- what bn_bwd_reduce_kernel would re-read dz for -- into
   * bnr_part[m-tile][3][Cout] (third row zero); simt_bn_bwd then starts at its finalize (simt_bn_bwd_desc.reduce_done_nblk =
   * simt_conv_mtiles(d)).  mask: bnr_mode 2 = y*scale+shift > 0, 3 = bit mask bnr_bits (simt_bn_apply_bits). */
  const void* bnr_y;             /* [B*Ho*Wo][bnr_ld] dtype_in: the saved pre-BN activation */
  const float *bnr_mean, *bnr_rstd, *bnr_scale, *bnr_shift;
  const unsigned char* bnr_bits;
  float* bnr_part;
  int32_t bnr_mode, bnr_ld;
  const void* w_frag;  /* optional (may be NULL): the SAME weights as `w` in MFMA-fragment order (simt_pack_weight with
                        * SIMT_PACK_FRAG(Npad / 16) in `mode`): [K / 64][Npad / 16][2][64 lanes][8] bf16, i.e. element (row, kcol) of the
                        * K-contiguous matrix sits at ((((kcol / 64) * (Npad / 16) + row / 16) * 2 + (kcol / 32) % 2) * 64 +
                        * (row % 16) + 16 * ((kcol / 8) % 4)) * 8 + kcol % 8.  No kernel of the library reads it: the form of the wide
                        * bf16 kernel that loaded its weight operand straight into registers instead of staging it through LDS was
                        * measured slower and removed (simt_conv_wants_frag is always 0); the field stays for the layout */
  const struct simt_fbn_desc* fbn;   /* optional (may be NULL): the train-mode BatchNorm behind this conv fused into the launch, below */
  int32_t cu_budget;   /* ABI 2.  Compute units this launch may plan for; 0 = all of the device (256); -1: A/B only, rounds 1-5 tile choice.  Data-parallel plans pass 256 minus the
                        * CUs the collective's persistent kernels hold (NCCL_MAX_NCHANNELS): the one-workgroup-per-CU tile lists of the wide convs
                        * are planned for that many CUs (M = 37 636: 236 tiles of 160 rows for any budget >= 236 -- the default plan already leaves
                        * 20 CUs free; a smaller budget re-plans).  Changes only the pixel rows per tile: every output element is bit-identical across budgets; the per-tile
                        * BatchNorm partial sums (stats / bnr_part: one slot per tile) regroup, i.e. their fp32 rounding may differ in the last bit. */
  int32_t reserved_;
  /* ABI 2.  BatchNorm + ReLU of the INPUT applied in the operand path (round 6; model/deeplab_multi.py:88-92: out = relu(bn2(conv2)), conv3(out)).
   * When in_scale != NULL the launch reads x as the RAW pre-BatchNorm activation y2, uses a = relu(x * in_scale[c] + in_shift[c]) (rounded to
   * bf16, bitwise what simt_bn_apply writes) as its operand and ALSO writes a to in_out [B*H*W][Cin] (the weight gradient of this conv and
   * the BatchNorm backward read it later) -- the separate simt_bn_apply launch and its re-read of y2 disappear.  Only launches for which
   * simt_conv_inbn_ok(d) != 0 (the row-streaming 1x1 kernel on Cin in {64, 128, 256} with BatchNorm statistics: a Bottleneck's conv3 in the
   * training forward) accept it; everywhere else the fields must be NULL. */
  const float *in_scale, *in_shift;
  void* in_out;
} simt_conv_desc;
/* Train-mode BatchNorm2d (frozen affine; model/deeplab_multi.py:63-70,81-91) fused into the PRODUCING conv launch -- round 4.  For a
 * launch whose workgroups are all co-resident (one round of the chip: simt_conv_fbn_ok), the pixel tile stays in LDS after the epilogue;
 * every workgroup publishes its per-channel tile sums as 8-byte {value, tag} granules (write-through stores), the first C/8 workgroups
 * poll the granules of 8 channels each, add them IN THE ORDER simt_bn_finalize / simt_bn_bwd's finalize use (bitwise the same constants)
 * and publish the constants the same way; every workgroup polls its channels' constants and normalises its tile from LDS:
 *   mode 1 (forward; needs d->stats):       y as usual, out = relu(y * scale + shift)   replaces simt_bn_finalize + simt_bn_apply
 *   mode 2 (backward; needs d->bnr_mode 2): out = scale * (g - c1 - xhat * c2)          replaces simt_bn_bwd; d->y (the raw dz) is NOT written
 * (d->stats / d->bnr_part themselves are not written in fused launches.)  Only a launch on the stream that owns the plan may wait like
 * this: kernels of the other streams (frozen forward, weight gradients) never wait on anything, so the co-residency the polling needs
 * always resolves.  A workgroup that has polled for ~2 s (another process's waiting launch on the same GPU, persistent collective kernels holding
 * CUs) does NOT trap: it sets the sticky error word (`err`, or work[SIMT_FBN_ERR_WORD]), every other poller of the launch sees it and the launch ends;
 * later fused launches that share the word bail out at their first failed poll.  What such a launch guarantees: a poller that gave up writes
 * nothing derived from its incomplete reads -- no constants, no mean / rstd / scale / shift / coef / d gamma / d beta, NO running-statistics
 * update, not its rows of `out` (workgroups whose polls had completed wrote theirs from complete sums: `out` is PARTIALLY written and must be
 * treated as undefined).  The caller reads the word (simt_amd: TrunkPlan.fbn_error(), raised by losses()) and rebuilds the plan with the
 * two-pass BatchNorm; the optimiser launches given the same word (simt_sgd_desc.skip_if, simt_adam_step_guarded) leave weights, momentum
 * buffers and Adam moments untouched while it is set.  `work` belongs to ONE BatchNorm and direction: its ticket counters only ever grow and
 * give every launch its generation = the granules' tag. */
#define SIMT_FBN_BAR_WORDS 144            /* uint64 words at the head of `work`: 8 ticket counters, one 128-byte line each (+ spare) */
#define SIMT_FBN_ERR_WORD 136             /* spare word of the head used as the error word when simt_fbn_desc.err is NULL */
typedef struct simt_fbn_desc {
  int32_t mode;          /* 1 forward, 2 backward */
  int32_t ldo;           /* row pitch of out in elements */
  void* out;             /* [B*Ho*Wo][ldo] bf16 */
  uint64_t* work;        /* [simt_conv_fbn_words(d)] uint64, zeroed ONCE by the caller: counters | [2][C] constants | [tiles][2|3][C] tile sums */
  const float *gamma, *beta;              /* forward: [C] or NULL (1 / 0) */
  float *running_mean, *running_var;      /* forward: updated with `momentum` like simt_bn_finalize, or NULL */
  float momentum, eps;
  float *mean, *rstd, *scale, *shift;     /* forward: OUT [C] each (the backward reads them) */
  float* coef;                            /* backward: OUT [3][C] = (sum g, sum g*xhat, 0) / count */
  float *dgamma, *dbeta;                  /* backward, trainable affine (model/deeplabv3.py's BatchNorm): OUT [C] = sum g*xhat, sum g; or NULL */
  uint64_t* err;                          /* optional: sticky error word shared by the fused launches of a plan (zeroed once by the caller; set
                                           * non-zero by a launch whose polling timed out); NULL: work[SIMT_FBN_ERR_WORD] */
} simt_fbn_desc;
int simt_conv_fprop(const simt_conv_desc* d, simt_stream_t stream);
/* Two INDEPENDENT convs of identical geometry in one launch (round 5): the trainable and the frozen ResNetMulti run the same 104 conv shapes on
 * the same image (tools/trainV2_simt.py:351-353 and :370 -> model/deeplab_multi.py:172-192); their layer-k convs differ only in weights, output
 * and epilogue (BatchNorm statistics | folded bias + ReLU [+ residual]).  d0 / d1: same B, H, W, Cin, Cout, taps, stride, Npad, output dtype.
 * Results are bit-identical to simt_conv_fprop(d0) followed by simt_conv_fprop(d1); pairs the fused kernels do not cover (different tile
 * variant, other epilogue combinations, d->fbn set) ARE run as those two launches.  simt_conv_pair_fused says which it will be. */
int simt_conv_fprop_pair(const simt_conv_desc* d0, const simt_conv_desc* d1, simt_stream_t stream);
int simt_conv_pair_fused(const simt_conv_desc* d0, const simt_conv_desc* d1);
/* 1 if simt_conv_fprop can run d with a fused BatchNorm (d->fbn): bf16 v2 kernel with the 3-slot ring -- 256-column tiles in both directions,
 * 128- / 64-column tiles (the small maps of model/deeplabv3.py) in the backward direction (d->bnr_mode 2) -- and a grid that is co-resident on
 * the current device (tiles <= compute units); d->fbn itself need not be set yet */
int simt_conv_fbn_ok(const simt_conv_desc* d);
long simt_conv_fbn_words(const simt_conv_desc* d);      /* uint64 words simt_fbn_desc.work needs for d (0 if !simt_conv_fbn_ok) */
/* 1 if the launch for d would use d->w_frag when given.  Always 0: the weights-direct form was measured slower and removed */
int simt_conv_wants_frag(const simt_conv_desc* d);
/* `mode` of simt_pack_weight / PackJob: low byte = layout mode 0 / 1 / 2 below; SIMT_PACK_FRAG(nt16) additionally stores the
 * destination in MFMA-fragment order (see simt_conv_desc.w_frag) with nt16 = Npad / 16 row blocks */
#define SIMT_PACK_FRAG(nt16) ((int)(nt16) << 8)
/* which kernel instantiation simt_conv_fprop runs for d (profiling / reporting / tests that must hit a given instantiation):
 * returns 0 (conv_igemm_kernel, fp32 parity + narrow outputs), 2 (conv_igemm2_kernel<bn, tm, nst>, the bf16 throughput kernel),
 * 4 (conv1x1_stream_kernel) or 5 (conv1x1_rows_kernel): the short-reduction / wide-output 1x1 shapes */
int simt_conv_variant(const simt_conv_desc* d, int* bn, int* tm, int* nst);
/* compile-time epilogue flavour of the bf16 v2 kernel the launch for d runs (the last template argument of conv_igemm2_kernel<bn, tm, nst,
 * fbn, epi>): 0 generic (run-time flags), 1 BatchNorm statistics, 2 fused BatchNorm-backward reduce (mask from y * scale + shift), 3 bias + ReLU,
 * 4 bit-masked residual + BatchNorm-backward reduce with the bit mask, 5 plain, 6 residual only, 7 BatchNorm-backward reduce with the bit mask
 * (+ optional plain residual), 8 ReLU-mask operand only (the BatchNorm-free VGG dgrads); the 2-slot short-K kernels are instantiated for 0 and
 * 4-8 only (1-3 are reported as 0 there); same results either way */
int simt_conv_epilogue_flavour(const simt_conv_desc* d);
/* number of pixel tiles (= statistics / bnr_part slots) the launch for d uses; 0 if d does not run on the bf16 v2 kernel */
int simt_conv_mtiles(const simt_conv_desc* d);
int simt_conv_inbn_ok(const simt_conv_desc* d);        /* ABI 2: may d carry in_scale / in_shift / in_out (see simt_conv_desc)? */

/* ---- convolution: wgrad (split-K over pixels, transposed MFMA operands) -------------------------------
 * slab[split][co][tap*Cin+ci] = sum_{m in split} dy[m][co] * x[pixel(m)*stride + (dy,dx)[tap]][ci]
 * then simt_wgrad_reduce sums the splits in fixed order into the OIHW fp32 gradient.
 * replaces the weight gradient autograd computes for the convs above (tools/trainV2_simt.py:428). */
typedef struct {
  const void* dy;      /* [B*Ho*Wo][ldd] dtype; channels >= Cd are ignored */
  const void* x;       /* [B][H][W][Cin] dtype */
  float* slab;         /* [nsplit][Cd][ntaps*Cin] fp32 workspace */
  int32_t B, H, W, Cin, Ho, Wo, Cd, ldd, stride, ntaps, nsplit, dtype;
  int16_t dy_[SIMT_MAX_TAPS], dx_[SIMT_MAX_TAPS];
} simt_wgrad_desc;
int simt_conv_wgrad(const simt_wgrad_desc* d, simt_stream_t stream);
int simt_wgrad_reduce(const float* slab, float* dst, int nsplit, int Cd, int Ktot, int Cin, int co_off, int tap_off,
                      int Cout, int RS, int accumulate, simt_stream_t stream);
/* Grouped launch: n <= SIMT_WGRAD_MULTI_MAX problems with the SAME nsplit (the convs of one Bottleneck: the same pixels) as one tile list,
 * so that a much coarser pixel split fills the chip (fewer, longer slabs; one launch).  Each problem keeps its own slab and its own
 * simt_wgrad_reduce; results equal simt_conv_wgrad's with that nsplit bit for bit.  The per-problem arguments live in a DEVICE table
 * the caller owns: simt_conv_wgrad_multi_prepare fills its host image (n * simt_conv_wgrad_multi_bytes() bytes) and returns the grid;
 * the caller copies it to device memory once and passes that to simt_conv_wgrad_multi.  simt_conv_wgrad_multi_ok: does the problem
 * qualify (the problems simt_conv_wgrad runs on its 128x256-tile bf16 kernel)? */
#define SIMT_WGRAD_MULTI_MAX 16
int simt_conv_wgrad_multi_ok(const simt_wgrad_desc* d);
int simt_conv_wgrad_multi_bytes(void);
int simt_conv_wgrad_multi_prepare(const simt_wgrad_desc* d, int n, void* table_host, int* grid, int* tile_co);
int simt_conv_wgrad_multi(const void* table_dev, int n, int grid, int nsplit, int tile_co, simt_stream_t stream);
/* dY channels per output tile of the bf16 kernel for this problem: 256 (Cd a multiple of 256 and enough pixels: conv_wgrad3, 256 x 256 tile, half the
 * staged bytes per MAC) or 128; a grouped launch takes 256 only if every problem does (returned by _prepare in *tile_co).  The split
 * count that fills the chip depends on it: tiles = ceil(Cd / tile_co) * ceil(ntaps * Cin / 256). */
#define SIMT_WGRAD3_MIN_PIXELS 16384   /* the 256-row tile needs B * Ho * Wo >= this (fewer pixels: the extra splits cost more than they save) */
int simt_conv_wgrad_tile_co(const simt_wgrad_desc* d);
/* The reduces of a grouped launch as ONE launch: a device table of n <= 2 * SIMT_WGRAD_MULTI_MAX jobs (the arguments of simt_wgrad_reduce; needs Cin % 4 == 0,
 * Ktot % 4 == 0, 16-byte aligned slab and dst).  Job j owns blocks [block0, block0 + simt_wgrad_reduce_blocks(Cout, RS, Cin)); `blocks` = their
 * total.  Per element the same sum in the same order as simt_wgrad_reduce: bitwise the same gradients. */
typedef struct {
  const float* slab;
  float* dst;
  int32_t nsplit, Cd, Ktot, Cin, co_off, tap_off, Cout, RS, accumulate, block0;
} simt_wgrad_reduce_job;
int simt_wgrad_reduce_multi(const simt_wgrad_reduce_job* jobs_dev, int n, int blocks, simt_stream_t stream);
int simt_wgrad_reduce_blocks(int Cout, int RS, int Cin);   /* 256-thread blocks of one job (3x3: a thread owns 4 channels x 9 taps) */

/* ---- tap-expanded ASPP classifier (bf16 throughput path; model/deeplab_multi.py:104-119) -------------------------
 * The N = Q = 22 dilated conv is re-associated into a plain GEMM with one output column per (tap, class) plus a
 * tap gather-sum (forward) / tap scatter (backward); see csrc/head_expand.hip.
 *   simt_tap_gather_sum: dst[m][n] = bias[n] + sum_t src[m + (dy,dx)[t]][t*QP + n]       (fp32 -> fp32)
 *   simt_tap_scatter   : dst[m][t*QP + n] = src[m - (dy,dx)[t]][n], 0 outside the image   (bf16 -> bf16)
 *   simt_wgrad_reduce_exp: slab[split][(tap_off+t)*QP + row_off + co][ci] -> OIHW fp32 gradient */
typedef struct {
  const void* src;
  const float* bias;   /* [Q] or NULL (gather_sum only) */
  void* dst;
  int32_t B, H, W, Q, QP, lds, ldd, ntaps;   /* lds / ldd: row pitch of src / dst in elements */
  int16_t dy[SIMT_MAX_TAPS], dx[SIMT_MAX_TAPS];
} simt_tap_desc;
int simt_tap_gather_sum(const simt_tap_desc* d, simt_stream_t stream);
int simt_tap_scatter(const simt_tap_desc* d, simt_stream_t stream);
int simt_wgrad_reduce_exp(const float* slab, float* dst, int nsplit, int Cd, int Cin, int QP, int row_off, int tap_off,
                          int Cout, int RS, simt_stream_t stream);

/* ---- weight packing / BN folding ------------------------------------------------------------------------ */
int simt_pack_weight(const float* w, void* dst, int Cout, int Cin, int RS, int row_off, int tap_off, long ldk, int Ck,
                     int mode, const float* cscale, int dtype, simt_stream_t stream);
/* batched form: jobs = device array of {const float* w; void* dst; const float* cscale; int64 ldk, total; int32 Cout, Cin, RS,
 * row_off, tap_off, Ck, mode, dtype} (72 bytes), chunks = device int32 [nchunks][2] (job, 32x32 (cout, cin) tile index) */
int simt_pack_weight_multi(const void* jobs, const void* chunks, int nchunks, int chunk, simt_stream_t stream);
int simt_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* scale,
                 float* shift, int C, simt_stream_t stream);

/* ---- BatchNorm2d, train mode with frozen affine (model/deeplab_multi.py:63-76; quirk: batch stats are used and
 * back-propagated through although gamma/beta never change) ------------------------------------------------ */
int simt_bn_finalize(const float* part, int nblk, int C, long count, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps, float* mean, float* rstd,
                     float* scale, float* shift, simt_stream_t stream);
int simt_bn_apply(const void* y, const float* scale, const float* shift, const void* res, const void* y2,
                  const float* scale2, const float* shift2, void* z, long M, int C, int relu, int dtype,
                  simt_stream_t stream);
/* same, and bits[(m*C + c) / 8] bit (c & 7) = (z[m][c] > 0): the ReLU mask of the block output (model/deeplab_multi.py:99-100)
 * for simt_bn_bwd's mask_mode 3 -- the backward then reads M*C/8 bytes instead of z (M*C elements) in both of its passes */
int simt_bn_apply_bits(const void* y, const float* scale, const float* shift, const void* res, const void* y2,
                       const float* scale2, const float* shift2, void* z, unsigned char* bits, long M, int C, int relu,
                       int dtype, simt_stream_t stream);
typedef struct {
  const void* dz;      /* [M][C] upstream gradient */
  const void* z;       /* [M][C] block output (mask_mode 1) or NULL */
  const void* y;       /* [M][C] raw conv output */
  const float *mean, *rstd, *scale, *shift;
  const void* y2;      /* second BN sharing the masked gradient (downsample branch) or NULL */
  const float *mean2, *rstd2, *scale2;
  float* part;         /* [simt_bn_bwd_nblk(M,C)][3][C] workspace */
  float* coef;         /* [3][C] workspace */
  void* dy;            /* [M][C] gradient wrt y */
  void* dy2;           /* [M][C] gradient wrt y2 or NULL */
  void* gout;          /* [M][C] masked gradient (may alias dz) or NULL */
  int64_t M;
  int32_t C, mask_mode, dtype; /* mask_mode: 0 none, 1 z>0, 2 y*scale+shift>0, 3 z = bit mask of simt_bn_apply_bits */
  float *dgamma, *dbeta;   /* [C] or NULL: gradients of a TRAINABLE affine (model/deeplabv3.py's torchvision BatchNorm) */
  float *dgamma2, *dbeta2; /* same for the second BN (y2) */
  int32_t reduce_done_nblk; /* > 0: `part` already holds that many [3][C] partial slots (written by the conv that produced dz,
                             * simt_conv_desc.bnr_*): skip the reduce pass */
} simt_bn_bwd_desc;
int simt_bn_bwd_nblk(long M, int C);
int simt_bn_bwd(const simt_bn_bwd_desc* d, simt_stream_t stream);

/* ---- stem: 7x7/s2 conv via im2col, BN+ReLU+MaxPool(3,2,1,ceil) (model/deeplab_multi.py:127-133,172-176) --- */
/* ---- direct 7x7 stride-2 pad-3 stem convolution (round 6; model/deeplab_multi.py:127,172-173: conv1 of the ResNets) ----
 * Replaces simt_im2col_stem + simt_conv_fprop on the im2col matrix for the bf16 throughput mode: the image patch of an 8 x 32 output tile is
 * staged in LDS as [row][col][channel], a filter ROW (7 taps x 3 channels = 21 contiguous values) is one 32-deep MFMA k-step.  Up to TWO weight
 * sets in one launch (the trainable and the frozen network convolve the same image, tools/trainV2_simt.py:351-353,370): per set
 *   y[s][m][0..63] = act( sum_{r,s,c} x[b][c][2 oy - 3 + r][2 ox - 3 + s] * w[s][o][r][s*3 + c] + bias[s][o] ),  bf16 NHWC,
 * stats[s] (optional): [simt_stem7_tiles][2][64] per-tile sum / sum of squares of the STORED values (BatchNorm batch statistics; hand
 * simt_stem7_tiles(...) as the slot count to simt_bn_finalize).  w[s]: simt_stem7_pack(conv1.weight [64][3][7][7] fp32, per-channel scale
 * or NULL) -> bf16 [64][7][32].  The weight gradient of the stem still runs on the im2col matrix (built in the backward). */
typedef struct {
  const float* x;          /* [B][3][H][W] fp32 (the reference's NCHW input tensor) */
  int32_t B, H, W, Ho, Wo;
  int32_t nsets;           /* 1 | 2 */
  const void* w[2];
  void* y[2];              /* [B*Ho*Wo][64] bf16 */
  const float* bias[2];    /* [64] or NULL */
  int32_t relu[2];
  float* stats[2];         /* or NULL */
} simt_stem_desc;
int simt_stem7_tiles(int B, int Ho, int Wo);
int simt_stem7_pack(const float* w_oihw, const float* cscale, void* dst, simt_stream_t stream);
int simt_stem7_fwd(const simt_stem_desc* d, simt_stream_t stream);
/* Weight gradient of the stem convolution straight from the image (replaces simt_im2col_stem + simt_conv_wgrad + simt_wgrad_reduce for conv1,
 * tools/trainV2_simt.py:428): dw[o][c][r][s] = sum_pixels dy[p][o] * x[b][c][2 oy - 3 + r][2 ox - 3 + s], fp32 accumulation, the per-workgroup partials
 * added in fixed order (bitwise reproducible).  part: [simt_stem7_wgrad_workgroups(B, Ho, Wo)][64 * 7 * 32] fp32 workspace; dw is overwritten. */
int simt_stem7_wgrad_workgroups(int B, int Ho, int Wo);
int simt_stem7_wgrad(const float* x_nchw, const void* dy, float* part, float* dw, int B, int H, int W, int Ho, int Wo, simt_stream_t stream);

int simt_im2col_stem(const float* x_nchw, void* A, int B, int Cin, int H, int W, int Ho, int Wo, int KH, int KW,
                     int stride, int pad, int ldk, int dtype, simt_stream_t stream);
int simt_bn_relu_maxpool(const void* y, const float* scale, const float* shift, void* p, unsigned char* idx, int B,
                         int H, int W, int C, int Hp, int Wp, int dtype, simt_stream_t stream);
int simt_maxpool_bwd(const void* dp, const unsigned char* idx, void* da, int B, int H, int W, int C, int Hp, int Wp,
                     int dtype, simt_stream_t stream);
int simt_scatter_stride(const void* src, void* dx, int B, int H, int W, int C, int Ho, int Wo, int stride, int dtype,
                        simt_stream_t stream);
int simt_colsum(const void* src, float* out, long M, int ld, int C, int accumulate, int dtype, simt_stream_t stream);
/* VGG trunk (model/deeplab_vgg.py:24-43): MaxPool2d(2,2) forward (+ arg-max bytes) and its backward fused with the ReLU
 * mask of the conv output y it pooled; bias gradients of wide layers (C <= 2048) */
int simt_maxpool2(const void* y, void* p, unsigned char* idx, int B, int H, int W, int C, int dtype, simt_stream_t stream);
int simt_maxpool2_bwd(const void* dp, const unsigned char* idx, const void* y, void* da, int B, int H, int W, int C, int dtype,
                      simt_stream_t stream);
int simt_colsum_wide(const void* src, float* out, long M, int ld, int C, int dtype, simt_stream_t stream);

/* ---- fused SimT head: upsample + softmax + per-pixel loss terms + anchors (tools/trainV2_simt.py:351-409,
 * :202-230 Placeholder_loss, utils/loss.py:14-40) ------------------------------------------------------- */
typedef struct {
  const float* pred1;   /* [B*h*w][ldp] fp32 low-res logits of the aux head (first Q channels) */
  const float* pred2;   /* [B*h*w][ldp] main head */
  const float* fixp;    /* [B*h*w][ldf] softmax probabilities of the frozen model's main head (first C channels) */
  const int64_t* label; /* [B][H][W] noisy pseudo labels, 255 = ignore */
  const float* T1;      /* [Q][C] transition matrices (simt_ntm_inner_loop / simt_sig_ntm) */
  const float* T2;
  float* part;          /* [simt_head_nblk][simt_head_part_floats] workspace */
  void* keys;           /* [simt_head_keys_count] u64 workspace (zeroed by the call) */
  float* hout;          /* [simt_head_hout_floats] result block, layout in csrc/head_loss.hip */
  float* g1;            /* [2][B][H][w][QP] workspace (simt_head_grad) */
  float* dpred1_f32;    /* [B*h*w][ld_f32] gradient outputs (any may be NULL) */
  float* dpred2_f32;
  void* dpred1_t;       /* [B*h*w][ld_t] gradient in grad_dtype for the dgrad GEMM (pad columns untouched) */
  void* dpred2_t;
  int32_t B, h, w, H, W, C, Q, ldp, ldf, QP, ld_f32, ld_t, grad_dtype;
  float th_high, th_low, lambda_seg, lambda_place, gscale;
  int32_t mode;         /* 0: SimT loss block.  1: warm-up stage (tools/trainV1_warmup.py:217-224): CE of both heads against
                         * `label` (ignore 255); fixp/T1/T2 unused (may be NULL); hout[0],[1] = loss_seg1/2, hout[14] = total */
  int32_t single;       /* 1: one-output model (model/deeplabv3.py, model/deeplab_vgg.py return ONE tensor): pred1 / T1 / dpred1_* are
                         * unused (may be NULL) and every auxiliary-head term is dropped; pred2 / T2 / dpred2_* carry the model's head.
                         * With mode 1 (the warm-up stage of such a model): hout[1] = hout[14] = CE of that head against `label`, g1's
                         * head-1 rows are not written, fixp / T1 / T2 may be NULL */
  int32_t up_half_pixel; /* 0: interp_target = nn.Upsample(bilinear, align_corners=True) (tools/trainV2_simt.py:301);
                          * 1: F.interpolate(bilinear), align_corners=False, the in-model upsample of model/deeplabv3.py:137 fused here */
  int32_t fix_logits;   /* 1: fixp holds the frozen model's low-res LOGITS; posterior = softmax(upsample(logits)) -- what
                         * trainV2_simt.py:354 computes for a model that upsamples inside.  0: fixp = low-res probabilities */
  uint8_t* conf_out;    /* optional (may be NULL): [B][H][W] the per-pixel `Conf_label_target` of trainV2_simt.py:357-362,387-393
                         * as simt_head_loss decided it: class index 0..Q-1, 255 = no confidence label (mode 1: the label itself) */
  uint8_t* label_ws;    /* optional workspace (may be NULL): [B][H][W].  With conf_out AND label_ws given, simt_head_loss also stores each pixel's
                         * checked noisy label and simt_head_grad reads the two byte maps back (they must still hold what simt_head_loss of the
                         * same inputs wrote) instead of deciding the labels again from fixp and the 8-byte labels: same values, fewer bytes */
} simt_head_desc;
int simt_head_nblk(int B, int H, int W);
int simt_head_part_floats(int Q, int C);
int simt_head_hout_floats(int Q, int C);
int simt_head_keys_count(void);
int simt_softmax_rows(const float* in, int ldi, float* out, int ldo, long M, int C, simt_stream_t stream);
int simt_head_loss(const simt_head_desc* d, simt_stream_t stream);
int simt_head_grad(const simt_head_desc* d, simt_stream_t stream);
/* Two views (the weak-view teacher): the frozen operand of pixel p = (b, y, x) is read from item fb = min(fix_item[p], B - 1)
 * of fixp instead of item b -- the confidence label of pass 1, of pass 2 when it decides the labels again, and the anchor rows of hout.
 * pred1 / pred2 / label stay at item b.  fix_item: [B][H][W] bytes (the item map of simt_class_mix_items);  NULL: simt_head_loss /
 * simt_head_grad, launch for launch.  mode 1 has no frozen operand: a map with it is refused. */
int simt_head_loss_views(const simt_head_desc* d, const uint8_t* fix_item, simt_stream_t stream);
int simt_head_grad_views(const simt_head_desc* d, const uint8_t* fix_item, simt_stream_t stream);

/* ---- NTM micro-solver (model/deeplab_multi.py:244-286, tools/trainV2_simt.py:326-339,412-424,435-436) ---- */
typedef struct {
  float* ntm[2];        /* [Q][C] NTM1/NTM2 parameters */
  float* w[2];          /* [Q][Q] sig_W weights (updated in place by Adam; diag := -1e4) */
  float* ntm_grad[2];   /* [Q][C] accumulated (+=): the inner-loop leak, SURVEY quirk 3 */
  float* w_m[2];        /* Adam exp_avg of w */
  float* w_v[2];        /* Adam exp_avg_sq of w */
  float* T_out[2];      /* [Q][C] T = sig_NTM() */
  const float* class_dist; /* [C] */
  int32_t Q, C, steps, step0; /* step0 = Adam steps already taken on w */
  float lr, beta1, beta2, eps; /* torch.optim.Adam semantics.  1 - beta and beta^step are formed in double from the betas as written (the shortest
                                * decimal that rounds to the float: 0.999f -> 0.999) and rounded once, as torch does from its double betas */
  int32_t single;       /* 1: only NTM / W number 1 (index [1]) exist -- one-output models; index [0] pointers may be NULL */
  const uint64_t* skip_if;   /* ABI 2.  Optional device word (simt_fbn_desc.err): the launch changes nothing while it is non-zero; NULL: always run */
} simt_ntm_inner_desc;
int simt_ntm_inner_loop(const simt_ntm_inner_desc* d, simt_stream_t stream);
typedef struct {
  const float* ntm[2];
  float* w[2];
  float* ntm_grad[2];
  const float* class_dist;
  const float* hout;    /* from simt_head_loss */
  float* lout;          /* [16]: total*gscale, loss_p1, loss_p2, loss_y1, loss_y2, Place, Convex, Volume, Anchor, vol_ok, log-vol x2,
                           [12] += hout[15] (labels outside [0,C) and != 255, ACCUMULATED until the caller clears it) */
  int32_t Q, C;
  float lambda_seg, lambda_convex, lambda_volume, lambda_anchor, gscale;
  int32_t single;       /* 1: Convex / Volume / Anchor / total over NTM [1] only, no lambda_seg terms */
} simt_ntm_post_desc;
int simt_ntm_post(const simt_ntm_post_desc* d, simt_stream_t stream);
int simt_sig_ntm(const float* ntm, const float* class_dist, const float* dT, float* T_out, float* dN_out, int Q, int C,
                 simt_stream_t stream);
int simt_sig_w(float* weight, const float* dW, float* W_out, float* dweight_out, int Q, simt_stream_t stream);
int simt_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                   int step, simt_stream_t stream);
/* ABI 2: the same step, skipped (parameter AND moments untouched) while *skip_if != 0 -- the guard simt_sgd_desc.skip_if gives the SGD launch */
int simt_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                           int step, const uint64_t* skip_if, simt_stream_t stream);

/* ---- fused SGD with duplicate-listing semantics (tools/trainV2_simt.py:296-297,434; model/deeplab_multi.py:194-237) --- */
typedef struct {
  const void* segs;    /* device array of {float* p; const float* g; float* buf; int64 n; int32 mult; int32 group} */
  const void* chunks;  /* device int32 [nchunks][2]: (segment index, chunk index inside the segment) */
  int32_t nchunks, chunk;
  float lr[4], wd[4];  /* per param group */
  float momentum, dampening;
  int32_t first_step;  /* 1: momentum buffers are created (= d_p) like torch's first step */
  const uint64_t* skip_if;   /* optional device word (simt_fbn_desc.err): the launch changes nothing while it is non-zero; NULL: always update */
} simt_sgd_desc;
int simt_sgd_multi(const simt_sgd_desc* d, simt_stream_t stream);

/* ---- multi-tensor AdamW (decoupled weight decay; torch.optim.AdamW's single-tensor order), every tensor listed once: DESIGN 7.23 ----
 * One launch per optimiser step in the launch shape of simt_sgd_multi: one 256-lane workgroup per (segment, chunk) entry, 16-byte loads and
 * stores where p, g, m and v are all 16-byte aligned at the chunk's start, dwords otherwise and for the tail (the same bits either way).
 * Per element, with g the gradient and `grp` the segment's group:
 *   p = p * decay[grp];  m = m + (g - m) * omb1;  v = v * beta2 + omb2 * g * g;  p = p - step_size[grp] * (m / (sqrtf(v) / bc2s + eps))
 * The caller forms the per-step constants in double and rounds each once to fp32, as simt_adam_step_guarded does for its own:
 *   step_size[grp] = lr / (1 - beta1^t),  decay[grp] = 1 - lr * wd,  bc2s = sqrt(1 - beta2^t),  omb = 1 - beta   (t = 1 on the first step).
 * SIMT_ERR_INVALID and no launch: NULL tables, nchunks <= 0, chunk <= 0, a beta outside [0, 1), eps <= 0, bc2s <= 0, a non-finite constant. */
typedef struct {
  const void* segs;    /* device array of {float* p; const float* g; float* m; float* v; int64 n; int32 group; int32 pad} */
  const void* chunks;  /* device int32 [nchunks][2]: (segment index, chunk index inside the segment), as simt_sgd_desc */
  int32_t nchunks, chunk;
  float step_size[4], decay[4];  /* per param group */
  float beta1, beta2, omb1, omb2;
  float bc2s, eps;
  int32_t first_step;  /* 1: the moments are created (m = g * omb1, v = omb2 * g * g); m and v are not read */
  const uint64_t* skip_if;   /* optional device word (simt_fbn_desc.err): the launch changes nothing while it is non-zero; NULL: always update */
} simt_adamw_desc;
int simt_adamw_multi(const simt_adamw_desc* d, simt_stream_t stream);
/* dst[i] (+)= src[i], fp32: bias of the fused 2-branch ASPP GEMM = sum of the branch biases (deeplab_multi.py:115-119) */
int simt_vec_acc(float* dst, const float* src, int n, int accumulate, simt_stream_t stream);

/* ---- utils/loss.py: CrossEntropy2d (:6-40) and EntropyLoss (:42-49) on NCHW fp32 predictions ----------------------
 * ws: simt_loss_ws_bytes() bytes of device scratch.  out[0] = loss (mean over valid pixels, weighted like
 * F.cross_entropy / F.nll_loss with reduction='mean'), out[1] = denominator.  Zero valid pixels -> NaN (reference). */
int simt_loss_ws_bytes(void);
int simt_ce2d_fwd(const float* pred, const int64_t* target, const float* weight, int n, int c, int h, int w,
                  int ignore_label, int is_softmax, void* ws, float* out, simt_stream_t stream);
int simt_ce2d_bwd(const float* pred, const int64_t* target, const float* weight, int n, int c, int h, int w,
                  int ignore_label, int is_softmax, const float* out, const float* grad_out, float* dpred,
                  simt_stream_t stream);
int simt_entropy2d(const float* x, int n, int c, int h, int w, void* ws, float* out, const float* grad_out, float* dx,
                   simt_stream_t stream);

/* ---- evaluation (tools/evaluate_cityscapes.py:96-162 evaluate_simt; :81-83 fast_hist) --------------------------------
 * pred[b][y][x] = argmax_c ( up(la)[c] + up(lb)[c] ), bilinear align_corners=True to (H, W), first index on ties;
 * lb may be NULL (single scale).  hist[n*gt + pred] += 1 for 0 <= gt < n (int64, accumulates across calls). */
int simt_upsample_sum_argmax(const float* la, int ha, int wa, int lda, const float* lb, int hb, int wb, int ldb, int B, int H,
                             int W, int C, int32_t* pred, simt_stream_t stream);
int simt_confusion_hist(const int64_t* gt, const int32_t* pred, long P, int n, int64_t* hist, simt_stream_t stream);
/* the same for a model that upsamples inside (model/deeplabv3.py:137): scale s is first resampled from its NHWC logits [B][h_s][w_s][ld_s]
 * to a VIRTUAL map [hi_s][wi_s] (align_corners=False, half-pixel, clamped at 0), that map to (H, W) (align_corners=True); pred = the
 * first-index arg-max of the sum over the scales.  lb may be NULL (single scale).  Nothing is written but pred. */
int simt_upsample2_sum_argmax(const float* la, int ha, int wa, int lda, int hia, int wia, const float* lb, int hb, int wb, int ldb,
                              int hib, int wib, int B, int H, int W, int C, int32_t* pred, simt_stream_t stream);
/* pseudo-label export (the save lines of evaluate_simt :150-156 / evaluate_warmup :214-219; trainV2_simt.py:353-359):
 * mode 0: out[b][y][x] = the label simt_upsample_sum_argmax writes (bit for bit), as uint8;
 * mode 1: la holds low-res PROBABILITIES (simt_softmax_rows of the logits), lb must be NULL: out = argmax_c up(la)[c] where
 *         max_c up(la)[c] > threshold (strictly), 255 elsewhere.
 * out: uint8 [B][H][W], 4-byte aligned.  counts: int64 [C+1] accumulated across calls (classes 0..C-1, then the 255s).  C <= 255. */
int simt_pseudo_label_u8(const float* la, int ha, int wa, int lda, const float* lb, int hb, int wb, int ldb, int B, int H, int W, int C,
                         int mode, float threshold, uint8_t* out, int64_t* counts, simt_stream_t stream);
/* the same for a model that upsamples inside (DeepLabv3), over the geometry of simt_upsample2_sum_argmax:
 * mode 0: out = the label simt_upsample2_sum_argmax writes (bit for bit), as uint8;
 * mode 1: la holds LOGITS, lb must be NULL: softmax over the first C channels at each virtual [hia][wia] sample (align_corners=False
 *         from la), the probabilities resampled to (H, W) (align_corners=True); out = their arg-max where max > threshold (strictly),
 *         255 elsewhere.
 * out / counts / C: as simt_pseudo_label_u8.  B*h*w*ld < 2^31 per scale. */
int simt_pseudo_label2_u8(const float* la, int ha, int wa, int lda, int hia, int wia, const float* lb, int hb, int wb, int ldb,
                          int hib, int wib, int B, int H, int W, int C, int mode, float threshold, uint8_t* out, int64_t* counts,
                          simt_stream_t stream);
/* online labels (the warm-up trainers' teacher): the confidence rule of mode 1 above, written as the int64 label the head
 * kernels read.  label[b][y][x] = arg where conf > threshold (strictly), 255 elsewhere; a NaN confidence or threshold gives 255.
 * family 0 (DeepLab-v2, VGG): (arg, conf) of simt_pseudo_label_u8 mode 1 (fix = low-res PROBABILITIES, align_corners=True), bit for bit;
 * family 1 (DeepLabv3): those of simt_pseudo_label2_u8 mode 1 called with hia = H, wia = W (fix = low-res LOGITS; softmax of their
 *   half-pixel resample to (H, W)), bit for bit; B*h*w*ld < 2^31.
 * Refused (SIMT_ERR_INVALID, nothing launched): a NULL pointer, a size <= 0, C > ld, C > 255, another family, label not 8-byte aligned,
 * the 2^31 limit of family 1.  The descriptor travels as kernel arguments: no device copy, no synchronisation. */
typedef struct {
  const float* fix;        /* [B*h*w][ld] fp32, first C channels.  family 0: probabilities (simt_softmax_rows); family 1: logits */
  int64_t* label;          /* out [B][H][W]: class index, 255 = ignore; every 8-byte word is written in full */
  int64_t* counts;         /* [C+1], accumulated across calls: classes 0..C-1, then the 255s (as simt_pseudo_label_u8) */
  int32_t B, h, w, ld, H, W, C, family;
  float threshold;
} simt_online_label_desc;
int simt_online_label(const simt_online_label_desc* d, simt_stream_t stream);
/* class-balanced pseudo labels (CBST / BDL: per-class confidence thresholds).  (arg, conf) of a pixel are the arg-max and the maximum
 * of mode 1 above, bit for bit: simt_pseudo_conf_u8 over the geometry of simt_pseudo_label_u8 (la = low-res PROBABILITIES),
 * simt_pseudo_conf2_u8 over that of simt_pseudo_label2_u8 (la = LOGITS), one scale.
 * hist != NULL: hist[arg][bin] += 1 for every pixel, bin = min(SIMT_CONF_BINS-1, max(0, (int)floorf(conf * SIMT_CONF_BINS))); int64
 *   [C][SIMT_CONF_BINS], accumulated across calls, exact and order independent; needs C <= 64.
 * out != NULL: out = arg where conf >= thr[arg], 255 elsewhere (uint8 [B][H][W], 4-byte aligned); counts as simt_pseudo_label_u8.
 *   thr: C floats in HOST memory, copied into the launch (no device buffer, no synchronisation); out needs thr and counts.
 * Both in one launch do both; both NULL is refused.  C <= 255. */
#define SIMT_CONF_BINS 256
int simt_pseudo_conf_u8(const float* la, int ha, int wa, int lda, int B, int H, int W, int C, const float* thr, uint8_t* out,
                        int64_t* counts, int64_t* hist, simt_stream_t stream);
int simt_pseudo_conf2_u8(const float* la, int ha, int wa, int lda, int hia, int wia, int B, int H, int W, int C, const float* thr,
                         uint8_t* out, int64_t* counts, int64_t* hist, simt_stream_t stream);
/* class-balanced online labels: one threshold per class, kept on the DEVICE and moved by every micro-batch.
 * State: thr[C], fp32, initialised by the caller (the warm-up trainers: to T for every class).  Per micro-batch, two launches:
 *
 * simt_online_label_cb -- label with the thresholds as they stand, and count in the same pass.  (arg, conf) of a pixel are those of
 *   simt_online_label (family 0: simt_pseudo_conf_u8's; family 1: simt_pseudo_conf2_u8's called with hia = H, wia = W), bit for bit.
 *   label[b][y][x] = arg where conf >= thr[arg], 255 elsewhere (a NaN confidence or threshold gives 255): the rule of simt_pseudo_conf*_u8;
 *   counts[C+1] as simt_online_label; hist[arg][bin] += 1 for EVERY pixel, bin as simt_pseudo_conf_u8 defines it (SIMT_CONF_BINS bins).
 *   thr is read from device memory when the kernel runs (into LDS at block start): no host copy, no synchronisation.
 *   Refused (SIMT_ERR_INVALID, nothing launched): a NULL pointer, a size <= 0, C > ld, C > 64 (the LDS histogram), another family, label or
 *   hist not 8-byte aligned, thr not 4-byte aligned, the 2^31 limit of family 1.
 *
 * simt_class_thresholds -- derive the batch thresholds from hist, fold them into thr, zero hist.  One small launch, no global atomics.
 *   Per class c, with n = the sum of hist[c][:] (exact 64-bit integers):
 *     n == 0: thr[c] stays, t = 0;
 *     else  k = min((int64)rint((double)n * drop), n - 1)          (drop = 1 - P formed by the caller in double; rint: half to even)
 *           b = the smallest bin whose inclusive cumulative count exceeds k
 *           t = fminf((float)b / SIMT_CONF_BINS, cap)
 *           thr[c] = thr[c] + omd * (t - thr[c])                    (fp32; subtract, multiply, add each rounded on its own: no FMA)
 *   t_out (optional) receives t; hist is zero afterwards (plain stores).  This is class_thresholds() of tools/make_pseudo_labels.py with
 *   cap, followed by the arithmetic form of simt_ema_desc.
 *   Refused: NULL hist / thr, C outside 1..64, hist not 8-byte aligned, thr / t_out not 4-byte aligned, drop outside [0, 1), omd outside
 *   (0, 1], a NaN cap. */
typedef struct {
  const float* fix;        /* as simt_online_label_desc */
  int64_t* label;          /* out [B][H][W] */
  int64_t* counts;         /* [C+1], accumulated */
  int64_t* hist;           /* [C][SIMT_CONF_BINS], accumulated */
  const float* thr;        /* [C] fp32 in DEVICE memory */
  int32_t B, h, w, ld, H, W, C, family;
} simt_online_label_cb_desc;
int simt_online_label_cb(const simt_online_label_cb_desc* d, simt_stream_t stream);
typedef struct {
  int64_t* hist;           /* [C][SIMT_CONF_BINS]: read, then zeroed */
  float* thr;              /* [C] in / out */
  float* t_out;            /* [C] out: the batch thresholds (0 for a class without pixels), or NULL */
  double drop;             /* 1 - P */
  int32_t C;
  float cap, omd;          /* omd = (float)(1 - M) */
} simt_class_thresholds_desc;
int simt_class_thresholds(const simt_class_thresholds_desc* d, simt_stream_t stream);
/* test-time augmentation (mirror / multi-scale): the label of n <= SIMT_TTA_MAX maps ("terms", one forward each), any of which may belong
 * to the horizontally mirrored frame.  Value of term t, channel c, at label pixel (b, y, x), fp32:
 *   one-resample family (hi == wi == 0): the value simt_upsample_sum_argmax forms for that map (align_corners=True, ATen's association);
 *     with `flip` every tap's column index ix is read at w-1-ix, weights unchanged -- bit for bit the plain term on the column-reversed map;
 *   two-resample family (hi, wi > 0): the value simt_upsample2_sum_argmax forms; with `flip` each virtual column vx of the outer
 *     (align_corners=True) taps becomes wi-1-vx before the inner (align_corners=False) taps are formed.
 * mode 0: s[c] = ((v_0[c] + v_1[c]) + v_2[c]) + ... in term order; label = first-index arg-max; written to pred and / or out (+ counts,
 *   whose 255 bin stays 0).
 * mode 1 (one-resample family; maps = simt_softmax_rows PROBABILITIES): p[c] = (v_0[c] + ... + v_{n-1}[c]) * (1.0f / n); (arg, conf) = its
 *   first-index arg-max and maximum; out (+ counts) as simt_pseudo_label_u8 mode 1 (thr == NULL: kept where conf > threshold) or as
 *   simt_pseudo_conf_u8 (thr != NULL: kept where conf >= thr[arg]); hist as simt_pseudo_conf_u8.  out, hist or both in one launch.
 * Refused (SIMT_ERR_INVALID, nothing launched): n outside 1..SIMT_TTA_MAX, terms of both families, mode 1 in the two-resample family, pred
 * in mode 1, thr / hist in mode 0, out without counts, nothing to write, C > ld of a term, hist with C > 64, B*h*w*ld >= 2^31 for a term.
 * The descriptor is read on the host during the call and travels as kernel arguments: no device copy, no synchronisation. */
#define SIMT_TTA_MAX 8
typedef struct {
  const float* l;          /* [B][h][w][ld] fp32, first C channels used */
  int32_t h, w, ld;
  int32_t hi, wi;          /* 0, 0: one resample (h, w) -> (H, W); > 0: two resamples through a virtual [hi][wi] map */
  int32_t flip;            /* the map belongs to the horizontally mirrored frame */
} simt_tta_term;
typedef struct {
  simt_tta_term t[SIMT_TTA_MAX];
  int32_t n;               /* 1 .. SIMT_TTA_MAX; all terms of one family */
  int32_t B, H, W, C;      /* C <= 255; C <= ld of every term */
  int32_t mode;            /* 0: logits, summed.  1: probabilities, averaged */
  float threshold;         /* mode 1 with thr == NULL */
  const float* thr;        /* mode 1: C floats in HOST memory (copied into the launch), or NULL */
  int32_t* pred;           /* [B][H][W] int32 arg-max, or NULL (mode 0 only) */
  uint8_t* out;            /* [B][H][W] uint8 labels, 4-byte aligned, or NULL */
  int64_t* counts;         /* [C+1] accumulated, required with out */
  int64_t* hist;           /* mode 1: [C][SIMT_CONF_BINS] accumulated, C <= 64, or NULL */
} simt_tta_desc;
int simt_tta_label(const simt_tta_desc* d, simt_stream_t stream);
/* F.interpolate(bilinear) of an NHWC fp32 map [B][h][w][lds] (first C channels) to NCHW fp32 [B][C][H][W] and its adjoint
 * (model/deeplabv3.py:137 upsamples inside the model with align_corners=False; align_corners=1 = interp_target) */
int simt_upsample_nchw(const float* src, int B, int h, int w, int lds, int C, int H, int W, int align_corners, float* dst,
                       simt_stream_t stream);
int simt_upsample_nchw_bwd(const float* ddst, int B, int h, int w, int lds, int C, int H, int W, int align_corners,
                           void* dsrc, int dtype, float* tmp, simt_stream_t stream); /* dsrc [B][h][w][lds] in dtype, first C
                           * channels; tmp: caller-owned scratch of B*C*H*w floats (the x-folded intermediate of the separable adjoint) */

/* ---- offline NTM utilities (tools/compute_ClassDistribution.py:49-51,66-86 `fast_hist(a, n)` = bincount of the pseudo labels;
 * tools/compute_ConfusionMatrix.py:54-56,68-98 `fast_hist(a, b, n33, n19)` = bincount(n19 * a + b) after label_mapping) -------------
 * hist[lut[a[p]] * nb + b[p]] += 1 over uint8 images (int64, accumulates across calls); a == NULL: one row (class distribution);
 * lut: 256-entry label_mapping table or NULL (identity); entries with row >= na or b >= nb (255 = ignore) are skipped. */
int simt_hist2d_u8(const unsigned char* a, const unsigned char* b, long P, int na, int nb, const unsigned char* lut, int64_t* hist,
                   simt_stream_t stream);

/* ---- input pipeline (dataset/cityscapes_dataset.py:101-120 after PNG decoding) -----------------------------------------
 * The reference resizes with Pillow on the CPU (Image.resize BICUBIC / NEAREST) and converts to float32 BGR - mean, CHW.
 * simt_resample_u8 applies ONE pass of Pillow's 8-bit separable resampler (Resample.c: 22-bit fixed-point coefficients,
 * result = clip8(((1 << 21) + sum) >> 22)) along x (axis 1: [N][H][W][C] -> [N][H][out][C]) or y (axis 0: -> [N][out][W][C]);
 * bounds [out][2] = (first source index, count) and kk [out][ksize] are the tables of precompute_coeffs /
 * normalize_coeffs_8bpc, computed by the caller in double: the output equals Pillow's byte for byte.  C in {1, 3}.
 * simt_image_to_input: [N][H][W][3] u8 RGB -> [N][3][H][W] fp32, channel c = rgb[2 - c] - mean_c (BGR - IMG_MEAN, :113-116);
 * rgb_order = 1 keeps RGB (the reference's --random-mirror branch reverses the channel axis, :108-111).
 * simt_label_nearest: dst[n][y][x] = (int64) src[n][ytab[y]][xtab[flip_x ? Wo-1-x : x]] (ImagingScaleAffine index tables). */
int simt_resample_u8(const unsigned char* src, unsigned char* dst, int N, int H, int W, int C, int out, int axis,
                     const int* bounds, const int* kk, int ksize, simt_stream_t stream);
int simt_image_to_input(const unsigned char* rgb, float* x, int N, int H, int W, float mean0, float mean1, float mean2,
                        int rgb_order, simt_stream_t stream);
int simt_label_nearest(const unsigned char* src, long long* dst, int N, int H, int W, int Ho, int Wo, const int* ytab,
                       const int* xtab, int flip_x, simt_stream_t stream);

/* ---- device-resident dataset cache (simt_amd/data/cache.py; csrc/dataset_cache.hip) -------------------------------------
 * The resized frame is uint8 (Pillow's resize returns uint8), so it can be kept in HBM exactly: image slot [h][w][3] u8 RGB
 * (what simt_resample_u8 writes), label slot [h][w] u8.
 * simt_label_nearest_u8: dst[n][y][x] = src[n][ytab[y]][xtab[x]] -- simt_label_nearest with a uint8 destination and no flip.
 * simt_cache_gather: one launch per batch.  For item b < B: x[b][c][y][x'] = img[b][y][x'][mirror[b] ? c : 2 - c] - mean[c]
 * (simt_image_to_input, rgb_order = mirror[b]) and lab_out[b][y][x'] = (int64) lab[b][y][mirror[b] ? w-1-x' : x']
 * (simt_label_nearest's flip_x), bit for bit.  Slots are given by pointer (any order, any slab, repeats allowed), each 16-byte
 * aligned like x and lab_out; lab_out NULL: images only (lab[] is not read).  The descriptor is read on the host during the call
 * and travels as kernel arguments: nothing is copied to the device and nothing synchronises.  Any h, w; B <= SIMT_GATHER_MAX. */
#define SIMT_GATHER_MAX 64
typedef struct {
  const unsigned char* img[SIMT_GATHER_MAX];
  const unsigned char* lab[SIMT_GATHER_MAX];
  unsigned char mirror[SIMT_GATHER_MAX];
  float* x;              /* [B][3][h][w] fp32 */
  long long* lab_out;    /* [B][h][w] int64, or NULL */
  int32_t B, h, w;
  float mean[3];
} simt_gather_desc;
int simt_label_nearest_u8(const unsigned char* src, unsigned char* dst, int N, int H, int W, int Ho, int Wo, const int* ytab,
                          const int* xtab, simt_stream_t stream);
int simt_cache_gather(const simt_gather_desc* d, simt_stream_t stream);

/* ---- random scale + crop on the device (simt_amd/data/scale_crop.py; csrc/scale_crop.hip) ---------------------------------
 * simt_scale_crop: one launch per batch.  Item b < B is the window of size w x h at origin (ox[b], oy[b]) of
 * S = Image.resize((ws, hs), BICUBIC) of its Hs x Ws source frame, ws / hs those of choice c[choice[b]]:
 *   x[b][p][y][x'] = S[y + oy][x' + ox][mirror[b] ? p : 2 - p] - mean[p] inside S, 0.0f outside;
 *   lab_out[b][y][x'] = (int64) lab[b][ytab[y + oy]][xtab[x'' + ox]], x'' = mirror[b] ? w-1-x' : x', inside, 255 outside
 * (the mirror rule of simt_cache_gather).  S is never stored: a workgroup owns SIMT_SCALE_CROP_TILE_H x SIMT_SCALE_CROP_TILE_W output
 * pixels, runs Pillow's horizontal pass for the source rows they need into LDS as uint8 and the vertical pass out of LDS, so the
 * result equals Pillow's byte for byte.  `tables` is ONE device buffer of int32; per choice the offsets (in int32) of bounds_x
 * [ws][2], coefficients_x [ws][ksx], bounds_y [hs][2], coefficients_y [hs][ksy] (resample.bicubic_tables) and of the NEAREST index
 * tables xtab [ws], ytab [hs].  max_rows: the most source rows one tile's vertical pass reads, over all choices, origins and tiles
 * (the caller computes it from bounds_y); the LDS the launch needs, simt_scale_crop_lds_bytes, must not exceed
 * SIMT_SCALE_CROP_LDS_MAX.  lab_out NULL: images only.  The descriptor travels as kernel arguments, like simt_gather_desc. */
#define SIMT_SCALE_CROP_MAX 64
#define SIMT_SCALE_CROP_CHOICES 16
#define SIMT_SCALE_CROP_TILE_H 16
#define SIMT_SCALE_CROP_TILE_W 64
#define SIMT_SCALE_CROP_LDS_MAX 65536
typedef struct {
  int32_t ws, hs, ksx, ksy;
  int32_t bounds_x, coef_x, bounds_y, coef_y, xtab, ytab;
} simt_scale_crop_choice;
typedef struct {
  const unsigned char* img[SIMT_SCALE_CROP_MAX];   /* [Hs][Ws][3] u8 RGB */
  const unsigned char* lab[SIMT_SCALE_CROP_MAX];   /* [Hs][Ws] u8 */
  int32_t ox[SIMT_SCALE_CROP_MAX], oy[SIMT_SCALE_CROP_MAX];
  unsigned char choice[SIMT_SCALE_CROP_MAX];
  unsigned char mirror[SIMT_SCALE_CROP_MAX];
  simt_scale_crop_choice c[SIMT_SCALE_CROP_CHOICES];
  const int32_t* tables;
  float* x;              /* [B][3][h][w] fp32 */
  long long* lab_out;    /* [B][h][w] int64, or NULL */
  int32_t B, Hs, Ws, h, w, n_choices, max_rows;
  int32_t n_tables;      /* int32 elements in `tables`: every offset + extent above is checked against it */
  float mean[3];
} simt_scale_crop_desc;
long simt_scale_crop_lds_bytes(const simt_scale_crop_desc* d);   /* < 0: the descriptor is invalid */
int simt_scale_crop(const simt_scale_crop_desc* d, simt_stream_t stream);

/* ---- rare-class crops: the window is picked on the device (simt_amd/data/rare_class.py; csrc/rare_crop.hip) ------------
 * DAFormer's rare-class sampling re-draws the crop until it holds enough pixels of the sampled class.  Here the host draws K candidate
 * windows (choice, ox, oy) per item, and three launches on one stream count, pick and crop -- the pick reaches the crop through `win`
 * in device memory, nothing is read back.
 *
 * simt_rare_crop_counts: for item b < B, candidate k < K and c = cls[b] < 255, with ws, hs, xtab, ytab those of choice
 *   ci = cand_choice[b][k] and (ox, oy) = (cand_ox[b][k], cand_oy[b][k]):
 *     count[b][k] = #{ (y, x) in h x w : 0 <= y + oy < hs, 0 <= x + ox < ws, lab[b][ytab[y + oy]][xtab[x + ox]] == c }
 *   -- (lab_out[b] == c).sum() of simt_scale_crop at that window (the mirror does not change it).  It leaves as
 *   parts[b][k][0 .. SIMT_RARE_CROP_PARTS-1], whose sum is the count; EVERY word is written by a plain store on every call (no atomics,
 *   nothing to zero).  cls[b] == 255: nothing is counted for b, its words are 0.
 * simt_rare_crop_pick: win[b] = (choice, ox, oy, count) of candidate k*, the smallest k with count[b][k] > min_count, or K - 1 when no
 *   candidate passes (DAFormer keeps the last crop tried); cls[b] == 255: k* = 0.  Reads `parts`, so it runs behind the counts.
 * simt_scale_crop_win: simt_scale_crop whose per-item (choice, ox, oy) are win[b][0..2], read on the device; x, lab_out, mirror, tables
 *   and LDS as there, bit for bit the launch of simt_scale_crop at those windows.  A choice >= n_choices is clamped to n_choices - 1 and
 *   an origin to its choice's range [min(0, ws - w), max(0, ws - w)] (hs, h likewise): whatever `win` holds, no table is read out of range.
 * All three refuse (SIMT_ERR_INVALID, nothing launched or written) what simt_scale_crop refuses and: K outside 1 .. SIMT_RARE_CROP_CANDS,
 * a candidate choice >= n_choices, a candidate origin outside its choice's range, min_count < 0, parts NULL or not 4-byte aligned, win
 * NULL or not 16-byte aligned, a NULL label pointer.  B <= SIMT_RARE_CROP_MAX: with K candidates per item the descriptor of 64 items
 * would not fit the kernel-argument segment.  The descriptor travels as kernel arguments, like simt_scale_crop_desc. */
#define SIMT_RARE_CROP_MAX 16
#define SIMT_RARE_CROP_CANDS 16
#define SIMT_RARE_CROP_PARTS 16
typedef struct {
  const unsigned char* img[SIMT_RARE_CROP_MAX];    /* [Hs][Ws][3] u8 RGB */
  const unsigned char* lab[SIMT_RARE_CROP_MAX];    /* [Hs][Ws] u8 */
  int32_t cand_ox[SIMT_RARE_CROP_MAX][SIMT_RARE_CROP_CANDS], cand_oy[SIMT_RARE_CROP_MAX][SIMT_RARE_CROP_CANDS];
  unsigned char cand_choice[SIMT_RARE_CROP_MAX][SIMT_RARE_CROP_CANDS];
  unsigned char mirror[SIMT_RARE_CROP_MAX];
  unsigned char cls[SIMT_RARE_CROP_MAX];           /* the class counted for item b; 255: none, candidate 0 is taken */
  simt_scale_crop_choice c[SIMT_SCALE_CROP_CHOICES];
  const int32_t* tables;
  float* x;              /* [B][3][h][w] fp32 */
  long long* lab_out;    /* [B][h][w] int64, or NULL */
  int32_t* parts;        /* [B][K][SIMT_RARE_CROP_PARTS] */
  int32_t* win;          /* [B][4]: choice, ox, oy, count */
  int32_t B, Hs, Ws, h, w, n_choices, max_rows, n_tables;
  int32_t K, min_count;
  float mean[3];
} simt_rare_crop_desc;
int simt_rare_crop_counts(const simt_rare_crop_desc* d, simt_stream_t stream);
int simt_rare_crop_pick(const simt_rare_crop_desc* d, simt_stream_t stream);
int simt_scale_crop_win(const simt_rare_crop_desc* d, simt_stream_t stream);

/* ---- ClassMix: class-mask mixing of batch items on the device (simt_amd/data/class_mix.py; csrc/class_mix.hip) ---------------
 * x [B][3][h][w] fp32 and lab [B][h][w] int64 are a finished batch; a label outside [0, n_classes) is "ignore".  Item i's partner is
 * j = partner[i].  P_j = the classes c < n_classes that occur in lab[j], n = |P_j|, k = (n + 1) / 2, S_j = the k classes of P_j with the
 * smallest rank[i][c] (rank[i] is a permutation of 0 .. n_classes-1).  For every pixel p: m = apply[i] && lab[j][p] in S_j;
 *   lab_out[i][p] = m ? lab[j][p] : lab[i][p];   x_out[i][ch][p] = m ? x[j][ch][p] : x[i][ch][p]   (a selection: no bit changes).
 * Output goes to separate buffers (x_out != x, lab_out != lab).  apply[i] == 0: a copy of item i, the partner is not read.
 * simt_label_presence: part[b * SIMT_CLASS_MIX_PARTS + g] = OR of 1u << l over the valid labels l of item b that workgroup g of
 * SIMT_CLASS_MIX_PARTS visits; every word is written with a plain store on every call (no atomics, nothing to zero).
 * simt_class_mix reads the partner's SIMT_CLASS_MIX_PARTS words of `part`, so simt_label_presence(lab, B, h * w, n_classes, part) runs
 * before it on the same stream.  The four batch bases are 16-byte aligned; any h, w with h * w < 2^31; B <= SIMT_CLASS_MIX_MAX (partners
 * cross any chunk's edge: a larger batch is refused, not split).  The descriptor travels as kernel arguments, like simt_gather_desc. */
#define SIMT_CLASS_MIX_MAX 32
#define SIMT_CLASS_MIX_CLASSES 32
#define SIMT_CLASS_MIX_PARTS 64
typedef struct {
  const float* x;            /* [B][3][h][w] fp32 */
  const long long* lab;      /* [B][h][w] int64 */
  float* x_out;              /* [B][3][h][w] fp32 */
  long long* lab_out;        /* [B][h][w] int64 */
  const uint32_t* part;      /* [B][SIMT_CLASS_MIX_PARTS]: simt_label_presence's words for `lab` */
  int32_t B, h, w, n_classes;
  uint8_t partner[SIMT_CLASS_MIX_MAX];
  uint8_t apply[SIMT_CLASS_MIX_MAX];
  uint8_t rank[SIMT_CLASS_MIX_MAX][SIMT_CLASS_MIX_CLASSES];
} simt_class_mix_desc;
int simt_label_presence(const long long* lab, int B, long hw, int n_classes, uint32_t* part, simt_stream_t stream);
int simt_class_mix(const simt_class_mix_desc* d, simt_stream_t stream);
/* simt_class_mix, and the item every pixel came from: item_out[i][p] = m ? partner[i] : i with the m above (apply[i] == 0: i everywhere).
 * item_out: [B][h][w] bytes at a 4-byte aligned base (a quad's four bytes leave as one dword when h * w % 4 == 0); NULL is refused.
 * x_out and lab_out are simt_class_mix's, bit for bit: same grid, same paste mask. */
int simt_class_mix_items(const simt_class_mix_desc* d, uint8_t* item_out, simt_stream_t stream);

/* ---- ClassMix behind a teacher (the warm-up trainers' online_mix; csrc/label_sweep.hip, csrc/class_mix.hip) -----------
 * The mix of a batch whose labels a teacher has just made on the device: two launches on one stream, the label a byte in between.
 *
 * simt_online_label_u8 / simt_online_label_cb_u8 -- simt_online_label / simt_online_label_cb with two differences.  Sources, label rule,
 *   counts (and hist, thr) are the parents', bit for bit.
 *   lab8: the labels leave as uint8 [B][H][W] -- byte for byte those of simt_pseudo_label_u8 / simt_pseudo_label2_u8 (hia = H, wia = W)
 *     mode 1, and the low byte of simt_online_label_cb's int64 word.
 *   part: [B][rows] words, rows = simt_online_label_parts(d) (the launch's workgroups; at most SIMT_ONLINE_LABEL_MAX_PARTS).
 *     part[b][g] = OR of 1u << l over the labels l < C of item b that workgroup g wrote; a 255 sets no bit; 0 where it saw none of the
 *     item.  EVERY word is written by a plain store on every call: no atomics on global memory, nothing to zero, no launch that folds.
 *     The OR of row b is item b's class presence, exactly (simt_label_presence's words for the widened labels).  Item-major, so that
 *     simt_class_mix_u8 reads an item's words as one contiguous run.
 *   Refused (SIMT_ERR_INVALID, nothing launched): what the parents refuse, C > SIMT_CLASS_MIX_CLASSES, B > SIMT_CLASS_MIX_MAX,
 *   H * W >= 2^31, lab8 not 16-byte aligned, counts (hist) not 8-byte aligned, part (thr) NULL or not 4-byte aligned.
 *   simt_online_label_parts reads B, H, W and family only (the cb launch of the same geometry writes the same rows); < 0: invalid.
 *
 * simt_class_mix_u8 -- simt_class_mix's selection over those bytes, into the buffers the next launches read.  With j = partner[i] and
 *   P_j = the classes whose bit is set in the OR of part[j][0 .. rows-1], below n_classes: S_j and m exactly as above (k = (n + 1) / 2
 *   classes of smallest rank[i]; a 255 is never pasted);
 *     lab_out[i][p] = (int64)(m ? lab8[j][p] : lab8[i][p]);   x_out[i][ch][p] = m ? x[j][ch][p] : x[i][ch][p]   (no bit changes).
 *   apply[i] == 0: x_out[i] = x[i], lab_out[i] = lab8[i] widened; the partner is not read.
 *   Refused: a NULL pointer; x, lab8, x_out or lab_out not 16-byte aligned, part not 4-byte aligned; B outside 2 .. SIMT_CLASS_MIX_MAX;
 *   n_classes outside 1 .. SIMT_CLASS_MIX_CLASSES; h, w <= 0 or h * w >= 2^31; rows outside 1 .. SIMT_ONLINE_LABEL_MAX_PARTS; x_out
 *   overlapping x; a partner >= B; a rank >= n_classes.  Any h, w otherwise (h * w % 4 != 0 takes the scalar flavour).
 * All descriptors travel as kernel arguments: no device copy, no synchronisation. */
#define SIMT_ONLINE_LABEL_MAX_PARTS 1024
typedef struct {
  const float* fix;        /* as simt_online_label_desc */
  uint8_t* lab8;           /* out [B][H][W] bytes: class index, 255 = ignore; 16-byte aligned */
  int64_t* counts;         /* [C+1], accumulated, as simt_online_label */
  uint32_t* part;          /* out [B][simt_online_label_parts()] */
  int32_t B, h, w, ld, H, W, C, family;
  float threshold;
} simt_online_label_u8_desc;
typedef struct {
  const float* fix;        /* as simt_online_label_cb_desc */
  uint8_t* lab8;           /* out [B][H][W] bytes; 16-byte aligned */
  int64_t* counts;         /* [C+1], accumulated */
  int64_t* hist;           /* [C][SIMT_CONF_BINS], accumulated */
  const float* thr;        /* [C] fp32 in DEVICE memory */
  uint32_t* part;          /* out [B][rows] */
  int32_t B, h, w, ld, H, W, C, family;
} simt_online_label_cb_u8_desc;
typedef struct {
  const float* x;            /* [B][3][h][w] fp32 */
  const uint8_t* lab8;       /* [B][h][w] bytes */
  float* x_out;              /* [B][3][h][w] fp32 */
  long long* lab_out;        /* [B][h][w] int64 */
  const uint32_t* part;      /* [B][rows]: the label launch's words for `lab8` */
  int32_t B, h, w, n_classes, rows;
  uint8_t partner[SIMT_CLASS_MIX_MAX];
  uint8_t apply[SIMT_CLASS_MIX_MAX];
  uint8_t rank[SIMT_CLASS_MIX_MAX][SIMT_CLASS_MIX_CLASSES];
} simt_class_mix_u8_desc;
int simt_online_label_parts(const simt_online_label_u8_desc* d);
int simt_online_label_u8(const simt_online_label_u8_desc* d, simt_stream_t stream);
int simt_online_label_cb_u8(const simt_online_label_cb_u8_desc* d, simt_stream_t stream);
int simt_class_mix_u8(const simt_class_mix_u8_desc* d, simt_stream_t stream);

/* ---- Quality-weighted online labels (the warm-up trainers' online_labels_weighted; csrc/label_sweep.hip, csrc/head_loss.hip,
 * csrc/class_mix.hip) -----------------------------------------------------------------------------------------------------------------
 * DACS / DAFormer / MIC: the threshold deletes no pixel.  The student trains on the teacher's arg-max everywhere and every pixel's
 * cross-entropy is multiplied by a weight q, the share of pixels whose confidence is above the threshold.
 *
 * simt_online_label_w / simt_online_label_w_u8 -- simt_online_label / simt_online_label_u8 with three differences.  Sources and families
 *   are the parents'.
 *   label / lab8 (and part): those of the parent launch at threshold = -INFINITY, bit for bit: the arg-max wherever the confidence is not
 *     NaN, 255 where it is.
 *   counts[C+1], accumulated: bin arg takes a pixel with conf > threshold, bin C every other pixel -- the counts of the parent launch at
 *     `threshold`, count for count.
 *   conf_part: [B][rows] uint32 words, rows = simt_online_label_parts() of the same B, H, W, family.  conf_part[b][g] = the number of pixels
 *     of item b with conf > threshold that workgroup g swept.  EVERY word is written by a plain store on every call: no global atomics,
 *     nothing to zero.  The sum of row b is the number of non-255 labels the parent launch at `threshold` writes into item b, exactly.
 *   Refused (SIMT_ERR_INVALID, nothing launched): what the parents refuse, B > SIMT_CLASS_MIX_MAX, H * W >= 2^31, conf_part NULL or not
 *   4-byte aligned.
 *
 * simt_label_quality -- conf_part -> q[B] fp32, one small launch of one workgroup behind the label launch on the same stream.  With n_b =
 *   the integer sum of row b and N = H * W:
 *     mode 0 ("item"):  q[b] = (float)((double)n_b / (double)N)
 *     mode 1 ("batch"): every q[b] = (float)((double)(n_0 + ... + n_{B-1}) / (double)(B * N))
 *   Integer sums, one conversion, one division, one rounding: np.float32(np.float64(n) / np.float64(N)).
 *   Refused: a NULL or misaligned pointer, B outside 1 .. SIMT_CLASS_MIX_MAX, rows outside 1 .. SIMT_ONLINE_LABEL_MAX_PARTS, H, W <= 0 or
 *   H * W >= 2^31, another mode.
 *
 * simt_head_loss_weighted / simt_head_grad_weighted -- simt_head_loss / simt_head_grad of a mode-1 descriptor (the warm-up stage's plain
 *   cross-entropy; two heads or single = 1) with a weight per pixel.  w: [B] fp32 in DEVICE memory.  Pixel p of item b has weight w[b]
 *   when w_item is NULL, else w[min(w_item[p], B - 1)] with w_item [B][H][W] bytes (the item map of simt_class_mix_u8_items).
 *     hout[0], hout[1] = sum_p w_p * CE_k(p) / N with N = hout[6] the number of labelled pixels, unchanged; hout[14] formed from them as
 *     before; hout[15], conf_out and label_ws unchanged.  Gradient: gscale * w_p * (softmax - onehot) / N through the same x- and
 *     y-reductions.  With w = 1 everywhere and no map both launches give what the unweighted ones give, bit for bit.
 *   Refused: what simt_head_loss / simt_head_grad refuse, mode 0, a NULL or misaligned w.
 *
 * simt_class_mix_u8_items -- simt_class_mix_u8, and the item every pixel came from: item_out[i][p] = m ? partner[i] : i (apply[i] == 0: i
 *   everywhere), [B][h][w] bytes, 4-byte aligned.  x_out and lab_out are simt_class_mix_u8's, bit for bit.  A NULL map is refused. */
typedef struct {
  const float* fix;        /* as simt_online_label_desc */
  int64_t* label;          /* out [B][H][W]: the arg-max (255: a NaN confidence) */
  int64_t* counts;         /* [C+1], accumulated: what simt_online_label at `threshold` accumulates */
  uint32_t* conf_part;     /* out [B][simt_online_label_parts()] */
  int32_t B, h, w, ld, H, W, C, family;
  float threshold;
} simt_online_label_w_desc;
typedef struct {
  const float* fix;        /* as simt_online_label_desc */
  uint8_t* lab8;           /* out [B][H][W] bytes; 16-byte aligned */
  int64_t* counts;         /* [C+1], accumulated */
  uint32_t* part;          /* out [B][rows]: the presence words of lab8 */
  uint32_t* conf_part;     /* out [B][rows] */
  int32_t B, h, w, ld, H, W, C, family;
  float threshold;
} simt_online_label_w_u8_desc;
typedef struct {
  const uint32_t* conf_part;   /* [B][rows] */
  float* q;                    /* out [B] */
  int32_t B, rows, H, W, mode; /* mode 0: per item; 1: one value for the batch */
} simt_label_quality_desc;
int simt_online_label_w(const simt_online_label_w_desc* d, simt_stream_t stream);
int simt_online_label_w_u8(const simt_online_label_w_u8_desc* d, simt_stream_t stream);
int simt_label_quality(const simt_label_quality_desc* d, simt_stream_t stream);
int simt_head_loss_weighted(const simt_head_desc* d, const float* w, const uint8_t* w_item, simt_stream_t stream);
int simt_head_grad_weighted(const simt_head_desc* d, const float* w, const uint8_t* w_item, simt_stream_t stream);
int simt_class_mix_u8_items(const simt_class_mix_u8_desc* d, uint8_t* item_out, simt_stream_t stream);

/* ---- A labelled source batch in the same step (the warm-up trainers' online_source; csrc/class_mix.hip, csrc/head_loss.hip) --
 * DACS: classes of a labelled SOURCE item pasted onto a TARGET item that a teacher has just labelled.  Target item i is paired with source
 * item i.
 *
 * simt_source_mix -- the cross-domain selection, into the buffers the student's forward and the head launches read.  part_s: the words of
 *   simt_label_presence(labs, B, h * w, n_classes, part_s), run before it on the same stream.  With
 *     P_i = the classes below n_classes whose bit is set in the OR of part_s[i][0 .. SIMT_CLASS_MIX_PARTS-1],
 *     k = (|P_i| + 1) / 2 and S_i = the k classes of P_i with the smallest rank[i] (simt_class_mix's rule),
 *     m(p) = apply[i] and 0 <= labs[i][p] < n_classes and labs[i][p] in S_i   (a 255 or an out-of-range source label is never pasted):
 *     x_out[i][ch][p] = m ? xs[i][ch][p] : xt[i][ch][p]   (no bit changes);   lab_out[i][p] = m ? labs[i][p] : (int64)lab8[i][p].
 *   apply[i] == 0: x_out[i] = xt[i], lab_out[i] = lab8[i] widened; source item i (xs, labs, part_s) is not read.
 * simt_source_mix_items -- the same, and item_out[i][p] = m ? B + i : i, [B][h][w] bytes, 4-byte aligned: the entry of a [2B] weight table
 *   (simt_head_loss_weighted_n) that the pixel carries -- target items first, source items behind them.  x_out and lab_out are
 *   simt_source_mix's, bit for bit.  A NULL map is refused.
 *   Refused (SIMT_ERR_INVALID, nothing launched): a NULL pointer; xs, labs, xt, lab8, x_out or lab_out not 16-byte aligned, part_s not
 *   4-byte aligned; B outside 1 .. SIMT_CLASS_MIX_MAX; n_classes outside 1 .. SIMT_CLASS_MIX_CLASSES; h, w <= 0 or h * w >= 2^31; a rank >=
 *   n_classes; x_out overlapping xs or xt; lab_out overlapping labs.  Any h, w otherwise (h * w % 4 != 0 takes the scalar flavour).
 *   NOT checked, the caller's responsibility (as for simt_class_mix_u8): lab_out must not overlap lab8, and item_out must overlap no input
 *   and no other output.
 *
 * simt_head_loss_weighted_n / simt_head_grad_weighted_n -- simt_head_loss_weighted / simt_head_grad_weighted with a table of nw entries,
 *   B <= nw <= SIMT_HEAD_WEIGHTS_MAX: pixel p of item b has weight w[b] when w_item is NULL, else w[min(w_item[p], nw - 1)].  The two
 *   launches without _n are the nw = B case of the same kernels.  Refused: what those refuse, nw outside B .. SIMT_HEAD_WEIGHTS_MAX. */
#define SIMT_HEAD_WEIGHTS_MAX 64
typedef struct {
  const float* xs;           /* [B][3][h][w] fp32: the source images */
  const long long* labs;     /* [B][h][w] int64: the source ground truth */
  const uint32_t* part_s;    /* [B][SIMT_CLASS_MIX_PARTS]: simt_label_presence's words for `labs` */
  const float* xt;           /* [B][3][h][w] fp32: the target images */
  const uint8_t* lab8;       /* [B][h][w] bytes: the teacher's labels of the target images */
  float* x_out;              /* [B][3][h][w] fp32 */
  long long* lab_out;        /* [B][h][w] int64 */
  int32_t B, h, w, n_classes;
  uint8_t apply[SIMT_CLASS_MIX_MAX];
  uint8_t rank[SIMT_CLASS_MIX_MAX][SIMT_CLASS_MIX_CLASSES];
} simt_source_mix_desc;
int simt_source_mix(const simt_source_mix_desc* d, simt_stream_t stream);
int simt_source_mix_items(const simt_source_mix_desc* d, uint8_t* item_out, simt_stream_t stream);
int simt_head_loss_weighted_n(const simt_head_desc* d, const float* w, int nw, const uint8_t* w_item, simt_stream_t stream);
int simt_head_grad_weighted_n(const simt_head_desc* d, const float* w, int nw, const uint8_t* w_item, simt_stream_t stream);

/* ---- Robust entropy of the target pass (the warm-up trainers' entropy_min; csrc/head_loss.hip) ------------------------------
 * simt_head_loss_entropy / simt_head_grad_entropy -- the mode-1 launches (two heads or single = 1) plus FDA's / ADVENT's label-free term on
 *   EVERY pixel.  For head k and pixel p, with v the Q upsampled logits, lse their log-sum-exp and q = softmax(v) as the passes form them:
 *     u_j  = lse - v_j                 (>= 0)
 *     H    = sum_j q_j * u_j           (a sum of non-negative terms, NOT lse - sum_j q_j v_j)
 *     e    = H / ln(Q)
 *     t    = e * e + eps               eps = 1e-8f, fixed: t > 0 always
 *     rho  = exp(eta * log(t))         any eta > 0; eta = 2 is FDA's Charbonnier penalty, eta = 0.5 MinEnt up to sqrt(eps) = 1e-4
 *     ent_k = sum over ALL B * H * W pixels of rho / (B * H * W)     labelled or not, whatever their weight or item-map byte
 *   hout[2] = ent_1, hout[3] = ent_2 (single: hout[3] only, hout[2] = 0).
 *   hout[14] = hout[1] + lambda_seg * hout[0] + lambda_ent * (hout[3] + lambda_seg * hout[2]);  single: hout[1] + lambda_ent * hout[3].
 *   hout[0], hout[1], hout[6], hout[15], conf_out and label_ws as the weighted / plain mode-1 launches give them: the cross-entropy still
 *   divides by the number of labelled pixels.
 *   Gradient, added to the cross-entropy's per-pixel row before the x-reduction, for every pixel of the image:
 *     d ent / d v_j = ge_k * (2 * eta * e * rho / t) / ln(Q) * (-q_j * (H - u_j)),   ge_2 = gscale * lambda_ent / (B * H * W),
 *     ge_1 = ge_2 * lambda_seg.
 *   w == NULL: every weight is 1 (nw must be 0 and w_item NULL); else w, nw and w_item as in simt_head_*_weighted_n.
 *   Every descriptor runs the run-time-count kernels, one image row per pass-2 block (g1 is [2][B][H][w][QP]).
 *   Refused (SIMT_ERR_INVALID, nothing launched, nothing written): what simt_head_loss / simt_head_grad refuse; mode 0; Q < 2; e NULL;
 *   lambda_ent or eta non-finite or <= 0; w NULL with a map or nw != 0; w misaligned; nw outside B .. SIMT_HEAD_WEIGHTS_MAX.  A zero lambda
 *   is the caller's business: it issues the launches above. */
typedef struct { float lambda_ent, eta; } simt_head_entropy;
int simt_head_loss_entropy(const simt_head_desc* d, const float* w, int nw, const uint8_t* w_item, const simt_head_entropy* e,
                           simt_stream_t stream);
int simt_head_grad_entropy(const simt_head_desc* d, const float* w, int nw, const uint8_t* w_item, const simt_head_entropy* e,
                           simt_stream_t stream);

/* ---- Uncertainty-rectified pseudo-label loss (WarmupTrainer's uncertainty_rectify; csrc/head_loss.hip) ---------------------
 * simt_head_loss_uncertain / simt_head_grad_uncertain -- the two-head mode-1 launches with Zheng & Yang's rectification (IJCV 2021): the KL
 *   divergence between the two heads' predictions is a pixel's label uncertainty; its cross-entropy is multiplied by exp(-KL) and the KL is
 *   added as a regulariser.  Per pixel p of the B * H * W upsampled pixels, head k in {1 (aux, pred1), 2 (main, pred2)}, o the other head,
 *   v the Q upsampled logits, lse their log-sum-exp and q = softmax(v) as the passes form them, u_j = lse - v_j >= 0:
 *     D_k   = KL(q_o || q_k) = sum_j q_o,j * (u_k,j - u_o,j)            (summed in that form; not clamped)
 *     R_k   = [ sum over labelled p of w_p * exp(-D_k) * u_k,label ] / N   N = labelled pixels (hout[6]); w_p as simt_head_*_weighted_n
 *                                                                          (w == NULL: 1)
 *     K_k   = sum over ALL p of D_k / (B * H * W)
 *     total = R_2 + lambda_kl * K_2 + lambda_seg * (R_1 + lambda_kl * K_1)
 *   The gradient flows through BOTH arguments of the KL; nothing is detached.  With a_k = w_p * exp(-D_k) / N (0 where unlabelled),
 *   c_k = lambda_kl / (B * H * W) - a_k * u_k,label, L_2 = 1 and L_1 = lambda_seg, the gradient row of head k, added per pixel before the
 *   x-reduction, is
 *     G_k,j = gscale * { L_k * [ a_k * (q_k,j - onehot_j) + c_k * (q_k,j - q_o,j) ] + L_o * c_o * q_k,j * ((u_o,j - u_k,j) - D_o) }
 *   lambda_kl enters every word through one product (gscale * lambda_kl / (B * H * W)): at w = 0 doubling it doubles every word exactly.
 *   hout[0], hout[1] = R_1, R_2;  hout[2], hout[3] = K_1, K_2;  hout[4], hout[5] = the mean over labelled pixels of exp(-D_k), the average
 *   rectification weight;  hout[14] = total;  hout[6], hout[15], conf_out, label_ws and every other scalar as the weighted / plain mode-1
 *   launches give them.
 *   w == NULL: every weight is 1 (nw must be 0 and w_item NULL); else w, nw and w_item as in simt_head_*_weighted_n.
 *   Every descriptor runs the run-time-count kernels, one image row per pass-2 block (g1 is [2][B][H][w][QP]).
 *   Departures from the published method: the cross-entropy keeps this project's division by N (the paper takes both means over all pixels);
 *   one lambda_seg serves both of a head's terms; there are no class weights.
 *   Refused (SIMT_ERR_INVALID, nothing launched, nothing written): what simt_head_loss / simt_head_grad refuse; mode 0; single = 1; pred1
 *   NULL; u NULL; lambda_kl non-finite or < 0 (0 is allowed: the rectified cross-entropy alone); w NULL with a map or nw != 0; w misaligned;
 *   nw outside B .. SIMT_HEAD_WEIGHTS_MAX. */
typedef struct { float lambda_kl; } simt_head_uncertainty;
int simt_head_loss_uncertain(const simt_head_desc* d, const float* w, int nw, const uint8_t* w_item, const simt_head_uncertainty* u,
                             simt_stream_t stream);
int simt_head_grad_uncertain(const simt_head_desc* d, const float* w, int nw, const uint8_t* w_item, const simt_head_uncertainty* u,
                             simt_stream_t stream);

/* ---- Photometric augmentation: colour jitter, then Gaussian blur, on a finished batch (simt_amd/data/photometric.py;
 * csrc/photometric.hip) -----------------------------------------------------------------------------------------------------------
 * Input is a finished batch x [B][3][h][w] fp32 as every loader path produces it: plane p holds colour - mean[p].  Output goes to another
 * buffer x_out.  Labels are not touched.
 * All arithmetic below is IEEE float32.  Every multiply and every add is rounded on its own (no contraction into FMA), in the order
 * written.  clamp(v) = min(max(v, 0), 1).
 * Per item i the descriptor carries jit[i], blur[i] (bytes), fb, fc, omfc, a 3x3 matrix A (row-major: A[3 * p + c]) and six blur weights
 * wk[0..5].  The three planes are treated as B, G, R by position, with grey weights wg = (0.114, 0.587, 0.299) as float32.  A mirrored
 * item, whose planes the reference's loader leaves in RGB order, and pixels pasted from such an item, get the weights of their plane
 * position.  This is documented, not corrected.
 *   Normalise.  v_p = clamp((x_p + mean[p]) * c255), with c255 = float32(1/255).
 *   Jitter (only if jit[i]), in fixed order:
 *     Brightness: v_p = clamp(fb * v_p).
 *     Contrast:   v_p = clamp(fc * v_p + omfc * m), with omfc = float32(1 - fc) from the host.  m is the item's grey mean after
 *                 brightness, defined exactly: g = (wg0*v0 + wg1*v1) + wg2*v2;  q = rint(g * 65536), ties to even, as an unsigned integer;
 *                 S = sum of q over the item, as a 64-bit integer (exact and order-free);  m = float32(float64(S) * inv), with
 *                 inv = float64(1 / (65536*h*w)) from the host.
 *     Saturation and hue, as one matrix: v'_p = clamp((A[p][0]*v0 + A[p][1]*v1) + A[p][2]*v2).  The host computes
 *                 A = H(theta) . (fs.I + (1-fs).1.wg^T) in float64, H(theta) the rotation by theta turns about the grey axis in YIQ space,
 *                 expressed in the plane order above; A is rounded once to float32.
 *   Blur (only if blur[i]): separable, radius 5, horizontal pass then vertical pass.  Indices outside the frame are reflected without
 *     repeating the edge: -k -> k, n-1+k -> n-1-k.  Per pass and plane: acc = wk0*c, then for k = 1..5 acc = acc + wk[k] * (l_k + r_k)
 *     (the neighbour sum is rounded first, then the product, then the add).  After the vertical pass, one clamp.  The host computes
 *     exp(-k^2 / 2 sigma^2) in float64 and sets any weight below 2^-24 to exactly 0, so no denormal ever arises; it then normalises so that
 *     wk0 + 2 sum wk[k] = 1, and rounds to float32.
 *   Back.  x_out_p = v_p * 255 - mean[p].
 *   Neither flag set: item i is copied bit for bit (NaN payloads and -0.0 survive, as in ClassMix).  With a flag set, inputs must be
 *     finite.
 * simt_grey_mean_parts (grid SIMT_PHOTOMETRIC_PARTS x B): part[b * SIMT_PHOTOMETRIC_PARTS + g] = the sum of q over the pixels of item b
 * that workgroup g visits; every word is written with a plain store on every call (no atomics, nothing to zero); 0, without reading x,
 * for an item with jit[b] == 0.  It reads x, part, B, h, w, mean, jit and fb of the descriptor.  simt_photometric reads the item's
 * SIMT_PHOTOMETRIC_PARTS words, so simt_grey_mean_parts runs before it on the same stream with the same descriptor.
 * Any h, w >= 6 (the reflection is defined) with h * w < 2^31; x_out != x; x and x_out 16-byte, part 8-byte aligned;
 * 1 <= B <= SIMT_PHOTOMETRIC_MAX (items are independent: a larger batch is split by the caller).  Anything else is refused with an error
 * code and no launch.  The descriptor travels as kernel arguments, like simt_class_mix_desc. */
#define SIMT_PHOTOMETRIC_MAX 32
#define SIMT_PHOTOMETRIC_PARTS 64
typedef struct {
  const float* x;                          /* [B][3][h][w] fp32 */
  float* x_out;                            /* [B][3][h][w] fp32 */
  unsigned long long* part;                /* [B][SIMT_PHOTOMETRIC_PARTS]: simt_grey_mean_parts writes, simt_photometric reads */
  double inv;                              /* 1 / (65536 * h * w) */
  int32_t B, h, w;
  float mean[3];
  float fb[SIMT_PHOTOMETRIC_MAX];
  float fc[SIMT_PHOTOMETRIC_MAX];
  float omfc[SIMT_PHOTOMETRIC_MAX];
  float A[SIMT_PHOTOMETRIC_MAX][9];
  float wk[SIMT_PHOTOMETRIC_MAX][6];
  uint8_t jit[SIMT_PHOTOMETRIC_MAX];
  uint8_t blur[SIMT_PHOTOMETRIC_MAX];
} simt_photometric_desc;
int simt_grey_mean_parts(const simt_photometric_desc* d, simt_stream_t stream);
int simt_photometric(const simt_photometric_desc* d, simt_stream_t stream);

/* ---- exponential moving average of the weights (simt_amd/ema.py): e <- e + omd * (w - e) over a segment table, ONE launch ------
 * The shadow model of a trainer: every floating tensor of `params` (weights, biases, BatchNorm affine and running statistics) has an fp32
 * twin `e`; one launch per optimiser step moves all of them towards the live tensors.  One workgroup of 256 lanes per chunk, like
 * simt_sgd_multi; 16-byte loads and stores where w and e are both 16-byte aligned at the chunk's start, dwords otherwise and for the tail.
 * ARITHMETIC CONTRACT (the kernel is held to it bit for bit; tests/_ema_ref.py is its numpy restatement):
 *   - every operation is IEEE binary32, rounded to nearest even on its own, gradual underflow honoured; nothing is contracted into an FMA;
 *   - omd == 1.0f:  e[i] = w[i] as a 32-bit word copy (NaN payloads and -0.0 survive);
 *   - otherwise:    t = w[i] - e[i];  u = omd * t;  e[i] = e[i] + u.
 *     Where w[i] == e[i] the VALUE of e[i] does not move (t = +0, u = +0, e + 0 = e) -- tensors no optimiser touches stay equal to the live
 *     ones as numbers, no tensor needs a mode of its own.  One bit pattern does change there: e = -0.0 with w = +-0.0 becomes +0.0
 *     (-0 + +0 = +0 under round to nearest); the restatement does the same;
 *   - w is never written.
 * Refused with SIMT_ERR_INVALID and no launch: omd outside (0, 1] or NaN, NULL segs or chunks, nchunks <= 0, chunk <= 0. */
typedef struct {
  const void* segs;        /* device array of {const float* w; float* e; int64_t n}  (24 bytes each) */
  const int32_t* chunks;   /* device [nchunks][2] = (segment, chunk index), as simt_sgd_desc */
  int32_t nchunks, chunk;  /* elements per chunk */
  float omd;               /* 1 - decay of THIS update, rounded once from float64 by the host; in (0, 1] */
  const uint64_t* skip_if; /* optional: the launch changes nothing while *skip_if != 0 (the fused-BatchNorm error word) */
} simt_ema_desc;
int simt_ema_multi(const simt_ema_desc* d, simt_stream_t stream);

/* ---- every eval-mode BatchNorm fold of a plan in ONE launch (simt_amd/ema_teacher.py) --------------------------------------------
 * The table-driven form of simt_bn_fold: a frozen plan whose weights move (the EMA teacher) re-derives the (scale, shift) pair of every
 * BatchNorm at each refresh -- 104 launches of at most 2 048 lanes for a ResNet-101, one launch here.  One workgroup of 256 lanes per chunk of
 * `chunk` channels of one segment; plain loads, plain stores, no LDS, no atomics, no scratch.
 * CONTRACT: for every segment and every c < C, scale[c] and shift[c] are, bit for bit, what simt_bn_fold writes for the same six pointers,
 * eps and C:   sc = gamma[c] / sqrtf(rv[c] + eps);  scale[c] = sc;  shift[c] = beta[c] - rm[c] * sc
 * -- the same source expression compiled under the same floating-point contraction setting as bn_fold_kernel (csrc/build.sh: one set of flags,
 * no pragma in either file), so the multiply-subtract of `shift` is fused, or not, exactly as it is there.  The yardstick is that kernel on
 * the GPU (tests/test_gpu_ema_teacher.py), not a host restatement.  Nothing but scale[0, C) and shift[0, C) of each segment is written.
 * The segment table exists twice: `segs` on the device for the kernel, `segs_host` in host memory for the checks below (the same `nsegs`
 * records; the caller keeps both alive and identical).
 * Refused with SIMT_ERR_INVALID and no launch: NULL d, segs, segs_host or chunks; nsegs <= 0, nchunks <= 0, chunk <= 0; a segment with
 * C <= 0 or a NULL pointer among its six. */
typedef struct {
  const float* gamma;        /* BatchNorm weight        [C] */
  const float* beta;         /* BatchNorm bias          [C] */
  const float* running_mean; /*                         [C] */
  const float* running_var;  /*                         [C] */
  float* scale;              /* out                     [C] */
  float* shift;              /* out                     [C] */
  int32_t C, reserved_;
} simt_bn_fold_seg;          /* 56 bytes */
typedef struct {
  const simt_bn_fold_seg* segs;      /* device array [nsegs] */
  const simt_bn_fold_seg* segs_host; /* host copy of the same records: what the refusals are decided on */
  const int32_t* chunks;             /* device [nchunks][2] = (segment, chunk index): channels [index * chunk, (index + 1) * chunk) of it */
  int32_t nsegs, nchunks, chunk;
  float eps;
} simt_bn_fold_desc;
int simt_bn_fold_multi(const simt_bn_fold_desc* d, simt_stream_t stream);

/* ---- MIC patch masking of a finished batch (simt_amd/data/patch_mask.py; csrc/patch_mask.hip) ------------------------------------
 * Masked Image Consistency (Hoyer et al., CVPR'23): square patches of the student's view are blanked.  x [B][3][h][w] fp32 is a finished
 * batch, every plane colour - mean, so a blanked pixel is +0.0f: the mean colour.  One launch.
 * CONTRACT (the kernel is held to it bit for bit; tests/_patch_mask_ref.py is its numpy restatement).  gh = ceil(h / patch),
 * gw = ceil(w / patch).  For every item i < B, plane p < 3 and pixel (y, x):
 *     m = (rows[i][y / patch] >> (x / patch)) & 1;     x_out[i][p][y][x] = m ? +0.0f : x[i][p][y][x]
 *   - a blanked word is the bit pattern 0x00000000; a kept word is a 32-bit word copy: NaN payloads, -0.0, infinities and denormals survive;
 *   - the three planes of an item share its mask; edge patches are partial when patch does not divide h or w;
 *   - bits at column >= gw of a row word and the words of rows >= gh are ignored;
 *   - out of place (x_out != x): x is never written, every word of x_out[0, B) is written, the blanked patches of x are not read;
 *   - in place (x_out == x): only the blanked words are stored, kept words are neither read nor written -- a sparse zero fill that moves the
 *     blanked share R of the batch's bytes (out of place: 2 - R of them).
 * Refused with SIMT_ERR_INVALID and no launch: a NULL d, x or x_out; B outside [1, SIMT_PATCH_MASK_MAX]; h < 1, w < 1 or patch < 1; gh or gw
 * above SIMT_PATCH_MASK_GRID; h * w >= 2^31; a base that is not 16-byte aligned; x_out overlapping x without being equal to it.
 * Items are independent: the caller splits a larger batch.  The descriptor is read on the host during the call and travels as kernel
 * arguments, like simt_class_mix_desc: no table is uploaded and nothing synchronises.  A wave owns one pixel row of an item (all three
 * planes) and takes the row's mask word from the kernel arguments as a wave-uniform value.  16-byte loads and stores when w % 4 == 0 and
 * patch % 4 == 0 (every row then starts on a 16-byte boundary and no quad straddles a patch), dwords otherwise.  No LDS, no atomics. */
#define SIMT_PATCH_MASK_MAX  16     /* items per launch */
#define SIMT_PATCH_MASK_GRID 32     /* patch rows and patch columns per item, at most */
typedef struct {
  const float* x;       /* [B][3][h][w] fp32 */
  float* x_out;         /* [B][3][h][w] fp32; x_out == x is allowed (in place) */
  int32_t B, h, w, patch;
  uint32_t rows[SIMT_PATCH_MASK_MAX][SIMT_PATCH_MASK_GRID];   /* bit c of rows[i][r]: patch (r, c) of item i is blanked */
} simt_patch_mask_desc;
int simt_patch_mask(const simt_patch_mask_desc* d, simt_stream_t stream);

/* ---- DAFormer's thing-class ImageNet feature distance (simt_amd/feat_dist.py; csrc/feat_dist.hip) ---------------------------------
 * The pass that trains on ground-truth labels adds  lambda * mean over kept cells m of || fs[m, :] - fi[m, :] ||_2 : fs [M][C] is the student's
 * layer-4 output (train-mode forward), fi [M][C] that of a frozen eval-mode trunk with ImageNet weights, M = B * h * w.  Three launches; the
 * gradient with respect to fs (`seed`) enters the backward as the `res` of the layer-4 head's input-gradient launch.
 * CONTRACT (tests/_feat_dist_ref.py is its numpy / float64 restatement).
 *   CELLS.  Cell (i, j) of item b, 0 <= i < h, 0 <= j < w, owns the label pixels of rows [(i*H)/h, ((i+1)*H)/h) and columns
 *     [(j*W)/w, ((j+1)*W)/w) (integer division); h <= H and w <= W, so no window is empty and the windows partition the label.  n = the pixels
 *     of the window.  Where H = s*h and W = s*w these are the s x s blocks of DAFormer's downscale_label_ratio.
 *   KEPT.  mask[cell] = 1 iff some class c with bit c of `classes` set has  (float)count_c >= min_ratio * (float)n  in binary32 with ONE
 *     multiply, count_c = the window pixels whose int64 label == c; else 0.  A label that is 255, negative or >= 64 matches no class and counts
 *     against the ratio.  0.5 < min_ratio <= 1: at most one class qualifies.  part[g] = the kept cells of workgroup g (plain store; the buffer
 *     holds simt_feat_dist_mask_parts(B, h, w) words); N = their sum.
 *   DISTANCE of a kept row:  diff_c = (float)fs[c] - (float)fi[c];  s = sum_c diff_c * diff_c in binary32 in a FIXED order (lane-local in
 *     element order, then the wave's xor butterfly);  d = sqrtf(s).  No atomics: a launch repeats bit for bit.
 *   SEED, in the features' dtype:  a kept row with d > 0:  seed[m][c] = round(((lam_g / (float)N) / d) * diff_c);  any other row (not kept, or
 *     d == 0, or d NaN): +0 in every column.  Rows that are not kept are never read from fs or fi.  EVERY row of seed is written by every
 *     launch: no memset is ever needed.  d[m] = the distance of a kept row, 0 elsewhere.  lam_g = (float)(lambda * gscale), gscale as in
 *     simt_head_desc.
 *   SCALARS (simt_feat_dist_finalize):  S = the sum over workgroups, in double and in index order, of the launch's per-workgroup binary32
 *     sums of d (simt_feat_dist_parts(M) of them);  out[0] = lambda * S / N, out[1] = S / N, out[2] = (float)N.  N == 0: all three are 0 and
 *     the seed is all +0 (torch's mean over an empty selection is NaN: a departure).
 * Refused with SIMT_ERR_INVALID, no launch and nothing written: a NULL descriptor or pointer; B, H, W, h or w < 1; h > H or w > W;
 * min_ratio outside (0.5, 1] or NaN; H * W or B * h * w >= 2^31; a label base that is not 8-byte aligned; (main pass, finalize) M < 1,
 * C < 8 or C % 8 != 0, ld != C, a dtype code other than SIMT_F32 / SIMT_BF16, n_kept_part < 1, fs / fi / seed not 16-byte aligned, a NaN
 * lam_g or lambda.  No LDS beyond 4 words per workgroup, no scratch, no atomics. */
typedef struct {
  const int64_t* label;    /* [B][H][W] */
  uint8_t* mask;           /* out [B*h*w] */
  int32_t* part;           /* out [simt_feat_dist_mask_parts(B, h, w)]: kept cells per workgroup */
  uint64_t classes;        /* bit c: class c is a thing class */
  int32_t B, H, W, h, w;
  float min_ratio;
} simt_feat_dist_mask_desc;
typedef struct {
  const void* fs;          /* [M][C] student features, dtype */
  const void* fi;          /* [M][C] ImageNet features, dtype */
  const uint8_t* mask;     /* [M] of simt_feat_dist_mask */
  const int32_t* kept_part;/* [n_kept_part] of simt_feat_dist_mask */
  void* seed;              /* out [M][C], dtype */
  float* d;                /* out [M] */
  float* part;             /* out [simt_feat_dist_parts(M)]: sum of d per workgroup */
  float* out;              /* out [3], written by simt_feat_dist_finalize */
  double lambda;
  int64_t M;
  int32_t C, ld, dtype, n_kept_part;
  float lam_g;             /* (float)(lambda * gscale) */
  int32_t reserved_;
} simt_feat_dist_desc;
int simt_feat_dist_mask_parts(int B, int h, int w);       /* 0: a geometry the launch refuses */
int simt_feat_dist_parts(long M);
int simt_feat_dist_mask(const simt_feat_dist_mask_desc* d, simt_stream_t stream);
int simt_feat_dist(const simt_feat_dist_desc* d, simt_stream_t stream);
int simt_feat_dist_finalize(const simt_feat_dist_desc* d, simt_stream_t stream);

/* ---- FDA: Fourier low-band style transfer of the source batch (simt_amd/data/fda.py; csrc/fda.hip) --------------------------------
 * Fourier Domain Adaptation (Yang & Soatto, CVPR'20): the low-frequency AMPLITUDE of every source image's spectrum is replaced by that of a
 * target image, the source PHASE is kept (so the source labels stay valid).  xs, xt [B][3][h][w] fp32 as the loaders hand them out (plane c holds
 * colour - mean[c]); source item i is paired with target item i (simt_source_mix's pairing); x_out has the same shape.
 * CONTRACT (tests/_fda_ref.py is its numpy restatement; the result is held to a tolerance, not bit for bit).  Per item and plane c:
 *   S = xs + mean[c], T = xt + mean[c]: FDA is defined on the raw 0..255 image -- the mean only moves the DC coefficient, but DC's amplitude is
 *     swapped, so it is added back first.
 *   Omega = {(u, v): -b <= u, v <= b}, frequencies taken mod h and mod w.  For (u, v) in Omega, with F_S and F_T the DFT coefficients
 *     F(u, v) = sum_x sum_y V[x][y] * e^{-2 pi i (u x / h + v y / w)}:
 *     D(u, v) = |F_T(u, v)| * p(u, v) - F_S(u, v),   p = F_S / |F_S|, or 1 where |F_S| == 0 (numpy's angle(0) = 0).
 *   x_out[x][y] = xs[x][y] + (1 / (h w)) * sum over Omega of Re(D(u, v) * e^{+2 pi i (u x / h + v y / w)}).
 *     D is Hermitian, so only v = 0 .. b are held: v = 0 has weight 1, v > 0 weight 2.  The output is NOT clipped (the published code does not
 *     clip either).  Only the (2b+1)^2 lowest frequencies change, so this IS the published fft2 / swap / ifft2 without either transform.
 *   TWIDDLES come from two tables the host builds in float64 and rounds to fp32: tw_w[k] = (cos, sin)(2 pi k / w) for k < w, tw_h likewise for
 *     h.  They are indexed by the INTEGER (v * y) mod w and (u * x) mod h: no device sinf / cosf ever sees an unreduced angle.
 *   All arithmetic is fp32; the order of the sums is the implementation's.  b = floor(min(h, w) * beta) is the caller's.
 * ONE call, four launches on `stream` (csrc/fda.hip): row pass over xs and xt, column pass + swap, column synthesis, apply.  Partial results
 * are plain stores into `work` (simt_fda_workspace_bytes(B, h, w, b) bytes, 0 for a geometry the call refuses); every word that is read is
 * written by the same call: no atomics, nothing to zero, no scratch.  xs and xt are never written.
 * Refused with SIMT_ERR_INVALID, nothing launched and nothing written: a NULL descriptor or pointer; xs, xt, x_out or work not 16-byte, tw_h or
 * tw_w not 8-byte aligned; x_out overlapping xs or xt; B outside 1 .. SIMT_FDA_MAX_ITEMS; h or w < 1; b < 0; 2b + 1 > min(h, w);
 * b > SIMT_FDA_MAX_BAND; h * w >= 2^31; 3 * B * h >= 2^31 (the flat pixel rows index the grids).  Any other h, w (w % 4 != 0 takes the scalar
 * flavour). */
#define SIMT_FDA_MAX_ITEMS 32
#define SIMT_FDA_MAX_BAND  64
typedef struct {
  const float* xs;     /* [B][3][h][w] fp32: the source images */
  const float* xt;     /* [B][3][h][w] fp32: the target images */
  float* x_out;        /* [B][3][h][w] fp32 */
  const float* tw_h;   /* [h][2] fp32: (cos, sin)(2 pi k / h) */
  const float* tw_w;   /* [w][2] fp32: (cos, sin)(2 pi k / w) */
  void* work;          /* simt_fda_workspace_bytes(B, h, w, b) bytes */
  int32_t B, h, w, b;
  float mean[3];
  int32_t reserved_;
} simt_fda_desc;
long simt_fda_workspace_bytes(int B, int h, int w, int b);
int simt_fda_transfer(const simt_fda_desc* d, simt_stream_t stream);

/* ---- ProDA's prototype weights on the teacher's output (simt_amd/proto.py; csrc/proto.hip) -----------------------------------------
 * Zhang et al., CVPR'21: the teacher's posterior of a feature cell is weighed by how close the cell's feature lies to running class
 * prototypes, before the label launch reads it.  F [M][ldF] (SIMT_F32 / SIMT_BF16, D columns used) is the input of the teacher's main
 * classifier, M = B * h * w; P [M][ldp] fp32 its low-res output -- probabilities (family 0) or logits (family 1), the `fix` of the label
 * launches; eta [C][D] fp32 the prototypes; n [C] int32 the updates every class has received (0: unseen).  Three launches.
 * CONTRACT (tests/_proto_ref.py is its numpy restatement, float32 sequential and float64).
 *   RECTIFY (simt_proto_rectify), per cell m.  For every class c with n[c] > 0:  s_c = sum_k ((float)F[m][k] - eta[c][k])^2 in binary32 in a
 *     FIXED order (lane-local in element order, then the wave's xor butterfly);  d_c = sqrtf(s_c).  d_min = the minimum over the seen classes
 *     (fminf: a NaN loses to a number).  A class with n[c] == 0 takes d_c = d_min: an unseen class is not penalised, and its row of eta is
 *     never read.  z_c = -(d_c - d_min) / temp.  Family 0:  r_c = expf(z_c) * P[m][c],  out[m][c] = r_c / sum_c r_c  (the sum by the
 *     butterfly over the lanes c < C).  Family 1:  out[m][c] = P[m][c] + z_c  -- the same weights in the logit domain: softmax(v + log w) =
 *     w * softmax(v) / sum.  Columns C .. ldp-1 of out are copies of P's.  If NO class is seen, out[m][:] is P[m][:] word for word.
 *     arg(v) = the first index of the maximum of v[0 .. C-1], a NaN counting as -inf.  conf = the maximum of out (family 0), or
 *     1 / sum_c expf(out_c - max) (family 1).  lab[m] (one byte) = arg(out) if conf > thr and no out_c is a NaN, else 255; thr = -inf keeps
 *     every such cell.  changed_part[g] = the number of workgroup g's cells with arg(out) != arg(P[m]) (plain store; the buffer holds
 *     simt_proto_parts(M) words, every one written by every launch).  out and P are distinct buffers.
 *   ACCUMULATE (simt_proto_accumulate).  Part p owns the cells 256 p .. min(256 p + 255, M - 1).  ws[(p * C + c) * D + k] = the sum, in cell
 *     order and binary32, from +0, of (float)F[m][k] over the part's cells with lab[m] == c; behind the parts * C * D sums, as int32 words,
 *     cnt[p * C + c] = the number of those cells.  parts = ceil(M / 256); the workspace holds simt_proto_ws_floats(M, C, D) =
 *     parts * C * (D + 1) words, every one written by every launch.  A byte >= C (255 among them) belongs to no class.
 *   UPDATE (simt_proto_update).  S_c[k] = the parts' sums added in part order from +0, cnt_c = the parts' counts.  For every class with
 *     cnt_c > 0:  mean = S_c / (float)cnt_c;  n[c] == 0: eta[c] = mean, a word copy;  else a = fmaxf((float)(1.0 - momentum), 1.f / (float)(n[c] + 1))
 *     and eta[c][k] = fmaf(a, mean[k] - eta[c][k], eta[c][k]);  then n[c] += 1.  A class with cnt_c == 0 keeps every word of eta[c] and n[c].
 *   No atomics: every launch repeats bit for bit.
 * Refused with SIMT_ERR_INVALID, nothing launched and nothing written: a NULL descriptor or pointer; M < 1 or M >= 2^31; C outside
 * 2 .. SIMT_PROTO_MAX_CLASSES; D outside 8 .. SIMT_PROTO_MAX_DIM or D % 8 != 0; ldF < D or ldF % 8 != 0 (rows start on 16-byte boundaries); ldp < C; a
 * dtype code other than SIMT_F32 / SIMT_BF16; a family other than 0 / 1; temp not a finite float > 0; a NaN thr; momentum outside [0, 1);
 * F, eta or ws not 16-byte aligned; P, out, n or changed_part not 4-byte aligned.
 * LDS: rectify 4 words; accumulate C * 256 * V floats (V = 4 / 2 / 1 for C <= 16 / 32 / 64: at most 64 KB); no scratch. */
#define SIMT_PROTO_MAX_CLASSES 64
#define SIMT_PROTO_MAX_DIM     4096
typedef struct {
  const void* F;           /* [M][ldF] teacher features, dtype */
  const float* P;          /* [M][ldp] the teacher's output */
  float* out;              /* out [M][ldp] the rectified map */
  const float* eta;        /* [C][D] */
  const int32_t* n;        /* [C] */
  uint8_t* lab;            /* out [M] */
  int32_t* changed_part;   /* out [simt_proto_parts(M)] */
  int64_t M;
  int32_t D, ldF, C, ldp, dtype, family;
  float temp, thr;
} simt_proto_rectify_desc;
typedef struct {
  const void* F;           /* [M][ldF] teacher features, dtype */
  const uint8_t* lab;      /* [M] of simt_proto_rectify */
  float* ws;               /* out [simt_proto_ws_floats(M, C, D)] */
  int64_t M;
  int32_t D, ldF, C, dtype;
} simt_proto_acc_desc;
typedef struct {
  const float* ws;         /* [simt_proto_ws_floats(M, C, D)] of simt_proto_accumulate */
  float* eta;              /* in/out [C][D] */
  int32_t* n;              /* in/out [C] */
  int64_t M;
  int32_t D, C;
  double momentum;
} simt_proto_update_desc;
int simt_proto_parts(long M);                             /* 0: an M the launch refuses */
long simt_proto_ws_floats(long M, int C, int D);          /* 0: a geometry the launches refuse */
int simt_proto_rectify(const simt_proto_rectify_desc* d, simt_stream_t stream);
int simt_proto_accumulate(const simt_proto_acc_desc* d, simt_stream_t stream);
int simt_proto_update(const simt_proto_update_desc* d, simt_stream_t stream);

/* ---- Prototype contrastive loss on the student's layer-4 features (simt_amd/proto_contrast.py; csrc/proto_contrast.hip) -------------
 * SePiCo (Xie et al., TPAMI'23) / the second half of ProDA: every pass of a micro-batch adds
 *     lambda * (1 / N) * sum over valid cells m of  -log softmax_seen( cos(f_m, eta_c) / T )[y_m]
 * fs [M][D] (SIMT_F32 / SIMT_BF16) is the student's layer-4 output, M = B * h * w; eta [C][D] fp32 and n [C] int32 are the prototypes of 7.26 as
 * they stand when the launch runs; y_m the cell's label.  Four launches; the gradient with respect to fs (`seed`) enters the backward as the `res`
 * of the layer-4 head's input-gradient launch, as in 7.22.
 * CONTRACT (tests/_proto_contrast_ref.py is its numpy restatement, float32 sequential and float64).
 *   CELL LABELS (simt_cell_labels).  The windows are exactly the CELLS rule of 7.22.  lab[cell] = c if class c < C has
 *     (float)count_c >= min_ratio * (float)n  in binary32 with ONE multiply, count_c = the window pixels whose int64 label == c; else 255.
 *     0.5 < min_ratio <= 1: at most one class qualifies (were two to pass in binary32, the lower id wins).  A label that is 255, negative or >= C
 *     matches no class and counts against the ratio.  C <= 64.  part[g] = the number of workgroup g's cells whose class has n[c] > 0 (plain
 *     store; the buffer holds simt_cell_labels_parts(B, h, w) words, every one written by every launch); a NULL n counts every labelled cell.
 *     With `classes` a set of class ids, (lab[cell] < C and lab[cell] in classes) == simt_feat_dist_mask's mask[cell].
 *   PREP (simt_proto_contrast_prep).  ne_c = sqrtf(sum_k eta[c][k]^2) in binary32 in a FIXED order (lane-local in element order, then the wave's
 *     xor butterfly).  Class c is SEEN iff n[c] > 0 and ne_c is a finite float > 0 (a seen prototype with ne_c == 0 is treated as unseen).
 *     phat[c][k] = eta[c][k] / ne_c for a seen class, +0 for every other row up to Cpad = 32 (C <= 32) or 64; phat holds
 *     simt_proto_contrast_phat_floats(C, D) = Cpad * D words, every one written by every launch.  hdr[0], hdr[1] = the low and high words of the
 *     seen set, hdr[3] = the number of seen classes; FEWER THAN TWO seen classes: the set is stored as 0.  A cell is VALID iff lab[m] < C and
 *     its class is in the stored set; hdr[2] = N = the number of valid cells.  Rows of eta of classes with n[c] <= 0 are never read.
 *   CONTRAST (simt_proto_contrast), per valid cell m.  nf = sqrtf(sum_k f[k]^2), f = (float)fs[m][:], in binary32 in a FIXED order.
 *     cos_c = (f . phat_c) / nf  (a k-ordered binary32 fmaf chain: mfma_f32_32x32x2f32);  s_c = cos_c / T  for seen c -- the restatement's
 *     (f . eta_c) / (nf * ne_c) / T up to two roundings.  lse = max + logf(sum expf(s_c - max)) over the seen classes, q_c = expf(s_c - lse),
 *     loss_m = lse - s_y.  With a_c = q_c - [c == y], k = lam_g / (float)N:
 *         seed[m][:] = round_dtype( (k / (T * nf)) * ( sum_c a_c * phat_c  -  ((sum_c a_c * cos_c) / nf) * f ) )
 *     the exact gradient of lam_g * loss_m / N with respect to f_m.  A row that is not valid: +0 in every column, and the row is never read from
 *     fs.  A valid row whose nf is 0 or not finite: loss 0, a +0 row, and it still counts in N (a stated departure, the analogue of 7.22's d == 0
 *     rule).  EVERY row of seed is written by every launch: no memset is ever needed.  d[m] = loss_m of a valid row, 0 elsewhere.  part[g] = the
 *     binary32 sum of workgroup g's losses, tile by tile (a tile: 32 consecutive cells, summed by the xor butterfly), by a plain store; the
 *     buffer holds simt_proto_contrast_parts(M) words.  N == 0 (no valid cell, or fewer than two seen classes): every output is +0 / 0.
 *     lam_g = (float)(lambda * gscale), as in simt_feat_dist_desc.
 *   SCALARS (simt_proto_contrast_finalize):  S = the sum of part[] in double and in index order;  out[0] = lambda * S / N, out[1] = S / N,
 *     out[2] = (float)N.  N == 0: all three are 0.
 *   No atomics: every launch repeats bit for bit.
 * Refused with SIMT_ERR_INVALID, nothing launched and nothing written: a NULL descriptor or pointer (simt_cell_labels: n may be NULL); B, H, W, h
 * or w < 1; h > H or w > W; min_ratio outside (0.5, 1] or NaN; H * W or B * h * w >= 2^31; a label base that is not 8-byte aligned; M < 1 or
 * M >= 2^31; C outside 2 .. SIMT_PROTO_MAX_CLASSES; D outside 8 .. SIMT_PROTO_MAX_DIM or D % 8 != 0; a dtype code other than SIMT_F32 / SIMT_BF16;
 * temp not a finite float > 0; a NaN lam_g or lambda; fs, seed, eta or phat not 16-byte aligned; n, hdr, d, part or out not 4-byte aligned.
 * Rows are dense: the leading dimension of fs, seed, eta and phat is D.
 * LDS: cell labels 4 words, prep 83 words, contrast and finalize none; no scratch. */
typedef struct {
  const int64_t* label;    /* [B][H][W] */
  uint8_t* lab;            /* out [B*h*w] */
  int32_t* part;           /* out [simt_cell_labels_parts(B, h, w)]: cells of a seen class per workgroup */
  const int32_t* n;        /* [C] of 7.26, or NULL: every class counts as seen */
  int32_t B, H, W, h, w, C;
  float min_ratio;
  int32_t reserved_;
} simt_cell_labels_desc;
typedef struct {
  const void* fs;          /* [M][D] student features, dtype */
  const uint8_t* lab;      /* [M] of simt_cell_labels */
  const float* eta;        /* [C][D] */
  const int32_t* n;        /* [C] */
  float* phat;             /* [simt_proto_contrast_phat_floats(C, D)]: out of prep, in of the main launch */
  uint32_t* hdr;           /* [4]: out of prep, in of the main launch and finalize */
  void* seed;              /* out [M][D], dtype */
  float* d;                /* out [M] */
  float* part;             /* out [simt_proto_contrast_parts(M)]: sum of the losses per workgroup */
  float* out;              /* out [3], written by simt_proto_contrast_finalize */
  double lambda;
  int64_t M;
  int32_t D, C, dtype;
  float temp;              /* T */
  float lam_g;             /* (float)(lambda * gscale) */
  int32_t reserved_;
} simt_proto_contrast_desc;
int simt_cell_labels_parts(int B, int h, int w);          /* 0: a geometry the launch refuses */
int simt_proto_contrast_parts(long M);                    /* 0: an M the launches refuse */
long simt_proto_contrast_phat_floats(int C, int D);       /* 0: a geometry the launches refuse */
int simt_cell_labels(const simt_cell_labels_desc* d, simt_stream_t stream);
int simt_proto_contrast_prep(const simt_proto_contrast_desc* d, simt_stream_t stream);
int simt_proto_contrast(const simt_proto_contrast_desc* d, simt_stream_t stream);
int simt_proto_contrast_finalize(const simt_proto_contrast_desc* d, simt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
