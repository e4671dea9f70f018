/*
 * mseg_hip.h — C ABI of libmseg_hip.so, the gfx950 (MI355X / CDNA4) kernel library under the
 * microbeSEG U-Net train / infer / watershed hot path.
 *
 * The reference (hip-satomi/microbeSEG) is pure Python on stock torch.nn / scipy / scikit-image and defines
 * no FFI of its own.  Each entry point below therefore cites the reference *call site* whose
 * library op it replaces.  All pointers are DEVICE pointers unless a name ends in `_host`; the library never
 * allocates user-visible memory, never synchronises the stream on the compute path, and returns 0 on success
 * or a negative MSEG_E* code (never throws across the boundary).  `stream` is a hipStream_t passed as void*.
 *
 * Activation tensors are NHWC fp32 ("pixel-major"): element (n, y, x, c) at ((n*H + y)*W + x)*C + c.
 * A network input/output with one channel is bit-identical in NCHW and NHWC, which is how the Python boundary
 * (NCHW, src/utils/unets.py:349,463) maps onto this layout without a copy.
 */
#ifndef MSEG_HIP_H
#define MSEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSEG_OK 0
#define MSEG_EINVAL (-1)   /* bad argument / unsupported shape */
#define MSEG_ELAUNCH (-2)  /* hipLaunch / runtime error (mseg_last_hip_error() has the hipError_t) */
#define MSEG_EWORKSPACE (-3)

/* activation ids — reference: src/utils/unets.py:115-124 (relu / leakyrelu / elu / mish), Mish at :81-89 */
#define MSEG_ACT_NONE 0
#define MSEG_ACT_RELU 1
#define MSEG_ACT_LEAKY 2 /* negative_slope 0.01 (torch default) */
#define MSEG_ACT_ELU 3   /* alpha 1.0 */
#define MSEG_ACT_MISH 4  /* x * tanh(softplus(x)), softplus threshold 20 */

/* normalisation ids — reference: src/utils/unets.py:127-134 */
#define MSEG_NORM_BN 0 /* BatchNorm2d, stats over (N,H,W) */
#define MSEG_NORM_GN 1 /* GroupNorm(8, C), stats over (C/8,H,W) per sample */
#define MSEG_NORM_IN 2 /* InstanceNorm2d, stats over (H,W) per (sample, channel), no affine */

/* A tensor operand that is *normalised on load*: value(n,p,c) = act(ptr[...]) * scale[n*ss + c] + shift[n*ss + c].
 * scale == NULL means "no affine" (identity), act == MSEG_ACT_NONE means no activation.
 * This is how conv -> activation -> norm (src/utils/unets.py:163-173: ConvBlock.forward) is executed without ever
 * materialising the normalised tensor: the producing conv stores z = conv(x)+b, the consumer applies act+norm. */
#define MSEG_ST_F32 0
#define MSEG_ST_BF16 1 /* tensor stored as bfloat16 in HBM (BASELINE configs[2]); all arithmetic stays fp32 */
typedef struct MsegSrc {
  const float* ptr;   /* [N][H][W][C]; holds bfloat16 elements when dtype == MSEG_ST_BF16 */
  const float* scale; /* [N][C] (ss == C) or [C] (ss == 0), or NULL; always fp32 */
  const float* shift;
  int32_t C;
  int32_t act;
  int32_t ss;
  int32_t dtype;      /* MSEG_ST_F32 / MSEG_ST_BF16 */
} MsegSrc;

/* ---- implicit-GEMM convolution family (fp32 MFMA v_mfma_f32_32x32x2_f32) ---------------------------------
 * Replaces nn.Conv2d 3x3 s1/s2 (unets.py:112,137,192), nn.ConvTranspose2d 2x2 s2 (unets.py:244) and the
 * data-gradients of both (autograd of the same modules, train.py:488).
 *   out[m][n] = bias[n] + sum_t sum_c  A_t[m][c] * w[t][n][c]
 * m indexes the "M-space" pixels (NB, Ho, Wo); A_t[m] is the source pixel selected by tap t:
 *   mode CONV : (iy, ix) = (oy*stride + ky - pad, ox*stride + kx - pad)
 *   mode TCONV: ty = oy + pad - ky must be divisible by stride, iy = ty / stride   (transposed conv = dgrad)
 * the source is the channel-concatenation of src[0..nsrc) (torch.cat([up, skip], 1): unets.py:373,492,502).
 * Epilogue PLAIN: dst = (n < split ? dst0[m*ld0 + n] : dst1[m*ld1 + n - split]) (+= if accN)   (split >= Ngemm: single dst)
 * Epilogue SCATTER2X2 (ConvTranspose2d as a 1x1 GEMM with N = 4*Cq): n = (a*2+b)*Cq + co,
 *   dst0[((img*2Ho + 2oy+a)*2Wo + 2ox+b)*Cq + co], bias index co.                                          */
#define MSEG_MODE_CONV 0
#define MSEG_MODE_TCONV 1
#define MSEG_EPI_PLAIN 0
#define MSEG_EPI_SCATTER2X2 1
#define MSEG_MORDER_LINEAR 0
#define MSEG_MORDER_PARITY 1 /* M ordered by (oy&1, ox&1) class first: lets stride-2 TCONV tiles skip dead taps */
#define MSEG_PREC_F32 0
#define MSEG_PREC_BF16 1

typedef struct MsegIgemm {
  MsegSrc src[2];
  const float* w;    /* packed [T][Npad][Kpad], Npad % 128 == 0, Kpad % 32 == 0, zero filled beyond Ngemm / Cin */
  const float* bias; /* [Ngemm] (PLAIN) / [Cq] (SCATTER2X2) or NULL */
  float* dst0;
  float* dst1;
  int32_t nsrc, Cin, Kpad, Npad;
  int32_t NB, Hi, Wi, Ho, Wo;
  int32_t KH, KW, stride, pad, mode, morder;
  int32_t Ngemm, epi, split, ld0, ld1, acc0, acc1, Cq;
  int32_t precision; /* MSEG_PREC_F32, or MSEG_PREC_BF16: bf16 matrix-core inputs, fp32 accumulate (BASELINE configs[2]) —
                      * 3x3 stride-1 launches only (MSEG_EINVAL otherwise); `w` then points at the bf16 copy of the
                      * packed weights (mseg_f32_to_bf16); bias stays fp32 */
  int32_t dst_dtype; /* MSEG_ST_F32 / MSEG_ST_BF16: element type of dst0 / dst1.  bf16 sources (MsegSrc.dtype) and bf16
                      * destinations need precision == MSEG_PREC_BF16 (MSEG_EINVAL otherwise) */
  /* optional split-K scratch (small batches: fewer 3x3 stride-1 tiles than workgroup slots).  ws == NULL or too small: the
   * launch simply is not split.  Size: mseg_igemm_workspace_bytes(). */
  void* ws;
  size_t ws_bytes;
  /* optional: statistics of the output for the normalisation that follows it, taken in the epilogue instead of by a pass
   * over the stored tensor (unets.py:127-134: conv -> act -> norm).  stats != NULL asks for per-tile partial sums
   * stats[row][0 / 1][Ngemm] = sum / sum of squares of act(z) over the pixels of partial row `row`, z as stored (i.e. of the
   * bf16-rounded value for a bf16 destination), act = stats_act (MSEG_ACT_NONE or MSEG_ACT_RELU).  Only some kernels can:
   * mseg_igemm_query() on the same descriptor reports in MsegKernelInfo.stats_rows how many rows the call will write
   * (0: none — the buffer is left untouched and the caller runs mseg_norm_stats); size the buffer for that.  Plain epilogue,
   * one destination, no accumulation.  Reduced by mseg_norm_stats_from_conv().                                           */
  float* stats;
  int32_t stats_act;
  int32_t reserved0;
} MsegIgemm;

int mseg_igemm(const MsegIgemm* p, void* stream);

/* Which kernel a call maps to.  The query runs the SAME dispatch code as the call it describes and launches nothing
 * (no device work, no stream): same argument checks, same return code (MSEG_EINVAL: no kernel for this descriptor, e.g.
 * MSEG_PREC_BF16 on a shape that has no bf16 kernel), so host code never has to restate a dispatch rule.
 * `name` is the instantiation as rocprofv3's kernel trace prints it, without "void " and the argument list. */
typedef struct MsegKernelInfo {
  char name[120];
  int32_t precision; /* MSEG_PREC_* the kernel computes in */
  int32_t launches;  /* kernel launches of the call (split-K partial + reduction = 2; one-off table initialisation counted) */
  uint32_t grid, block;
  size_t workspace;  /* split-K scratch bytes the call uses (0: none) */
  int32_t stats_rows; /* partial rows the call writes to MsegIgemm.stats (0: the kernel takes no statistics) */
  int32_t reserved0;
} MsegKernelInfo;
int mseg_igemm_query(const MsegIgemm* p, MsegKernelInfo* info);
/* name of the main kernel of this thread's last mseg_igemm / mseg_wgrad / mseg_first_conv_fwd / mseg_first_conv_fwd_raw /
 * mseg_first_wgrad call that launched ("" before the first; a refused call leaves it as it was) */
const char* mseg_last_kernel(void);
/* round-to-nearest-even conversion of n floats to bf16 (the packed weights of a MSEG_PREC_BF16 launch) */
int mseg_f32_to_bf16(const float* src, uint16_t* dst, size_t n, void* stream);
/* bytes of split-K scratch this launch would use (0: it would not be split) */
size_t mseg_igemm_workspace_bytes(const MsegIgemm* p);
/* Test / ablation hook: on = 0 sends the 64 -> 64 channel bf16-storage layers (level 0 of the U-Nets) back to the
 * tile-per-workgroup kernel instead of the persistent one that keeps the layer's weights in LDS.  Same results either
 * way (the tests compare both).  Process-wide; default 1. */
int mseg_igemm_set_persistent(int on);
/* Test / ablation hook: on = 0 sends the 128-channel-tile bf16 layers back from 256-pixel to 128-pixel tiles
 * (igemm_halo_bf16w4m_kernel -> igemm_halo_bf16w4_kernel).  Same results up to the fp32 accumulation order.  Default 1. */
int mseg_igemm_set_wide_tiles(int on);
/* Test / ablation hook for the one-workgroup-per-CU kernel with DMA-streamed weights (igemm_p8.hip: 3x3 stride-1 layers
 * with >= 128 output channels on bf16 tensors): 0 = off (the tile-per-workgroup kernels above), 1 = on (default),
 * 2 = on, 128-channel layers on 256-pixel instead of 512-pixel tiles.  Same results up to the fp32 accumulation order. */
int mseg_igemm_set_p8(int mode);

/* weight gradient: G[t][mch][nch] = sum_p P[p][mch] * Q[gather(p, t)][nch], written to dst[(mch*Nch + nch)*T + t]
 * which *is* torch's layout for both Conv2d.weight (Cout,Cin,KH,KW) [P = dz, Q = conv input] and
 * ConvTranspose2d.weight (Cin,Cout,2,2) [P = convT input, Q = d(convT output), KH=KW=2, stride 2, pad 0].
 * gather: (qy, qx) = (py*stride + ky - pad, px*stride + kx - pad).  Split-K over pixels into `ws`, then a
 * fixed-order reduction (deterministic).  Nch_store <= Nch lets a zero-padded Q (first layer, Cin=1->4) drop pads. */
typedef struct MsegWgrad {
  MsegSrc P;
  MsegSrc Q[2];
  float* ws;  /* >= mseg_wgrad_workspace_bytes() */
  float* dst; /* [Mch][Nch_store][T] */
  int32_t nq, Nch, Nch_store;
  int32_t NB, Hp, Wp, Hq, Wq;
  int32_t KH, KW, stride, pad;
  int32_t splits; /* 0 = choose */
  int32_t phase;  /* 0 = partial + reduce, 1 = split-K partial kernel only, 2 = reduction only (profiling) */
  int32_t precision; /* MSEG_PREC_F32, or MSEG_PREC_BF16: P and Q rounded to bf16 for the matrix cores, fp32 accumulate —
                      * 3x3 stride-1 weight gradients with a plain P only (MSEG_EINVAL otherwise) */
  int32_t reserved;
} MsegWgrad;

size_t mseg_wgrad_workspace_bytes(const MsegWgrad* p);
int mseg_wgrad(const MsegWgrad* p, void* stream);
int mseg_wgrad_query(const MsegWgrad* p, MsegKernelInfo* info);

/* The network's first convolution, Conv2d(ch_in <= 4, Cout, 3, padding=1) (unets.py:303-304,413-414), and its weight
 * gradient for ch_in == 1: HBM-bound VALU kernels (9..36 multiply-adds per output), not worth a 32-channel matrix-core
 * K-step.  x4: raw network input, NHWC with 4 channels (zero padded); w / dW: torch layout (Cout, Cin, 3, 3);
 * z, dz: [N][H][W][Cout].  Cout % 4 == 0, Cout <= 256, 256 % (Cout / 4) == 0 — otherwise MSEG_EINVAL (use mseg_igemm). */
/* z_dtype / dz_dtype: MSEG_ST_F32 or MSEG_ST_BF16 — how z is stored / dz is read (the network input x4 is always fp32) */
int mseg_first_conv_fwd(const float* x4, const float* w, const float* bias, int N, int H, int W, int Cin, int Cout,
                        void* z, int z_dtype, void* stream);
/* K14 on the device — the frame normalisation of the inference loop (reference: infer.py:346-348,
 * infer_script_local.py:130-132: min / max of the frame, top / left padding with min (utils.py:124-163),
 * 2 * (f32(x) - min) / (max - min) - 1) without the host touching a pixel:
 *   mseg_frame_minmax        raw: [npix] uint8 (MSEG_PIX_U8) / uint16 (MSEG_PIX_U16) -> minmax[2] on the device ({~min, max})
 *   mseg_first_conv_fwd_raw  the first convolution Conv2d(1, Cout, 3, padding=1) of ONE frame, reading the raw frame and
 *                            normalising / padding while it loads: the same fp32 operations in the same order as the host
 *                            formula (bit-identical input values); z: [H0 + pad_top][W0 + pad_left][Cout]
 *   mseg_frame_normalize     the normalised, padded frame itself (fp32 [H0 + pad_top][W0 + pad_left]) for networks whose
 *                            first layer does not take the kernel above                                                   */
#define MSEG_PIX_U8 0
#define MSEG_PIX_U16 1
#define MSEG_PIX_I32 2 /* label stacks: mseg_stack_relabel, mseg_cell_measure, mseg_cell_links, mseg_stack_drift, mseg_cell_hull, mseg_cell_midline, mseg_cell_order_stats */
#define MSEG_PIX_F32 3 /* mseg_clahe_u16 only: fp32 holding the integers 0..65535 */
int mseg_frame_minmax(const void* raw, int dtype, size_t npix, uint32_t* minmax, void* stream);
int mseg_first_conv_fwd_raw(const void* raw, int dtype, int H0, int W0, int pad_top, int pad_left, const uint32_t* minmax,
                            const float* w, const float* bias, int Cout, void* z, int z_dtype, void* stream);
int mseg_frame_normalize(const void* raw, int dtype, int H0, int W0, int pad_top, int pad_left, const uint32_t* minmax,
                         float* out, void* stream);
/* The same for a group of N raw frames of one size, [N][H0][W0], every frame with its own extrema: minmax [N][2], out fp32
 * [N][H0 + pad_top][W0 + pad_left].  One launch each; every value bit-identical to the one-frame calls on that frame. */
int mseg_frames_minmax(const void* raw, int dtype, int N, size_t npix_per_frame, uint32_t* minmax, void* stream);
int mseg_frames_normalize(const void* raw, int dtype, int N, int H0, int W0, int pad_top, int pad_left,
                          const uint32_t* minmax, float* out, void* stream);
size_t mseg_first_wgrad_workspace_bytes(int N, int H, int W, int Cout);
int mseg_first_wgrad(const float* x4, const void* dz, int dz_dtype, int N, int H, int W, int Cout, float* dW, void* ws,
                     void* stream);

/* strided repack of a weight tensor into the zero-padded [T][Rpad][Cpad] GEMM operand:
 *   dst[(t*Rpad + r)*Cpad + c] = (r < R && c < C) ? src[t*st + r*sr + c*sc] : 0                             */
int mseg_pack_weight(const float* src, float* dst, int T, int R, int Rpad, int C, int Cpad, int st, int sr, int sc,
                     void* stream);

/* Every repack of a network in one launch, after an optimizer step (replaces the per-layer repacks of the conv
 * weights the forward / data-gradient kernels consume: unets.py:112,137,192,244 hold them in torch's layout).
 * `jobs_dev`: njobs records in DEVICE memory, sorted by first_block; job j owns blocks [first_block[j],
 * first_block[j] + mseg_pack_job_blocks(T, Rpad, Cpad)), total_blocks in all.  dst / dst16 (bf16 operand) may be NULL. */
typedef struct MsegPackJob {
  const float* src;
  float* dst;
  uint16_t* dst16;
  int32_t T, R, Rpad, C, Cpad, st, sr, sc;
  uint32_t first_block;
  uint32_t reserved;
} MsegPackJob;
unsigned mseg_pack_job_blocks(int T, int Rpad, int Cpad);
int mseg_pack_weights_multi(const MsegPackJob* jobs_dev, int njobs, unsigned total_blocks, void* stream);

/* ---- normalisation (BatchNorm2d / GroupNorm(8) / InstanceNorm2d applied AFTER the activation) --------------
 * forward statistics of a = act(z) over an NHWC tensor, fp64 accumulation:
 *   mseg_norm_stats: fills scale/shift ([N][C], ss = C for GN/IN; [C], ss = 0 for BN) such that
 *   y = a*scale + shift, and mean/rstd ([C] BN, [N][8] GN, [N][C] IN) for the backward.
 *   BN training additionally updates running_mean/var with `momentum` (unbiased var), torch semantics
 *   (unets.py:127-128; torch BatchNorm2d defaults eps 1e-5, momentum 0.1).
 * ws: scratch of mseg_norm_workspace_bytes(N, HW, C) bytes.  Its first 64 KiB hold the arrival counters of the in-kernel
 * reductions (the last workgroups of a pass finish the sums and write the tables: no separate reduction launches):
 * ZERO them once after allocating ws (hipMemset); every call leaves them zero.  One ws per concurrent stream.          */
size_t mseg_norm_workspace_bytes(int N, int HW, int C);
/* 1 = the last workgroups of a pass finish the reductions inside the pass kernel, 0 = a pass is followed by separate
 * reduction / finalize launches (same results, bit for bit).  Default 0 (measured faster at batch 32); MSEG_NORM_TAILS in
 * the environment sets it for a process. */
int mseg_norm_set_tails(int on);
/* How a BatchNorm pass's partial sums (and a bias gradient's) become the per-channel results.  2 (default): ONE launch
 * without a hand-off between workgroups — a workgroup owns four channels and does the reduction over the chunks, the sum
 * over the samples and the finalize arithmetic itself, in the order of the launches it replaces (any channel count);
 * 1: the reduction launch whose last workgroup to arrive also finalizes (<= 256 channels, else two launches); 0: always
 * the separate reduction and finalize / column-sum launches; -1: back to the default.  Same bits in every mode.
 * MSEG_NORM_FINISH in the environment sets it for a process. */
int mseg_norm_set_finish(int on);
/* st: MSEG_ST_F32 / MSEG_ST_BF16 = storage of the activation tensors of the call (z, act_out; gy, dz, act_in below).  With
 * bf16 storage a thread owns 8 channels (C % 8 == 0) and the statistics are those of the values as stored.           */
int mseg_norm_stats(const void* z, int N, int HW, int C, int st, int act, int norm, const float* gamma,
                    const float* beta, float eps, float* scale, float* shift, float* mean, float* rstd,
                    float* running_mean, float* running_var, float momentum, void* act_out, void* ws, void* stream);
/* BatchNorm statistics from the partial sums a convolution's epilogue left (MsegIgemm.stats: part[rows][2][C], C = the
 * launch's Ngemm): the same tables, running statistics and saved mean / rstd as mseg_norm_stats(norm = MSEG_NORM_BN) on the
 * stored tensor, without reading it.  count = N * H * W values per channel.  Fixed summation order (rows in 16 slices, then
 * the slices).  ws: as for mseg_norm_stats.                                                                             */
int mseg_norm_stats_from_conv(const float* part, int rows, int C, long long count, const float* gamma, const float* beta,
                              float eps, float* scale, float* shift, float* mean, float* rstd, float* running_mean,
                              float* running_var, float momentum, void* ws, void* stream);
/* act_out (nullable): also store a = act(z).  Used for the expensive activations (mish / elu / leakyrelu): consumers then
 * read `a` with MSEG_ACT_NONE instead of re-evaluating the activation for each of the 9 taps in their K-loops.
 * mseg_activation: a = act(z) alone (eval-mode BatchNorm has no statistics pass).                              */
int mseg_activation(const void* z, int N, int HW, int C, int st, int act, void* act_out, void* stream);
/* eval-mode BatchNorm: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean*scale */
int mseg_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, int C, float* scale, float* shift, void* stream);
/* backward through y = norm(act(z)): given gy = dL/dy writes dz = dL/dz (may alias gy), dgamma, dbeta
 * (NULL for IN) and optionally dbias_prev[c] = sum_p dz (the producing conv's bias gradient).               */
int mseg_norm_bwd(const void* gy, const void* z, int N, int HW, int C, int st, int act, int norm, const float* gamma,
                  const float* mean, const float* rstd, void* dz, float* dgamma, float* dbeta, float* dbias,
                  const void* act_in /* nullable: a = act(z) stored by the forward */, void* ws, void* stream);

/* MaxPool2d(2, 2) of a norm-on-load operand (pool_method = 'max': unets.py:306-307,363-364).  Forward writes the plain
 * pooled tensor [N][H/2][W/2][C]; backward routes gout to the first maximum of each window (torch's rule) and writes
 * (or accumulates into) gin = dL/d(normalised operand), [N][H][W][C].  fp32 tensors only: H and W even, C % 4 == 0 and
 * src->dtype == MSEG_ST_F32, otherwise MSEG_EINVAL and nothing is launched (there is no bf16-storage form).       */
int mseg_maxpool2x2_fwd(const MsegSrc* src, int N, int H, int W, float* out, void* stream);
int mseg_maxpool2x2_bwd(const MsegSrc* src, int N, int H, int W, const float* gout, float* gin, int accumulate,
                        void* stream);

/* ---- 1x1 output heads (unets.py:347,460-461) ------------------------------------------------------------
 * out (NCHW, [N][Co][HW]) = W[Co][C] . norm-on-load(src) + b ; Co <= 4.                                      */
int mseg_head_fwd(const MsegSrc* src, int N, int HW, const float* w, const float* b, int Co, float* out_nchw,
                  void* stream);
/* gy[N][HW][C] = sum_co gout[n][co][p] * W[co][c];  dW[Co][C], db[Co] (fp64 accumulation, deterministic) */
size_t mseg_head_bwd_workspace_bytes(int N, int HW, int C, int Co);
int mseg_head_bwd(const MsegSrc* src, int N, int HW, const float* w, int Co, const float* gout_nchw, void* gy,
                  int gy_dtype /* MSEG_ST_*: storage of the gradient written to gy */, float* dW, float* db, void* ws,
                  void* stream);

/* softmax over the 3 boundary classes of logits [3][Hp][Wp] -> probabilities [Hp-pad_y][Wp-pad_x][3] (HWC), top/left
 * padding cropped: F.softmax(dim=1) + slice + transpose in front of boundary_postprocessing (infer.py:371-374). */
int mseg_softmax3_hwc(const float* logits_chw, int Hp, int Wp, int pad_y, int pad_x, float* probs_hwc, void* stream);

/* ---- losses (src/training/losses.py) -----------------------------------------------------------------------
 * smooth-L1 (beta 1, mean) / L1 / MSE of one head, forward value and gradient in one pass (losses.py:24-32).
 * kind: 0 smooth_l1, 1 l1, 2 l2.  loss_out[0] = mean loss; grad = d(loss)/d(pred) * gscale_dev[0] (or 1).    */
size_t mseg_loss_workspace_bytes(size_t n);
int mseg_regression_loss(const float* pred, const float* target, size_t n, int kind, float* loss_out,
                         void* ws, void* stream);
int mseg_regression_loss_bwd(const float* pred, const float* target, size_t n, int kind, const float* gscale_dev,
                             float* grad, void* stream);
/* ce_dice (losses.py:71-97): CE(logits, y) + 0.5 * sum_{c=1,2} c * (1 - (2 sum g p + 1)/(sum g^2 + sum p^2 + 1)),
 * logits NCHW [N][3][HW], labels int64 [N][HW].  sums[6] = {sum g1 p1, sum p1^2, sum g1, sum g2 p2, sum p2^2, sum g2}
 * are exposed so a data-parallel caller can all-reduce them between the two calls.        */
int mseg_ce_dice_fwd(const float* logits, const int64_t* labels, int N, int HW, int with_dice, double* sums6,
                     double* ce_sum, void* ws, void* stream);
/* dice_weight: 1 for single-process training; the world size under data parallelism (the Dice term is a function
 * of GLOBAL sums, so its per-rank gradient must survive the 1/world averaging of the gradient all-reduce).   */
int mseg_ce_dice_bwd(const float* logits, const int64_t* labels, int N, int HW, int with_dice, const double* sums6,
                     double total_px, double dice_weight, const float* gscale_dev, float* grad, void* stream);

/* ---- instance masks -> polygon ROIs --------------------------------------------------------
 * Replaces get_indices_pandas + the per-instance cv2_countour loop (src/utils/hull_polygon.py:8-89, called from
 * src/inference/infer.py:274-287) for a whole uint16 label image [H][W] (0 = background) on the device.
 * mseg_polygons_find: start candidates (pixels whose W / NW / N / NE neighbours carry another label) into cand_px, and
 *   per candidate its label (cand_id) and the length of the OUTER border that starts there (cand_len; 0 when the
 *   candidate is not the raster-first pixel of an outer border).  *n_cand_dev = candidates found; if it exceeds
 *   `capacity` the surplus was dropped and the caller repeats the call with larger arrays.
 * mseg_polygons_trace: polygon k starts at pixel start_px[k] and owns points offsets[k] .. offsets[k+1]-1 of points_yx
 *   ((row, col) int32 pairs, in the order cv2.findContours(..., CHAIN_APPROX_NONE) lists an outer border: from the
 *   top-left-most pixel DOWN the left side, every visited pixel, 8-connected foreground).                              */
int mseg_polygons_find(const uint16_t* labels, int H, int W, int32_t* cand_px, int32_t* cand_id, int32_t* cand_len,
                       int capacity, int32_t* n_cand_dev, void* stream);
int mseg_polygons_trace(const uint16_t* labels, int H, int W, const int32_t* start_px, const int64_t* offsets, int n_poly,
                        int32_t* points_yx, void* stream);

/* ---- fused optimizers (train.py:379-428, ranger2020.py:101-208) --------------------------------------------- */
/* torch.optim.Adam(amsgrad=True, weight_decay=0) on ONE flat range (train.py:380-385): p, g, exp_avg, exp_avg_sq,
 * max_exp_avg_sq of n elements; `step` = 1-based step count.  Hyper-parameters are doubles (python floats): 1 - beta,
 * the bias corrections and lr / bc1 are evaluated in fp64 and rounded to fp32 once, as torch does.                   */
int mseg_adam_amsgrad_step(float* p, const float* g, float* m, float* v, float* vmax, size_t n, double lr,
                           double beta1, double beta2, double eps, int step, void* stream);
/* The same update with learning rate and step count in DEVICE memory (no per-step host scalar: the launch can be recorded
 * in a hipGraph and replayed).  `state` = 4 doubles on the device: [0] learning rate (the host rewrites it when a scheduler
 * changes it), [1] steps done so far (this call adds 1 before it updates), [2..3] scratch of the call.  Two launches: a
 * one-thread kernel that advances the counter and derives lr / (1 - beta1^step), sqrt(1 - beta2^step) in fp64, and the
 * update.                                                                                                               */
int mseg_adam_amsgrad_step_dev(float* p, const float* g, float* m, float* v, float* vmax, size_t n, double* state,
                               double beta1, double beta2, double eps, void* stream);
/* One Ranger update of one parameter tensor (ranger2020.py:142-206): gradient centralisation over dims 1.. (do_gc, rows =
 * shape[0]), moments, rectified or plain-momentum update with step_lr = step_size * lr (host-side RAdam buffer,
 * ranger2020.py:160-176), and the lookahead blend every k-th step (lookahead = 1).                              */
int mseg_ranger_step(float* p, const float* g, float* m, float* v, float* slow, size_t n, int rows, double beta1,
                     double beta2, double eps, double step_lr, int rectified, int do_gc, int lookahead, double alpha,
                     void* stream);
/* The same update for many parameter tensors (ranger2020.py:117-206, the loop over group['params']): `jobs` are njobs
 * records in HOST memory; they travel in kernel arguments, 48 per launch.  rows > 0: gradient centralisation with rows =
 * shape[0]; rows = 0: none.  step_lr / flags are per tensor because the reference keeps `step` per parameter.         */
typedef struct MsegRangerJob {
  float* p;
  const float* g;
  float* m;        /* exp_avg     */
  float* v;        /* exp_avg_sq  */
  float* slow;     /* slow_buffer */
  uint64_t n;
  int32_t rows;
  float step_lr;   /* step_size * lr */
  uint32_t flags;  /* bit 0: rectified (N_sma > threshold), bit 1: lookahead blend this step */
  uint32_t reserved;
} MsegRangerJob;
int mseg_ranger_step_multi(const MsegRangerJob* jobs, int njobs, double beta1, double beta2, double eps, double alpha,
                           void* stream);

/* ---- inference post-processing (src/inference/postprocessing.py) --------------------------------------------
 * distance_postprocessing(border, cell, th_seed, th_cell) (postprocessing.py:7-59) and
 * boundary_postprocessing(softmax probs HWC) (postprocessing.py:62-90): gaussian(0.5) -> thresholds -> 8-conn CCL
 * -> small-seed removal -> relabel -> marker watershed (4-conn), labels bit-exact.  Inputs: device fp32 [H][W]
 * (distance) / [H][W][3] (boundary); output: device uint16 [H][W].  `col_major_ids` selects the id numbering the
 * reference gets for (H,W,1) inputs.  status_dev[0] receives flags (bit0: exact
 * serial path was used).                                                                                        */
size_t mseg_postproc_workspace_bytes(int H, int W);
/* Test / tuning hook of the per-component watershed flood (one wavefront per mask component, csrc/postproc.hip):
 * heap_rows = rows of the wave's queue kept in LDS (1..16, the rest spills to the workspace); tile_small_px /
 * tile_large_px = bounding-box capacities (pixels incl. a 1 px rim) of the two LDS-staged launches (<= 8192 / <= 30720;
 * 0 = probe global memory instead).  Negative values restore the defaults.  Results never depend on these values; the
 * tests use them to drive the spill and global-probe paths.  Process-wide. */
int mseg_postproc_tuning(int heap_rows, int tile_small_px, int tile_large_px);
/* Test / ablation hook: the marker phase of a constant-image flood (the boundary method: watershed(image = mask), every key
 * ties) — 1 (default) = the closed form of what the reference's binary heap does with equal keys (markers surface in the
 * preorder of the implicit heap tree, array slots turn into pushed entries in its postorder, a marker still in the array's
 * last slot jumps the queue; 64 pops per step), 0 = the replay of the heap itself.  Same pop and push order, same labels. */
int mseg_postproc_set_const_stream(int on);
int mseg_distance_postprocess(const float* border, const float* cell, int H, int W, float th_cell, float th_seed,
                              int col_major_ids, uint16_t* labels, int32_t* n_instances_dev, int32_t* status_dev,
                              void* ws, size_t ws_bytes, void* stream);
int mseg_boundary_postprocess(const float* probs_hwc, int H, int W, uint16_t* labels, int32_t* n_instances_dev,
                              int32_t* status_dev, void* ws, size_t ws_bytes, void* stream);
/* The same in three calls, so that the frames of a stack (infer.py:250-259: a 2D+t stack, frame by frame) can be in flight
 * together: _pre per frame on its OWN workspace (thresholds, components, marker list), ONE _flood_batch for up to 8 frames
 * — the boundary method's flood is one wavefront busy for ~45 ms per 2048 x 2048 frame, a latency and not a load, and the
 * batch launch runs one workgroup per frame — then _post per frame.  ws_list: B host pointers to the frames' device
 * workspaces.  pre + flood_batch(B = 1) + post makes the launches of mseg_boundary_postprocess: same labels bit for bit. */
int mseg_boundary_postprocess_pre(const float* probs_hwc, int H, int W, void* ws, size_t ws_bytes, void* stream);
int mseg_boundary_flood_batch(void* const* ws_list, int B, int H, int W, void* stream);
int mseg_boundary_postprocess_post(int H, int W, uint16_t* labels, int32_t* n_instances_dev, int32_t* status_dev, void* ws,
                                   size_t ws_bytes, void* stream);

/* Threshold sweep of the evaluation (EvalWorker.inference, src/evaluation/eval.py:127-131,397-409: one
 * distance_postprocessing per (th_cell, th_seed) pair on the same prediction).  The smoothed cell map is computed once;
 * th_cell / th_seed are HOST arrays of nth floats; labels [nth][H][W], n_instances_dev / status_dev [nth] (nullable). */
int mseg_distance_postprocess_sweep(const float* border, const float* cell, int H, int W, const float* th_cell,
                                    const float* th_seed, int nth, int col_major_ids, uint16_t* labels,
                                    int32_t* n_instances_dev, int32_t* status_dev, void* ws, size_t ws_bytes,
                                    void* stream);

/* Distance post-processing of N frames of one size in ONE chain of launches (a stack of small frames: the per-frame chain
 * is ~45 launches over a few tens of thousands of pixels).  border / cell point at the un-padded origin of frame 0 inside
 * the (possibly padded) predictions and are read in place: element (f, y, x) lies at f * frame_stride + y * row_stride + x
 * (strides in floats).  labels [N][H][W], n_instances_dev / status_dev [N] (nullable): frame i gets, bit for bit, what
 * mseg_distance_postprocess returns for it alone — a frame whose flood meets a tie is redone by the exact serial flood over
 * that frame only (one workgroup per frame).  The number of launches does not depend on N.  N <= 65535,
 * N * (H + 1) * W < 2^31; ws: mseg_postproc_batch_workspace_bytes(N, H, W) bytes.                                        */
size_t mseg_postproc_batch_workspace_bytes(int N, int H, int W);
int mseg_distance_postprocess_batch(const float* border, const float* cell, int N, int H, int W, long long row_stride,
                                    long long frame_stride, float th_cell, float th_seed, int col_major_ids,
                                    uint16_t* labels, int32_t* n_instances_dev, int32_t* status_dev, void* ws,
                                    size_t ws_bytes, void* stream);

/* ---- training augmentation on the device (src/training/mytransforms.py:12-406) ------------------
 * The reference pipeline Flip -> Contrast -> Scaling -> Rotate -> Blur -> Noise -> ToTensor runs per sample on the CPU; here
 * the host draws every sample's random decisions along the same decision tree and these calls apply them to a batch of
 * fp32 planes [N][H][W] (uint16 value range until the final normalisation).  All *_dev arguments are device arrays.
 *   flip: codes[N] in 0..7 = identity, fliplr, flipud, rot90, rot180, rot270, fliplr+rot90, flipud+rot90 (np.rot90: ccw).
 *   affine: mats[N][6], source (x, y) = (m0 x + m1 y + m2, m3 x + m4 y + m5) of destination pixel (x, y); bilinear
 *           (nearest != 0: order 0 for uint8 labels), constant border 0; apply[N] == 0 copies the sample.
 *   blur: scipy.ndimage.gaussian_filter semantics (radius int(4 sigma + 0.5), 'reflect'); sigma <= 0 copies.
 *   stats: {min, max, mean}[N] (+ 65536-bin histogram per sample when hist != NULL).
 *   contrast_params / contrast: choice[N][4] = {mode, a, b, -}: mode 1 stretch to the (a, b) percentiles
 *           (np.percentile + rescale_intensity), mode 2 contrast factor a and gamma b (mytransforms.py:103-122).
 *   clahe: choice[s][0] == 3: contrast-limited adaptive histogram equalisation (equalize_adapthist defaults: 8 x 8 tiles,
 *           256 bins, clip limit 0.01; mytransforms.py:92-95), other samples copied; ws >= mseg_aug_clahe_workspace_bytes(N).
 *   noise_normalize: additive Gaussian noise of sigma = frac[N] * max (0: none), clip to uint16, then ToTensor's
 *           min_max_normalization to [-1, 1] with (vmin, vmax).                                                     */
int mseg_aug_u16_to_f32(const uint16_t* in, float* out, size_t n, void* stream);
int mseg_aug_flip(const float* in, float* out, int N, int H, int W, const int32_t* codes_dev, void* stream);
int mseg_aug_affine(const float* in, float* out, int N, int H, int W, const float* mats_dev, const int32_t* apply_dev,
                    int nearest, void* stream);
int mseg_aug_blur(const float* in, float* tmp, float* out, int N, int H, int W, const float* sigmas_dev, void* stream);
int mseg_aug_stats(const float* in, int N, int H, int W, float* stats_dev, uint32_t* hist_dev, void* stream);
int mseg_aug_contrast_params(const float* stats_dev, const uint32_t* hist_dev, const float* choice_dev, int N, int HW,
                             float* par_dev, void* stream);
int mseg_aug_contrast(const float* in, float* out, int N, int H, int W, const float* par_dev, void* stream);
size_t mseg_aug_clahe_workspace_bytes(int N);
int mseg_aug_clahe(const float* in, float* out, int N, int H, int W, const float* choice_dev, void* ws, void* stream);
int mseg_aug_noise_normalize(const float* in, float* out, int N, int H, int W, const float* frac_dev,
                             const float* stats_dev, uint32_t seed, float vmin, float vmax, void* stream);

/* ---- library-exact CLAHE (csrc/clahe.hip) -----------------------------------------------------------------
 * (65535 * skimage.exposure.equalize_adapthist(img, clip_limit=0.01)).astype(np.uint16) of scikit-image 0.18.3, bit for
 * bit, for N images [N][H][W] of one shape (src/training/mytransforms.py:92-95, src/inference/inference_dataset.py:63-77).
 *   in:  uint8 (MSEG_PIX_U8, taken * 257 like img_as_uint), uint16 (MSEG_PIX_U16) or fp32 holding integers 0..65535
 *        (MSEG_PIX_F32); out: uint16 (MSEG_PIX_U16) or fp32 (MSEG_PIX_F32) holding the uint16 result.
 *   apply_dev: int32[N] on the device, 0 = copy the image through unchanged (the stored value; fp32 -> fp32 value-exact);
 *        NULL = all images.  ws >= mseg_clahe_workspace_bytes(N, H, W) (0 for an unsupported shape).
 *   MSEG_EINVAL: H or W < 8 (the tile H / 8 x W / 8 would be empty), H * W >= 2^31, N > 65535, a dtype not listed, in == out;
 *   MSEG_EWORKSPACE: ws_bytes too small.  Nothing is launched in either case.                                          */
size_t mseg_clahe_workspace_bytes(int N, int H, int W);
int mseg_clahe_u16(const void* in, int in_dtype, int N, int H, int W, const int32_t* apply_dev, void* out, int out_dtype,
                   void* ws, size_t ws_bytes, void* stream);

/* ---- label creation for the boundary method (first part) --------------------------------------------
 * boundary_label (mode 0) / border_label (mode 1) of src/training/train_data_representations.py:75-125 for a batch of
 * instance masks [N][H][W] (uint16): 2 = boundary / touching border, 1 = cell interior, 0 = background; exact.       */
int mseg_label_boundary(const uint16_t* mask, int N, int H, int W, int mode, uint8_t* out, void* stream);

/* ---- label creation for the distance method (second part) ---------------------------------------------
 * distance_label(label, search_radius) of src/training/train_data_representations.py:261-361 (with bottom_hat_closing
 * :40-72) for a batch of instance masks [N][H][W] (uint16): cell_out = per-cell normalised Euclidean distance transform
 * inside the search window around the rounded centroid; neighbor_out = neighbour distances (inverse normalised distance
 * to the other cells of the window, gaps between close cells from the disk(3) bottom-hat transform, borders of touching
 * cells), rescaled and closed with a 3x3 grey closing.  Both float32 [N][H][W].  ws: device scratch of at least
 * mseg_label_distance_workspace_bytes(N, H, W) bytes (0 = unsupported shape; H, W <= 32767).                          */
size_t mseg_label_distance_workspace_bytes(int N, int H, int W);
int mseg_label_distance(const uint16_t* mask, int N, int H, int W, int search_radius, float* cell_out,
                        float* neighbor_out, void* ws, size_t ws_bytes, void* stream);
/* bottom_hat_closing(label) of train_data_representations.py:40-72 alone: root_out[N][H][W] = raster index (inside its image)
 * of the first pixel of the gap component a pixel belongs to, -1 outside the gaps (the rank of a root among the distinct
 * roots of an image + 1 is measure.label's id); corr_out = 0 outside, 1 inside a gap, 0.8 on the 4-neighbour rim of a gap
 * with minor_axis_length >= 3.  Same workspace as mseg_label_distance.                                                */
int mseg_label_bottom_hat(const uint16_t* mask, int N, int H, int W, int32_t* root_out, float* corr_out, void* ws,
                          size_t ws_bytes, void* stream);
/* j4_label(label, k_neighbors, se_radius) of train_data_representations.py:157-216 (Pena et al. 2020): 0 background,
 * 1 cell, 2 touching (another instance inside the (2k+1)^2 window), 3 gap (bottom-hat with disk(se_radius)); uint8.
 * tmp: device scratch of N*H*W bytes.                                                                                 */
int mseg_label_j4(const uint16_t* mask, int N, int H, int W, int k_neighbors, int se_radius, uint8_t* tmp, uint8_t* out,
                  void* stream);
/* cell_distance_label(label, search_radius, apply_clipping, clip_val) of train_data_representations.py:219-258: the cell
 * distances alone; clip_val == 0: normalised per cell (label types 'cell_dist'), > 0: min(d, clip_val) / clip_val
 * ('cell_dist_clipped', clip_val 5).  Same workspace as mseg_label_distance.                                          */
int mseg_label_cell_distance(const uint16_t* mask, int N, int H, int W, int search_radius, float clip_val,
                             float* cell_out, void* ws, size_t ws_bytes, void* stream);
/* Largest skimage regionprops major_axis_length over the cells of each mask (CreateLabelsWorker.create_labels,
 * src/training/train.py:73-78, which sets search_radius = ceil(0.75 * ceil(max major axis))): out_dev double [N].    */
size_t mseg_label_major_axis_workspace_bytes(int N);
int mseg_label_max_major_axis(const uint16_t* mask, int N, int H, int W, double* out_dev, void* ws, size_t ws_bytes,
                              void* stream);

/* ---- evaluation helpers (EvalWorker.calc_scores, src/evaluation/eval.py:248-256) -----------------
 * mseg_eval_relabel: border_correction(mask, border_width) (src/utils/utils.py:25-47: instances not visible inside the
 *   frame minus its border are deleted) followed by skimage.measure.label (8-neighbours of EQUAL value connect; new ids
 *   1..K in raster order of each component's first pixel) -> lab_out int32 [H][W], *n_out_dev = K.
 * mseg_eval_pair_counts: the integer statistics of get_fast_aji_plus (src/evaluation/stats_utils.py:98-179) for two
 *   contiguous label images: area_t[nt+1], area_p[np+1], inter[nt+1][np+1] (device arrays, zeroed by the call).     */
size_t mseg_eval_workspace_bytes(int H, int W);
int mseg_eval_relabel(const uint16_t* mask, int H, int W, int border_width, int32_t* lab_out, int32_t* n_out_dev,
                      void* ws, size_t ws_bytes, void* stream);
int mseg_eval_pair_counts(const int32_t* true_lab, const int32_t* pred_lab, int H, int W, int nt, int np,
                          int32_t* area_t, int32_t* area_p, int32_t* inter, void* stream);

/* ---- analysis / result export (AnalysisWorker.analyze_data src/inference/analysis.py:112-170,
 * ResultExportWorker.export_data src/inference/result_export.py:112-190) --------------------------------------------------
 * Polygons of a whole stack in the reference's iteration order, as CSR arrays: polygon k (0-based) owns the (row, col)
 * int32 pairs rc[2*voff[k]] .. rc[2*voff[k+1]-1], already clamped to the image as make_coordinates clamps them
 * (analysis.py:214-234), and lies in frame frame[k] (frames outside 0..T-1 are skipped).
 * mseg_roi_fill: mask[T][H][W] int32 = the value the reference's stack holds after `mask[t, rr, cc] = cell_id` for every
 *   polygon (skimage.draw.polygon, analysis.py:126-128): the last polygon covering a pixel wins (atomicMax of k + 1), and
 *   cell ids 65536 .. 66534 wrap to k & 0xFFFF as in the reference's uint16 stack (int32 from cell_id 66535 on,
 *   analysis.py:136-137).  Zeroes mask itself.
 * mseg_roi_outline: outlines[T][H][W] uint8 0/1 = polygon_perimeter(r, c, shape, clip=True) (analysis.py:130-132):
 *   skimage.draw.line along every edge of the closed polygon, in-image pixels only.  Zeroes outlines itself.
 * mseg_stack_relabel: per frame skimage.measure.label(frame, background=0) (analysis.py:139-140) of a uint16
 *   (MSEG_PIX_U16) or int32 (MSEG_PIX_I32) stack: lab_out int32, k_out_dev[t] = components of frame t.  T*H*W < 2^31.
 * mseg_region_stats: per frame t and label l in 1..K_t (K_t = label_off[t+1] - label_off[t], label_off on the device,
 *   label_off[T] = n_labels) the regionprops area / axis_major_length / axis_minor_length (analysis.py:158-164) at index
 *   label_off[t] + l - 1 (area 0: label absent), and total_area[t] = the sum of all label values of frame t (np.sum of the
 *   mask, analysis.py:156).  Integer moment sums with 64-bit atomics (deterministic).  Every sum is exact whenever its
 *   true value fits uint64, at any frame width.
 * mseg_overlay_rgb: out = uint8(clip(255 * f32(img) / max(img), 0, 255)) with outline pixels (255, 255, 0)
 *   (result_export.py:183-190); img uint8 / uint16 [T][H][W] (C == 1; out [T][H][W][3]) or [T][H][W][C] with C >= 3
 *   (out [T][H][W][C], channels 0..2 of outline pixels replaced).  The maximum is taken over the stack on the device.    */
size_t mseg_roi_fill_workspace_bytes(int n_poly);
int mseg_roi_fill(const int32_t* rc, const int64_t* voff, const int32_t* frame, int n_poly, int T, int H, int W,
                  int32_t* mask, void* ws, size_t ws_bytes, void* stream);
int mseg_roi_outline(const int32_t* rc, const int64_t* voff, const int32_t* frame, int n_poly, int64_t n_vert, int T, int H,
                     int W, uint8_t* outlines, void* stream);
size_t mseg_stack_relabel_workspace_bytes(int T, int H, int W);
int mseg_stack_relabel(const void* values, int dtype, int T, int H, int W, int32_t* lab_out, int32_t* k_out_dev, void* ws,
                       size_t ws_bytes, void* stream);
size_t mseg_region_stats_workspace_bytes(int64_t n_labels);
int mseg_region_stats(const int32_t* labels, int T, int H, int W, const int64_t* label_off, int64_t n_labels, int64_t* area,
                      double* major, double* minor, uint64_t* total_area, void* ws, size_t ws_bytes, void* stream);
size_t mseg_overlay_workspace_bytes(void);
int mseg_overlay_rgb(const void* img, int dtype, int T, int H, int W, int C, const uint8_t* outlines, uint8_t* out,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- per-cell table of a segmented stack (csrc/cells.hip) — an extension, the reference has no such table --
 * labels: uint16 (MSEG_PIX_U16) or int32 (MSEG_PIX_I32) [T][H][W]; label_off: int64 [T + 1] on the device as in
 * mseg_region_stats: cell l of frame t has slot label_off[t] + l - 1, label_off[T] = n_labels; ids beyond a frame's table
 * (and negative ones) are ignored, ids that are absent keep area 0.  H * W < 2^31 - 512.
 * mseg_cell_measure: img is the intensity image, uint8 (MSEG_PIX_U8) or uint16 (MSEG_PIX_U16), read in place: element
 *   (t, ch, y, x) lies at t * frame_stride + ch * chan_stride + y * row_stride + x * pix_stride, in elements ([T,C,H,W],
 *   [T,H,W], [H,W,3] and [3,H,W] sources without a copy).  C == 0 or img == NULL: shape only, no channel buffer is touched.
 *   Outputs (all integers, written whole by the call, exact and independent of summation order):
 *     shape      uint64 [6][n_labels]     area, sum_y, sum_x, sum_yy, sum_xx, sum_xy of the cell's pixel coordinates
 *     bbox       int32  [n_labels][4]     min_row, min_col, max_row + 1, max_col + 1 (scikit-image's half-open box)
 *     ch_sums    uint64 [2][C][n_labels]  sum and sum of squares of the cell's pixel values per channel
 *     ch_minmax  uint32 [2][C][n_labels]  min and max
 *     bg_sums    uint64 [3][T][C]         count, sum and sum of squares over the background (label 0) of a frame
 *     bg_minmax  uint32 [2][T][C]         its min and max
 *   An absent cell has zeros everywhere (bbox and min included), and so has a frame without background pixels.
 *   Every sum is exact whenever its true value fits uint64, at any frame width.
 * mseg_cell_links: for every frame t >= 1 and cell l of it, pred[slot] = the label m of frame t - 1 (1 <= m <= K_{t-1})
 *   that shares the most pixels (same y, x) with l, ties to the smallest m, 0 where nothing overlaps; overlap[slot] = that
 *   pixel count; frame 0 gets zeros.  The (l, m) pairs of a frame pair are counted in an open-addressing table of
 *   table_cap entries (a power of two, 64 <= table_cap <= 2^31; a table of more than H * W entries cannot fill up);
 *   status: int32 [T] on the device, status[t] != 0: the table of the pair (t - 1, t) was full, pred / overlap of frame t
 *   are then NOT valid and the pair has to be redone with a larger table.  ws >= mseg_cell_links_workspace_bytes (12 bytes
 *   per table entry and frame pair + 8 per cell; 0 = bad arguments).                                                     */
int mseg_cell_measure(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                      const void* img, int img_dtype, int C, int64_t frame_stride, int64_t chan_stride, int64_t row_stride,
                      int64_t pix_stride, uint64_t* shape, int32_t* bbox, uint64_t* ch_sums, uint32_t* ch_minmax,
                      uint64_t* bg_sums, uint32_t* bg_minmax, void* stream);
size_t mseg_cell_links_workspace_bytes(int T, int64_t n_labels, int64_t table_cap);
int mseg_cell_links(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                    int64_t table_cap, int32_t* pred, int32_t* overlap, int32_t* status, void* ws, size_t ws_bytes,
                    void* stream);

/* ---- drift-compensated linking (csrc/drift.hip, csrc/cells.hip) — an extension ---------------------------
 * labels, dtype and label_off as for mseg_cell_links.  A pixel is foreground, F_t(y, x), when its id is in 1 .. K_t (ids
 * beyond the frame's table and negative ids are background).
 * mseg_stack_drift: R = max_drift, 0 <= R <= 128; scores: uint32 [T - 1][2R + 1][2R + 1] on the device, written whole by
 *   the call; for the pair (t - 1, t), t >= 1:
 *     scores[t - 1][dy + R][dx + R] = #{(y, x): 0 <= y < H, 0 <= x < W, 0 <= y - dy < H, 0 <= x - dx < W,
 *                                              F_t(y, x) and F_{t-1}(y - dy, x - dx)}
 *   = the foreground of frame t - 1 moved by (dy, dx) and laid over the foreground of frame t; pixels moved out of the
 *   frame count nothing.  T == 1 writes nothing.  Integers only, independent of the order of arrival.  H * W < 2^31 - 512.
 *   ws >= mseg_stack_drift_workspace_bytes (one bit per pixel, rows padded to 64-bit words + 5 words; 0 = bad arguments);
 *   MSEG_EINVAL: bad arguments, R outside 0 .. 128, a dtype not listed; MSEG_EWORKSPACE: ws_bytes too small.
 * mseg_cell_links_shifted: mseg_cell_links (same outputs, workspace, status word and tie rule) with another pairing: pixel
 *   (y, x) of frame t pairs with (y - dy_t, x - dx_t) of frame t - 1, or with nothing where that lies outside the frame.
 *   shift: int32 [T][2] = (dy_t, dx_t) on the device, entry 0 unused; any int32 is legal (|dy| >= H or |dx| >= W: no
 *   pairs).  All shifts zero: the outputs of mseg_cell_links, byte for byte.                                             */
size_t mseg_stack_drift_workspace_bytes(int T, int H, int W);
int mseg_stack_drift(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int max_drift,
                     uint32_t* scores, void* ws, size_t ws_bytes, void* stream);
int mseg_cell_links_shifted(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                            int64_t table_cap, const int32_t* shift, int32_t* pred, int32_t* overlap, int32_t* status,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- linking under a tile-wise displacement field (csrc/drift.hip, csrc/cells.hip) — an extension ---------
 * labels, dtype, label_off and the foreground F_t as above.  tile = B, one of 64, 128, 256; frame t is cut into
 * ty = ceil(H / B) x tx = ceil(W / B) tiles, tile (j, i) = rows jB .. min((j + 1)B, H) - 1, columns iB .. min((i + 1)B, W) - 1.
 * mseg_stack_flow: r = radius, 0 <= r <= 32; base: int32 [T][2] = (by_t, bx_t) on the device, entry 0 unused, the shift of
 *   the pair (t - 1, t) around which its tiles search; any int32 is legal.  scores: uint32 [T - 1][ty][tx][2r + 1][2r + 1]
 *   on the device, written whole by the call:
 *     scores[t - 1][j][i][ey + r][ex + r] = #{(y, x) in tile (j, i) of frame t: 0 <= y - by_t - ey < H,
 *                                              0 <= x - bx_t - ex < W, F_t(y, x) and F_{t-1}(y - by_t - ey, x - bx_t - ex)}
 *   The source is read from the whole of frame t - 1, not from the tile: cells that enter a tile from a neighbouring tile
 *   count; a source outside the frame counts nothing.  Summed over the tiles this is mseg_stack_drift's score at the shift
 *   base + e.  T == 1 writes nothing.  Every score is one plain store: identical bytes from run to run.
 *   H * W < 2^31 - 512.  ws >= mseg_stack_flow_workspace_bytes (= mseg_stack_drift_workspace_bytes; 0 = bad arguments);
 *   MSEG_EINVAL: bad arguments, a tile not listed, r outside 0 .. 32, a dtype not listed; MSEG_EWORKSPACE: ws_bytes too
 *   small; either way nothing is written.
 * mseg_cell_links_field: mseg_cell_links (same outputs, workspace, pair table, status word, redo rule and tie rule) with
 *   another pairing: pixel (y, x) of frame t pairs with (y - field[t][y / B][x / B][0], x - field[t][y / B][x / B][1]) of
 *   frame t - 1, or with nothing where that lies outside the frame.  field: int32 [T][ty][tx][2] on the device, frame 0
 *   unused; any int32 is legal.  A field constant over every frame: the outputs of mseg_cell_links_shifted with that shift,
 *   byte for byte.  MSEG_EINVAL also for a tile not listed.                                                               */
size_t mseg_stack_flow_workspace_bytes(int T, int H, int W);
int mseg_stack_flow(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int tile, int radius,
                    const int32_t* base, uint32_t* scores, void* ws, size_t ws_bytes, void* stream);
int mseg_cell_links_field(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                          int64_t table_cap, int tile, const int32_t* field, int32_t* pred, int32_t* overlap,
                          int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- links across missed frames (csrc/cells.hip) — an extension -------------------------------------------
 * mseg_cell_links_gap: mseg_cell_links (same outputs, workspace, pair table, status word per frame t, redo rule and tie
 *   rule) against frame t - gap instead of frame t - 1, 1 <= gap <= 5, and between flagged cells only.  want, open: uint8
 *   [n_labels] on the device in label_off order; want[slot] != 0: the cell of frame t takes part, open[slot] != 0: the cell
 *   of frame t - gap may be found.  Pixel (y, x) of frame t pairs with (y - dy, x - dx) of frame t - gap, or with nothing
 *   where that lies outside the frame: shift == NULL and tile == 0: (dy, dx) = (0, 0); tile == 0 with shift: int32 [T][2],
 *   one (dy, dx) per frame t; tile one of 64, 128, 256 with shift: int32 [T][ty][tx][2] in the layout of
 *   mseg_cell_links_field.  The motion is the caller's, ALREADY COMPOSED over the gap; any int32 is legal.  pred[slot] names
 *   a label of frame t - gap; pred / overlap are 0 for cells with want == 0, for frames t < gap, and everywhere when
 *   gap >= T (MSEG_OK).  Ids that are no cell of their frame index no flag.  gap == 1 with all flags set: the outputs of
 *   mseg_cell_links / _shifted / _field, byte for byte.  MSEG_EINVAL also for a gap outside 1 .. 5, a tile without a shift
 *   and a tile not listed; nothing is written then.                                                                        */
int mseg_cell_links_gap(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                        int64_t table_cap, int gap, int tile, const int32_t* shift, const uint8_t* want,
                        const uint8_t* open, int32_t* pred, int32_t* overlap, int32_t* status, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- per-cell outline measures (csrc/hull.hip) — an extension --------------------------------------------
 * labels, dtype and label_off as for mseg_cell_links.  A cell is the union of the closed unit squares of its pixels: pixel
 * (y, x) is the square with the corners (y, x) .. (y + 1, x + 1), so corners are integer points in 0..H x 0..W.  A cell may
 * be disconnected and may have holes; ids beyond a frame's table and negative ids are not a cell.
 * mseg_cell_hull: bbox is the device array mseg_cell_measure writes ([n_labels][4] = r0, c0, r1, c1, zeros for absent cells);
 *   row_off: int64 [n_labels + 1] on the device: cell s owns the corner rows row_off[s] .. row_off[s + 1] - 1 of the
 *   workspace, r1 - r0 + 1 of them for a present cell and none for an absent one; n_rows = row_off[n_labels].
 *   out: int64 [10][n_labels], written whole, ten zeros for an absent id:
 *     0 perimeter   unit edges with a pixel of the cell on one side and a pixel that is not of the cell, or the outside of
 *                   the frame, on the other (the edges of holes count)
 *     1 hull_n      vertices of the convex hull of the cell's corners; strict: no three consecutive vertices are collinear
 *     2 hull_area2  twice the hull's area
 *     3 feret2      the largest squared distance between two corners
 *     4 .. 7        ay, ax, by, bx: the pair that attains it, a < b in (y, x) order; of ties the smallest a, then b
 *     8, 9          minw_num, minw_den2: the smallest caliper width is num / sqrt(den2).  Per hull edge e = (ey, ex) with
 *                   g = gcd(|ey|, |ex|): num = (largest |cross| of a corner against the edge's line) / g, den2 =
 *                   (ey^2 + ex^2) / g^2; the edge with the smallest num^2 / den2 wins (compared exactly, in 128 bits),
 *                   ties to the smaller den2
 *   status: int32 [1] on the device, written whole.  A pixel of a cell that lies outside the box given for that cell (or
 *   whose corner rows lie outside the cell's rows) is skipped and sets status[0] != 0: the outputs are then NOT valid; no
 *   write ever leaves the cell's own rows.  Integers only, int32 / 64-bit atomics: identical bytes from run to run.
 *   ws >= mseg_cell_hull_workspace_bytes (24 bytes per corner row; 0 = bad arguments).  MSEG_EINVAL: bad sizes, a dtype not
 *   listed, H * W >= 2^31 - 512; MSEG_EWORKSPACE: ws_bytes too small; nothing is launched on either.  n_labels == 0: status alone. */
size_t mseg_cell_hull_workspace_bytes(int64_t n_labels, int64_t n_rows);
int mseg_cell_hull(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                   const int32_t* bbox, const int64_t* row_off, int64_t n_rows, int64_t* out, int32_t* status, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- per-cell midline (csrc/midline.hip) — an extension --------------------------------------------------
 * labels, dtype and label_off as for mseg_cell_links.  A cell is the set of pixels of frame t whose id is l, 1 <= l <= K_t.
 * Ids beyond the frame's table and negative ids are not a cell, neither as a pixel nor as a neighbour; nor are the pixels of
 * other cells or anything outside the frame.  Every cell is thinned ALONE: two touching cells do not see each other.
 * Thinning: Guo & Hall 1989, algorithm A1, fully parallel, two sub-passes.  The neighbours of p = (y, x), clockwise from
 * north: P2 = (y-1, x), P3 = (y-1, x+1), P4 = (y, x+1), P5 = (y+1, x+1), P6 = (y+1, x), P7 = (y+1, x-1), P8 = (y, x-1),
 * P9 = (y-1, x-1); each is 1 if that pixel belongs to the cell in the current state, else 0.
 *   C  = (!P2 & (P3 | P4)) + (!P4 & (P5 | P6)) + (!P6 & (P7 | P8)) + (!P8 & (P9 | P2))
 *   N1 = (P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8),  N2 = (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9),  N = min(N1, N2)
 *   m0 = (P6 | P7 | !P9) & P8 for sub-pass 0,  m1 = (P2 | P3 | !P5) & P4 for sub-pass 1
 * Sub-pass k deletes every pixel of the cell with C == 1, 2 <= N <= 3 and m_k == 0; all decisions of a sub-pass are taken on
 * the state before it.  A round is sub-pass 0 followed by sub-pass 1; rounds repeat until a whole round deletes nothing.
 * mseg_cell_midline: bbox as for mseg_cell_hull ([n_labels][4] = r0, c0, r1, c1 with r1, c1 exclusive, zeros for absent
 *   cells).  Cell s owns a bitmap of (r1 - r0 + 2) rows of ceil((c1 - c0 + 2) / 64) 64-bit words (the box and a ring of one
 *   empty pixel) in each of the two buffers of the workspace; word_off: int64 [n_labels + 1] on the device, the cumulative sum
 *   of these word counts, none for an absent cell; n_words = word_off[n_labels].
 *   out: int64 [12][n_labels], written whole, twelve zeros for an absent id; S = the surviving pixels of the cell:
 *     0 skel_n     |S|
 *     1 n_orth     unordered pairs of S that are 4-neighbours
 *     2 n_diag     unordered pairs of S that are diagonal neighbours and whose two common 4-neighbours are both not in S
 *     3 n_end      pixels of S with exactly one 8-neighbour in S
 *     4 n_branch   pixels of S whose crossing number (0 -> 1 steps in P2, P3, ..., P9, P2, taken on S) is >= 3
 *     5 rounds     rounds run, the last, empty one included (a one-pixel cell: 1)
 *     6, 7, 8      e0_y, e0_x, e0_d2: the first end point in (y, x) order, and the squared distance from its centre to the
 *                  centre of the nearest position that is not of the cell; rows -1 and H and columns -1 and W count as such
 *     9, 10, 11    e1_y, e1_x, e1_d2: the last end point in (y, x) order, likewise
 *   skel_n == 1: that pixel is e0 and e1 (n_end stays 0); n_end == 1: e0 == e1; n_end == 0 and skel_n > 1: planes 6 .. 11 are 0.
 *   skeleton: uint8 [T][H][W] on the device or NULL; written whole: 1 on S of every cell, 0 elsewhere.
 *   status: int32 [1] on the device, written whole.  Bit 0: a pixel of a cell lies outside the box given for it (or the
 *   cell's box and words do not fit each other or the frame): it is skipped, and no write leaves the cell's own words.
 *   Bit 1: a cell was still changing after (r1 - r0) + (c1 - c0) + 2 rounds, the cap that bounds the loop; a correct build
 *   never reaches it.  With either bit set the outputs are NOT valid.  Integers only, order-free integer atomics: identical
 *   bytes from run to run.  ws >= mseg_cell_midline_workspace_bytes (16 bytes per word, each buffer rounded up to 256 bytes; 0 =
 *   bad arguments).  MSEG_EINVAL: bad sizes, a dtype not listed, H * W >= 2^31 - 512; MSEG_EWORKSPACE: ws_bytes too small;
 *   nothing is launched and nothing written on either.  n_labels == 0: status (and skeleton, if given) alone.            */
size_t mseg_cell_midline_workspace_bytes(int64_t n_labels, int64_t n_words);
int mseg_cell_midline(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                      const int32_t* bbox, const int64_t* word_off, int64_t n_words, int64_t* out, uint8_t* skeleton,
                      int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- per-cell order statistics (csrc/order_stats.hip) — an extension --------------------------------------
 * labels, label_dtype, label_off, img, img_dtype and the four element strides as for mseg_cell_measure: the image is uint8
 * or uint16 and is read in place, whatever its strides.  Ids beyond a frame's table and negative ids are neither cell nor
 * background.  bbox is the device array mseg_cell_measure writes ([n_labels][4] = r0, c0, r1, c1, half-open, zeros for an
 * absent cell).  1 <= R <= 16, 1 <= C.  ranks: int64 [R][n_labels] on the device, bg_ranks: int64 [R][T]; ranks count from 0.
 * mseg_cell_order_stats: outputs, written whole, integers only, identical bytes from run to run:
 *     values     uint32 [R][C][n_labels]  values[j][c][s] = the element of rank ranks[j][s] in the ascending multiset of the
 *                                         channel-c values of the pixels of cell s that lie inside its box
 *     bg_values  uint32 [R][T][C]         the same for the label-0 pixels of frame t and bg_ranks[j][t]
 *   An absent cell (an all-zero box) and a frame without background pixels get zeros; their ranks are not read as ranks.
 *   status: int32 [1] on the device, written whole.  With m = the number of the cell's pixels found inside its box (clipped
 *   to the frame), a rank outside 0 .. m - 1 writes 0 for that entry and sets status[0] != 0; the same holds for a frame's
 *   background count.  With the status word set the outputs are NOT valid.  This is how a box that does not cover its cell
 *   is caught.  No read or write ever leaves the arrays as sized here.
 *   Exact radix select: a 256-bin histogram of the high byte (uint8: of the value), a prefix over the bins, and for uint16
 *   a second walk for the low-byte histograms of the bins the ranks fell into.  Cells: one wave per cell slot, histograms
 *   in LDS, no workspace.  Background: whole-frame passes, histograms merged in the workspace with integer atomics.
 *   ws >= mseg_cell_order_stats_workspace_bytes (T * C * (256 + R * 256 + 4 R) words of 4 bytes, each of the three arrays
 *   rounded up to 256 bytes; nothing per cell; 0 = bad arguments).  MSEG_EINVAL: bad sizes, R or C out of range, a dtype not
 *   listed, H * W >= 2^31 - 512; MSEG_EWORKSPACE: ws_bytes too small; nothing is launched and nothing written on either.
 *   n_labels == 0: only the background is measured (bbox, ranks and values may be NULL).                                  */
size_t mseg_cell_order_stats_workspace_bytes(int T, int64_t n_labels, int C, int R);
int mseg_cell_order_stats(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                          const void* img, int img_dtype, int C, int64_t frame_stride, int64_t chan_stride,
                          int64_t row_stride, int64_t pix_stride, const int32_t* bbox, int R, const int64_t* ranks,
                          const int64_t* bg_ranks, uint32_t* values, uint32_t* bg_values, int32_t* status, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- per-cell intensity profile along the cell axis (csrc/profile.hip) — an extension ----------------------
 * labels, label_dtype, label_off, img, img_dtype, C and the four element strides as for mseg_cell_order_stats: the image is
 * uint8 or uint16 and is read in place, whatever its strides.  bbox is the device array mseg_cell_measure writes
 * ([n_labels][4] = r0, c0, r1, c1, half-open, zeros for an absent cell).  dir: int32 [n_labels][2] on the device = (uy, ux),
 * the cell's direction in (row, column); the caller makes it (floor(16384 cos o + 0.5), floor(16384 sin o + 0.5) for an
 * orientation o), the device never sees a float of it.  2 <= N <= 32, 1 <= C <= 8.  For cell s, over its pixels (y, x) inside
 * its box (clipped to the frame):
 *     q      = uy y + ux x                                   in int64
 *     qmin, qmax = the extremes of q
 *     b      = floor((q - qmin) N / (qmax - qmin + 1))       exact, then clamped to 0 .. N - 1 (exact arithmetic never leaves
 *                                                            that range; the clamp keeps any dir inside the arrays)
 * mseg_cell_profile: outputs, written whole, integers only, identical bytes from run to run:
 *     count   uint32 [N][n_labels]     count[b][s]   = the pixels of cell s in bin b
 *     sums    uint64 [C][N][n_labels]  sums[c][b][s] = the sum of their channel-c values (exact: < 2^31 * 65535)
 *     extent  int64  [2][n_labels]     qmin, qmax
 *   Bin 0 is the end with the smaller projection.  A one-pixel cell, and a cell whose pixels share one q, lie in bin 0.
 *   Pixels of other cells and background inside the box, ids beyond the frame's table and negative ids do not count.  An
 *   absent cell (an all-zero box), and a box that holds no pixel of its cell, get zeros everywhere.  b is exact while
 *   (qmax - qmin + 1) N < 2^63, which holds for every |uy|, |ux| <= 2^20 (H W < 2^31): an fp32 estimate of the quotient,
 *   corrected by the 64-bit remainder.
 *   There is no status word: a box that does not cover its cell shows as sum_b count[b][s] != the cell's area, which the
 *   caller checks.  No read or write ever leaves the arrays as sized here.
 *   One wave per cell slot, two walks over the box (the extremes by a wave reduction, then the bins in LDS), plain stores;
 *   no global atomics, no workspace.  MSEG_EINVAL: bad sizes, N or C out of range, a dtype not listed, H * W >= 2^31 - 512;
 *   nothing is launched and nothing written.  n_labels == 0: nothing to do (bbox, dir and the outputs may be NULL).        */
int mseg_cell_profile(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                      const void* img, int img_dtype, int C, int64_t frame_stride, int64_t chan_stride, int64_t row_stride,
                      int64_t pix_stride, const int32_t* bbox, const int32_t* dir, int N, uint32_t* count, uint64_t* sums,
                      int64_t* extent, void* stream);

/* ---- per-cell neighbourhood (csrc/neighbors.hip) — an extension ------------------------------------------
 * labels, dtype and label_off as for mseg_cell_links: cell l of frame t has slot label_off[t] + l - 1; ids beyond the frame's
 * table and negative ids are not a cell, neither as a pixel nor as a neighbour: they count as background.  H * W < 2^31 - 512.
 * radius = R, 1 <= R <= 32.  table_cap: entries of the pair table of every frame, a power of two, 64 <= table_cap <= 2^31.
 * All within one frame, for two different cells a < b:
 *   edges(a, b) = the unit pixel edges with a pixel of a on one side and a pixel of b on the other (4-neighbour pairs)
 *   d2(a, b)    = the smallest dy^2 + dx^2 over pixels p of a and q of b, (dy, dx) the difference of their coordinates
 *   the pair EXISTS when d2(a, b) <= R^2 (an edge-sharing pair has d2 = 1; one touching at a corner only has d2 = 2)
 * mseg_cell_neighbors: outputs, all integers, written whole by the call, identical values from run to run:
 *   out: int64 [9][n_labels], nine zeros for an absent id:
 *     0 contact_edges        the sum of edges(a, .) over all other cells
 *     1 border_edges         unit edges between a pixel of the cell and the outside of the frame
 *     2 free_edges           unit edges between a pixel of the cell and a pixel that is not of a cell
 *     3 n_touch              cells b with edges(a, b) > 0
 *     4 n_near               existing pairs the cell is in (n_touch <= n_near)
 *     5 nn_label             the other cell of the existing pair with the smallest d2, ties to the smallest label; 0: none
 *     6 nn_d2                that pair's d2; 0: none
 *     7 contact_label        the cell sharing the most edges, ties to the smallest label; 0: none shares an edge
 *     8 contact_label_edges  that pair's edges; 0: none
 *     planes 0 + 1 + 2 = plane 0 (perimeter) of mseg_cell_hull; the edges of holes count.
 *   pairs: int32 [pair_cap][5] = frame, a, b, edges, d2: one row per existing pair, a < b, in no particular order.
 *   n_pairs: int64 [1] on the device: the existing pairs of the whole stack, always the full count; beyond pair_cap rows
 *     nothing is written (which pairs are then written is unspecified).  pairs == NULL with pair_cap == 0 is legal.
 *   status: int32 [T] on the device; status[t] != 0: the pair table of frame t was full, frame t's slots of out and its pair
 *     rows are then NOT valid, n_pairs is a lower bound, and the frame has to be redone with a larger table.  A frame of K
 *     cells has at most K (K - 1) / 2 pairs.
 *   ws >= mseg_cell_neighbors_workspace_bytes (16 bytes per table entry and frame + 16 per cell, each of the five arrays
 *   rounded up to 256 bytes; 0 = bad arguments).  MSEG_EINVAL: bad sizes, R outside 1 .. 32, a dtype not listed, a table_cap
 *   that is not a power of two in range, H * W >= 2^31 - 512; MSEG_EWORKSPACE: ws_bytes too small; nothing is launched and no
 *   output is touched on either.  n_labels == 0: status and n_pairs = 0 alone.                                           */
size_t mseg_cell_neighbors_workspace_bytes(int T, int64_t n_labels, int64_t table_cap);
int mseg_cell_neighbors(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                        int radius, int64_t table_cap, int64_t* out, int32_t* pairs, int64_t pair_cap, int64_t* n_pairs,
                        int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- per-cell fluorescent foci (csrc/spots.hip) — an extension ---------------------------------------------
 * labels, label_dtype, label_off, img, img_dtype, C and the four element strides as for mseg_cell_order_stats: the image is
 * uint8 or uint16 and is read in place, whatever its strides.  For one channel plane v of one frame, scale = s in 1 .. 5 and
 * threshold = thr in 1 .. 65535 grey levels:
 *   B_k(v) = the separable smoothing with the binomial taps C(2k, j), j = 0 .. 2k, along rows, then along columns, in ONE
 *            pass of 2k + 1 taps over the plane extended by its edge values (coordinates clamped); not normalised
 *   D      = 16^s B_s(v) - B_2s(v): a difference of Gaussians (sigma = sqrt(s / 2) and sqrt(s)) in units of 16^(2s) per grey
 *            level, exact in int64 (every term < 65535 * 16^10 < 2^56)
 *   pixel p is a SPOT iff D(p) >= thr * 16^(2s) and, for each of its up to eight neighbours q inside the frame, D(p) > D(q),
 *            or D(p) == D(q) and p comes before q in raster order.  Two 8-adjacent pixels are never both spots: a frame has
 *            at most ceil(H / 2) * ceil(W / 2) spots per channel.
 *   A spot belongs to the label under p: 0 is background; an id beyond the frame's table or a negative id is neither.
 * mseg_cell_spots: outputs, all integers, written whole by the call, identical values from run to run:
 *   cell_count  int32 [C][n_labels]   spots of channel c on cell slot s
 *   bg_count    int32 [T][C]          spots of frame t and channel c on label 0
 *   spots       MsegSpot [spot_cap]   one record per spot (whatever its label), in no particular order, zeros behind the last
 *   n_spots     int64 [1] on the device: the spots of the whole call, always the full count; beyond spot_cap records nothing
 *               is written (which spots are then written is unspecified).  spots == NULL with spot_cap == 0 is legal.
 *   status      int32 [1] on the device; != 0: the list was too short (n_spots > spot_cap); the counts are valid all the same.
 *   One workgroup per 32 x 64 tile of one frame and channel; the tile and a ring of 2s + 1 pixels in LDS.
 *   ws >= mseg_cell_spots_workspace_bytes (256 bytes: the two tap rows; 0 = bad arguments).  MSEG_EINVAL: bad sizes, scale
 *   outside 1 .. 5, threshold outside 1 .. 65535, C < 1, a dtype not listed, a NULL pointer where one is needed, H * W >=
 *   2^31 - 512; MSEG_EWORKSPACE: ws_bytes too small; nothing is launched and nothing written on either.  n_labels == 0:
 *   cell_count may be NULL, every spot is background or neither.                                                          */
typedef struct MsegSpot {
  int32_t frame, channel, y, x, label, value; /* value: the pixel's own value */
  int64_t d;                                  /* D(p); the response in grey levels is d / 16^(2s) */
} MsegSpot;
size_t mseg_cell_spots_workspace_bytes(int T, int64_t n_labels, int C);
int mseg_cell_spots(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                    const void* img, int img_dtype, int C, int64_t frame_stride, int64_t chan_stride, int64_t row_stride,
                    int64_t pix_stride, int scale, int threshold, int32_t* cell_count, int32_t* bg_count, MsegSpot* spots,
                    int64_t spot_cap, int64_t* n_spots, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- training-set preparation (DataCropWorker src/utils/data_cropping.py:157-264,286,
 * DataImportWorker src/utils/data_import.py:125-194, DataExportWorker src/utils/data_export.py:100-101) -----------------
 * mseg_frame_stats: out[4] (device) = {min, max, sum v, sum v^2} of one uint8 / uint16 frame, exact, one pass (replaces
 *   np.min / np.max / np.mean / np.std of data_cropping.py:172 and data_import.py:129-130; the host derives mean and std
 *   from the integers).  npix < 2^31, so the sum of squares stays below 2^63.  64-bit integer atomics only.
 * mseg_crops_extract: K crops of S x S out of one frame [H][W] in one launch, crop k starting at row origin_yx[2k], column
 *   origin_yx[2k+1] (device); pixels beyond the frame take pad_value (the bottom / right padding of data_cropping.py:
 *   178-180).  With f = f32(v), every operation rounded to fp32 in the order written:
 *     crops_raw  [K][S][S] source dtype  v                                                    (data_cropping.py:261)
 *     crops_show [K][S][S] uint8         trunc(255 * (f - lo) / (hi - lo))                    (data_cropping.py:205-206)
 *     crops_u16  [K][S][S] uint16        trunc(clip(65535 * (f - lo) / (hi - lo), 0, 65535))  (data_export.py:100-101)
 *     x          [K][1][S][S] fp32       2 * (f - lo) / (hi - lo) - 1                         (data_cropping.py:286)
 *   Any output pointer may be NULL.  crops_show is meant for lo <= v <= hi (the frame's extrema).  hi <= lo: MSEG_EINVAL
 *   (the reference divides by zero on a constant frame).
 * mseg_crop_census: for the grid of ny x nx crops of S x S that starts at (y0, x0) inside a uint8 / uint16 label mask
 *   [H][W]: cells[i] = distinct non-zero ids of crop i = h * nx + w (len(get_nucleus_ids(mask_crop))), area[i] = its
 *   non-zero pixels (data_import.py:177-178); slot ny * nx holds both for the whole grid region (data_import.py:166; ids
 *   span crops, so it is not the sum).  A 64-Kbit presence bitmap per crop in LDS, one in the workspace for the region.
 * mseg_crops_overlay: rgb[K][S][S][3] = show replicated three times, outline pixels (255, 255, 0)
 *   (data_cropping.py:214-215,238-240).                                                                                   */
int mseg_frame_stats(const void* raw, int dtype, size_t npix, uint64_t* out, void* stream);
int mseg_crops_extract(const void* raw, int dtype, int H, int W, int K, const int32_t* origin_yx, int S, int pad_value,
                       int lo, int hi, void* crops_raw, uint8_t* crops_show, uint16_t* crops_u16, float* x, void* stream);
size_t mseg_crop_census_workspace_bytes(void);
int mseg_crop_census(const void* mask, int dtype, int H, int W, int y0, int x0, int ny, int nx, int S, int32_t* cells,
                     int64_t* area, void* ws, size_t ws_bytes, void* stream);
int mseg_crops_overlay(const uint8_t* show, const uint8_t* outlines, uint8_t* rgb, int K, int S, void* stream);

/* ---- device-resident training set (replaces the per-epoch file reads of src/training/training_dataset.py
 * :40-63 behind TrainWorker.resident) ----------------------------------------------------------------------------------
 * One batch out of a plane of a training set held in HBM.  src: [n][HW] elements of src_dtype (MSEG_PIX_*);
 * idx_dev: int32[N], 0 <= idx < n (validated by the caller on the host); dst: [N][HW] of the type dst_mode names.
 * Repeated indices and N > n are legal, N == 0 is a no-op.  Pairs (any other: MSEG_EINVAL, nothing is launched):
 *   MSEG_PIX_U16 -> MSEG_GATHER_RAW   uint16, the bits unchanged (DeviceAugment widens them: mseg_aug_u16_to_f32)
 *   MSEG_PIX_U16 -> MSEG_GATHER_NORM  fp32  2 * (f32(clip(v, lo, hi)) - lo) / (hi - lo) - 1, every operation rounded to
 *                                     fp32 in this order: the bits of utils.min_max_normalization; hi <= lo: MSEG_EINVAL
 *   MSEG_PIX_F32 -> MSEG_GATHER_RAW   fp32, the bits unchanged (distance labels)
 *   MSEG_PIX_U8  -> MSEG_GATHER_I64   int64 (boundary label for the loss)
 *   MSEG_PIX_U8  -> MSEG_GATHER_F32   fp32, exact (boundary label for DeviceAugment)
 * lo / hi are used by MSEG_GATHER_NORM only.  Crop offsets are 64-bit.  16-byte accesses for every crop whose source and
 * destination addresses allow them, element accesses for the others (odd HW).                                           */
#define MSEG_GATHER_RAW 0
#define MSEG_GATHER_F32 1
#define MSEG_GATHER_NORM 2
#define MSEG_GATHER_I64 3
int mseg_set_gather(const void* src, int src_dtype, long long n, long long HW, const int32_t* idx_dev, int N, void* dst,
                    int dst_mode, float lo, float hi, void* stream);

/* ---- test-time augmentation for inference (csrc/tta.hip) — an extension, the reference has none ---------
 * Transform codes are those of mseg_aug_flip, extended to rectangles; for a plane a of H x W:
 *   0 a, 1 fliplr, 2 flipud, 3 rot90, 4 rot180, 5 rot270, 6 rot90(fliplr(a)) = a.T, 7 rot90(flipud(a))   (numpy's names)
 * 3, 5, 6 and 7 transpose (their result is W x H); the inverse of 3 is 5 and of 5 is 3, every other code is its own.
 * mseg_tta_expand: src [n][H0][W0] uint8 (MSEG_PIX_U8) / uint16 (MSEG_PIX_U16) with minmax [n][2] from mseg_frames_minmax,
 *   or fp32 (MSEG_PIX_F32: already normalised, minmax ignored); codes: k <= 8 codes on the HOST, all transposing or all
 *   not (MSEG_EINVAL otherwise, nothing is launched).  out fp32 [k][n][Hm + pad_top][Wm + pad_left], Hm x Wm = H0 x W0
 *   or W0 x H0: member m of frame f is T_code[m](f), padded top / left with the value the host formula gives the pad
 *   value `min` (-1) and normalised with the frame's own extrema — every value is the bits mseg_frames_normalize gives
 *   for the transformed frame.  One launch whatever n and k; every element of out is written once.
 * mseg_tta_merge: dst(f, ch, y, x) = (((p_0 + p_1) + p_2) + ... + p_{k-1}) * (1 / k), fp32 in descriptor order, p_m =
 *   member m's prediction mapped back by the inverse of its code.  A descriptor's ptr is element (frame 0, channel 0,
 *   row 0, pixel 0) of the member's un-padded prediction, in the member's own orientation (W x H for a transposing
 *   code), and the strides are in elements; dst has its own four strides, so CHW planes and HWC-3 probabilities go
 *   through the same kernel.  k in {1, 2, 4, 8} (the scale is exact), n <= 65535.  No atomics, no workspace; every source
 *   element is read once, every destination element stored once.  Offsets are 64-bit.                                  */
typedef struct MsegTtaMember {
  const float* ptr;
  int64_t frame_stride, chan_stride, row_stride, pix_stride;
  int32_t code;
  int32_t reserved;
} MsegTtaMember;
int mseg_tta_expand(const void* src, int dtype, int n, int H0, int W0, const uint32_t* minmax, const int32_t* codes, int k,
                    int pad_top, int pad_left, float* out, void* stream);
int mseg_tta_merge(const MsegTtaMember* members, int k, int n, int C, int H, int W, float* dst, long long dst_frame_stride,
                   long long dst_chan_stride, long long dst_row_stride, long long dst_pix_stride, void* stream);

/* ---- inference at a chosen resolution (csrc/resample.hip) — an extension ---------------------------------
 * Separable, anti-aliased linear resampling with pixel-centre alignment.  The rule is a table per axis, made on the HOST
 * (inference/resample.py axis_table): output index i takes count[i] <= taps source elements from first[i] on, with the
 * fp32 weights weight[i][0 .. taps) (zero beyond count[i]).  MsegResampleAxis carries the table on the device (first,
 * count, weight) and the same first / count on the host: the call validates the host copy (1 <= taps <= 12, n_out > 0,
 * 1 <= count <= taps, every window inside [0, n_in), first and first + count not decreasing) and sizes its tiles from it;
 * anything else is MSEG_EINVAL and nothing is launched.  The kernels compute no weights.  A value is
 * sum_y w_y (sum_x w_x v): fp32 fmaf from 0 in ascending tap order, x before y; it does not depend on the tile, the launch
 * or the other frames of the launch.  One launch whatever n; every destination element is stored once; no atomics, no
 * workspace; offsets are 64-bit; n <= 65535.
 * mseg_resample_frames: src [n][yaxis.n_in][xaxis.n_in] uint8 (MSEG_PIX_U8) / uint16 (MSEG_PIX_U16) with minmax [n][2] from
 *   mseg_frames_minmax, or fp32 (MSEG_PIX_F32: already normalised, minmax ignored).  A raw pixel enters the filter as the
 *   value mseg_frames_normalize gives it.  out fp32 [n][yaxis.n_out + pad_top][xaxis.n_out + pad_left]; the top / left
 *   padding is -1, the normalised frame minimum.
 * mseg_resample_planes: src is element (frame 0, channel 0, row 0, pixel 0) of the un-padded source, yaxis.n_in x xaxis.n_in
 *   per frame and channel, with four strides in elements; dst is yaxis.n_out x xaxis.n_out with its own four strides, so
 *   CHW planes and HWC-3 probabilities go through the same kernel.                                                        */
typedef struct MsegResampleAxis {
  const int32_t* first;        /* device [n_out] */
  const int32_t* count;        /* device [n_out] */
  const float* weight;         /* device [n_out][taps] */
  const int32_t* host_first;   /* host copy of first */
  const int32_t* host_count;   /* host copy of count */
  int32_t n_in, n_out, taps;
  int32_t reserved;
} MsegResampleAxis;
int mseg_resample_frames(const void* src, int dtype, int n, const uint32_t* minmax, const MsegResampleAxis* yaxis,
                         const MsegResampleAxis* xaxis, int pad_top, int pad_left, float* out, void* stream);
int mseg_resample_planes(const float* src, long long src_frame_stride, long long src_chan_stride, long long src_row_stride,
                         long long src_pix_stride, int n, int C, const MsegResampleAxis* yaxis,
                         const MsegResampleAxis* xaxis, float* dst, long long dst_frame_stride, long long dst_chan_stride,
                         long long dst_row_stride, long long dst_pix_stride, void* stream);

/* ---- misc ---------------------------------------------------------------------------------------------------- */
int mseg_version(void);
const char* mseg_strerror(int code);
int mseg_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MSEG_HIP_H */
