/* libfacevae — MI355X (gfx950) C-ABI for the FaceVAE training step.
 *
 * Plain C ABI: raw device pointers, sizes, a dtype enum and an explicit hipStream_t
 * (passed as void*).  No torch types.  Every entry returns an int status (FV_OK = 0;
 * >0 = FV_E_* or a hipError_t); the message of the last failure on the calling thread is
 * available from fv_last_error().  Nothing aborts, nothing allocates device memory on
 * the hot path: callers size workspaces with the *_ws_bytes / *_elems helpers.
 *
 * Activations are NHWC ("channels_last") with a channel stride `ld*` ≥ valid channels.
 * Conv weights are handed over in the reference parameter layout
 * (nn.Conv2d.weight [Cout][Cin][k][k], fp32) and re-laid out per forward by
 * fv_conv_weight_prep into the kernel layout [rows][Kpad] with k = (r*k + s)*cin + ci.
 *
 * Which reference interface each entry replaces (file:line in Luh1124/face-vae):
 *   fv_conv2d_fwd            F.conv2d inside _ConvBlock / nn.Conv2d (modules.py:32-42,
 *                            models.py:934,1096,1099) incl. nn.Upsample (modules.py:81)
 *                            folded into addressing, BN-apply+act prologue (NAC,
 *                            modules.py:13,31-39), bias/residual (modules.py:125)/sigmoid
 *                            (models.py:1110) epilogue and BN statistics partials.
 *   fv_conv2d_bwd_data       conv backward-data == transposed conv (ConvTranspose2dELR's
 *                            F.conv_transpose2d, models_utils.py:498-499, stride 1 case).
 *   fv_conv2d_bwd_weight     conv weight/bias gradient (autograd of modules.py:32).
 *   fv_spectral_norm_*       torch.nn.utils.spectral_norm as used by modules.py:14,32.
 *   fv_bn_*                  nn.SyncBatchNorm train/eval (modules.py:19; logger.py:55).
 *   fv_reparam_*             flatten_vae_nl split + reparameterisation (models.py:559-561).
 *   fv_kl_*                  KLDivergenceLoss (losses.py:385-393).
 *   fv_mse_*                 ReconLoss / nn.MSELoss (losses.py:396-403).
 *   fv_l1_*                  PerceptualLoss pixel term nn.L1Loss (losses.py:128,135).
 *   fv_conv3d_*             nn.Conv3d of ResBlock3D (modules.py:52-56,133-135; AFE models.py:935).
 *   fv_conv3dg_*            nn.Conv3d of DownBlock3D / UpBlock3D (modules.py:59-94) and of the MFE's
 *                           compress / mask_conv (models.py:1054, 1057): general-channel implicit GEMM.
 *   fv_grid_sample3d_*, fv_occlusion_*, fv_sparse_motion_*, fv_heatmap_*, fv_motion_mask_*
 *                            warp path: models.py:1076-1078,1103,1106; utils.py:123-179.
 *   fv_stem7s2_*, fv_maxpool3s2_*   HPE_EDE.pre_layers (models.py:1003): the 7x7 stride-2 stem conv and
 *                            nn.MaxPool2d(3, 2, 1).
 *   fv_subsample2_*, fv_bn2_add_relu_fwd   ResBottleneck (modules.py:138-152): the stride of its
 *                            stride-2 1x1 convs and relu(down_sample(x) + layers(x)).
 *   fv_pose_pool_fwd, fv_pose_head_*   torch.mean, fc_*, softmax expectation (models.py:1025-1036).
 *   fv_ckd_resize_fwd, fv_ckd_softargmax_*   CKD's F.interpolate (models.py:978) and
 *                            heatmap2kp(out2heatmap(.)) (utils.py:106-118).
 *   fv_efe_kpcat_*           EFE_conv5's torch.cat((x, kp2gaussian_3d(kpc)), 1) (models.py:790-791).
 *   fv_tps_warp_*            Transform.transform_frame / warp_coordinates (trainer.py:106-129): the random
 *                            affine + thin-plate-spline warp of the equivariance term.
 *   fv_hopenet_prep_fwd, fv_pw_infer_*   the frozen Hopenet teacher (trainer.py:16-88, 278-280): ImageNet
 *                            normalisation + nearest resize, and its 1x1 convs with the batch norm folded in.
 *   fv_mfe_input_fwd, fv_motion_warp_fwd, fv_frames_u8   the inference data flow of evaluate.py: the
 *                            MFE's hourglass input, mask blend + warp, and the uint8 frame output.
 *   fv_frames_from_u8, fv_pose_kp_fwd, fv_pose_kp_new_fwd   the uint8 way in (img_as_float32) and
 *                            transform_kp / transform_kp_with_new_pose (utils.py:53-76) with Rs inv(Rd).
 *   fv_adam_step             torch.optim.Adam(lr, betas=(0.5,0.999)) (logger.py:60-61).
 *   fv_comm_*                distributed.py:24-31 init_process_group("nccl") + DDP's
 *                            gradient all-reduce (logger.py:55,58) + SyncBN collectives.
 */
#ifndef FACEVAE_H
#define FACEVAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FV_ABI_VERSION 2

enum fv_status {
  FV_OK = 0,
  FV_E_BADARG = 1001,
  FV_E_UNSUPPORTED = 1002,
  FV_E_COMM = 1003
};

enum fv_dtype { FV_F32 = 0, FV_BF16 = 1, FV_F64 = 2 };

int fv_abi_version(void);
const char* fv_last_error(void);

/* ---------------------------------------------------------------- convolution ---- */
typedef struct fv_conv_desc {
  int dtype;         /* FV_F32 (exact fp32 MFMA) or FV_BF16 (bf16 MFMA, fp32 accumulate) */
  int n, h, w;       /* output spatial size (== conv input size unless upsample) */
  int cin;           /* channel stride of x: power of two >= 8 (zero padded channels) */
  int cin_valid;     /* real input channels (<= cin) */
  int cout;          /* valid output channels */
  int ldy;           /* channel stride of y and res (>= cout; ignored for out_nchw_f32) */
  int ksize;         /* 1, 3 or 7; stride 1, padding ksize/2 */
  int upsample;      /* 1: x is (h/2, w/2), nearest x2 upsample folded into addressing */
  int pro_act;       /* 1: conv input is act(x*scale[c]+shift[c]) (BN-apply + act) */
  float pro_slope;   /* act slope for negatives: 0 = ReLU, 0.2 = LeakyReLU */
  int epi_sigmoid;   /* 1: y = sigmoid(conv + bias [+ res]) */
  int out_nchw_f32;  /* 1: store y as NCHW fp32 [n][cout][h][w] */
} fv_conv_desc;

/* elements of the kernel-layout weight buffers (wk for fwd, wt for bwd-data) */
size_t fv_conv_wk_elems(const fv_conv_desc* d);
size_t fv_conv_wt_elems(const fv_conv_desc* d);
/* number of BN partial records written by fv_conv2d_fwd (stats: [records][2][cout], each
 * (sum, sum of squares) over `block_pixels` consecutive output pixels, the last one short) */
int fv_conv2d_stats_blocks(const fv_conv_desc* d);
int fv_conv2d_stats_block_pixels(const fv_conv_desc* d);

/* w_param [cout][cin_valid][k][k] fp32 -> wk [rows][Kpad], wt [rows_t][Kpad_t] (either may be
 * NULL), both scaled by 1/sigma[0] when sigma != NULL (spectral norm), dtype d->dtype. */
int fv_conv_weight_prep(const fv_conv_desc* d, const float* w_param, const float* sigma,
                        void* wk, void* wt, void* stream);
/* The same for n convs in ONE launch (the generic layouts only: fv_conv_weight_prep_batchable(d)
 * != 0; all descriptors of one dtype, n <= FV_WPREP_MAX): descs is an array of n descriptors,
 * w_params / sigmas / wks / wts arrays of n pointers (sigma, wt entries may be NULL). */
#define FV_WPREP_MAX 24
int fv_conv_weight_prep_batchable(const fv_conv_desc* d);
int fv_conv_weight_prep_multi(int n, const fv_conv_desc* descs, const float* const* w_params,
                              const float* const* sigmas, void* const* wks, void* const* wts, void* stream);

/* y = epi(conv(pro(x), wk) + bias [+ res]); stats (optional) receives per-record
 * (sum, sum of squares) of the pre-sigmoid output per channel. */
int fv_conv2d_fwd(const fv_conv_desc* d, const void* x, const void* wk, const float* bias,
                  const float* pro_scale, const float* pro_shift, const void* res, void* y,
                  float* stats, void* stream);

/* dx[n][h'][w'][cin] = conv_transpose(dy, w) at the conv INPUT resolution of `d` with
 * upsample == 0 (dgrad at the upsampled resolution when d->upsample; see
 * fv_upsample2x_bwd).  dy has channel stride ldy_dy (>= cout, multiple of 8). */
int fv_conv2d_bwd_data(const fv_conv_desc* d, const void* dy, int ldy_dy, const void* wt,
                       void* dx, void* stream);
/* 1 when, for this upsample descriptor, fv_conv2d_bwd_data writes dx directly at the LOW
 * (conv input, h/2 x w/2) resolution -- the gradient of the upsample's input, computed as a
 * stride-2 4x4 conv over dy -- and wt (fv_conv_wt_elems / fv_conv_weight_prep) holds those
 * 4x4 weights; then no fv_upsample2x_bwd follows.  0 otherwise. */
int fv_conv2d_dgrad_lowres(const fv_conv_desc* d);

/* The kernel family fv_conv2d_fwd (dgrad == 0) or fv_conv2d_bwd_data (dgrad != 0) dispatches `d` to,
 * for a call with / without a residual, BN statistics and store-pass records (sr_mode 0 / 1 / 2):
 * a pure host query for tests and tools, -1 for a descriptor the entries reject.  A data gradient
 * reports the kind its transposed forward descriptor runs, or one of the two low-res kinds. */
typedef enum fv_conv_kernel {
  FV_CONVK_V1 = 0,             /* conv_fwd_kernel (register-staged; fp32, BN prologue, odd shapes) */
  FV_CONVK_V2,                 /* conv_fwd_v2 (bf16, DMA-fed) */
  FV_CONVK_C1S,                /* conv1x1_stream */
  FV_CONVK_HALO3_FWD3,         /* conv3_halo_fwd3 (3x3, linear halo, pairs of taps) */
  FV_CONVK_HALO3_FWD2,         /* conv3_halo_fwd2 (3x3, swizzled halo) */
  FV_CONVK_SUBPIX_V2,          /* upsample + 3x3 as 4 sub-pixel phases on conv_fwd_v2 */
  FV_CONVK_SUBPIX_HALO,        /* ... on conv3_halo_fwd3 */
  FV_CONVK_UPBAND,             /* ... on conv3up_band_fwd */
  FV_CONVK_HALO7,              /* conv_halo_fwd (7x7) */
  FV_CONVK_C74,                /* conv7c4_fwd (7x7, <= 4 real input channels, packed weights) */
  FV_CONVK_C64,                /* conv3c64_fwd (3x3, 64 input channels, sliding band) */
  FV_CONVK_C7N,                /* conv7_n3_fwd2 (7x7, 64 -> <= 4 channels, NCHW fp32) */
  FV_CONVK_DGRAD_LOWRES_HALO,  /* data gradient of upsample + 3x3 at the low resolution, conv3_halo_fwd3 */
  FV_CONVK_DGRAD_LOWRES_V2     /* ... on conv_fwd_v2 */
} fv_conv_kernel;
int fv_conv2d_fwd_kernel(const fv_conv_desc* d, int dgrad, int has_res, int has_stats, int sr_mode);

/* weight gradient w.r.t. the effective (post-SN) weight, split over pixels:
 * slab [nsplit][rows][Kpad] fp32 and bias slab [nsplit][rows] fp32 (sizes from the queries). */
int fv_conv2d_wgrad_nsplit(const fv_conv_desc* d);
size_t fv_conv2d_wgrad_slab_elems(const fv_conv_desc* d);
size_t fv_conv2d_wgrad_bias_slab_elems(const fv_conv_desc* d);
int fv_conv2d_bwd_weight(const fv_conv_desc* d, const void* x, const float* pro_scale,
                         const float* pro_shift, const void* dy, int ldy_dy, float* slab,
                         float* bias_slab, void* stream);
/* reduce the slabs into dw_param [cout][cin_valid][k][k] (fp32, reference layout) and
 * db [cout] (db may be NULL).  The slab contents are scratch afterwards: the reduce may use
 * them for its partial sums. */
int fv_conv2d_wgrad_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab,
                           float* dw_param, float* db, void* stream);

/* ---- stride-2 3x3 convolution, padding 1 (the patch discriminator's down blocks) ----
 * The entries take a fv_conv_desc with ksize == 3, upsample == 0, pro_act == 0, no sigmoid and
 * NHWC output (anything else: FV_E_UNSUPPORTED), dtype FV_F32 or FV_BF16.  (h, w) is the OUTPUT
 * size; the input is (in_h, in_w) = (2h, 2w), NHWC with channel stride cin -- an odd input size,
 * or any other in_h / in_w, returns FV_E_UNSUPPORTED.
 * Weights: wk [rows][Kpad] is the generic forward image (it does not depend on the stride);
 * wt holds the data gradient's four phase images (input-pixel parities (row, column): 1, 2, 2
 * or 4 live taps of the 9), so that the transposed conv multiplies no zero taps.  Both are
 * scaled by 1/sigma[0] when sigma != NULL; either of wk / wt may be NULL. */
size_t fv_conv2d_s2_wk_elems(const fv_conv_desc* d);
size_t fv_conv2d_s2_wt_elems(const fv_conv_desc* d);
int fv_conv2d_s2_weight_prep(const fv_conv_desc* d, const float* w_param, const float* sigma, void* wk, void* wt,
                             void* stream);
/* y[n][h][w][ldy] = conv(x, wk, stride 2, padding 1) + bias (bias may be NULL) */
int fv_conv2d_s2_fwd(const fv_conv_desc* d, int in_h, int in_w, const void* x, const void* wk, const float* bias,
                     void* y, void* stream);
/* dx[n][2h][2w][cin] (every padded channel written, the padded ones 0); dy has channel stride
 * ldy_dy == cout padded to a power of two >= 8, its padding channels finite. */
int fv_conv2d_s2_bwd_data(const fv_conv_desc* d, int in_h, int in_w, const void* dy, int ldy_dy, const void* wt,
                          void* dx, void* stream);
/* weight gradient: per-split fp32 slabs, then the reduce into dw_param [cout][cin_valid][3][3]
 * and db [cout] (bias_slab / db may be NULL); dy channel stride a multiple of 8 >= cout. */
size_t fv_conv2d_s2_wgrad_slab_elems(const fv_conv_desc* d);
size_t fv_conv2d_s2_wgrad_bias_slab_elems(const fv_conv_desc* d);
int fv_conv2d_s2_bwd_weight(const fv_conv_desc* d, int in_h, int in_w, const void* x, const void* dy, int ldy_dy,
                            float* slab, float* bias_slab, void* stream);
int fv_conv2d_s2_wgrad_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab, float* dw_param,
                              float* db, void* stream);

/* store-pass reductions of the halo-staged 3x3 kernels (fused into the bf16 store of the
 * output tile; one record per 256-pixel tile and wave, [records][2][cout] fp32):
 *   mode 1 (fv_conv2d_fwd_sr): (sum, sum of squares) of the stored output AFTER the residual
 *          add -- the statistics of the next BatchNorm (ResBlock2D's x + t feeding the next
 *          block's NAC, modules.py:125 -> 13);
 *   mode 2 (fv_conv2d_bwd_data_sr): the SyncBatchNorm backward sums (sum g, sum g * yhat) of
 *          the BN whose output gradient the data gradient produces: g = dx * act'(gamma * yhat
 *          + beta), yhat = (bn_input - mean) * invstd (replaces fv_bn_act_bwd_reduce's pass).
 * fv_conv2d_sr_records (dgrad = 1 for the data gradient of d) gives the record count, 0 when
 * the launch path of d has no store-pass records (then use the separate passes). */
typedef struct fv_store_reduce {
  int mode;                /* 1 or 2 */
  float* records;          /* [records][2][cout] */
  const void* bn_input;    /* mode 2: the BN input y, NHWC like the output */
  const float *mean, *invstd, *gamma, *beta;
  float slope;             /* act slope (0 ReLU, 0.2 LeakyReLU) */
} fv_store_reduce;
int fv_conv2d_sr_records(const fv_conv_desc* d, int dgrad, int* record_pixels);
int fv_conv2d_fwd_sr(const fv_conv_desc* d, const void* x, const void* wk, const float* bias, const void* res, void* y,
                     const fv_store_reduce* sr, void* stream);
int fv_conv2d_bwd_data_sr(const fv_conv_desc* d, const void* dy, int ldy_dy, const void* wt, void* dx,
                          const fv_store_reduce* sr, void* stream);
/* BN backward from store-pass records: dgamma / dbeta (either may be NULL) and k [2][c] over
 * `count` elements (fv_bn_bwd_finalize's outputs); red (optional, [2][c] doubles) receives the
 * rank-local sums for a SyncBN all-reduce, then k comes from fv_bn_bwd_finalize_dev. */
int fv_bn_bwd_from_records(const float* records, int nrec, int record_pixels, long pixels, int c, long count,
                           float* dgamma, float* dbeta, float* k, double* red, void* ws, void* stream);

/* ------------------------------------------- transposed conv (k4, s2, p1) ---- */
/* ConvTranspose2dELR (models_utils.py:404-516; F.conv_transpose2d at :497-498) with
 * kernel 4, stride 2, padding 1, run as the sub-pixel phases of an upsample descriptor:
 * d->upsample = 1, d->ksize = 3, d->h/w = OUTPUT size, cin/cout = the module's inch/outch.
 * Forward = fv_conv2d_fwd(d, x, wk, bias, ...); data gradient = fv_conv2d_bwd_data(d, dy,
 * ldy, wt, dx) (dx at the input resolution); weight gradient = fv_conv2d_bwd_weight(d, ...)
 * then fv_convt_wgrad_reduce.  w is the module parameter [cin][cout][4][4] fp32; the
 * effective weight is gain * w, normalised per output channel over dims [0,2,3]
 * (F.normalize, eps 1e-12: models_utils.py:461-470) when demod; inv [cout] receives
 * 1/max(norm, eps) and is read back by the weight-gradient reduce.  bf16 only. */
int fv_convt_supported(const fv_conv_desc* d);
int fv_convt_weight_prep(const fv_conv_desc* d, const float* w, int demod, float gain, float* inv,
                         void* wk, void* wt, void* stream);
/* slabs of fv_conv2d_bwd_weight(d, ...) -> dw [cin][cout][4][4] = dL/dw (through gain and
 * demod) and db [cout] (may be NULL). */
int fv_convt_wgrad_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab,
                          const float* w, int demod, float gain, const float* inv, float* dw,
                          float* db, void* stream);

/* any geometry / fp32 (convt.hip, direct kernels; NHWC, x channel stride ldx, out stride ldy):
 * W_eff = gain * W [/ max(||W[:, o, :, :]||, 1e-12) when demod] -> we [cin][cout][k][k] fp32
 * (inv [cout] receives the inverse norms); out = conv_transpose2d(x, W_eff, stride, pad) + bias;
 * the data gradient; g = dL/dW_eff (+ db); fv_convt_weight_grad turns g into dL/dW in place. */
int fv_convt_eff_weight(const float* w, int cin, int cout, int k, int demod, float gain, float* inv, float* we,
                        void* stream);
int fv_convt_weight_grad(const float* w, int cin, int cout, int k, int demod, float gain, const float* inv, float* g,
                         void* stream);
int fv_convt_direct_fwd(int dtype, const void* x, int n, int hi, int wi, int cin, int ldx, const float* we,
                        const float* bias, int cout, int ldy, int k, int stride, int pad, void* y, void* stream);
int fv_convt_direct_dgrad(int dtype, const void* dy, int n, int hi, int wi, int cin, int ldx, const float* we,
                          int cout, int ldy, int k, int stride, int pad, void* dx, void* stream);
int fv_convt_direct_wgrad(int dtype, const void* x, const void* dy, int n, int hi, int wi, int cin, int ldx, int cout,
                          int ldy, int k, int stride, int pad, float* g, float* db, void* stream);
/* per-sample channel affine y[n][p][c] = x[n][p][c] * sa[n][c] (+ sb[n][c]) (the weight
 * modulation x * (affine(w) * 0.1 + 1) and the per-sample demodulation of
 * models_utils.py:486-495, moved onto the activations) and its backward (dx may be NULL) */
int fv_chan_scale_fwd(int dtype, const void* x, int n, long hw, int c, int ld, const float* sa, const float* sb,
                      void* y, void* stream);
int fv_chan_scale_bwd(int dtype, const void* g, const void* x, int n, long hw, int c, int ld, const float* sa, void* dx,
                      float* da, float* db, void* stream);

/* ------------------------------------------------- fp8 conv path (config C5) ---- */
/* OCP e4m3 operands with per-tensor power-of-two scales: a tensor v is stored as
 * fp8(v * s), s = 2^floor(log2(448 / amax|v|)), with dq = 1 / s (a device float) beside it.
 * fv_conv2d_fwd_fp8 / fv_conv2d_bwd_data_fp8 are the forward and data gradient of a 3x3 conv
 * (fv_conv2d_fp8_supported: channel counts multiples of 128, w % 64 == 0, h % 4 == 0) on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with fp32 accumulation, the epilogue multiplying by
 * dq_x * dq_w; output bf16 NHWC as fv_conv2d_fwd (bias, residual, BN partials alike).  They
 * replace the same F.conv2d calls as fv_conv2d_fwd / fv_conv2d_bwd_data (modules.py:32). */
size_t fv_fp8_ws_bytes(void);
/* y[i] = fp8(x[i] * s) for count elements (bf16 or f32 input), dq[0] = 1 / s */
int fv_quantize_fp8(int dtype_in, const void* x, long count, uint8_t* y, float* dq, void* ws,
                    void* stream);
int fv_conv2d_fp8_supported(const fv_conv_desc* d);
size_t fv_conv_fp8_wk_bytes(const fv_conv_desc* d);
size_t fv_conv_fp8_wt_bytes(const fv_conv_desc* d);
/* w_param [cout][cin][3][3] fp32 (/ sigma when given) -> wk [cout][9 cin] and/or the
 * transposed, flipped wt [cin][9 cout] (k = tap * channels + c), one scale: dq[0] */
int fv_conv_weight_prep_fp8(const fv_conv_desc* d, const float* w_param, const float* sigma,
                            uint8_t* wk, uint8_t* wt, float* dq, void* ws, void* stream);
/* fv_conv_weight_prep_fp8 for n <= FV_WPREP_MAX convs in two launches (the per-step weight
 * quantization of an fp8 model): arrays of n descriptors / pointers as fv_conv_weight_prep_multi
 * (wts[i] may be NULL), dqs[i] one float each; ws = n * fv_fp8_ws_bytes() bytes.  Bit-identical
 * to n fv_conv_weight_prep_fp8 calls. */
int fv_conv_weight_prep_fp8_multi(int n, const fv_conv_desc* descs, const float* const* w_params,
                                  const float* const* sigmas, uint8_t* const* wks, uint8_t* const* wts,
                                  float* const* dqs, void* ws, void* stream);
int fv_conv2d_fwd_fp8(const fv_conv_desc* d, const uint8_t* x8, const float* x_dq, const uint8_t* wk,
                      const float* w_dq, const float* bias, const void* res, void* y, float* stats,
                      void* stream);
/* BN partial records written by fv_conv2d_fwd_fp8 (as fv_conv2d_stats_blocks / _pixels) */
int fv_conv2d_fp8_stats_blocks(const fv_conv_desc* d);
int fv_conv2d_fp8_stats_block_pixels(const fv_conv_desc* d);
/* dx [n][h][w][cin] bf16 from dy8 [n][h][w][cout] fp8 and wt */
int fv_conv2d_bwd_data_fp8(const fv_conv_desc* d, const uint8_t* dy8, const float* dy_dq,
                           const uint8_t* wt, const float* wt_dq, void* dx, void* stream);
/* Delayed scaling (the product path): a "site" (fv_fp8_site_bytes, zero-initialised device
 * memory, one per conv operand: activation or output gradient) keeps a 16-deep amax history.
 * fv_quantize_fp8_site quantizes in ONE pass with s from max(history) (saturating at +-448)
 * and records the call's amax; seeded = 0 (the site's first call) quantizes exactly
 * (amax pass + quantize pass) and fills the history.  The *_site convs read dq from the site
 * and move the recorded amax into the history (so a site's calls must alternate quantize ->
 * conv, in stream order).  Replaces the per-call amax pass of fv_quantize_fp8. */
size_t fv_fp8_site_bytes(void);
int fv_quantize_fp8_site(int dtype_in, const void* x, long count, uint8_t* y, void* site, int seeded,
                         void* ws, void* stream);
int fv_conv2d_fwd_fp8_site(const fv_conv_desc* d, const uint8_t* x8, void* site, const uint8_t* wk,
                           const float* w_dq, const float* bias, const void* res, void* y, float* stats,
                           void* stream);
/* fv_conv2d_fwd_fp8_site + the store-pass reduction of fv_conv2d_fwd_sr (mode 1 only: the
 * (sum, sum of squares) of the stored, residual-added output, in the records
 * fv_conv2d_sr_records(d, 0, ...) sizes) */
int fv_conv2d_fwd_fp8_site_sr(const fv_conv_desc* d, const uint8_t* x8, void* site, const uint8_t* wk,
                              const float* w_dq, const float* bias, const void* res, void* y,
                              const fv_store_reduce* sr, void* stream);
int fv_conv2d_bwd_data_fp8_site(const fv_conv_desc* d, const uint8_t* dy8, void* site, const uint8_t* wt,
                                const float* wt_dq, void* dx, void* stream);
/* Data-parallel global scaling (BASELINE config C5 at N > 1; the fp8 counterpart of SyncBN's
 * global statistics, modules.py:120-121 under logger.py:54-58): with the deferred roll on, the
 * *_site convs leave each call's amax in its site; once per step the caller gathers every
 * site's in-flight amax (fv_fp8_sites_inflight, `sites` = device array of site pointers),
 * all-reduces it with MAX (fv_comm_allreduce op 2) and rolls all sites at once
 * (fv_fp8_sites_roll), so every rank quantizes with the same scales.  A site's first call
 * takes the exact amax (fv_fp8_amax), all-reduced, as its seed (fv_fp8_site_seed) and then
 * quantizes as a seeded site.  Process-wide switch. */
int fv_fp8_set_deferred_roll(int on);
int fv_fp8_amax(int dtype_in, const void* x, long count, float* amax, void* ws, void* stream);
int fv_fp8_site_seed(void* site, const float* amax, void* stream);
int fv_fp8_sites_inflight(int n, const uint64_t* sites, float* amax, void* stream);
int fv_fp8_sites_roll(int n, const uint64_t* sites, const float* amax, void* stream);
/* fp8 weight gradient of a 3x3 conv (k = (tap, ci), pixel-pair MFMA K = 128) from the e4m3 copies
 * of its input (x8, dequantisation factor x_dq) and output gradient (dy8, dy_dq) -- the operands
 * the fp8 forward and data gradient consumed: slab / bias slab sized by fv_conv2d_wgrad_slab_elems,
 * reduced by fv_conv2d_wgrad_fp8_reduce.  Supported when
 * fv_conv2d_wgrad_fp8_supported(d) (128-multiple channels, the sliding-row plan). */
int fv_conv2d_wgrad_fp8_supported(const fv_conv_desc* d);
int fv_conv2d_bwd_weight_fp8(const fv_conv_desc* d, const uint8_t* x8, const float* x_dq, const uint8_t* dy8,
                             const float* dy_dq, float* slab, float* bias_slab, void* stream);
/* reduce of fv_conv2d_bwd_weight_fp8's slabs -> dw (param layout) [+ db]: the fp8 weight
 * gradient splits a batch over fewer slabs than the bf16 plan (images per split chosen for
 * about 512 blocks), so its slabs are summed by this entry, not fv_conv2d_wgrad_reduce */
int fv_conv2d_wgrad_fp8_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab, float* dw_param,
                               float* db, void* stream);
/* layout probe: c[16][16] = a[16][128] . b[16][128]^T through one scaled fp8 MFMA tile */
int fv_fp8_mfma_probe(const uint8_t* a, const uint8_t* b, float* c, void* stream);
/* test probe: 64 lanes each read 8 bytes by ds_read_b64_tr_b8 at LDS byte offset lane_addr[lane]
 * (< 4088, 8-aligned) of a 4 KB LDS image holding byte i = i & 255; out [64][2] ints */
int fv_tr8_probe(const int* lane_addr, int* out, void* stream);

/* ------------------------------------------------ 3x3x3 conv (AFE ResBlock3D) ---- */
/* nn.Conv3d(cin, cout, 3, 1, 1) of ConvBlock3D / ResBlock3D (modules.py:52-56, 133-135) in the
 * AFE trunk (models.py:935, 943-944).  Activations NDHWC ([n][d][h][w][c], torch
 * channels_last_3d), weights in the reference layout [cout][cin][3][3][3] fp32, re-laid out
 * per forward by fv_conv3d_weight_prep (wk: forward, wt: data gradient; fv_conv3d_wk_bytes
 * each).  bf16 with cin = cout = 32 and w = 64 runs the MFMA kernels (BN partials available:
 * fv_conv3d_stats_blocks > 0); any other shape, and fp32 (parity mode), the direct kernels. */
typedef struct fv_conv3d_desc {
  int dtype;         /* FV_F32 or FV_BF16 */
  int n, d, h, w;    /* spatial size (stride 1, padding 1: output == input) */
  int cin, cout;     /* channels (dense, channel stride == count) */
} fv_conv3d_desc;
size_t fv_conv3d_wk_bytes(const fv_conv3d_desc* d);
int fv_conv3d_weight_prep(const fv_conv3d_desc* d, const float* w_param, void* wk, void* wt, void* stream);
/* fv_conv3d_weight_prep of n convs of one shape in one launch (host pointer tables; wk[i] / wt[i]
 * may be NULL) */
int fv_conv3d_weight_prep_multi(const fv_conv3d_desc* d, int n, const float* const* w_param, void* const* wk,
                                void* const* wt, void* stream);
/* BN partial records ([records][2][cout] (sum, sum of squares), block_pixels voxels each) that
 * fv_conv3d_fwd writes when stats != NULL; 0 = not available for this shape */
int fv_conv3d_stats_blocks(const fv_conv3d_desc* d);
int fv_conv3d_stats_block_pixels(const fv_conv3d_desc* d);
/* y = conv3d(x, wk) + bias [+ res] */
int fv_conv3d_fwd(const fv_conv3d_desc* d, const void* x, const void* wk, const float* bias, const void* res,
                  void* y, float* stats, void* stream);
/* dx [n][d][h][w][cin] from dy [n][d][h][w][cout] and wt */
int fv_conv3d_bwd_data(const fv_conv3d_desc* d, const void* dy, const void* wt, void* dx, void* stream);
/* dw [cout][cin][3][3][3] fp32 and db [cout] (may be NULL), deterministic; ws of
 * fv_conv3d_wgrad_ws_bytes bytes (0 = none needed) */
size_t fv_conv3d_wgrad_ws_bytes(const fv_conv3d_desc* d);
int fv_conv3d_bwd_weight(const fv_conv3d_desc* d, const void* x, const void* dy, float* dw, float* db, void* ws,
                         void* stream);
/* AFE.forward's x.view(N, C, D, H, W) of the mid_conv output (models.py:941-942) between the
 * build's layouts: src NHWC [n][hw][c*d_count] -> dst NDHWC [n][d][hw][c] (inverse = 0), or back
 * (inverse = 1: src NDHWC, dst NHWC) */
int fv_depth_split(int dtype, const void* src, int n, int hw, int c, int d_count, int inverse, void* dst,
                   void* stream);

/* ------------------------------- general 3-D conv (MFE hourglass, compress, mask) ---- */
/* nn.Conv3d(cin, cout, k, 1, k / 2), k = 1 / 3 / 7, of the MFE (models.py:1054-1057, 1063, 1072-1075):
 * the "CNA" ConvBlock3D of DownBlock3D / UpBlock3D (modules.py:59-94), the 1x1x1 compress and the
 * 7x7x7 mask conv.  An implicit GEMM on the matrix units for both dtypes (bf16: 16x16x32 bf16
 * MFMA; fp32: the exact 16x16x4 f32 MFMA), fp32 accumulation.  Activations NDHWC, dense; weights
 * in the reference layout [cout][cin][k][k][k] fp32, re-laid out per forward by
 * fv_conv3dg_weight_prep.  cin must be a positive multiple of 8; cout, d, h, w are free.
 * upsample = 1 folds UpBlock3D's nn.Upsample(scale_factor=(1, 2, 2)) (modules.py:81, 94) into the
 * gather: x is then [n][d][h / 2][w / 2][cin] and is read at (d, h >> 1, w >> 1).
 * Unsupported descriptors (cin % 8 != 0, another ksize, upsample with odd h or w) return
 * FV_E_UNSUPPORTED from every entry (the byte queries return 0). */
typedef struct fv_conv3dg_desc {
  int dtype;         /* FV_F32 or FV_BF16 */
  int n, d, h, w;    /* OUTPUT volume */
  int cin, cout;     /* channels (dense, channel stride == count) */
  int ksize;         /* 1, 3 or 7 (cubic), stride 1, padding ksize / 2 */
  int upsample;      /* 1: nearest (1, 2, 2) upsample of x in front of the conv */
} fv_conv3dg_desc;
int fv_conv3dg_check(const fv_conv3dg_desc* d);
/* bytes of the forward (wk) and data-gradient (wt: transposed, taps flipped) weight layouts */
size_t fv_conv3dg_wk_bytes(const fv_conv3dg_desc* d);
size_t fv_conv3dg_wt_bytes(const fv_conv3dg_desc* d);
int fv_conv3dg_weight_prep(const fv_conv3dg_desc* d, const float* w_param, void* wk, void* wt, void* stream);
/* y [n][d][h][w][cout] = conv3d(x, wk) + bias (bias may be NULL) */
int fv_conv3dg_fwd(const fv_conv3dg_desc* d, const void* x, const void* wk, const float* bias, void* y,
                   void* stream);
/* dx [n][d][h][w][cin] at the OUTPUT resolution from dy [n][d][h][w][cout] and wt; with upsample
 * the caller then sums the 2x2 phases (fv_upsample2x_bwd on the [n][d * h][w][cin] alias) */
int fv_conv3dg_bwd_data(const fv_conv3dg_desc* d, const void* dy, const void* wt, void* dx, void* stream);
/* backward of the folded upsample for ANY cin % 8 == 0: out [n][d][h / 2][w / 2][cin] = the 2x2
 * phase sums of g [n][d][h][w][cin] (fv_upsample2x_bwd takes 8 * 2^k channels only) */
int fv_conv3dg_upsample_bwd(const fv_conv3dg_desc* d, const void* g, void* out, void* stream);
/* dw[cout][cin][k][k][k] fp32 and db [cout] (may be NULL) from x (the conv's input, low
 * resolution under upsample) and dy: voxel-split fp32 slabs summed in a fixed order, no float
 * atomics (bit-reproducible); ws of fv_conv3dg_wgrad_ws_bytes bytes */
size_t fv_conv3dg_wgrad_ws_bytes(const fv_conv3dg_desc* d);
int fv_conv3dg_bwd_weight(const fv_conv3dg_desc* d, const void* x, const void* dy, float* dw, float* db, void* ws,
                          void* stream);

/* ------------------------------------------------------- warp path (Generator / MFE) ---- */
/* F.grid_sample(in, grid, mode="bilinear" (trilinear), padding_mode="zeros",
 * align_corners=True) for 5-D input (models.py:1103; utils.py:175): in NDHWC [B/group][Di][Hi][Wi][C],
 * grid [B][Do][Ho][Wo][3] fp32 (x -> W, y -> H, z -> D), out NDHWC [B][Do][Ho][Wo][C]; output
 * batch b samples input batch b / group (group = K + 1 for create_deformed_source_image's
 * repeat, utils.py:168-172).  dtype FV_F32 / FV_BF16 for in / out / gout. */
int fv_grid_sample3d_fwd(int dtype, const void* in, const float* grid, int B, int Di, int Hi, int Wi, int Do,
                         int Ho, int Wo, int C, int group, void* out, void* stream);
/* gin (fp32, input layout, zeroed by the caller; float atomics) += dL/din, ggrid = dL/dgrid;
 * either may be NULL */
int fv_grid_sample3d_bwd(int dtype, const void* in, const float* grid, const void* gout, int B, int Di, int Hi,
                         int Wi, int Do, int Ho, int Wo, int C, int group, float* gin, float* ggrid, void* stream);
/* gin (dtype, input layout, every element written) = dL/din without float atomics: the output
 * voxels are bucketed by their base input cell (count, scan, fill in ws), each bucket is ordered
 * by voxel index, and each input cell sums the buckets whose corner it is (bit-reproducible).
 * ws: fv_grid_sample3d_bwd_input_ws_bytes bytes = 4 B per input cell key + 24 B per OUTPUT voxel
 * (key/rank + record): for create_deformed_source_image (group K+1, B = N (K+1) grids) at N = 8,
 * K = 15, 16x64x64 that is ~200 MB per backward. */
size_t fv_grid_sample3d_bwd_input_ws_bytes(int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int group);
int fv_grid_sample3d_bwd_input(int dtype, const float* grid, const void* gout, int B, int Di, int Hi, int Wi, int Do,
                               int Ho, int Wo, int C, int group, void* gin, void* ws, void* stream);
int fv_f32_to(int dtype, const float* a, void* b, long n, void* stream);
/* fs * occlusion (models.py:1106): x [P][C] NHWC, occ [P] fp32; backward dx = g*occ (may be
 * NULL), docc[p] = sum_c g x (may be NULL) */
int fv_occlusion_fwd(int dtype, const void* x, const float* occ, long P, int C, void* y, void* stream);
int fv_occlusion_bwd(int dtype, const void* g, const void* x, const float* occ, long P, int C, void* dx, float* docc,
                     void* stream);
/* create_sparse_motions (utils.py:139-152) with J = Rs inv(Rd) [N][3][3]: out [N][K+1][D][H][W][3] */
int fv_sparse_motion_fwd(const float* kp_s, const float* kp_d, const float* J, int N, int K, int D, int H, int W,
                         float* out, void* stream);
/* backward sums [N][K][12] = (sum_v g_k, sum_v g_k (id - kp_d[k])^T) of the motion gradient g */
int fv_sparse_motion_bwd(const float* g, const float* kp_d, int N, int K, int D, int H, int W, float* sums,
                         void* stream);
/* create_heatmap_representations (utils.py:130-137, kp2gaussian_3d 123-129): out [N][K+1][D][H][W] */
int fv_heatmap_fwd(const float* kp_s, const float* kp_d, int N, int K, int D, int H, int W, float var, float* out,
                   void* stream);
int fv_heatmap_bwd(const float* g, const float* kp_s, const float* kp_d, int N, int K, int D, int H, int W, float var,
                   float* dkp_s, float* dkp_d, void* stream);
/* MFE mask softmax + deformation (models.py:1076-1078): prob = softmax over K1 of logits
 * [N][K1][V]; def [N][V][3] = sum_k prob_k sm[N][K1][V][3] */
int fv_motion_mask_fwd(const float* logits, const float* sm, int N, int K1, long V, float* prob, float* def,
                       void* stream);
int fv_motion_mask_bwd(const float* prob, const float* sm, const float* gdef, const float* gprob, int N, int K1,
                       long V, float* dlogits, float* dsm, void* stream);

/* ------------------------------------------------------------ perceptual loss ---- */
/* The VGG feature stacks of PerceptualLoss (losses.py:33-151) run their convs on
 * fv_conv2d_fwd / fv_conv2d_bwd_data and their per-channel normalisations
 * (apply_imagenet_normalization / apply_vggface_normalization, utils.py:182-193) and the
 * 0.5x bilinear downscale (== 2x2 average on even sizes, losses.py:148-149) on fv_bn_act_fwd
 * (slope 1 = identity, scale/shift = the affine, pool = the average).  The rest: */
int fv_relu_bwd(int dtype, const void* g, const void* y, long n, void* dx, void* stream);
int fv_maxpool2_fwd(int dtype, const void* x, int n, int h, int w, int c, void* y, void* stream);
int fv_maxpool2_bwd(int dtype, const void* x, const void* g, int n, int h, int w, int c, void* dx, void* stream);
int fv_avgpool2_bwd(int dtype, const void* g, int n, int h, int w, int c, void* dx, void* stream);
/* nn.L1Loss over bf16 / f32 operands (criterion of losses.py:127, 142-151) */
size_t fv_l1t_ws_bytes(void);
int fv_l1t_fwd(int dtype, const void* a, const void* b, long n, float* loss, void* ws, void* stream);
int fv_l1t_bwd(int dtype, const void* a, const void* b, long n, const float* gout, float scale, void* da,
               void* stream);

/* ------------------------------------------------------------- spectral norm ---- */
size_t fv_spectral_norm_ws_bytes(int rows, int cols);
/* one power iteration (u, v updated in place) when power_iter, then sigma = u.(W v) */
int fv_spectral_norm_fwd(const float* w, int rows, int cols, float* u, float* v, float* sigma,
                         int power_iter, void* ws, void* stream);
/* g_orig = g_sn/sigma - <g_sn, w>/sigma^2 * u v^T   (in place allowed: g_orig == g_sn) */
int fv_spectral_norm_bwd(const float* w, const float* g_sn, int rows, int cols, const float* u,
                         const float* v, const float* sigma, float* g_orig, void* ws,
                         void* stream);

/* batched form for all spectral-normed convs of a model (4 launches).  The caller builds
 * the table once on the host (fv_spectral_norm_batch_build writes it into table_host, which
 * the caller copies to device memory of fv_spectral_norm_batch_table_bytes) and keeps the
 * workspace (fv_spectral_norm_batch_ws_floats floats) alive.  usnap/vsnap receive the u, v
 * used for sigma (what the backward needs). */
typedef struct fv_sn_layer {
  const float* w;
  float* u;
  float* v;
  float* sigma;
  float* usnap;
  float* vsnap;
  int rows, cols;
} fv_sn_layer;
size_t fv_spectral_norm_batch_ws_floats(const fv_sn_layer* layers, int nlayers);
size_t fv_spectral_norm_batch_table_bytes(int nlayers);
int fv_spectral_norm_batch_build(const fv_sn_layer* layers, int nlayers, float* ws, void* table_host,
                                 int* nblocks3);
int fv_spectral_norm_fwd_batch(const void* table_dev, int nlayers, const int* nblocks3, int power_iter,
                               void* stream);

/* ---------------------------------------------------------------- batch norm ---- */
size_t fv_bn_ws_bytes(int c);
/* Conv-record folds (fv_bn_*_partials, fv_bn_bwd_from_records) run in ONE launch: level 1
 * chunk partials + level 2 by each 16-channel group's last-arriving block (bn.hip
 * fold16_part_kernel: sc1 stores, arrival tickets in a per-device pool; bit-reproducible). */
/* (count, sum, centred-M2) conv partials -> stats [3][c] doubles (count, sum, sumsq) */
int fv_bn_stats_from_partials(const float* partials, int nblocks, int block_pixels,
                              long total_pixels, int c, double* stats, void* ws, void* stream);
/* statistics of an NHWC tensor (pixels x c, channel stride ldc) -> stats [3][c] */
int fv_bn_stats_tensor(int dtype, const void* x, long pixels, int c, int ldc, double* stats,
                       void* ws, void* stream);
/* mean/var from stats (already all-reduced for SyncBN) -> save_mean, save_invstd and the
 * fused affine scale = gamma*invstd, shift = beta - mean*scale; running stats updated
 * with momentum and the unbiased variance when training.  In eval mode the running
 * statistics are used and stats may be NULL. */
int fv_bn_finalize(const double* stats, int c, const float* gamma, const float* beta, float eps,
                   float momentum, int training, float* running_mean, float* running_var,
                   long long* num_batches_tracked, float* save_mean, float* save_invstd, float* scale,
                   float* shift, void* stream);
/* single-process training forms (no SyncBN exchange between the statistics and finalize):
 * statistics + finalize (+ num_batches_tracked += 1) in one launch (two for a tensor) */
int fv_bn_stats_finalize_partials(const float* partials, int nblocks, int block_pixels, long total_pixels,
                                  int c, const float* gamma, const float* beta, float eps, float momentum,
                                  float* running_mean, float* running_var, long long* num_batches_tracked,
                                  float* save_mean, float* save_invstd, float* scale, float* shift,
                                  void* ws, void* stream);
int fv_bn_stats_finalize_tensor(int dtype, const void* x, long pixels, int c, int ldc, const float* gamma,
                                const float* beta, float eps, float momentum, float* running_mean,
                                float* running_var, long long* num_batches_tracked, float* save_mean,
                                float* save_invstd, float* scale, float* shift, void* ws, void* stream);
/* out = [avgpool2](act(y*scale + shift)); y [n][h][w][ldc], out [n][h/p][w/p][c] */
int fv_bn_act_fwd(int dtype, const void* y, int n, int h, int w, int c, int ldc,
                  const float* scale, const float* shift, float slope, int pool, void* out,
                  void* stream);
/* sums over pixels of g and g*yhat with g = dout_full * act'(.) -> red [2][c] doubles */
int fv_bn_act_bwd_reduce(int dtype, const void* dout, const void* y, int n, int h, int w, int c,
                         int ldc, const float* mean, const float* invstd, const float* gamma,
                         const float* beta, float slope, int pool, double* red, void* ws,
                         void* stream);
/* dgamma/dbeta and the two BN-backward coefficients k [2][c] = red / count (k may be NULL:
 * dgamma/dbeta only; dgamma/dbeta may be NULL) */
int fv_bn_bwd_finalize(const double* red, int c, long count, float* dgamma, float* dbeta,
                       float* k, void* stream);
/* the same with the element count read per channel from device memory (row 0 of the
 * all-reduced [3][c] statistics record: the global count, also for uneven per-rank batches) */
int fv_bn_bwd_finalize_dev(const double* red, int c, const double* count, float* dgamma,
                           float* dbeta, float* k, void* stream);
/* single-process form of fv_bn_act_bwd_reduce + fv_bn_bwd_finalize (two launches) */
int fv_bn_act_bwd_reduce_finalize(int dtype, const void* dout, const void* y, int n, int h, int w, int c,
                                  int ldc, const float* mean, const float* invstd, const float* gamma,
                                  const float* beta, float slope, int pool, long count, float* dgamma,
                                  float* dbeta, float* k, void* ws, void* stream);
/* dx = gamma*invstd*(g - k0 - yhat*k1) [+ addend]; dx/addend [n][h][w][ldc] */
int fv_bn_act_bwd_apply(int dtype, const void* dout, const void* y, int n, int h, int w, int c,
                        int ldc, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, float slope, int pool, const float* k,
                        const void* addend, void* dx, void* stream);
/* the same two passes (no pool, ldc == c) also writing an e4m3 copy of their output for an fp8
 * conv that consumes it: out8 / dx8 [n][h][w][c] bytes = the bf16 output quantized with the
 * delayed scale of `site` (the consumer's fv_fp8_site_bytes site, already seeded), bit-identical
 * to fv_quantize_fp8_site over the output; the site's in-flight amax and dq are updated the
 * same way.  Replaces the separate quantize pass (one read of the output).  out / dx may be NULL:
 * then only the e4m3 copy is written (its values are still the bf16-rounded outputs) -- for a
 * consumer whose forward, data gradient and weight gradient all run on the e4m3 operands. */
int fv_bn_act_fwd_q8(int dtype, const void* y, int n, int h, int w, int c, const float* scale,
                     const float* shift, float slope, void* out, void* out8, void* site, void* stream);
int fv_bn_act_bwd_apply_q8(int dtype, const void* dout, const void* y, int n, int h, int w, int c,
                           const float* mean, const float* invstd, const float* gamma,
                           const float* beta, float slope, const float* k, const void* addend,
                           void* dx, void* dx8, void* site, void* stream);

/* ------------------------------------------------------ elementwise / layout ---- */
int fv_nchw_to_nhwc(int dtype_out, const float* x, int n, int c, int hw, int ldc, void* out,
                    void* stream);
int fv_nhwc_to_nchw(int dtype_in, const void* x, int n, int c, int hw, int ldc, float* out,
                    void* stream);
int fv_cast(int dtype_in, const void* x, int dtype_out, void* y, long count, void* stream);
/* g_src[n][i][j][c] = sum_{a,b} g[n][2i+a][2j+b][c]  (nearest x2 upsample backward) */
int fv_upsample2x_bwd(int dtype, const void* g, int n, int h_src, int w_src, int c, void* out,
                      void* stream);
/* dpre (NHWC, channel stride ldc, zero padded) = dy * y * (1 - y), dy/y NCHW fp32 */
int fv_sigmoid_bwd_to_nhwc(int dtype_out, const float* dy, const float* y, int n, int c, int hw,
                           int ldc, void* dpre, void* stream);

/* --------------------------------------------------------- latent and losses ---- */
size_t fv_loss_ws_bytes(void);
/* h [P][2L] (NHWC, mu = channels [0,L), logstd = [L,2L)); eps NCHW fp32 [n][L][hw];
 * mu/logstd/z [P][L] NHWC */
int fv_reparam_fwd(int dtype, const void* h, const float* eps, int n, int L, int hw, void* mu,
                   void* logstd, void* z, void* stream);
/* the same, also writing the KL mean of (mu, logstd) to kl[0] (KLDivergenceLoss forward,
 * losses.py:392) from the values it already holds; ws of fv_reparam_ws_bytes bytes */
size_t fv_reparam_ws_bytes(int n, int L, int hw);
int fv_reparam_kl_fwd(int dtype, const void* h, const float* eps, int n, int L, int hw, void* mu,
                      void* logstd, void* z, float* kl, void* ws, void* stream);
/* 1 when (L, hw) runs the tiled reparameterisation (hw % 32 == 0, L <= 496): only then may
 * fv_reparam_kl_fwd leave mu/logstd NULL (the caller reads them as channel slices of h) while
 * still reducing the KL */
int fv_reparam_tiled(int L, int hw);
/* dh = [dz + dmu | dz*exp(logstd)*eps + dlogstd]; dz/dmu/dlogstd may be NULL */
int fv_reparam_bwd(int dtype, const void* h, const float* eps, int n, int L, int hw,
                   const void* dz, const void* dmu, const void* dlogstd, void* dh, void* stream);
/* the same plus the KL gradient (KLDivergenceLoss backward, losses.py:392) folded in:
 * kl_grad = device fp32 dLoss/dKL (NULL: none); dh += kl_grad / (n L hw) *
 * [mu | exp(2 logstd) - 1] -- the separate fv_kl_bwd pass and its dmu/dlogstd tensors vanish */
int fv_reparam_kl_bwd(int dtype, const void* h, const float* eps, int n, int L, int hw,
                      const void* dz, const void* dmu, const void* dlogstd, const float* kl_grad,
                      void* dh, void* stream);
int fv_kl_fwd(int dtype, const void* mu, const void* logstd, long count, float* loss, void* ws,
              void* stream);
int fv_kl_bwd(int dtype, const void* mu, const void* logstd, long count, const float* gout,
              void* dmu, void* dlogstd, void* stream);
int fv_mse_fwd(const float* a, const float* b, long count, float* loss, void* ws, void* stream);
int fv_mse_bwd(const float* a, const float* b, long count, const float* gout, float* da,
               float* db, void* stream);
int fv_l1_fwd(const float* a, const float* b, long count, float* loss, void* ws, void* stream);
int fv_l1_bwd(const float* a, const float* b, long count, const float* gout, float* da,
              float* db, void* stream);

/* ----------------------------------------------------------------- optimiser ---- */
typedef struct fv_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long numel;
} fv_adam_tensor;
#define FV_ADAM_CHUNK 4096
/* multi-tensor Adam (torch.optim.Adam math, no weight decay / amsgrad).  `tensors` is a
 * DEVICE array of descriptors; `blocks` a DEVICE array of nblocks (tensor, chunk) int pairs,
 * one per FV_ADAM_CHUNK elements of each tensor; `step` is the step count after increment. */
int fv_adam_step(const fv_adam_tensor* tensors, const int* blocks, int nblocks, double lr,
                 double beta1, double beta2, double eps, long step, void* stream);
/* The same update with the step count kept on the DEVICE (graph-replayable, as
 * torch.optim.Adam(capturable=True)): one launch increments *step_dev (fp64) and writes the
 * bias-correction coefficients (lr / (1 - beta1^t), sqrt(1 - beta2^t), computed in fp64 as
 * the host path does) to coef_ws (2 floats), the update kernel reads them. */
int fv_adam_step_dev(const fv_adam_tensor* tensors, const int* blocks, int nblocks, double lr,
                     double beta1, double beta2, double eps, double* step_dev, float* coef_ws,
                     void* stream);

/* ------------------------------------------------- batched spectral-norm backward ---- */
/* g <- g / sigma - (<g, w> / sigma^2) u v^T in place for n layers in two launches (the
 * per-layer fv_spectral_norm_bwd is two launches each); ws >= 256 * n floats. */
#define FV_SNB_MAX 24
typedef struct fv_sn_bwd_layer {
  const float* w;
  float* g;
  const float* u;
  const float* v;
  const float* sigma;
  int rows, cols;
} fv_sn_bwd_layer;
int fv_spectral_norm_bwd_multi(int n, const fv_sn_bwd_layer* layers, float* ws, void* stream);

/* ------------------------------------------------------------------ staging ---- */
/* stream-ordered host -> device copy of `bytes` from PINNED host memory (descriptor tables of
 * the batched spectral norm / Adam launches); captured into a HIP graph as a memcpy node. */
int fv_copy_h2d_async(void* dst, const void* src_pinned, size_t bytes, void* stream);

/* ------------------------------------------------------------ communication ---- */
typedef void* fv_comm_t;
int fv_comm_unique_id(uint8_t out[128]);
int fv_comm_init(const uint8_t id[128], int nranks, int rank, int device, fv_comm_t* comm);
/* op: 0 = sum, 1 = average, 2 = max (anything else: FV_E_BADARG); dtype: FV_F32 / FV_BF16 /
 * FV_F64 */
int fv_comm_allreduce(fv_comm_t comm, void* buf, size_t count, int dtype, int op,
                      void* stream);
int fv_comm_allgather(fv_comm_t comm, const void* send, void* recv, size_t count_per_rank,
                      int dtype, void* stream);
int fv_comm_broadcast(fv_comm_t comm, void* buf, size_t count, int dtype, int root,
                      void* stream);
int fv_comm_destroy(fv_comm_t comm);
/* Failure detection (replaces the teardown the reference gets from mp.spawn, train.py:54, and
 * NCCL_ASYNC_ERROR_HANDLING under init_process_group("nccl"), distributed.py:24-31):
 * *result = ncclCommGetAsyncError (0 = success, 7 = in progress; other values also set
 * fv_last_error), host-only, callable from a watchdog thread; fv_comm_count = ncclCommCount;
 * fv_comm_abort = ncclCommAbort (outstanding collectives abandoned, handle freed). */
int fv_comm_async_error(fv_comm_t comm, int* result);
int fv_comm_count(fv_comm_t comm, int* nranks);
int fv_comm_abort(fv_comm_t comm);

/* ------------------------------------------------- patch discriminator pieces ---- */
/* Instance norm + LeakyReLU over a dense NHWC tensor [n][h][w][c] (c a power of two in
 * [8, 512], dtype FV_F32 / FV_BF16): nn.InstanceNorm2d(c, affine=True) followed by
 * LeakyReLU(slope).  Statistics are per (sample, channel) over the h*w plane: biased variance,
 * invstd = 1 / sqrt(var + eps); there are no running statistics.  mean / invstd are fp32
 * [n][c].  All sums are fixed-order (fp32 runs, then fp64): bit-reproducible, and a sample's
 * results depend on that sample alone.  ws: fv_in_ws_bytes bytes of scratch.
 *   fwd:        y = leaky(gamma * xhat + beta), xhat = (x - mean) * invstd
 *   bwd_reduce: with g = dout * leaky'(gamma * xhat + beta): dgamma[c] = sum g * xhat,
 *               dbeta[c] = sum g (over samples and pixels), k [n][2][c] = the plane means of
 *               (g, g * xhat)
 *   bwd_apply:  dx = gamma * invstd * (g - k0 - xhat * k1) */
size_t fv_in_ws_bytes(int n, int h, int w, int c);
int fv_in_stats(int dtype, const void* x, int n, int h, int w, int c, float eps, float* mean, float* invstd, void* ws,
                void* stream);
int fv_in_act_fwd(int dtype, const void* x, int n, int h, int w, int c, const float* mean, const float* invstd,
                  const float* gamma, const float* beta, float slope, void* y, void* stream);
int fv_in_act_bwd_reduce(int dtype, const void* dout, const void* x, int n, int h, int w, int c, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, float slope, float* dgamma,
                         float* dbeta, float* k, void* ws, void* stream);
int fv_in_act_bwd_apply(int dtype, const void* dout, const void* x, int n, int h, int w, int c, const float* mean,
                        const float* invstd, const float* gamma, const float* beta, float slope, const float* k,
                        void* dx, void* stream);
/* Discriminator input: out NHWC [n][h][w][ldc] of `dtype` (ldc a power of two in [8, 32],
 * >= 3 + k) from the NCHW fp32 image [n][3][h][w] and the keypoints kp [n][k][kp_stride]
 * (kp_stride >= 2; kp may be NULL when k == 0).  Channels 0-2: the image; channel 3 + j:
 * exp(-0.5 ((gx - kp[j][0])^2 + (gy - kp[j][1])^2) / 0.01) with gx = 2 w / (W - 1) - 1,
 * gy = 2 h / (H - 1) - 1; the padding channels 0.  h, w >= 2. */
int fv_disc_input_fwd(int dtype, const float* img, const float* kp, int n, int h, int w, int k, int kp_stride, int ldc,
                      void* out, void* stream);

/* ------------------------------------------------------ head pose estimator pieces ---- */
/* The operators of HPE_EDE (models.py:990-1037; ResBottleneck modules.py:138-152) that the 1x1 /
 * 3x3 convolution and batch-norm entries above do not cover.  dtype FV_F32 (exact) or FV_BF16
 * (fp32 accumulation).  Every cross-thread sum has a fixed order and no float atomics: reruns are
 * bit-identical.  Unsupported shapes return FV_E_UNSUPPORTED (the size queries return 0).
 *
 * Stem: nn.Conv2d(3, cout, 7, 2, 3) of pre_layers[0] (models.py:1003) as an implicit GEMM on the
 * matrix units.  x is the NCHW fp32 image [n][3][h][w], read directly (rounded to bf16 in bf16
 * mode); h and w even; y is NHWC [n][h/2][w/2][cout] of `dtype`, cout a multiple of 8.  wk is the
 * weight image [cout rounded up to 16][160] of `dtype` with k = (r*7 + s)*3 + ci (147 valid
 * columns, the rest zero), written by fv_stem7s2_weight_prep from the parameter [cout][3][7][7].
 * stats (may be NULL): fv_stem7s2_stats_blocks records [2][cout] of (sum, sum of squares) over
 * fv_stem7s2_stats_block_pixels pixels each of the fp32 pre-rounding outputs (bias included),
 * the layout fv_bn_stats_finalize_partials consumes.  bwd_weight: dw [cout][3][7][7] and db
 * [cout] (db may be NULL) from dy NHWC [n][h/2][w/2][cout]; the pixels are split into fp32 slabs
 * in ws (fv_stem7s2_wgrad_ws_bytes) that are summed in split order.
 * There is NO data gradient: the stem's input is the image, which is data (trainer.py:272-273). */
size_t fv_stem7s2_wk_elems(int cout);
int fv_stem7s2_weight_prep(int dtype, const float* w, int cout, void* wk, void* stream);
int fv_stem7s2_stats_blocks(int n, int h, int w);
int fv_stem7s2_stats_block_pixels(void);
int fv_stem7s2_fwd(int dtype, const float* x, int n, int h, int w, int cout, const void* wk, const float* bias,
                   void* y, float* stats, void* stream);
size_t fv_stem7s2_wgrad_ws_bytes(int n, int h, int w, int cout);
int fv_stem7s2_bwd_weight(int dtype, const float* x, const void* dy, int n, int h, int w, int cout, float* dw,
                          float* db, void* ws, void* stream);
/* nn.MaxPool2d(3, 2, 1) (models.py:1003) over dense NHWC [n][h][w][c], h and w even, c a multiple
 * of 8; padding behaves as -inf.  argmax [n][h/2][w/2][c] uint8: the winning tap 0..8 in row-major
 * window order (input pixel (2 oy - 1 + tap / 3, 2 ox - 1 + tap % 3)); the first in-bounds tap wins
 * ties and NaN propagates, as torch's `val > maxval || isnan(val)`.  With scale != NULL the pooled
 * value is act(x * scale[c] + shift[c]) rounded to `dtype` (the expression and rounding of
 * fv_bn_act_fwd, slope in [0, 1]).  bwd is a gather: dx [n][h][w][c], every element written, is the
 * sum of g over the (at most four) windows whose argmax is that element, in window order; with
 * the prologue it is the gradient with respect to the activation output. */
int fv_maxpool3s2_fwd(int dtype, const void* x, int n, int h, int w, int c, const float* scale, const float* shift,
                      float slope, void* y, uint8_t* argmax, void* stream);
int fv_maxpool3s2_bwd(int dtype, const void* g, const uint8_t* argmax, int n, int h, int w, int c, void* dx,
                      void* stream);
/* y[n][i][j][c] = x[n][2i][2j][c] (the stride of ResBottleneck's stride-2 1x1 convs, modules.py:143);
 * bwd: dx = g at the even pixels, 0 elsewhere, every element written.  h, w even, c % 8 == 0. */
int fv_subsample2_fwd(int dtype, const void* x, int n, int h, int w, int c, void* y, void* stream);
int fv_subsample2_bwd(int dtype, const void* g, int n, int h, int w, int c, void* dx, void* stream);
/* Bottleneck join (modules.py:152): out = relu(ya * sa[c] + ha[c] + (sb ? yb * sb[c] + hb[c] : yb))
 * over `pixels` x c dense NHWC elements, c % 8 == 0. */
int fv_bn2_add_relu_fwd(int dtype, const void* ya, const float* sa, const float* ha, const void* yb, const float* sb,
                        const float* hb, long pixels, int c, void* out, void* stream);
/* out = a + b over n elements (n % 8 == 0; out aliases neither input): the block-input gradient of a
 * ResBottleneck is the sum of its two branches' gradients, and no existing addend slot sits there
 * (the BN apply's addend is at the BN input, which has out_channels / 4 channels). */
int fv_add2(int dtype, const void* a, const void* b, long n, void* out, void* stream);
/* Pose head (models.py:1025-1036).  pool: feat [n][c] fp32 = mean over the hw plane of x NHWC
 * [n][hw][c].  head_fwd: w / b are HOST arrays of five device pointers (fc_yaw, fc_pitch, fc_roll,
 * fc_t, fc_scale: [rows][c] and [rows] fp32 with rows n_bins, n_bins, n_bins, 3, 1); out [n][7] =
 * (yaw, pitch, roll, t0, t1, t2, scale) with angle = (sum_j j p_j - n_bins / 2) * 3 pi / 180 and p
 * the softmax of the head's logits, saved in prob [n][3][n_bins].  head_bwd: from g_out [n][7],
 * dw / db (HOST arrays of five device pointers, summed over the samples in order) and dx NHWC
 * [n][hw][c] of `dtype` = dfeat / hw broadcast over the plane; ws: fv_pose_head_ws_bytes. */
int fv_pose_pool_fwd(int dtype, const void* x, int n, int hw, int c, float* feat, void* stream);
int fv_pose_head_fwd(const float* feat, int n, int c, int n_bins, const float* const* w, const float* const* b,
                     float* out, float* prob, void* stream);
size_t fv_pose_head_ws_bytes(int n, int c, int n_bins);
int fv_pose_head_bwd(int dtype, const float* g_out, const float* feat, const float* prob, int n, int hw, int c,
                     int n_bins, const float* const* w, float* const* dw, float* const* db, void* dx, void* ws,
                     void* stream);

/* ------------------------------------------------ canonical keypoint detector pieces ---- */
/* The head and the tail of CKD (models.py:948-987) around the conv / batch-norm entries above.
 * dtype FV_F32 or FV_BF16 storage, fp32 arithmetic, no float atomics, every cross-thread sum in a
 * fixed order (reruns are bit-identical).  Unsupported arguments return FV_E_UNSUPPORTED.
 *
 * Resize: F.interpolate(x, mode="bilinear", align_corners=False, recompute_scale_factor=True) of the
 * NCHW fp32 image x [n][3][h][w] to ho x wo (the caller passes floor(h * s), floor(w * s)).  The
 * sampling scale is h / ho (w / wo) in fp32, the source index scale * (o + 0.5) - 0.5 clamped at
 * 0, the upper neighbour clamped at the last row / column, and the blend
 * h0 (w0 a + w1 b) + h1 (w0 c + w1 d).  y is dense NHWC [n][ho][wo][8] of `dtype`: channels 0-2 the
 * result, 3-7 zero -- the first conv's input with cin_valid = 3.  There is no backward. */
int fv_ckd_resize_fwd(int dtype, const float* x, int n, int h, int w, int ho, int wo, void* y, void* stream);
/* Soft-argmax (out2heatmap + heatmap2kp, utils.py:106-118) of the logits z, dense NDHWC
 * [n][d * h * w][k] of `dtype` (rows of k elements, no alignment assumed):
 *   kp[n][k][:] = sum_v softmax_v(z[n][v][k] / T) (2 w / (W-1) - 1, 2 h / (H-1) - 1, 2 d / (D-1) - 1)
 * with the heatmap never written.  d, h, w >= 2; 1 <= k <= 256; d * h * w * k < 2^31.  The maximum
 * is taken on z and the exponent is (z - max z) / T, so a common offset of the logits costs no
 * accuracy.  Exponentials, coordinates and products are fp32; the running sums are fp64.  stat
 * [n][k][8] fp32 = (max_v z, sum_v exp((z - max z) / T), kp hi[3], kp lo[3]) for the backward, hi = kp
 * and hi + lo the fp64 quotient: at a peaked heatmap kp is within 1e-3 of the peak's coordinate and
 * the backward's (grid - kp) needs the digits below fp32.  ws: fv_ckd_softargmax_ws_bytes (the
 * per-chunk partials; 0 for unsupported arguments).
 * bwd: dz[n][v][k] = (1 / T) p sum_j g_kp[n][k][j] (grid_j(v) - kp[n][k][j]) with
 * p = exp((z - stat.max) / T) / stat.sum, in `dtype` and the layout of z; every element written. */
size_t fv_ckd_softargmax_ws_bytes(int n, int k, int d, int h, int w);
int fv_ckd_softargmax_fwd(int dtype, const void* z, int n, int k, int d, int h, int w, float temperature, float* kp,
                          float* stat, void* ws, void* stream);
int fv_ckd_softargmax_bwd(int dtype, const void* z, const float* g_kp, const float* stat, int n, int k, int d, int h,
                          int w, float temperature, void* dz, void* stream);

/* ---------------------------------------------- expression feature extractor pieces ---- */
/* EFE_conv5 (models.py:724-799) between the conv / batch-norm entries above: the concatenation
 * torch.cat((out_conv(x), kp2gaussian_3d(kpc, x.shape[2:])), 1) (models.py:790-791, utils.py:130-136).
 * dtype FV_F32 or FV_BF16 storage, fp32 arithmetic, no float atomics, every cross-thread sum in a fixed
 * order (reruns are bit-identical).  d, h, w >= 2; 1 <= k <= 256; cp must be the 2k channels padded
 * to 8 * a power of two; d * h * w * cp < 2^31; anything else returns FV_E_UNSUPPORTED.
 *
 * fwd: z dense NDHWC [n][d * h * w][k] of `dtype` (rows of k elements, no alignment assumed), kpc
 * [n][k][3] fp32 with (x, y, z) = (along W, along H, along D).  out [n][d * h * w][cp] of `dtype`:
 * channels [0, k) are z bit for bit, channel k + i is exp(-0.5 |grid(v) - kpc[n][i]|^2 / kp_variance)
 * on the grid 2 i / (size - 1) - 1, computed in fp32 and rounded once, channels [2k, cp) are zero.
 * bwd: from g_out [n][d * h * w][cp], dz [n][d * h * w][k] = channels [0, k) of g_out (every element
 * written) and dkpc[n][i][j] = sum_v g_out[n][v][k + i] G (grid_j(v) - kpc[n][i][j]) / kp_variance,
 * G recomputed in fp32 from kpc, the sums carried in fp64.  ws: fv_efe_kpcat_ws_bytes (the per-chunk
 * partials; 0 for unsupported arguments). */
int fv_efe_kpcat_fwd(int dtype, const void* z, const float* kpc, int n, int k, int cp, int d, int h, int w,
                     float kp_variance, void* out, void* stream);
size_t fv_efe_kpcat_ws_bytes(int n, int k, int cp, int d, int h, int w);
int fv_efe_kpcat_bwd(int dtype, const void* g_out, const float* kpc, int n, int k, int cp, int d, int h, int w,
                     float kp_variance, void* dz, float* dkpc, void* ws, void* stream);

/* ------------------------------------------------------ equivariance transform ---- */
/* Transform (trainer.py:91-129; FOMM's random affine + thin-plate-spline warp).  For a point
 * p = (x, y) of sample b:
 *   T(p) = theta_b[:, :2] p + theta_b[:, 2] + r(p) (1, 1),  r(p) = sum_q c_{b,q} d_q^2 log(d_q + 1e-6),
 *   d_q = |x - qx| + |y - qy| (L1, as the reference), q over the pts x pts control lattice
 *   make_coordinate_grid_2d((pts, pts)) (utils.py:79-88): coordinate i is 2 (i / (pts - 1)) - 1 in
 *   fp32, x fastest; the lattice is computed in the kernel.
 * theta [n][2][3] and cparams [n][pts^2] are fp32 in DEVICE memory, read when the kernel runs.  fp32
 * throughout, logf, the sum over q in ascending order, no atomics: reruns are bit-identical.  A point
 * on a control point contributes 0 * log(1e-6) = 0.  2 <= pts <= 16; 1 <= n <= 65535; anything else
 * returns FV_E_UNSUPPORTED.
 *
 * Frame (transform_frame, trainer.py:106-110): y[n][c][i][j] = F.grid_sample(x, T(grid),
 * align_corners=True, padding_mode="reflection") with grid(i, j) = (2 (j / (w - 1)) - 1,
 * 2 (i / (h - 1)) - 1), bilinear, in ATen's arithmetic: ((g + 1) / 2) (size - 1), reflected about 0 and
 * size - 1 (fabs, fmod by the span, parity of the flip count), clipped to [0, size - 1], floor, four
 * corners, a corner outside the image contributing 0.  x and y dense NCHW fp32 [n][c][h][w]; h, w >= 2;
 * c >= 1; h * w < 2^31 - 256.  There is no backward: the frame is data (trainer.py:271-272).
 * Coordinates (warp_coordinates, trainer.py:112-129): out[n][m][:] = T(coords[n][m][:]), [n][m][2] fp32,
 * m >= 1.  bwd, in the coordinates only (theta and cparams are constants):
 *   g_coords = theta[:, :2]^T g_out + (g_out.x + g_out.y) grad r,
 *   dr/dx = sum_q c_q (2 d_q log(d_q + 1e-6) + d_q^2 / (d_q + 1e-6)) sign(x - qx), sign(0) = 0. */
int fv_tps_warp_frame_fwd(const float* x, const float* theta, const float* cparams, int n, int c, int h, int w, int pts,
                          float* y, void* stream);
int fv_tps_warp_coords_fwd(const float* coords, const float* theta, const float* cparams, int n, int m, int pts, float* out,
                           void* stream);
int fv_tps_warp_coords_bwd(const float* coords, const float* g_out, const float* theta, const float* cparams, int n, int m,
                           int pts, float* g_coords, void* stream);

/* ------------------------------------------------------ frozen Hopenet teacher pieces ---- */
/* The inference path of the frozen Hopenet teacher (trainer.py:16-88, called at trainer.py:278-280)
 * beyond the stem, pool, 3x3 conv and pose-head entries above.  Inference only: no entry here has
 * a gradient, nothing is saved, no BN records are written.  No float atomics, every sum in a fixed
 * order: reruns are bit-identical.
 *
 * Preprocessing: y = F.interpolate((x - mean[c]) / std[c], size=(ho, wo)) (nearest; utils.py:182-186
 * and trainer.py:280) in one launch, bit-equal to torch on the CPU: fp32 subtraction, IEEE division,
 * and ATen's legacy nearest source index min((int)floorf(dst * scale), in - 1) with
 * scale = (float)in / (float)out in fp32.  x NCHW fp32 [n][3][h][w], y NCHW fp32 [n][3][ho][wo] (what
 * fv_stem7s2_fwd reads); mean and std are HOST arrays of 3 floats, read by the call.
 * 1 <= n <= 65535, every size >= 1, h * w and ho * wo < 2^31 - 256; else FV_E_UNSUPPORTED. */
int fv_hopenet_prep_fwd(const float* x, int n, int h, int w, int ho, int wo, const float* mean, const float* std, float* y,
                        void* stream);
/* Pointwise (1x1) convolution of a frozen network on the matrix units (FV_BF16: bf16 MFMA with fp32
 * accumulation; FV_F32: the exact fp32 MFMA), with the batch norm folded into the weights and a
 * per-channel shift, the stride folded into the pixel addressing and the ReLUs and the residual add
 * into the load and the store:
 *   y[p][co] = out_act(sum_ci in_act(x[src(p)][ci]) (w[co][ci] scale[co]) + shift[co] + res[p][co])
 * x dense NHWC [n][h][w][cin], y and res dense NHWC [n][h / stride][w / stride][cout], all of `dtype`;
 * src(p) is input pixel (stride i, stride j) of output pixel (i, j).  wk [cout][cin] of `dtype`
 * (fv_pw_infer_wk_elems) is written by weight_prep from the parameter w [cout][cin] (fp32) and scale
 * [cout] (NULL: 1): the product is formed in fp32 and rounded once.  shift [cout] fp32 and res may be
 * NULL.  The accumulator, shift and residual are added in fp32 and rounded once at the store.  The
 * pixel count needs no padding: short and partial tiles are predicated.  y aliasing x or res:
 * FV_E_BADARG.  cin / cout not multiples of 32 in [32, 4096], stride outside {1, 2}, odd h or w at
 * stride 2, n < 1, n * h * w >= 2^31 - 256: FV_E_UNSUPPORTED (wk_elems returns 0). */
typedef struct fv_pw_desc {
  int dtype;            /* FV_F32 or FV_BF16 */
  int n, h, w;          /* INPUT size, dense NHWC with `cin` channels */
  int stride;           /* 1, or 2: output (h/2, w/2) takes input pixel (2i, 2j); h, w even */
  int cin, cout;        /* multiples of 32 in [32, 4096] */
  int in_relu;          /* 1: the conv reads max(x, 0) */
  int out_relu;         /* 1: y = max(., 0) */
} fv_pw_desc;
size_t fv_pw_infer_wk_elems(const fv_pw_desc* d);
int fv_pw_infer_weight_prep(const fv_pw_desc* d, const float* w, const float* scale, void* wk, void* stream);
int fv_pw_infer_fwd(const fv_pw_desc* d, const void* x, const void* wk, const float* shift, const void* res, void* y,
                    void* stream);

/* --------------------------------------------------- reenactment inference (Animator) ---- */
/* Inference only: no gradient, nothing saved, no atomics (reruns are bit-identical).  Shared
 * arguments: kp_s [Ns][K][3], kp_d [N][K][3], J [N][3][3] (= Rs inv(Rd)), all fp32; Ns is 1 or N,
 * and with Ns == 1 every driving sample reads source 0 (volume and kp_s).  Volumes are dense NDHWC of
 * `dtype` (FV_F32 or FV_BF16).  Motion k of a voxel is the identity grid point id for k = 0 and
 * J (id - kp_d[k-1]) + kp_s[k-1] otherwise; sampling is trilinear, zeros padding, align_corners=True.
 * D, H, W >= 2; one lane per (voxel, motion) resp. (voxel, 8 channels), and the lane count N D H W (K+1)
 * resp. N D H W C / 8 must stay below 2^31 - 256.
 *
 * The MFE's hourglass input (models.py:1066-1071) in one launch, without the sparse-motion, heat-map
 * and per-motion sample tensors: out [N][D][H][W][(K+1)(C2+1)], channel k (C2+1) = the heat value (0 for
 * k = 0, else G(kp_d[k-1]) - G(kp_s[k-1]), G(kp) = exp(-|id - kp|^2 / (2 var))), channels
 * k (C2+1) + 1 + c = fc [Ns][D][H][W][C2] sampled at motion k.  C2 + 1 <= 16; out 16-byte aligned. */
int fv_mfe_input_fwd(int dtype, const void* fc, const float* kp_s, const float* kp_d, const float* J, int N, int Ns,
                     int K, int C2, int D, int H, int W, float var, void* out, void* stream);
/* Mask blend and warp (models.py:1076-1078, 1103) in one launch: per voxel the softmax over the K + 1
 * logits (logits [N][D][H][W][K+1] of `dtype`, the layout mask_conv writes), deformation = sum_k p_k
 * motion_k with the motions recomputed, and fs [Ns][D][H][W][C] sampled there.  out [N][D][H][W][C] of
 * `dtype`, deformation [N][D][H][W][3] fp32, prob [N][K+1][D][H][W] fp32 or NULL (the other two
 * outputs do not depend on it).  C a multiple of 8. */
int fv_motion_warp_fwd(int dtype, const void* logits, const void* fs, const float* kp_s, const float* kp_d,
                       const float* J, int N, int Ns, int K, int C, int D, int H, int W, void* out, float* deformation,
                       float* prob, void* stream);
/* Side-by-side frames (evaluate.py:39-44): driving and generated [N][3][H][W] fp32 NCHW ->
 * out [N][H][2W][3] uint8, driving left; byte = trunc(255.0f * min(max(x, 0), 1)), one fp32 multiply
 * and a truncation, bit-equal to numpy's clip(0, 1) and (255 * a).astype(uint8).  out 4-byte aligned. */
int fv_frames_u8(const float* driving, const float* generated, int N, int H, int W, void* out, void* stream);
/* The way in: frames [T][H][W][3] uint8 -> out [T][3][H][W] fp32 = x * fp32(1 / 255), one rounded fp32
 * multiply (skimage's img_as_float32, data.u8_to_float).  32-bit loads when `frames` is 4-byte aligned. */
int fv_frames_from_u8(const void* frames, int T, int H, int W, float* out, void* stream);
/* transform_kp (utils.py:53-59) and the motion Jacobian in one launch, all fp32:
 * R [N][3][3] = Ry(pitch) Rx(yaw) Rz(roll) (the reference's naming of the axes), kp [N][K][3] =
 * R (scale kp_c) + t with kp_c [Nc][K][3], Nc 1 or N, scale [N], and, for a non-null Rs [Ns][3][3] (Ns 1
 * or N), J [N][3][3] = Rs inv(R), the inverse taken in closed form (adjugate over determinant).  Rs NULL:
 * J is not written (and may be NULL). */
int fv_pose_kp_fwd(const float* kp_c, const float* yaw, const float* pitch, const float* roll, const float* t,
                   const float* scale, const float* Rs, int N, int Nc, int Ns, int K, float* kp, float* R, float* J,
                   void* stream);
/* transform_kp_with_new_pose (utils.py:62-76): R = Ry(new_pitch) Rx(new_yaw) Rz(new_roll), kp [N][K][3] =
 * R kp_in + t + (R inv(R_old)) delta, R_old from (yaw, pitch, roll), then z += 0.33 - mean(z) over all
 * N K keypoints of the call (one block, one fixed-order sum).  kp_in and delta [N][K][3].  J as above.
 * N K <= 65536. */
int fv_pose_kp_new_fwd(const float* kp_in, const float* yaw, const float* pitch, const float* roll, const float* t,
                       const float* delta, const float* new_yaw, const float* new_pitch, const float* new_roll,
                       const float* Rs, int N, int Ns, int K, float* kp, float* R, float* J, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FACEVAE_H */
