/*
 * vaegan_hip.h -- C ABI of the MI355X (gfx950) VAE-GAN training-path kernels.
 *
 * Drop-in boundary: the reference has no FFI layer -- its hot path is
 * the nn.Module / Optimizer API used by vaegan_code.py:65-135, and every FLOP executes inside
 * third-party ATen kernels.  This library replaces those ATen kernels.  Each entry point
 * below names the reference call site(s) it serves.  Plain pointers + sizes only; all
 * pointers are DEVICE pointers unless stated; every call is asynchronous on `stream`
 * (a hipStream_t passed as void*) and performs no allocation and no host synchronisation,
 * so call sequences can be captured into a hipGraph.
 *
 * Return value: 0 on success, a negative VG_E* code for rejected arguments (shape/alignment
 * checks are done on the host BEFORE launch), or a positive hipError_t from the launch.
 *
 * Internal activation layout: NHWC ("pixel-major"), channel count padded to a multiple of
 * 16 bytes (pad channels are zero).  dtype: VG_F32 (exact f32 MFMA, the parity path) or
 * VG_BF16 (bf16 storage, f32 accumulate).  Parameters/gradients/optimizer state are f32 in
 * the reference layouts (OIHW / [Cin][Cout][kh][kw]); `vg_pack_weights` produces the
 * K-major operand copies the GEMM kernels read.
 */
#ifndef VAEGAN_HIP_H
#define VAEGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VG_F32  0
#define VG_BF16 1
#define VG_FP8  2   /* OCP e4m3fn operands, f32 accumulate, bf16 output: vg_gather_gemm fprop only (BASELINE configs[4],
                     * a roofline run -- the reference has no fp8 semantics).  X: [..][IC] fp8, IC % 16 == 0; W: packed
                     * [nphase][N][Kp] fp8 holding weight * 2^VG_FP8_WSHIFT (N(0, 0.02) weights would sit in e4m3's
                     * subnormals); the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) undoes the shift through
                     * its E8M0 operand scale.  Y, bias, stats as for VG_BF16 (Y is bf16). */
#define VG_FP8_WSHIFT 6

#define VG_EINVAL   (-1)   /* bad shape / size / flag                                  */
#define VG_EALIGN   (-2)   /* pointer or channel count violates the 16-byte contract   */
#define VG_ENOSUP   (-3)   /* unsupported configuration                                */

#define VG_MAX_PHASE 4

/* Activation codes for the fused BN/activation kernels. */
#define VG_ACT_NONE    0
#define VG_ACT_RELU    1   /* nn.ReLU(True)          gan_code.py:23-43            */
#define VG_ACT_LRELU   2   /* nn.LeakyReLU(slope)    main_vae.py:25, gan_code.py:62-82 */
#define VG_ACT_TANH    3   /* nn.Tanh()              gan_code.py:50 (vg_tnconv epilogue only) */

#define VG_ABI_VERSION 31  /* 2: vg_pack_desc.tile_start, SyncBN / WGAN / data-path entry points; 3: in-kernel noise (vg_*_rng);
                             4: vg_bn_finalize_act_forward, vg_bn_backward_finalize_apply;
                             7: vg_bce_pair_forward_backward;
                             8: vg_head_backward; round-3 prune -- the opt-in experiments of ABI 5 / 6 that measured slower (input prologue of
                                vg_tn_desc / vg_ew_desc, vg_gg_desc.bnb_*) are gone from the descriptors; vg_reload_switches;
                             9: vg_step_prologue, vg_adam_step(lr < 0);
                             10 (round 4): vg_adam_apply replaces the lr < 0 overload of vg_adam_step (which now rejects it);
                             11: degraded-pair data path: vg_gather_degrade_u8, vg_degrade_params, vg_rand_u01;
                             12: latent prior: vg_latent_hist (+ _ws_bytes), vg_latent_sample, vg_to_u8;
                             13: Resize + CenterCrop on the device: vg_resize_u8 (+ _lds_bytes, _band);
                             14: feature-space metrics: vg_feat_stats_accum, vg_knn_radius2, vg_manifold_cover (+ _ws_bytes each);
                             15: KID: vg_kid_scores (+ _ws_bytes);
                             16: Discriminator-feature reconstruction loss: vg_feat_mse_forward_backward;
                             17: SSIM reconstruction loss: vg_ssim_loss_forward_backward (+ _ws_floats);
                             18: region-weighted MSE for degraded pairs: vg_region_mse_forward_backward (+ _ws_doubles);
                             19: vg_gather_gemm_plan / vg_gg_plan: the launcher's kernel choice as a host-only query;
                             20: vg_bn_launch_plan / vg_bn_plan: the BatchNorm launchers' geometry as a host-only query;
                             21: vg_gg_plan.timing_family / .ws_bytes: callers size their buffers from the plan record; the four
                                 side queries of vg_gather_gemm (slab count, timer family, tile rows, workspace bytes) and the
                                 "supported" query of vg_bn_finalize_act_forward (vg_bn_launch_plan(VG_BN_PLAN_FUSED).fused) are gone;
                             22: weight averaging: vg_ema_update;
                             23: vg_wgrad_plan / vg_wg_plan, vg_edge_wgrad_plan / vg_ew_plan replace vg_wgrad_ws_bytes / vg_edge_wgrad_ws_bytes;
                             24: gradient-norm clipping: vg_grad_norm_clip, vg_adam_apply_clip;
                             25: differentiable augmentation: vg_diffaug_params, vg_diffaug_forward, vg_diffaug_backward (+ _ws_floats);
                             26: learning-rate schedules and decoupled weight decay: vg_lr_sched, vg_step_prologue_sched, vg_adamw_apply;
                             27: vg_tnconv_plan / vg_tn_plan: the tiling vg_tnconv launches, as a host-only query;
                             28: Gaussian-mixture prior: vg_gmm_log_resp, vg_gmm_moments (+ _ws_bytes), vg_gmm_sample;
                             29: tiled denoising of images larger than the network: vg_tile_gather, vg_tile_blend;
                             30: k-means: vg_kmeans_assign, vg_kmeans_update (+ _ws_bytes), vg_kmeans_seed (+ _ws_bytes),
                                 vg_kmeans_plan / vg_km_plan;
                             31: decoded prior samples as the third Discriminator stream: vg_prior_forward (+ _rng),
                                 vg_head_backward_g, vg_nhwc_grad_tanh_to_nhwc;
                                 (added within 31, nothing changed) multi-scale SSIM loss: vg_msssim_loss_forward_backward
                                 (+ _ws_bytes); timing family 5;
                                 (added within 31, nothing changed) test-time latent refinement: vg_bn_act_backward_eval,
                                 vg_masked_mse_rows (+ _ws_doubles), vg_latent_adam / VG_LATENT_*;
                                 (added within 31, no version move, nothing changed) classical-denoiser baseline:
                                 vg_nlm_denoise, vg_noise_sigma;
                                 (added within 31, no version move, nothing changed) noise models of the degraded pairs and
                                 the median baseline: vg_gather_degrade_u8_ex, vg_degrade_params_ex / VG_NOISE_*,
                                 VG_DRAW_DEGRADE_IMPULSE / _SALT, vg_median_filter;
                                 (added within 31, no version move, nothing changed) spectral generation metric:
                                 vg_spectrum_profiles (+ _ws_bytes), vg_spectrum_accum */
int vg_abi_version(void);
/* The library reads its optional kernel-selection switches (VG_* environment variables, DESIGN.md "Runtime switches")
 * ONCE, when it is loaded; nothing on a launch path calls getenv.  A process that changes one of them afterwards
 * (tests, A/B scripts) calls this to have them read again.  Returns 0. */
int vg_reload_switches(void);
/* Live kernel timing for the roofline report: while enabled, gather-GEMM (family 0) and wgrad (family 1)
 * launches carry a HIP start/stop event pair on their stream (hipExtLaunchKernelGGL); collect() synchronises,
 * sums the kernel times in ms, returns the launch count and resets the family.  Do not enable during capture.
 * Further families: 2 edge layers, 3 fp8 gather-GEMM, 4 BatchNorm / activation passes, 5 every launch of the multi-scale
 * SSIM loss (csrc/msssim.hip).  VG_EINVAL for a family outside 0 .. 5. */
int vg_timing_enable(int on);
/* Kernel launches issued by this library since it was loaded (every hipLaunchKernelGGL / hipExtLaunchKernelGGL of csrc/;
 * memsets and copies are runtime calls, not counted).  bench.py: launches per training iteration. */
uint64_t vg_launch_count(void);
int vg_timing_collect(int family, double* total_ms /* host */, int* launches /* host */);
/* Which tile configuration the launcher would pick (for tests / bench reporting). */
const char* vg_build_info(void);

/* ------------------------------------------------------------------------------------------
 * Gather-GEMM: the one implicit-GEMM kernel behind
 *   nn.Conv2d forward            (main_vae.py:23, gan_code.py:61-84)
 *   nn.ConvTranspose2d forward   (gan_code.py:21-49)  -- 4-phase sub-pixel form for k4 s2 p1
 *   their data gradients (autograd convolution_backward dgrad of vaegan_code.py:104,133)
 *   nn.Linear forward / dgrad    (main_vae.py:47-48, 55-56) -- as a full-extent convolution
 *
 *   Y[b, gy*OSY+ooy[p], gx*OSX+oox[p], n] = bias[n] +
 *        sum_{a<TH, c<TW, ci<IC} X[b, gy*SY + y0[p] + DY*a, gx*SX + x0[p] + DX*c, ci]
 *                                 * W[p][n][(a*TW + c)*IC + ci]
 *   for p < nphase, b < B, gy < GH, gx < GW, n < N; out-of-range input pixels read as 0,
 *   out-of-range output pixels are skipped.  Optionally emits per-channel partial
 *   (sum y, sum y*y) slabs for train-mode BatchNorm (nn.BatchNorm2d, main_vae.py:24).
 * ---------------------------------------------------------------------------------------- */
typedef struct vg_gg_desc {
    const void* X;        /* [B][IH][IW][IC]                                   */
    const void* W;        /* packed [nphase][N][Kp] (Kp = padded TH*TW*IC)     */
    void*       Y;        /* [B][OH][OW][OC]                                   */
    const float* bias;    /* [N] or NULL                                       */
    float*      stats;    /* partial slabs [nparts][2][N] or NULL              */
    int32_t B, GH, GW;
    int32_t IH, IW, IC;
    int32_t SY, SX, DY, DX, TH, TW;
    int32_t y0[VG_MAX_PHASE], x0[VG_MAX_PHASE];
    int32_t N, Kp;
    int32_t OH, OW, OC, OSY, OSX;
    int32_t ooy[VG_MAX_PHASE], oox[VG_MAX_PHASE];
    int32_t nphase;
    int32_t stats_capacity;   /* number of [2][N] slabs `stats` can hold       */
    float*  ws;               /* optional split-K workspace (f32 partial tiles) */
    int64_t ws_bytes;
    const void* zeros;        /* >= 64 zero bytes, 16-byte aligned: source of out-of-image taps on the LDS-DMA path
                                 (NULL selects the register-staged path)       */
    int32_t act;              /* VG_ACT_*: activation applied in the epilogue (layers WITHOUT BatchNorm, e.g. the
                                 Discriminator's first Conv2d + LeakyReLU(0.2), gan_code.py:61-62); not with `stats` */
    float   act_slope;
    /* Fused activation BACKWARD of the layer below (optional; a data-gradient launch whose output Y is
     * dL/d(activated output) of a BatchNorm-less layer): Y is multiplied by act'(mask_x) on its way out, mask_x being
     * that layer's (activated) output in the same [B][OH][OW][OC] layout -- saves the separate vg_act_backward pass. */
    const void* mask_x;
    int32_t mask_act;
    float   mask_slope;
} vg_gg_desc;

/* Skinny problems -- few output tiles but a long K, e.g. the data gradient of the 1x1-input ConvTranspose2d (M=B,
 * K=16*1024) -- are split along K over gridDim.z where d->ws holds vg_gg_plan.ws_bytes; the f32 partial tiles are summed
 * in fixed order by a second kernel.  d->stats needs room for vg_gg_plan.nparts slabs (stats_capacity). */
int vg_gather_gemm(const vg_gg_desc* d, int dtype, void* stream);

/* What vg_gather_gemm launches for a descriptor under the current switches (host-only query; needs no GPU).  The launcher
 * builds this same record and launches from it, so the query cannot drift from the launch.  Pointers of the descriptor are
 * only tested against NULL / for alignment (bias, stats, ws + ws_bytes, zeros and mask_x all take part in the choice), so a
 * caller asks BEFORE it allocates: with any non-NULL placeholder for `stats`, and one for `ws` with ws_bytes "enough" (e.g.
 * 1 << 62), the record is exactly the plan of the launch that then passes nparts slabs and a workspace of ws_bytes. */
#define VG_GG_GENERIC  0   /* gg_kernel  (conv_gemm.hip): bm x bn tile, one phase per workgroup                              */
#define VG_GG_NARROWK  1   /* ggn_kernel (conv_narrowk.hpp): 3-channel input; detail = { NT = N / 16, KC = Kp / 32 }         */
#define VG_GG_PHASE4   2   /* ggq_kernel (conv_phase4.hpp): four phases per workgroup; detail = { NR: patch DMA rounds, 0 }  */
#define VG_GG_PATCH    3   /* ggp_kernel (conv_patch.hpp): input patch in LDS; detail = { NR: patch DMA rounds, NR_ argument } */
#define VG_GG_REDUCE_NONE  0
#define VG_GG_REDUCE_FLAT  1   /* splitk_reduce_kernel: elementwise over a flat output, no statistics */
#define VG_GG_REDUCE_TILE  2   /* splitk_reduce2_kernel: per tile, with phases / statistics           */
typedef struct vg_gg_plan {
    int32_t family;            /* VG_GG_*                                                                              */
    int32_t bm, bn;            /* output tile; one statistics slab covers bm rows                                      */
    int32_t detail[2];         /* the template arguments beyond the tile (see the family)                              */
    int32_t dma;               /* 1: operands staged by LDS-DMA (the ring of gg_kernel; always 1 for families 2, 3)    */
    int32_t ksplit;            /* K slices (1: K is not split)                                                         */
    int32_t stages_per_split;  /* main-loop stages per slice (0 when K is not split)                                   */
    int32_t nstages;           /* main-loop stages of the whole K (generic family; 0 otherwise): the last slice holds
                                  nstages - (ksplit - 1) * stages_per_split of them                                    */
    int32_t reduce;            /* VG_GG_REDUCE_*: the second launch of a split                                          */
    int32_t n_major;           /* 1: workgroups are dealt XCD-major over the n tiles                                   */
    int32_t nparts;            /* statistics slabs the launch writes (0 without d->stats)                              */
    int32_t timing_family;     /* vg_timing_* family of the launch: 0 gather-GEMM (MFMA-bound), 2 edge layer (family
                                  VG_GG_NARROWK: 3-channel image side, HBM-bound), 3 fp8 operands                      */
    int64_t ws_bytes;          /* split-K workspace the launch can use: what the split PLANNED for this descriptor needs,
                                  whether or not d->ws was passed (0: K is never split).  ksplit is that split where
                                  d->ws_bytes >= ws_bytes, 1 with a smaller (or no) workspace                          */
} vg_gg_plan;
int vg_gather_gemm_plan(const vg_gg_desc* d, int dtype, vg_gg_plan* out);

/* ------------------------------------------------------------------------------------------
 * Weight gradient (autograd convolution_backward wgrad; Linear weight grad):
 *   dW[np*s_np + cq*s_cq + (a*TW+c)*s_t] (+)= sum_{b,gy,gx}
 *        P[b, gy, gx, np] * Q[b, gy*SY + y0 + DY*a, gx*SX + x0 + DX*c, cq]
 * P is dense over the (GH,GW) grid, Q is gathered.  Conv2d: P=dY, Q=X; ConvTranspose2d:
 * P=X, Q=dY.  Output f32 in the reference parameter layout.  Deterministic: split-M partial
 * slabs in `ws` are reduced in fixed order.  accumulate!=0 adds into dW (autograd semantics
 * of two D passes summed into one .grad, vaegan_code.py:99-104).
 * ---------------------------------------------------------------------------------------- */
typedef struct vg_wg_desc {
    const void* P;        /* [B][GH][GW][PC]                                   */
    const void* Q;        /* [B][QH][QW][QC]                                   */
    float*      dW;       /* f32, reference layout                             */
    float*      ws;       /* workspace, ws_bytes                               */
    int64_t     ws_bytes;
    int32_t B, GH, GW, PC, NP;        /* NP real rows (<= PC)                   */
    int32_t QH, QW, QC, NQ;           /* NQ real channels (<= QC)               */
    int32_t SY, SX, DY, DX, TH, TW, y0, x0;
    int32_t s_np, s_cq, s_t;          /* element strides into dW               */
    int32_t accumulate;
    const void* zeros;                /* >= 64 zero bytes (16-byte aligned) for the LDS-DMA path; NULL = register path */
} vg_wg_desc;

int vg_wgrad(const vg_wg_desc* d, int dtype, void* stream);

/* What vg_wgrad launches for a descriptor under the current switches (host-only query; needs no GPU).  The launcher builds
 * this same record and launches from it, so the query cannot drift from the launch.  The query validates the geometry like
 * a launch; pointers of the descriptor are only tested against NULL / for alignment: `zeros` takes part in the choice of the
 * main kernel (NULL: register-staged) and the 16-byte alignment of `dW` in the choice of the reduce kernel (the streaming
 * one stores 16-byte vectors); P, Q and ws are not looked at.  So a caller asks BEFORE it allocates, with the zero page (or
 * any non-NULL placeholder) and dW (or a placeholder of its alignment), and passes a workspace of ws_bytes to the launch. */
#define VG_WG_MAIN_F32       0   /* wgrad_kernel<VG_F32>: 64 x 64 tile, 32-row stages                                       */
#define VG_WG_MAIN_BF16_REG  1   /* wgrad_bf16_kernel: 128 x 128 tile, operands staged through registers                    */
#define VG_WG_MAIN_BF16_DMA  2   /* wgrad_bf16_dma_kernel: 128 x 128 tile, LDS-DMA staging, one role per wave               */
#define VG_WG_MAIN_WS        3   /* wgrad_bf16_ws_kernel<nqt, nprod>: wave-specialised, 128 x (128 * nqt) per workgroup     */
#define VG_WG_RED_STREAM     0   /* wgrad_reduce_t_kernel: streaming transpose-reduce, one contiguous run of dW per block   */
#define VG_WG_RED_GENERIC    1   /* wgrad_reduce_kernel<reduce_tt, reduce_vc>                                               */
typedef struct vg_wg_plan {
    int32_t main;              /* VG_WG_MAIN_*                                                                          */
    int32_t nqt, nprod;        /* VG_WG_MAIN_WS: kq tiles per workgroup and producer waves (<1,8>, <2,4>, <2,8>); else 0 */
    int32_t tile;              /* output tile edge: 64 (f32) | 128 (bf16)                                               */
    int32_t tiles_kq, tiles_np;/* tiles over K = TH*TW*QC and over PC; the main grid is (tiles_kq / max(nqt, 1), tiles_np,
                                  nsplit)                                                                               */
    int32_t nsplit;            /* splits of the pixel rows M = B*GH*GW = slabs in the workspace                         */
    int32_t rows_per_split;    /* whole stages; the last split holds M - (nsplit - 1) * rows_per_split rows             */
    int32_t stage_rows;        /* pixel rows per main-loop stage                                                        */
    int32_t xcd_order;         /* 1: workgroups are dealt so that one XCD owns whole splits                             */
    int32_t reduce;            /* VG_WG_RED_*: the second launch                                                         */
    int32_t reduce_tt;         /* generic reduce: taps per thread, 4 | 16 (0 for the streaming one, as the next two)    */
    int32_t reduce_vc;         /*                 channels per thread, 1 | 4                                            */
    int32_t reduce_spl;        /*                 threads that share the slabs of one element, 1 | 8 | 32               */
    int64_t ws_bytes;          /* slab workspace the launch needs: nsplit * tiles_np * tiles_kq * tile * tile * 4       */
} vg_wg_plan;
int vg_wgrad_plan(const vg_wg_desc* d, int dtype, vg_wg_plan* out);

/* ------------------------------------------------------------------------------------------
 * Operand packing: f32 parameter tensor (reference layout) -> K-major GEMM operand
 *   dst[p][n][(a*TW+c)*IC + ci] = src[n*s_n + ci*s_c + kh(p,a)*KW + kw(p,c)]   (0 in padding)
 *   kh(p,a) = kh0[p] + kh_step*a,  kw(p,c) = kw0[p] + kw_step*c
 * tap_in_n != 0 selects the "taps are part of N" form used by the 1x1-input ConvTranspose2d
 * (gan_code.py:21): dst[(kh*KW+kw)*CO + co][ci] = src[ci*s_c + co*s_n + kh*KW+kw].
 * ---------------------------------------------------------------------------------------- */
typedef struct vg_pack_desc {
    const float* src;
    void*        dst;
    int32_t nphase, N, C, IC, TH, TW, Kp;
    int32_t s_n, s_c, KW;
    int32_t kh0[VG_MAX_PHASE], kw0[VG_MAX_PHASE], kh_step, kw_step;
    int32_t tap_in_n, KHW;          /* KHW = taps of the FULL kernel (KH*KW) */
    int32_t tile_start;             /* vg_pack_weights_multi only: first flat tile of this descriptor */
} vg_pack_desc;
int vg_pack_weights(const vg_pack_desc* d, int dtype, void* stream);
/* Same, for a whole network in one launch: `descs_dev` is an array of n <= 64 descriptors in DEVICE memory (their
 * src/dst pointers are stable: parameters live in the optimizer's flat buffer).  The launch is one workgroup
 * per tile: descriptor i must carry tile_start = sum of vg_pack_tile_count() of the descriptors before it, and
 * total_tiles is the sum over all of them. */
int vg_pack_tile_count(const vg_pack_desc* d);
int vg_pack_weights_multi(const vg_pack_desc* descs_dev, int n, int64_t total_tiles, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm (train / eval) + activation, NHWC rows = B*H*W, C channels (C % 4 == 0).
 * nn.BatchNorm2d semantics: biased batch variance for normalisation,
 * unbiased for running_var, running = (1-m)*running + m*batch, eps inside the sqrt.
 * ---------------------------------------------------------------------------------------- */
/* Reduce the conv epilogue's partial slabs -> mean/invstd, scale/shift; update running stats. */
int vg_bn_finalize(const float* stats, int nparts, int C, int64_t count,
                   const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps,
                   float* mean, float* invstd, float* scale, float* shift, void* stream);
/* The same two reductions for `groups` independent row blocks in ONE launch (a Discriminator iteration's real and
 * fake batches run as one 2B-row pass): slabs of group g start at stats + g*nparts_per_group*2*C; coeffs is
 * [groups][4][C] = mean, invstd, scale, shift; coef is [groups][3][C]; running statistics and dgamma/dbeta are
 * updated group after group, the order in which the reference's separate calls would update them. */
int vg_bn_finalize_grouped(const float* stats, int nparts_per_group, int groups, int C, int64_t count_per_group,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           float momentum, float eps, float* coeffs, void* stream);
/* vg_bn_finalize_grouped + vg_bn_act_forward in ONE launch, for small layers (bf16, <= 200 slab rows per group, tensor <= 9 MB,
 * C % 64 == 0): every workgroup of the elementwise pass re-derives the coefficients of its 64
 * channels from the slab (same double-precision sums, another order: coefficients may differ from vg_bn_finalize_grouped
 * in the last bit).  Writes coeffs [groups][4][C] and the running statistics like vg_bn_finalize_grouped.
 * vg_bn_launch_plan(VG_BN_PLAN_FUSED).fused says whether a shape qualifies (VG_BN_FUSED_FWD=0 turns the path off); the
 * launch returns VG_ENOSUP otherwise.  rows = all groups' rows; x, y: [rows][C] bf16. */
int vg_bn_finalize_act_forward(const void* x, void* y, const float* stats, int nparts_per_group, int groups, int C,
                               int64_t rows, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, float* coeffs, int act, float slope,
                               int dtype, void* stream);
/* Backward twin: vg_bn_backward_finalize_grouped + vg_bn_act_backward_apply in one launch, same eligibility
 * (the same plan with the column-reduce partial count as nparts_per_group); VG_ENOSUP otherwise. */
int vg_bn_backward_finalize_apply(const void* x, const void* dy, void* dx, const float* partial, int nparts_per_group,
                                  int groups, int C, int64_t rows, const float* gamma, const float* coeffs,
                                  float* dgamma, float* dbeta, int accumulate, int act, float slope, int dtype,
                                  void* stream);
int vg_bn_backward_finalize_grouped(const float* partial, int nparts_per_group, int groups, int C,
                                    int64_t count_per_group, const float* gamma, const float* coeffs,
                                    float* dgamma, float* dbeta, int accumulate, float* coef, void* stream);
/* Synchronised BatchNorm (statistics over the global batch of a one-process-per-GPU job).
 * The reference is single-process (vaegan_code.py:29-35), so "the batch" of nn.BatchNorm2d is the whole batch;
 * these three calls let N ranks reproduce that: vg_slab_sums -> host all-reduce(SUM) of the f64 [2][C] vector
 * -> vg_bn_finalize_sums with the GLOBAL count.  Backward: vg_bn_act_backward_reduce -> vg_slab_sums ->
 * all-reduce -> vg_bn_backward_finalize_sums (dgamma/dbeta from the LOCAL sums: the gradient all-reduce
 * averages them afterwards; dx coefficients from the GLOBAL sums). */
int vg_slab_sums(const float* slabs, int nparts, int C, double* sums, void* stream);
int vg_bn_finalize_sums(const double* sums, int C, int64_t count, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps,
                        float* mean, float* invstd, float* scale, float* shift, void* stream);
int vg_bn_backward_finalize_sums(const double* global_sums, const double* local_sums, int C, int64_t count,
                                 const float* gamma, const float* invstd, float* dgamma, float* dbeta,
                                 int accumulate, float* coef, void* stream);
/* Eval mode: scale/shift from running statistics. */
int vg_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int C,
                      float* scale, float* shift, void* stream);
/* y = act(scale[c]*x + shift[c]); scale/shift NULL -> pure activation.
 * groups > 1: the rows are `groups` equal, independent row blocks (e.g. the real and the fake batch of one
 * Discriminator iteration, vaegan_code.py:96-97, run as one launch) with their own coefficient sets:
 * group g reads scale[g*gstride + c] (same for shift / mean / invstd below). */
int vg_bn_act_forward(const void* x, void* y, const float* scale, const float* shift,
                      int64_t rows, int C, int act, float slope, int groups, int64_t gstride,
                      int dtype, void* stream);
/* Same, additionally writing y8 = e4m3(y) (same [rows][C] layout, one byte per element; VG_BF16 only): the operand of
 * the next layer's VG_FP8 forward GEMM, produced in the pass that produces the bf16 activation. */
int vg_bn_act_forward_fp8(const void* x, void* y, void* y8, const float* scale, const float* shift, int64_t rows,
                          int C, int act, float slope, int groups, int64_t gstride, int dtype, void* stream);
/* Standalone per-channel statistics of an NHWC tensor (used when no conv epilogue produced them). */
int vg_channel_stats(const void* x, int64_t rows, int C, float* stats, int stats_capacity,
                     int* nparts_out, int dtype, void* stream);
/* Backward pass 1: dz = dy_act * act'(z), z = scale*x+shift; partial sums of dz and dz*xhat.
 * With groups > 1 the slabs of group g are parts [g*nparts_out, (g+1)*nparts_out). */
int vg_bn_act_backward_reduce(const void* x, const void* dy, const float* scale, const float* shift,
                              const float* mean, const float* invstd,
                              int64_t rows, int C, int act, float slope,
                              float* partial, int partial_capacity, int* nparts_out,
                              int groups, int64_t gstride, int dtype, void* stream);
/* Backward finalize: dgamma, dbeta (accumulate optional) and the two per-channel coefficients. */
int vg_bn_backward_finalize(const float* partial, int nparts, int C, int64_t count,
                            const float* gamma, const float* invstd,
                            float* dgamma, float* dbeta, int accumulate,
                            float* coef /* [3][C]: a, b, c */, void* stream);
/* Backward pass 2: dx = a[c]*dz - b[c]*xhat - c[c]   (dz recomputed from dy, x); group g uses coef + g*cstride. */
int vg_bn_act_backward_apply(const void* x, const void* dy, void* dx,
                             const float* scale, const float* shift,
                             const float* mean, const float* invstd, const float* coef,
                             int64_t rows, int C, int act, float slope, int groups, int64_t gstride,
                             int64_t cstride, int dtype, void* stream);
/* What the BatchNorm launchers launch for a shape under the current switches (host-only query; needs no GPU).  Every
 * launcher builds this same record and launches from it, so the query cannot drift from the launch.
 *   VG_BN_PLAN_REDUCE   vg_channel_stats (one group) / vg_bn_act_backward_reduce: a "block" is one slab row (part)
 *   VG_BN_PLAN_FORWARD  vg_bn_act_forward(_fp8)
 *   VG_BN_PLAN_APPLY    vg_bn_act_backward_apply
 *   VG_BN_PLAN_FUSED    vg_bn_finalize_act_forward / vg_bn_backward_finalize_apply (needs nparts_per_group)
 * rows = all groups' rows.  aligned16: whether every tensor of the launch (and the e4m3 twin's 8 bytes) meets the
 * alignment that the 16-byte bf16 vectors need; the launchers test their pointers.  nparts_per_group: slab rows per
 * group, read by VG_BN_PLAN_FUSED only.  A shape the one-launch form refuses gives fused = 0 and no geometry. */
#define VG_BN_PLAN_REDUCE   0
#define VG_BN_PLAN_FORWARD  1
#define VG_BN_PLAN_APPLY    2
#define VG_BN_PLAN_FUSED    3
typedef struct vg_bn_plan {
    int32_t kind;              /* VG_BN_PLAN_*                                                                          */
    int32_t vec;               /* channels per thread: 4, or 8 (16-byte bf16 vectors)                                   */
    int32_t threads_per_row;   /* of a full column block; a ragged last column block has C / vec - (col_blocks - 1) *
                                  256 of them and its own 256 / that rows per pass                                      */
    int32_t rows_per_pass;     /* rows a workgroup covers at once; 256 % threads_per_row threads idle                   */
    int32_t rows_per_block;    /* rows a workgroup owns (the last one of a group may own fewer); reduce: rows per part  */
    int32_t blocks_per_group;  /* gridDim.x of the streaming passes; reduce: parts (slab rows) per group                */
    int32_t col_blocks;        /* gridDim.y: blocks of 256 threads' columns; fused: slices of 64 channels               */
    int32_t groups;            /* gridDim.z (reduce: gridDim.x = blocks_per_group * groups)                             */
    int32_t fused;             /* VG_BN_PLAN_FUSED: 1 when the one-launch form is taken, 0 when refused                 */
} vg_bn_plan;
int vg_bn_launch_plan(int kind, int64_t rows, int C, int groups, int dtype, int aligned16, int nparts_per_group,
                      vg_bn_plan* out);
/* Activation-only backward (first Discriminator layer has no BN, gan_code.py:61-62). */
int vg_act_backward(const void* x, const void* dy, void* dx, int64_t n, int act, float slope,
                    int dtype, void* stream);
/* dbias[c] (+)= sum over rows of dy[row][c]  (Conv2d bias grad, main_vae.py:23; Linear bias). */
int vg_bias_grad(const void* dy, int64_t rows, int C, int NC, float* dbias, int accumulate,
                 float* ws, int ws_capacity, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Edge layers (3-channel side at the image boundary; HBM-bound)
 * ---------------------------------------------------------------------------------------- */
/* Narrow-N transposed convolution, bf16:
 *     Y[b][oy][ox][n] = sum_{c,kh,kw} X[b][iy][ix][c] * W[c][n][kh][kw],  oy = iy*S - P + kh, ox = ix*S - P + kw
 * = nn.ConvTranspose2d(C, N, K, S, P).forward (the Generator's last layer, gan_code.py:49: C->3, k3 s1 p1) and the
 * data gradient of nn.Conv2d(N, C, K, S, P) (the image gradient below the Discriminator's first layer,
 * gan_code.py:61: 3->C, k4 s2 p1, reached by loss.backward() at vaegan_code.py:133).  N <= 4, K*K*N <= 64.
 * Computed as ONE GEMM per input pixel over the channels, Pm[pix][(kh,kw,n)] = X[pix][:] . Wp[(kh,kw,n)][:], followed
 * by the K*K-tap col2im sum inside the workgroup's LDS tile: every input byte is read once.
 * Wp: [K*K*N][Wpitch] bf16, row j = (kh*K + kw)*N + n, = vg_pack_weights with tap_in_n=1 of the [C][N][K][K]
 * (ConvTranspose2d) / [C][N][K][K]-viewed (Conv2d [Cout=C][Cin=N][K][K]) weight.
 * Outputs: Y NHWC bf16 [B][OH][OW][OC=8] (channels >= N zero) and/or Y_nchw f32 [B][N][OH][OW].
 * act = VG_ACT_TANH applies tanh (gan_code.py:50) to both; with noise (eps NCHW f32, or rng+draw: in-kernel
 * N(0,1)) Y becomes act(.) + sigma*noise while Y_nchw stays act(.) -- vaegan_code.py:83 and :92 in one pass. */
typedef struct vg_tn_desc {
    const void* X;          /* [B][IH][IW][C] bf16, C = 16, 32 or 64 */
    const void* Wp;
    void* Y;                /* or NULL */
    float* Y_nchw;          /* or NULL */
    const float* eps;       /* or NULL */
    const uint64_t* rng;    /* or NULL */
    int32_t draw;
    float sigma;
    int32_t B, IH, IW, C, N, K, S, P, OH, OW, OC, Wpitch, act;
} vg_tn_desc;
/* Weight gradient of the edge layers, bf16 operands, f32 result:
 *     dW[c*s_c + n*s_n + kh*K + kw] (+)= sum_{b,py,px} Wd[b][py][px][c] * Nr[b][py*S - P + kh][px*S - P + kw][n]
 * Wd: the WIDE operand [B][WH][WW][C] (C = 16 | 32 | 64): dY of nn.Conv2d(N, C, K, S, P) (gan_code.py:61, main_vae.py:23 --
 * then dW is the [C][N][K][K] weight gradient, s_c = N*K*K, s_n = K*K) or the input of nn.ConvTranspose2d(C, N, K, S, P)
 * (gan_code.py:49 -- dW is [C][N][K][K] as well).  Nr: the 3-channel tensor on the other side, [B][NH][NW][8] bf16 with
 * channels >= N zero (the image, or the image gradient).  N <= 3, K = 3 | 4, S = 1 | 2.
 * ws: vg_ew_plan.ws_bytes bytes of scratch (one [K*K*4 padded][C] f32 partial per workgroup, summed in fixed
 * order: bitwise reproducible).  zeros: >= 64 readable zero bytes. */
typedef struct vg_ew_desc {
    const void* Wd;
    const void* Nr;
    float* dW;
    float* ws;
    int64_t ws_bytes;
    const void* zeros;
    int32_t B, WH, WW, C, NH, NW, N, K, S, P, s_c, s_n, accumulate;
} vg_ew_desc;
int vg_edge_wgrad(const vg_ew_desc* d, void* stream);
/* What vg_edge_wgrad launches for a descriptor (host-only query; needs no GPU): the record the launcher builds and launches
 * from.  The query validates the geometry like a launch and looks at no pointer of the descriptor; a shape the kernel does
 * not take gives the launch's error code.  A workgroup walks tiles of rows_per_tile rows of the wide operand (all of one
 * image); the second launch sums the `grid` partials. */
typedef struct vg_ew_plan {
    int32_t ct;                /* edge_wgrad_kernel<ct>: tiles of 16 wide channels, C / 16 = 1 | 2 | 4                   */
    int32_t jt;                /* tiles of 16 (tap, narrow channel) rows: 3 (K = 3) | 4 (K = 4)                          */
    int32_t rows_per_tile;     /* R: rows of the wide operand per tile (<= 256 pixels, patch of the narrow one in LDS)   */
    int32_t tiles_per_img;     /* ceil(WH / R)                                                                           */
    int32_t ntiles;            /* B * tiles_per_img                                                                      */
    int32_t grid;              /* workgroups: min(ntiles, 512), each walks several tiles                                 */
    int64_t ws_bytes;          /* grid * jt * 16 * C * 4                                                                 */
} vg_ew_plan;
int vg_edge_wgrad_plan(const vg_ew_desc* d, vg_ew_plan* out);
int vg_tnconv_supported(const vg_tn_desc* d);     /* 0 if vg_tnconv takes this shape, else the error code */
int vg_tnconv(const vg_tn_desc* d, void* stream);
/* What vg_tnconv launches for a descriptor (host-only query; needs no GPU; ABI 27): the record the launcher builds and
 * launches from.  The query validates the geometry like a launch; of the descriptor's pointers it reads only whether rng
 * is NULL (in-kernel noise moves the column step of the tiling to 4) -- the NULL and alignment tests of X, Wp, Y and Y_nchw
 * belong to the launch.  A shape the kernel does not take gives the launch's error code.  One workgroup per tile of
 * ro x co output pixels; its input window is at most npix pixels, tc of them per row ((ro - 1 + K - 1) / S + 1 rows at most). */
typedef struct vg_tn_plan {
    int32_t nt;                /* tnconv_kernel<nt, kc, npix, K, S>: tiles of 16 (tap, n) columns, ceil(K*K*N / 16) = 1..4 */
    int32_t kc;                /* chunks of 32 input channels: 1 (C = 16 | 32) | 2 (C = 64)                                */
    int32_t npix;              /* input pixels of the LDS product tile: 512 (nt <= 2) | 256                                */
    int32_t tc;                /* input columns per window row, a multiple of 16; tc == IW: whole rows (then tiles_x == 1) */
    int32_t ro;                /* output rows per tile, a multiple of S (the last row tile may hold fewer)                 */
    int32_t co;                /* output columns per tile (the last column tile may hold fewer); whole rows: OW            */
    int32_t tiles_y;           /* ceil(OH / ro)                                                                            */
    int32_t tiles_x;           /* ceil(OW / co)                                                                            */
    int32_t grid;              /* workgroups: B * tiles_y * tiles_x                                                        */
    int32_t quad_noise;        /* rng set and OW % 4 == 0: tile columns start and end on multiples of 4, and a launch
                                  without eps draws its noise once per quad of lanes (else, with rng, once per element)  */
} vg_tn_plan;
int vg_tnconv_plan(const vg_tn_desc* d, vg_tn_plan* out);

/* ------------------------------------------------------------------------------------------
 * Layout / pointwise / losses
 * ---------------------------------------------------------------------------------------- */
/* NCHW f32 [B][C][H][W] -> NHWC dtype [B][H][W][CP] (pad channels zero); optional fused
 * instance noise out = x + sigma*eps (vaegan_code.py:91-92), eps NCHW f32 or NULL. */
int vg_nchw_to_nhwc(const float* x, const float* eps, float sigma, void* y,
                    int B, int C, int H, int W, int CP, int dtype, void* stream);
/* Data path (dataset_code.py:137-178): the whole image set lives in HBM as u8 [N][H][W][C] (CelebA-HQ 256x256:
 * 5.9 GB of the 288 GB); a batch is assembled on the device from the sampler's indices with ToTensor +
 * Normalize((0.5,),(0.5,)) arithmetic (dataset_code.py:147-150): out[b][c][h][w] = (u/255 - 0.5)/0.5, f32 NCHW. */
int vg_gather_normalize_u8(const uint8_t* images, int64_t N, const int64_t* idx, int B, int C, int H, int W,
                           float* out, void* stream);
/* Denoise-evaluation input (vaegan_code.py:153-154): noisy = clamp(x + sigma*eps, lo, hi), written both as the
 * NHWC engine tensor and (optionally, y_nchw != NULL) as NCHW f32 for the caller. */
int vg_noisy_clamp_to_nhwc(const float* x, const float* eps, float sigma, float lo, float hi, void* y,
                           float* y_nchw, int B, int C, int H, int W, int CP, int dtype, void* stream);
/* NHWC dtype -> NCHW f32, optional tanh (gan_code.py:50). */
int vg_nhwc_to_nchw(const void* x, float* y, int B, int C, int H, int W, int CP,
                    int apply_tanh, int dtype, void* stream);
/* The Generator's output in one pass (vaegan_code.py:83,92): y_nchw = tanh(x) (NCHW f32) and
 * y_noisy_nhwc = tanh(x) + sigma*eps (NHWC dtype, padded channels 0), eps NCHW f32. */
int vg_nhwc_tanh_to_nchw_noisy(const void* x, float* y_nchw, const float* eps, float sigma, void* y_noisy_nhwc,
                               int B, int C, int H, int W, int CP, int dtype, void* stream);
/* Gradient of the above: dy NCHW f32 -> dx NHWC dtype, optionally * (1 - t*t) with t = tanh output (NCHW f32). */
int vg_nchw_grad_to_nhwc(const float* dy, const float* tanh_out, void* dx,
                         int B, int C, int H, int W, int CP, int dtype, void* stream);
/* Same with a second gradient branch that already sits in the engine layout: dx = (dy + add_nhwc) * (1 - t*t).
 * vaegan_code.py:117,133: the reconstruction's gradient is d(MSE)/d(recon) (NCHW f32) plus the Discriminator's
 * input gradient through the instance-noise add (NHWC) -- one pass instead of layout change + add + layout change. */
int vg_nchw_grad_add_to_nhwc(const float* dy, const void* add_nhwc, const float* tanh_out, void* dx,
                             int B, int C, int H, int W, int CP, int dtype, void* stream);
/* The tail backward of a Generator output that has no MSE branch (ABI 31; the decoded prior samples, DESIGN.md section
 * 4.4o): dx = add_nhwc * (1 - t*t), t the NCHW f32 Tanh output, add_nhwc / dx in the engine layout, pad channels of dx
 * zero.  Bit-identical in value to vg_nchw_grad_add_to_nhwc on dy == 0 (a zero may differ in sign) without reading a zero
 * tensor: H * W % 4 == 0 and a 16-byte aligned t take four pixels per thread (16-byte loads of t), anything else one pixel
 * per thread.  VG_EINVAL: a NULL pointer, a size <= 0, CP < C; VG_EALIGN: CP % 4 != 0 or add_nhwc / dx not 16-byte
 * aligned; VG_ENOSUP: an unknown dtype. */
int vg_nhwc_grad_tanh_to_nhwc(const void* add_nhwc, const float* tanh_out, void* dx,
                              int B, int C, int H, int W, int CP, int dtype, void* stream);
/* Reparameterisation (vaegan_code.py:75-77): lv=clamp(logvar,-10,10); z=mu+exp(.5 lv)*eps.
 * mulv: [B][MP] dtype, the fused fc_mu|fc_logvar output (main_vae.py:55-56): columns [0,L) = mu,
 * [L,2L) = logvar.  eps: [B][L] f32.  z: [B][ZP] dtype (pad = 0).  lv_clamped: [B][L] f32. */
int vg_reparam_forward(const void* mulv, const float* eps, void* z, float* lv_clamped,
                       int B, int L, int MP, int ZP, int dtype, void* stream);
/* The prior latent in the Generator's input layout (ABI 31): z [B][ZP] dtype = eps [B][L] f32, pad
 * columns zero -- vg_reparam_forward on mu = 0, logvar = 0 bit for bit (f32 exact, bf16 round-to-nearest-even), without the
 * mulv and lv_clamped tensors.  One 16 / 8-byte store per four columns.  VG_EINVAL: a NULL pointer, B or L <= 0, ZP < L;
 * VG_EALIGN: ZP % 4 != 0 or z not 16-byte aligned; VG_ENOSUP: an unknown dtype or B * ZP >= 2^31. */
int vg_prior_forward(const float* eps, void* z, int B, int L, int ZP, int dtype, void* stream);
/* KL (vaegan_code.py:114): out[0] = -0.5*sum(1+lv-mu^2-exp(lv)) / divisor. */
int vg_kl_forward(const void* mulv, const float* lv_clamped, int B, int L, int MP, float divisor,
                  float* out, int dtype, void* stream);
/* d(mu|logvar) [B][MP] dtype from dz [B][ZP] dtype and kl_scale = alpha_kl*min(1,epoch/50)/B
 * (vaegan_code.py:114,117); the clamp passes gradient on [-10,10] only. */
int vg_reparam_kl_backward(const void* mulv, const float* lv_clamped, const float* eps,
                           const void* dz, float kl_scale, void* dmulv,
                           int B, int L, int MP, int ZP, int dtype, void* stream);
/* Discriminator head (gan_code.py:84-85,89): p[b] = sigmoid(dot(x[b,:], w)), x NHWC-flattened. */
int vg_dot_sigmoid_forward(const void* x, const void* w, float* p, int B, int K, int dtype, void* stream);
/* dlogit[b] = dp[b]*p*(1-p); dx[b,k] = dlogit[b]*w[k]  (dx NULL -> skipped). */
int vg_dot_sigmoid_backward(const float* p, const float* dp, const void* w, void* dx, float* dlogit,
                            int B, int K, int dtype, void* stream);
/* dw[k] (+)= sum_b dlogit[b]*x[b,k] -> f32 in reference layout via perm (k_nhwc -> offset). */
int vg_dot_wgrad(const void* x, const float* dlogit, float* dw, int B, int K, int C, int HW,
                 int accumulate, int dtype, void* stream);
/* nn.BCELoss (vaegan_code.py:46): mean_b -(t*max(log p,-100)+(1-t)*max(log(1-p),-100));
 * loss[0] (+)= value when accumulate; dp[b] = gscale*(p-t)/max(p*(1-p),1e-12)/B (dp NULL ok). */
int vg_bce_forward_backward(const float* p, float target, int B, float gscale,
                            float* loss, int accumulate, float* dp, void* stream);
/* The Discriminator loss of one update, both halves in one launch (vaegan_code.py:98-103; ABI 7): p = [B real | B fake],
 * loss[0] (+)= BCE(p[:B], target0) + BCE(p[B:], target1), dp likewise [2B] -- bit-identical to two vg_bce_forward_backward
 * calls, the second accumulating. */
int vg_bce_pair_forward_backward(const float* p, float target0, float target1, int B, float gscale,
                                 float* loss, int accumulate, float* dp, void* stream);
/* Backward of BCE(sigmoid(head)) in ONE launch (round 3; vaegan_code.py:99-104 and :115,133 behind the Discriminator's last
 * Conv2d, gan_code.py:84-85): for p = [B rows with target0 | B rows with target1] (groups = 2) or B rows with target0
 * (groups = 1):  loss[0] (+)= sum of the groups' BCE means;  dlogit[r] = gscale * (p - t) / max(p (1 - p), 1e-12) / B * p (1 - p);
 * dx[r,k] = dlogit[r] * w[k] (dx NULL: skipped);  dw[k] (+)= sum_r dlogit[r] * x[r,k] in the reference layout (dw NULL:
 * skipped);  dlogit optional output.  Bit-identical to vg_bce[_pair]_forward_backward + vg_dot_sigmoid_backward +
 * vg_dot_wgrad (same arithmetic, lane mappings and summation orders).  B * groups <= 4096, K % 4 == 0. */
int vg_head_backward(const float* p, const void* x, const void* w, void* dx, float* dw, float* dlogit, int B, int groups,
                     float target0, float target1, float gscale, float* loss, int accumulate_loss, int accumulate_dw,
                     int K, int C, int HW, int dtype, void* stream);
/* vg_head_backward for groups in 1..3 with one target per group (ABI 31; the Discriminator update of the prior stream,
 * p = [B real | B reconstructed | B decoded prior samples]): rows [g B, (g + 1) B) are held against
 * target<g>; targets of groups that do not exist are ignored.  loss[0] (+)= the sum of the groups' BCE means, added in group
 * order; dlogit, dx and dw as documented for vg_head_backward.  Bit-identical to `groups` calls of vg_bce_forward_backward
 * (the later ones accumulating) followed by vg_dot_sigmoid_backward and vg_dot_wgrad over all groups * B rows; for
 * groups <= 2 bit-identical to vg_head_backward, which forwards to it.  VG_EINVAL: a NULL p / x / w / loss, B <= 0, groups
 * outside 1..3, C * HW != K; VG_EALIGN: K % 4 != 0; VG_ENOSUP: B * groups > 4096 or an unknown dtype. */
int vg_head_backward_g(const float* p, const void* x, const void* w, void* dx, float* dw, float* dlogit, int B, int groups,
                       float target0, float target1, float target2, float gscale, float* loss, int accumulate_loss,
                       int accumulate_dw, int K, int C, int HW, int dtype, void* stream);
/* Sibling loop train_wgan (gan_code.py:306-315, :328): loss[0] (+)= sign*mean_b p[b]; dp[b] = sign*gscale/B. */
int vg_mean_forward_backward(const float* p, float sign, int B, float gscale,
                             float* loss, int accumulate, float* dp, void* stream);
/* WGAN weight clipping `p.data.clamp_(-c, c)` (gan_code.py:320-321) over a flat parameter buffer. */
int vg_clamp(float* p, int64_t n, float lo, float hi, void* stream);
/* nn.MSELoss(mean) (vaegan_code.py:47) on NCHW f32 tensors; d_a = gscale*2*(a-b)/n (NULL ok). */
int vg_mse_forward_backward(const float* a, const float* b, int64_t n, float gscale,
                            float* loss, float* d_a, float* ws, int ws_capacity, void* stream);
/* Discriminator-feature reconstruction loss (Larsen et al. 2016, eq. 2; ABI 16; csrc/featloss.hip) on two flat engine-layout
 * activations of `dtype` (VG_F32 / VG_BF16), f_real being a constant:
 *   loss[0] (+)= (1/n) sum_i (a_i - b_i)^2                  (accumulate_loss != 0: added to what the slot holds)
 *   d_inout[i] = round_dtype(float(d_inout[i]) + f32(gscale 2 / n) (a_i - b_i))   (d_inout NULL: loss only)
 * i.e. the loss gradient is ADDED onto the gradient already standing in d_inout, in the pass that reads a and b; f32
 * arithmetic, one rounding on the store.  Two launches (partials + gradient; one wave for the final sum), fixed summation
 * order, no atomics, capturable.  ws: ws_capacity f32 partial sums (1024 are used at most).  Pointers 16-byte aligned
 * (VG_EALIGN).  Padded channel rows are the caller's business: pass only activations without padding. */
int vg_feat_mse_forward_backward(const void* f_fake, const void* f_real, void* d_inout, int64_t n, float gscale, float* loss,
                                 int accumulate_loss, float* ws, int ws_capacity, int dtype, void* stream);
/* SSIM reconstruction loss (ABI 17; csrc/ssimloss.hip): the contract of vg_ssim below made differentiable.  a (reconstruction)
 * and b (target, a constant) are NCHW f32 in [-1, 1], u = (a + 1) / 2, v = (b + 1) / 2; g = the normalised 11-tap Gaussian
 * (sigma 1.5), w = g (x) g; over the interior pixels p in [5, H - 5) x [5, W - 5) (what the metric keeps after its crop; no
 * padding is ever read), with c1 = 1e-4, c2 = 9e-4:
 *   mu_u = sum w u, mu_v = sum w v, s_uu = sum w u^2 - mu_u^2, s_vv likewise, s_uv = sum w u v - mu_u mu_v
 *   S = (2 mu_u mu_v + c1)(2 s_uv + c2) / ((mu_u^2 + mu_v^2 + c1)(s_uu + s_vv + c2))
 *   loss[0] (+)= 1 - (1 / n) sum_p S(p),  n = B C (H - 10)(W - 10)      (accumulate_loss != 0: added to what the slot holds)
 *   d[q] += gscale * d(1 - mean S) / d a[q]     for every pixel q of the H x W plane            (d NULL: forward only)
 * i.e. the loss gradient is ADDED onto the gradient already standing in d (same shape as a).  Two launches (tiles: forward
 * and backward, one read-modify-write of d per element by its one owner; one wave for the final sum), fixed summation
 * order, no atomics, capturable.  ws: vg_ssim_loss_ws_floats(B, C, H, W) f32 partial sums (one per 32 x 32 tile of every
 * plane); ws_capacity in floats.  VG_EINVAL: a, b or loss NULL, B or C < 1, H or W < 11, ws NULL or too small.  No alignment
 * beyond that of a float is required. */
int vg_ssim_loss_forward_backward(const float* a, const float* b, float* d, int B, int C, int H, int W, float gscale,
                                  float* loss, int accumulate_loss, float* ws, int ws_capacity, void* stream);
int64_t vg_ssim_loss_ws_floats(int B, int C, int H, int W);      /* VG_EINVAL (negative) for sizes outside the contract */
/* Multi-scale SSIM reconstruction loss (csrc/msssim.hip; an addition within ABI 31): the maps of the SSIM loss above over a
 * 2x pyramid (Wang, Simoncelli & Bovik 2003).  a (reconstruction) and b (target, a constant): NCHW f32 [B][C][H][W] in
 * [-1, 1]; M scales, 1 <= M <= 5, with weights w_0 .. w_{M-1} (host memory, read at call time, each finite and > 0).
 *   Pyramid: a_0 = a, b_0 = b; level j + 1 is the 2 x 2 mean of level j, stride 2, no padding: H_{j+1} = floor(H_j / 2),
 *     W_{j+1} = floor(W_j / 2), a trailing odd row / column is dropped (F.avg_pool2d(x, 2)); f32: ((x00 + x01) + (x10 + x11))
 *     * 0.25f, every level rounded to f32 and the next formed from the rounded one.  Every level needs H_j, W_j >= 11.
 *   Per level, on u = (a_j + 1) / 2, v = (b_j + 1) / 2 over the interior [5, H_j - 5) x [5, W_j - 5), with the Gaussian, c1, c2,
 *     A1, A2, B1, B2 of the block above:  cs = A2 / B2,  S = (A1 / B1)(A2 / B2).  No padding is ever read.
 *   m_{b,j} = mean of cs (j < M - 1) or of S (j = M - 1) over the channels and interior pixels of IMAGE b at level j (per image,
 *     not per channel), n_j = C (H_j - 10)(W_j - 10).
 *   P_b = prod_j m_{b,j}^{w_j} if every m_{b,j} > 0, else 0 (the "relu" normalisation);
 *   loss[0] (+)= 1 - (1 / B) sum_b P_b                               (accumulate_loss != 0: added to what the slot holds)
 *   k_{b,j} = w_j P_b / (m_{b,j} B n_j) if every m_{b,.} > 0, else 0: an image on the clamp contributes the value 0 and a
 *     gradient of exactly 0; no NaN or Inf comes out of 0^(w - 1).
 *   g_j = -k_{b,j} d(sum_p map_j(p)) / d a_j over every pixel of the level-j plane (the closed form of the block above; for
 *     the cs levels Du = -cs / B2, Dc = 2 / B2, Dm = -2 mu_u Du - mu_v Dc);
 *   d[q] += gscale sum_j 4^-j g_j[q >> j]   over the levels whose plane contains q >> j: the adjoint of the floor-pooling
 *     chain; base pixels in dropped trailing rows / columns get no coarse contribution.             (d NULL: forward only)
 * Maps in f32 with one constant per 32 x 32 tile and input subtracted before the moments at every level (as ssimloss.hip);
 * per-image sums, P_b and k in f64, summed in a fixed order.  No atomics: the same inputs give the same bits, run to run and
 * eagerly vs. replayed from a graph; no host synchronisation.  Identical images give m = 1 exactly at every level, loss 0.
 * Launches: pyramid (M > 1), forward tiles of all levels, finalize, and with d backward tiles of all levels and the collapse
 * onto d: 3 without and 5 with the gradient (2 and 4 at M = 1), whatever M.
 * per_scale: f32 [B][M] receives the m_{b,j}; NULL skips it.  ws: vg_msssim_ws_bytes(B, C, H, W, M) bytes (pyramids of a, b
 * and of the gradient, tile partials, coefficients), 8-byte aligned (VG_EALIGN).  VG_EINVAL: a, b, loss or weights_host NULL,
 * B or C < 1, M outside 1 .. 5, a level under 11 x 11, a weight <= 0 or not finite, ws NULL or too small. */
int vg_msssim_loss_forward_backward(const float* a, const float* b, float* d, int B, int C, int H, int W, int M,
                                    const float* weights_host, float gscale, float* loss, int accumulate_loss,
                                    float* per_scale, void* ws, int64_t ws_bytes, void* stream);
int64_t vg_msssim_ws_bytes(int B, int C, int H, int W, int M);   /* VG_EINVAL (negative) for sizes outside the contract */
/* Region-weighted reconstruction MSE (ABI 18; csrc/regionloss.hip): the pixel MSE of a reconstruction a against the clean
 * image b (a constant), both NCHW f32 [B][C][H][W], split by each image's occlusion rectangle, for training on and evaluating
 * degraded pairs.  rects: f32 [B][8] in the layout vg_degrade_params writes; entries 2..5 = {rect_h, rect_w, x, y} are read;
 * NULL: no image has a hole.  Pixel (h, w) of image i is in the hole iff y <= h < y + rect_h and x <= w < x + rect_w, in every
 * channel; the comparisons are made in f32 (y + rect_h and x + rect_w are f32 sums).  rect_h == 0 or rect_w == 0: an empty
 * hole; a rectangle reaching past the image is clipped by it; a NaN entry makes every comparison false (no hole).  The
 * rectangle enters comparisons only: no address is formed from it, no content of rects can cause an out-of-range access.
 * Arithmetic: d = a - b in f32, q = d d in f32, q accumulated in f64 into S_hole and S_valid; with n = B C H W:
 *   loss[0]     = (float)((S_valid + (double)w_hole S_hole) / n)                 written, not accumulated; NULL skips it
 *   hole_mse[0] = (float)(S_hole / n_hole), 0 when n_hole == 0                   NULL skips it
 *   d_a[e]      = d * coef_region, coef_valid = (float)(2 (double)gscale / n),
 *                 coef_hole = (float)(2 (double)gscale (double)w_hole / n)       written in full; NULL skips the gradient
 *   stats[0..3] += {S_hole, S_valid, n_hole, n_valid}                            f64, ALWAYS accumulated (an evaluation pass
 *                 keeps one f64[4] for a whole epoch); n_hole is the exact count of hole elements after clipping; NULL skips it
 * Two launches (per-workgroup f64 partials of the two sums and the count in ws; one wave for the final pass), fixed summation
 * order, no atomics: the same inputs give the same bits, eagerly and replayed from a graph.  16-byte loads along W with a
 * per-lane mask where W % 4 == 0 and the pointers are 16-byte aligned, one element per lane otherwise.  ws: at least
 * vg_region_mse_ws_doubles(B, C, H, W) doubles; ws_doubles is its capacity.  VG_EINVAL: a or b NULL, a size < 1, w_hole < 0 or
 * not finite, ws NULL or too small, every output NULL.  VG_EALIGN: rects not 8-byte aligned (its rows are read as 8-byte
 * pairs).  HBM-bound: 12 B per element with the gradient, 8 B without. */
int vg_region_mse_forward_backward(const float* a, const float* b, const float* rects, int B, int C, int H, int W,
                                   float w_hole, float gscale, float* loss, float* hole_mse, float* d_a, double* stats,
                                   double* ws, int ws_doubles, void* stream);
int vg_region_mse_ws_doubles(int B, int C, int H, int W);        /* <= 0 (VG_EINVAL) for B, C, H or W < 1 */
/* ------------------------------------------------------------------------------------------
 * Test-time latent refinement (csrc/refine.hip; additions within ABI 31): descend on the latent z of
 * frozen, eval-mode networks so that G(z) matches a degraded input outside its occlusion rectangle (GAN-inversion inpainting,
 * Yeh et al. 2017).  The reference never differentiates an eval-mode network; these are the three launches that the forward
 * and data-gradient chains above lack for it.
 * ---------------------------------------------------------------------------------------- */
/* Backward of y = act(scale[c] x + shift[c]) with CONSTANT coefficients -- the eval-mode BatchNorm that vg_bn_eval_coeffs feeds
 * to vg_bn_act_forward (groups = 1):  dx = dy act'(z) scale[c],  z = fmaf(scale[c], x, shift[c]) in f32, the expression of
 * vg_bn_act_forward, so the activation mask agrees with the forward pass bit for bit; act' as in vg_bn_act_backward_reduce:
 * ReLU passes dy where z > 0 and 0 elsewhere (z == 0 and a NaN z included), LeakyReLU passes dy where z > 0 and dy * slope
 * elsewhere, VG_ACT_NONE passes dy.  Every product is an f32 product; the result is rounded once to the storage type.
 * x, dy, dx: [rows][C] in dtype (VG_F32 | VG_BF16), C the padded channel count; dx may alias dy.  One streaming launch with the
 * thread -> (row, channel column) mapping of vg_bn_act_backward_apply: 16-byte vectors (4 f32; 8 bf16 where C % 8 == 0 and x,
 * dy, dx are 16-byte aligned), else 8-byte vectors of 4 bf16; a ragged last block of 256 columns.  Three tensor-sized streams
 * (12 B per element f32, 6 B bf16), HBM-bound; timing family 4.  VG_EINVAL: a NULL pointer, rows or C < 1, an activation
 * other than NONE / RELU / LRELU; VG_ENOSUP: an unknown dtype; VG_EALIGN: C % 4 != 0, x / dy / dx not aligned to the narrowest
 * vector (16 bytes f32, 8 bytes bf16), scale / shift not 16-byte aligned.  All checked before the launch. */
int vg_bn_act_backward_eval(const void* x, const void* dy, void* dx, const float* scale, const float* shift, int64_t rows,
                            int C, int act, float slope, int dtype, void* stream);
/* Per-image context loss: the mean squared error of a against b (a constant), both NCHW f32 [B][C][H][W], over the elements
 * OUTSIDE image i's occlusion rectangle, one value per image, and its gradient.  rects and the hole rule are those of
 * vg_region_mse_forward_backward, word for word: f32 [B][8], entries 2..5 = {rect_h, rect_w, x, y}; pixel (h, w) is in the
 * hole iff y <= h < y + rect_h and x <= w < x + rect_w in every channel, compared in f32; an empty rectangle has no hole, a
 * rectangle past the image is clipped by it, a NaN entry makes every comparison false (no hole), rects == NULL: no image has
 * a hole; the rectangle enters comparisons only, no address is formed from it.  With d = a - b in f32, q = d d in f32
 * accumulated in f64 into S_valid_i, and n_valid_i the exact count of image i's elements outside its hole:
 *   loss_rows[i] = (float)(S_valid_i / n_valid_i), 0 when n_valid_i == 0                          NULL skips it
 *   d_a[e]       = (float)(2 (double)gscale / n_valid_i) * d outside the hole, exactly 0 inside   written in full; NULL skips it
 * (the gradient of gscale * loss_rows[i]; images do not share a term, so gscale is NOT divided by B).
 * Two launches: a grid of (workgroups per image, B) -- a workgroup's f64 partial in ws is of ONE image -- and one wave per
 * image for the final pass; fixed summation order, no atomics: the same inputs give the same bits eagerly and replayed.  With
 * loss_rows NULL only the first runs.  16-byte loads along W where W % 4 == 0 and a, b, d_a are 16-byte aligned, one element per
 * lane otherwise.  ws: at least vg_masked_mse_rows_ws_doubles(B, C, H, W) doubles; ws_doubles is its capacity.  VG_EINVAL: a or
 * b NULL, a size < 1, B > 65535, C H W >= 2^31 - 2^19, gscale not finite, both outputs NULL, ws NULL or too small; VG_EALIGN:
 * rects or ws not 8-byte aligned, a tensor not 4-byte aligned.  HBM-bound: 12 B per element with the gradient, 8 B without. */
int vg_masked_mse_rows(const float* a, const float* b, const float* rects, int B, int C, int H, int W, float gscale,
                       float* loss_rows, float* d_a, double* ws, int ws_doubles, void* stream);
int vg_masked_mse_rows_ws_doubles(int B, int C, int H, int W);   /* <= 0 (VG_EINVAL) for sizes outside the contract */
/* The optimiser over latents: objective, keep-best and one Adam step per image row, one wave per row, no value leaves the
 * device.  State per row (all f32 but t): master z [B][L], m [B][L], v [B][L], the row's own step count t [B] (int32: rows
 * do not share a counter), best_loss [B], best_z [B][L].  dz, z_in, z_out: [B][ZP] in dtype (the Generator's stage-0 data
 * gradient / input, ZP the padded latent width); loss_rows [B] (vg_masked_mse_rows); p [B]: the Discriminator's
 * probabilities, or NULL (no adversarial term).
 *   VG_LATENT_INIT    z = best_z = (float)z_in, m = v = 0, t = 0, best_loss = +inf; z_out (optional) = z_in, padding lanes 0.
 *   VG_LATENT_UPDATE  1. J = loss_rows[i] + alpha_adv (-max(log p_i, -100)) [p given] + prior_weight (1 / (2 L)) sum_l z_l^2
 *                        (nn.BCELoss' clamp; formed in f64, rounded to f32); objective[i] = J when objective != NULL;
 *                     2. J < best_loss[i] (strict: a tie keeps the earlier iterate, a NaN never wins): best_loss[i] = J,
 *                        best_z[i] = the z that was just evaluated;
 *                     3. g = (float)dz + prior_weight z / L; torch.optim.Adam (no weight decay, no amsgrad) with bias
 *                        corrections from t_i + 1: m = beta1 m + (1 - beta1) g, v = beta2 v + (1 - beta2) g g,
 *                        z -= lr / (1 - beta1^(t+1)) * m / (sqrt(v) / sqrt(1 - beta2^(t+1)) + eps); t_i += 1;
 *                     4. z_out = z in dtype, padding lanes 0.
 *                     Each stored value (m, v, z) is formed in f64 from the f32 state and rounded once; beta^(t+1) is formed by
 *                     square-and-multiply in f64 (r = 1; while n: if n odd r *= b; b *= b; n >>= 1), not by pow().
 *   VG_LATENT_TRACK   steps 1 and 2 only (the last iterate's objective, after the loop).
 * One launch of B waves.  VG_EINVAL: an unknown mode, B or L < 1, ZP < L, a NULL pointer the mode reads or writes (z,
 * best_loss, best_z always; m, v, t, z_in for INIT; loss_rows for UPDATE / TRACK; m, v, t, dz, z_out for UPDATE), lr or eps
 * negative or not finite, a beta outside [0, 1) (UPDATE), alpha_adv or prior_weight negative or not finite; VG_ENOSUP: an unknown
 * dtype; VG_EALIGN: ZP % 4 != 0, dz / z_in / z_out not aligned to an element. */
#define VG_LATENT_INIT   0
#define VG_LATENT_UPDATE 1
#define VG_LATENT_TRACK  2
int vg_latent_adam(float* z, float* m, float* v, int* t, float* best_loss, float* best_z, const void* dz,
                   const float* loss_rows, const float* p, const void* z_in, void* z_out, float* objective, int B, int L,
                   int ZP, double lr, double beta1, double beta2, double eps, float alpha_adv, float prior_weight, int mode,
                   int dtype, void* stream);
/* Mean SSIM of two NCHW f32 image batches in [-1,1] (rescaled to [0,1] as vaegan_code.py:170-174 does):
 * gaussian 11x11, sigma 1.5, k1 .01, k2 .03, data_range 1, 5-pixel border cropped.  out[0] = mean. */
int vg_ssim(const float* a, const float* b, int B, int C, int H, int W, float* out, float* ws, int ws_capacity,
            void* stream);
/* ------------------------------------------------------------------------------------------
 * In-kernel N(0,1) noise: the three `torch.randn_like` draws of an iteration (vaegan_code.py:77 eps of the
 * reparameterisation, :91 instance noise on the real batch, :92 on the reconstruction) generated where they are
 * consumed instead of being materialised by a separate generator launch.
 * rng: device memory, two 64-bit words {seed, iteration counter}.  Counter-based Philox4x32-10 keyed by the seed;
 * counter = (element index >> 2 in the reference's NCHW / [B][L] order, draw id 0..255, iteration counter); one block
 * gives four normals (two Box-Muller pairs, cosine and sine of each): element i is component i & 3 of block i >> 2.
 * Word layout (Philox4x32-10 of Salmon et al., SC'11, as Random123 publishes it: multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85, ten rounds), with blk = i >> 2, step = the iteration counter (the epoch position in
 * "Degraded pairs" below), draw in [0, 256) and step < 2^56:
 *   counter c0 = blk & 0xFFFFFFFF             key k0 = seed & 0xFFFFFFFF
 *           c1 = blk >> 32                        k1 = seed >> 32
 *           c2 = step & 0xFFFFFFFF
 *           c3 = ((step >> 32) << 8 | draw) & 0xFFFFFFFF
 * so the draw ids are 256 disjoint streams of every (seed, step).  Output words (w0, w1, w2, w3); a uniform is
 * u01(w) = (w >> 8) * 2^-24.  Normals, in f32: u(w) = ((float)w + 0.5f) * 2^-32 in (0, 1], r = sqrt(-2 ln max(u(wa), 1e-30f)),
 * t = 6.283185307179586f * u(wb); components 0, 1 = r cos t, r sin t of (wa, wb) = (w0, w1), components 2, 3 those of
 * (w2, w3); logarithm, sine and cosine are the fast device intrinsics, so |n| <= sqrt(-2 ln 2^-33) = 6.77.
 * tests/_philox_ref.py restates exactly this on the host (tests/test_philox_cpu.py, tests/test_gpu_philox.py).
 * The `_rng` forms of the consuming kernels are identical to their eps-pointer forms with
 * eps[i] = N(seed, iteration, draw, i); vg_randn materialises exactly that tensor (tests, and callers that want
 * the draw itself).  vg_rng_advance (one thread) bumps the iteration counter: launch it once at the top of every
 * iteration, inside the captured graph, so that every replay draws fresh noise while forward and backward of one
 * iteration see the same eps.  Device streams can never equal the reference's CPU generator:
 * parity runs inject host noise through the eps-pointer forms.
 * ---------------------------------------------------------------------------------------- */
int vg_rng_advance(uint64_t* rng, void* stream);
int vg_randn(float* out, int64_t n, const uint64_t* rng, int draw, void* stream);
/* One pass over x (NCHW f32) -> y_noisy = x + sigma * noise AND y_plain = x, both NHWC bf16 with CP = 8 channels: the
 * Encoder's input and the Discriminator's noisy real batch (vaegan_code.py:74, :91).  Exactly one of eps (injected noise,
 * NCHW f32) / rng (+ draw).  VG_ENOSUP unless bf16, CP == 8, C <= 4, H * W % 4 == 0 (convert twice then). */
int vg_nchw_to_nhwc_pair(const float* x, const float* eps, const uint64_t* rng, int draw, float sigma, void* y_noisy,
                         void* y_plain, int B, int C, int H, int W, int CP, int dtype, void* stream);
/* vg_mse_forward_backward in two halves: the partial sums (+ gradient) here, the final sum inside the KL launch below
 * (vaegan_code.py:113-114 are evaluated back to back; the separate one-wave finalize launch was 4.7 us). */
int vg_mse_partial(const float* a, const float* b, int64_t n, float gscale, float* d_a, float* ws, int ws_capacity,
                   int* nparts_out, void* stream);
int vg_kl_forward_mse_final(const void* mulv, const float* lv_clamped, int B, int L, int MP, float divisor, float* out,
                            const float* mse_ws, int mse_nparts, int64_t mse_n, float* mse_loss, int dtype, void* stream);
int vg_nchw_to_nhwc_rng(const float* x, const uint64_t* rng, int draw, float sigma, void* y,
                        int B, int C, int H, int W, int CP, int dtype, void* stream);          /* vaegan_code.py:91 */
int vg_nhwc_tanh_to_nchw_noisy_rng(const void* x, float* y_nchw, const uint64_t* rng, int draw, float sigma,
                                   void* y_noisy_nhwc, int B, int C, int H, int W, int CP, int dtype,
                                   void* stream);                                             /* vaegan_code.py:83,92 */
int vg_reparam_forward_rng(const void* mulv, const uint64_t* rng, int draw, void* z, float* lv_clamped,
                           int B, int L, int MP, int ZP, int dtype, void* stream);            /* vaegan_code.py:75-78 */
/* vg_prior_forward on draw `draw` of the current iteration (ABI 31): equal to the injected form fed what vg_randn
 * materialises for that draw.  VG_EINVAL also for draw outside [0, 256). */
int vg_prior_forward_rng(const uint64_t* rng, int draw, void* z, int B, int L, int ZP, int dtype, void* stream);
int vg_reparam_kl_backward_rng(const void* mulv, const float* lv_clamped, const uint64_t* rng, int draw,
                               const void* dz, float kl_scale, void* dmulv, int B, int L, int MP, int ZP,
                               int dtype, void* stream);
/* ------------------------------------------------------------------------------------------
 * Degraded pairs (dataset_code.py:13-65, CelebADatasetV0 with noise_max_std set: `return noisy_img, clean_img`).
 * vg_gather_degrade_u8 assembles, in ONE pass over the resident u8 [N][H][W][C] set and idx[B]:
 *   clean  f32 [B][C][H][W]: normalize != 0: (u/255 - 0.5)/0.5, bit-identical to vg_gather_normalize_u8;
 *                            normalize == 0: u/255 (V0's ToTensor without Normalize);
 *   noisy  f32 [B][C][H][W]: add_noise (:35-42) of clean, see below;
 *   nhwc   (optional, NULL to skip) noisy again as the engine input [B][H][W][CP] in dtype (VG_F32 / VG_BF16, pad channels
 *          zero, 16-byte aligned), bit-identical to vg_nchw_to_nhwc(noisy).
 * Per image, in the reference's order, every f32 product / sum rounded on its own:
 *   base  = (rect and the pixel lies in the image's rectangle) ? 2*f - 1 : clean      (f: fill uniform of that element)
 *   noisy = min(max(base + (n * s) * noise_max_std, -1), 1)         (n ~ N(0,1) per element, ONE s ~ U[0,1) per image)
 * The rectangle covers rows y .. y + rect_h - 1 and columns x .. x + rect_w - 1 in every channel; rect_h or rect_w == 0
 * is an empty rectangle.  Its integer ranges are fixed on the host (data.degrade_bounds: python round(), as the
 * reference): rect_h, rect_w in [min_size, max_size], x in [x0, x1 - rect_w), y in [y0, y1 - rect_h).  rect == 0: no
 * rectangle, the six bounds are ignored.
 *
 * Random draws.  Philox4x32-10 exactly as for the in-kernel N(0,1) noise below: key = seed, and the counter word that
 * carries the iteration there carries pos = pos0 + b here, the sample's POSITION IN THE EPOCH'S ORDER (not its batch slot):
 * a sample's degradation does not depend on batch size, rank or world size.  seed and pos0 travel by value; every position
 * pos0 .. pos0 + B - 1 is below 2^56 (VG_EINVAL otherwise: position 2^56 would wrap onto position 0).
 * With e = c*H*W + h*W + w, the element's index within its image, and word(draw, i) = output word i & 3 of Philox block
 * i >> 2 of that draw at (seed, pos):
 *   draw VG_DRAW_DEGRADE_NORMAL: n = element e of what vg_randn(out, C*H*W, {seed, pos}, draw) materialises;
 *   draw VG_DRAW_DEGRADE_FILL:   f = u01(word(draw, e)) -- a rectangle pixel uses the uniform AT ITS OWN index
 *                                (vg_rand_u01(out, C*H*W, {seed, pos}, draw) materialises all of them);
 *   draw VG_DRAW_DEGRADE_PARAMS: s = u01(word 0), rect_h = rint(word 1, min_size, max_size + 1),
 *                                rect_w = rint(word 2, min_size, max_size + 1), x = rint(word 3, x0, x1 - rect_w),
 *                                y = rint(word 4, y0, y1 - rect_h);
 *   u01(w) = (w >> 8) * 2^-24 in [0, 1);   rint(w, lo, hi) = lo + (((uint64)(w >> 8) * (hi - lo)) >> 24) in [lo, hi).
 * The three ids are outside 0..2, the draws of a training iteration.
 * vg_rand_u01: the uniform twin of vg_randn: out[i] = u01(word(draw, i)) at rng = {seed, counter} (device memory).
 * vg_degrade_params: out f32 [B][8] = {s, sigma = s * noise_max_std, rect_h, rect_w, x, y, 0, 0} of positions
 * pos0 .. pos0 + B - 1 (rect == 0: the four geometry entries are 0); for inspection, plots and tests.
 * idx outside [0, N) is clamped to 0 (the host validates).  VG_EINVAL for empty ranges or a rectangle outside the image.
 *
 * Noise models (not in the reference; added within ABI 31).  vg_gather_degrade_u8_ex and vg_degrade_params_ex take the same
 * arguments plus `int kind, float impulse_max_p, float salt_ratio`; the two entry points above are the model
 * (VG_NOISE_GAUSSIAN, impulse_max_p = 0) and the _ex entries called with it write the same bits.  Per element, all f32, every
 * product, sum, quotient and root rounded on its own (no fused multiply-add):
 *   base = the clean value, or the rectangle fill 2*f - 1                                                  (as above)
 *   lo   = normalize ? -1 : 0,   span = normalize ? 2 : 1                      (black and the width of the value mapping)
 *   g    = max((base - lo) / span, 0)          (the intensity in [0, 1]; the max matters: with normalize == 0 a rectangle
 *                                               fill can be negative)
 *   f    = 1        VG_NOISE_GAUSSIAN (0)  additive noise, the reference's model
 *        = g        VG_NOISE_SPECKLE  (1)  multiplicative speckle: standard deviation proportional to the intensity
 *        = sqrt(g)  VG_NOISE_SHOT     (2)  signal-dependent shot noise: variance proportional to the intensity (the normal
 *                                          approximation of Poisson counts; the root is the correctly rounded one)
 *   t    = min(max(base + ((n * s) * noise_max_std) * f, -1), 1)
 * with the same n, s and noise_max_std as above: s * noise_max_std is the standard deviation AT WHITE (g = 1) for all three
 * kinds, and f = 1 is the expression above bit for bit.
 * Impulses (salt and pepper) on top, only when impulse_max_p > 0: p_b = s * impulse_max_p is the image's hit probability;
 *   element e is hit when u01(word(VG_DRAW_DEGRADE_IMPULSE, e)) < p_b, and a hit element becomes
 *   1 (salt) when u01(word(VG_DRAW_DEGRADE_SALT, e)) < salt_ratio, else lo (pepper), whatever t was.
 * The salt word is evaluated only where an element is hit (as the fill word only where the rectangle is touched); both are
 * materialised by vg_rand_u01(out, C*H*W, {seed, pos}, draw).  clean is never touched; the NHWC copy carries the impulses.
 * vg_degrade_params_ex: out f32 [B][8] = {s, s * noise_max_std, rect_h, rect_w, x, y, p_b = s * impulse_max_p, (float)kind}.
 * VG_EINVAL: kind outside 0..2; impulse_max_p or salt_ratio outside [0, 1] or not finite; everything the two entry points
 * above refuse.
 * ---------------------------------------------------------------------------------------- */
#define VG_DRAW_DEGRADE_NORMAL 16
#define VG_DRAW_DEGRADE_FILL   17
#define VG_DRAW_DEGRADE_PARAMS 18
#define VG_DRAW_DEGRADE_IMPULSE 19
#define VG_DRAW_DEGRADE_SALT 20
#define VG_NOISE_GAUSSIAN 0
#define VG_NOISE_SPECKLE  1
#define VG_NOISE_SHOT     2
int vg_gather_degrade_u8_ex(const uint8_t* images, int64_t N, const int64_t* idx, int B, int C, int H, int W, uint64_t seed,
                            uint64_t pos0, float noise_max_std, int rect, int normalize, int min_size, int max_size, int x0,
                            int x1, int y0, int y1, float* clean, float* noisy, void* nhwc, int CP, int dtype, int kind,
                            float impulse_max_p, float salt_ratio, void* stream);
int vg_degrade_params_ex(uint64_t seed, uint64_t pos0, int B, float noise_max_std, int rect, int H, int W, int min_size,
                         int max_size, int x0, int x1, int y0, int y1, float* out, int kind, float impulse_max_p,
                         float salt_ratio, void* stream);
int vg_gather_degrade_u8(const uint8_t* images, int64_t N, const int64_t* idx, int B, int C, int H, int W, uint64_t seed,
                         uint64_t pos0, float noise_max_std, int rect, int normalize, int min_size, int max_size, int x0,
                         int x1, int y0, int y1, float* clean, float* noisy, void* nhwc, int CP, int dtype, void* stream);
int vg_degrade_params(uint64_t seed, uint64_t pos0, int B, float noise_max_std, int rect, int H, int W, int min_size,
                      int max_size, int x0, int x1, int y0, int y1, float* out, void* stream);
int vg_rand_u01(float* out, int64_t n, const uint64_t* rng, int draw, void* stream);
/* ------------------------------------------------------------------------------------------
 * Latent prior (main_vae.py:415-436 vals_to_hist / sample_distribution, used by evaluate_vae :452-512 and sample_vae
 * :594-626): the aggregate-posterior histogram prior.  The Encoder's (mu | logvar) rows of the whole data set stay on
 * the device; their per-column histograms are fitted there and latent draws come out in the Generator's input layout.
 *
 * vg_latent_hist: per-column np.histogram(x[:, c], bins=n_bins) + np.cumsum(counts / N) of x f32 [N][D], rows
 * `row_stride` elements apart (row_stride >= D; the [N][2L] mu | logvar matrix is fitted in one call, D = 2L).
 *   range   lo_c = min_n x[n][c], hi_c = max_n x[n][c]; lo_c == hi_c: lo_c -= 0.5f, hi_c += 0.5f (numpy _get_outer_edges).
 *   edges   f32 [D][n_bins + 1] (numpy >= 2 keeps float32 input in float32), every operation rounded on its own, no
 *           fused multiply-add: step = (hi - lo) / n_bins; e_k = fl(fl(k * step) + lo) for k < n_bins; e_{n_bins} = hi.
 *   counts  int32 [D][n_bins]: x falls in the bin b with e_b <= x < e_{b+1}, the last bin closed on the right.
 *   cdf     f64 [D][n_bins]: cdf_b = cdf_{b-1} + (double)counts_b / (double)N, summed SEQUENTIALLY in bin order -- what
 *           np.cumsum(freqs / n) computes; its last entry is often 1 - 1 ulp, and the sampler has to see the doubles the
 *           reference sees.
 *   status  int32 [1]: non-zero if some column's range (or its width) is not finite (numpy raises ValueError there);
 *           the other outputs are then unspecified, but every access stays in bounds.
 * Four launches: column min / max partials, edges (+ zeroed counts), binning into an LDS histogram flushed with integer
 * atomics (order-independent: the result is deterministic), one-workgroup cdf.  1 <= N <= 2^31 - 1, D >= 1,
 * 1 <= n_bins <= 1024, else VG_EINVAL.  ws: vg_latent_hist_ws_bytes() bytes of scratch, 4-byte aligned.
 *
 * vg_latent_sample: n draws from a fitted prior with L latent dimensions: histogram columns [0, L) are mu, [L, 2L) logvar.
 * Per output element (j, c), j < n, c < 2L, with u, v in [0, 1):
 *   idx = first b with cdf[c][b] >= u (np.searchsorted, side left), CLAMPED to n_bins - 1;
 *   out = (float)(x0 + (x1 - x0) * v), x0 = (double)edges[c][idx], x1 = (double)edges[c][idx + 1], in f64, every
 *         operation rounded on its own (legacy np.random.uniform is low + (high - low) * d), ONE final rounding to f32.
 * Draws: injected -- u and v f64 [n][2L] (both or neither; the reference's draws are 53-bit doubles), eps f32 [n][L] --
 * or, where the pointer is NULL, generated from rng = {seed, counter} (device memory) like every other in-kernel draw:
 *   u = u01(word(VG_DRAW_LATENT_U, j*2L + c)), v = u01(word(VG_DRAW_LATENT_V, j*2L + c))   (u01, word: "Degraded pairs" above;
 *       what vg_rand_u01(out, n*2L, rng, draw) materialises, 24 bits, exact in f64),
 *   eps = element j*L + i of what vg_randn(out, n*L, rng, VG_DRAW_LATENT_EPS) materialises.
 * Outputs, each optional (NULL), at least one:
 *   mulv f32 [n][2L]: the sampled mu | logvar;
 *   z    [n][ZP] in dtype (VG_F32 / VG_BF16, pad columns zero, 16-byte aligned): the Generator's input,
 *        z = mu + exp(0.5 * clamp(logvar, -10, 10)) * eps (main_vae.py:487), eps needed only for z.
 * Deviations from the reference, both inert in its own use: (a) the clamp of idx -- sample_distribution indexes
 * bins[i, idx + 1] unclamped and raises IndexError if u > cdf[-1]; that needs u > 1 - ~1e-14, which a 24-bit device
 * uniform (at most 1 - 2^-24) never is; (b) the logvar clamp -- main_vae.py:487 has none, the engine's reparameterisation
 * clamps as vaegan_code.py:75 does; inert for |logvar| < 10.
 *
 * vg_to_u8: how generated images leave the device (main_vae.py:492,498-499): x f32 [B][C][H][W] in [-1, 1] ->
 * t = fl(fl(fl(x + 1) / 2) * 255), clamped to [0, 255], truncated toward zero (a NaN gives 0).  grid_cols == 0: y u8
 * [B][C][H][W]; grid_cols > 0: ONE picture y u8 [rows*H][grid_cols*W][C], rows = ceil(B / grid_cols), image i at tile
 * (i / grid_cols, i % grid_cols), unused tiles zero (the vaegan_fake_epoch_*.jpg grid of vaegan_code.py:209-216).
 * ---------------------------------------------------------------------------------------- */
#define VG_DRAW_LATENT_U   32
#define VG_DRAW_LATENT_V   33
#define VG_DRAW_LATENT_EPS 34
int64_t vg_latent_hist_ws_bytes(int64_t N, int D, int n_bins);     /* VG_EINVAL (negative) for sizes outside the contract */
int vg_latent_hist(const float* x, int64_t N, int D, int64_t row_stride, int n_bins, float* edges, int32_t* counts,
                   double* cdf, int32_t* status, void* ws, int64_t ws_bytes, void* stream);
int vg_latent_sample(const float* edges, const double* cdf, int n_bins, int L, int64_t n, const double* u, const double* v,
                     const float* eps, const uint64_t* rng, float* mulv, void* z, int ZP, int dtype, void* stream);
int vg_to_u8(const float* x, uint8_t* y, int B, int C, int H, int W, int grid_cols, void* stream);
/* ------------------------------------------------------------------------------------------
 * Gaussian-mixture prior (ex-post density estimation: Ghosh et al. 2020, "From Variational to Deterministic
 * Autoencoders"; not in the reference, whose two priors are N(0, I) and the per-column histograms above).  A
 * full-covariance mixture of K Gaussians fitted by EM to the Encoder's mu rows of the whole data set keeps the
 * correlations between latent dimensions that the histogram prior discards.  The two GEMM-shaped phases of an EM
 * iteration and the sampler run here; the K small D x D steps between them (weights, means, Cholesky, triangular
 * inverse) are the caller's, in f64 on the host (latent.GaussianMixturePrior).
 * Throughout: x f32 [N][D], rows `row_stride` elements apart (row_stride >= D: mulv[:, :L] is fitted without a copy);
 * every parameter and every sum f64, 8-byte aligned (else VG_EALIGN); 1 <= N <= 2^31 - 1, 1 <= D <= 256, 1 <= K <= 64.
 * Outside these limits, on a NULL required pointer or with too small a workspace: VG_EINVAL before any launch.
 * Deterministic: no floating-point atomics, the same inputs give the same bits on every call.
 *
 * vg_gmm_log_resp (E-step): mean f64 [K][D]; prec_chol f64 [K][D][D], scikit-learn's precisions_cholesky_: UPPER
 * triangular U_k with inverse(Sigma_k) = U_k U_k^T (entries below the diagonal are never read); log_coef f64 [K] =
 * log w_k + sum_i log U_k[i][i] - D/2 log(2 pi).  Per row, d = (double)x - mean_k:
 *     y_j        = sum_i d_i U_k[i][j]                   on v_mfma_f64_16x16x4_f64, D staged padded with zeros to 16
 *     log_prob_k = log_coef_k - 0.5 * sum_j y_j^2        the sum of squares is the MFMA's epilogue
 *     m          = max_k log_prob_k
 *     log_norm   = m + log(sum_k exp(log_prob_k - m))    k ascending
 *     resp_k     = exp(log_prob_k - log_norm)
 * Outputs, each optional (NULL), at least one: log_prob f64 [N][K], log_norm f64 [N], resp f64 [N][K].  The order of the
 * additions inside y and inside the sum of squares is the kernel's; where every intermediate is exactly representable
 * the result is exact.  exp and log are the device library's f64 functions.  A NaN in a row makes its log_norm NaN.
 * One launch: a workgroup owns up to 64 rows, whose x tile stays in LDS for all K components.
 *
 * vg_gmm_moments (M-step sums), with d = (double)x - shift_k (shift f64 [K][D]) and r = resp f64 [N][K]:
 *     nk[k] = sum_n r_nk      s1[k][i] = sum_n r_nk d_i      s2[k][i][j] = sum_n r_nk d_i d_j      (f64 [K], [K][D], [K][D][D])
 *     loglik_sum[0] = sum_n log_norm[n]      (both optional; loglik_sum needs log_norm)
 * The outputs are OVERWRITTEN; s2 is the full matrix, exactly symmetric (the entries below the diagonal are copies).  The centred form is deliberate: with shift = the current
 * means, Sigma_k = s2/nk - delta delta^T with delta = s1/nk loses nothing to cancellation as EM converges.
 * The shape is (r * d)^T d on v_mfma_f64_16x16x4_f64 (r_nk * d_i is rounded once, then every product and sum is f64):
 * the 16 x 16 blocks of the upper triangle of s2_k, one accumulator each, over a FIXED row split -- rows in ascending
 * order inside a split, the splits' partials added in split order by a second launch, the scheme of vg_feat_stats_accum.
 * For D <= 112 one workgroup holds all blocks of a component, so x is read once per component.  Two launches.
 * ws: vg_gmm_moments_ws_bytes(N, D, K) bytes, 8-byte aligned = 8 * splits * (K * (256 NB + 16 TB + 1) + 1) with
 * TB = ceil(D / 16), NB = TB (TB + 1) / 2 and the row split: s = min(max(1, 768 / (ceil(NB / 32) K)), ceil(N / 64)) parts
 * asked for, rows_per_split = ceil(N / s) rounded up to a multiple of 16, splits = ceil(N / rows_per_split) <= s (N =
 * 200 000, D = 100, K = 10: s = 76, 2 640 rows each, 76 splits; K = 1: s = 768, 272 rows each, 736 splits).  VG_EINVAL
 * (negative) outside the limits.
 *
 * vg_gmm_sample: n draws.  cdf f64 [K] = cumulative weights; mean f64 [K][D]; cov_chol f64 [K][D][D]: the LOWER factor
 * L_k of Sigma_k (entries above the diagonal are never read).  Per draw j, with u in [0, 1) and eps f32 [D]:
 *     k     = first index with cdf[k] > u (np.searchsorted(cdf, u, side="right")), CLAMPED to K - 1
 *     z64_i = mean_k[i] + s_i,   s_i = sum_{c <= i} L_k[i][c] * (double)eps_c, c ascending, each step one fused multiply-add
 *     z32   = (float)z64, one rounding
 * Draws: injected -- u f64 [n], eps f32 [n][D] -- or, where the pointer is NULL, generated from rng = {seed, counter}
 * (device memory) like every other in-kernel draw: u = u01(word(VG_DRAW_GMM_U, j)), eps = element j*D + i of what
 * vg_randn(out, n*D, rng, VG_DRAW_GMM_EPS) materialises (u01, word: "Degraded pairs" above).
 * Outputs, each optional (NULL), at least one: comp int32 [n] = k; z32 f32 [n][D]; z [n][ZP] in dtype (VG_F32 / VG_BF16,
 * ZP >= D, pad columns zero, 16-byte aligned): z32 cast to the engine dtype, the Generator's input.  One launch.
 * ---------------------------------------------------------------------------------------- */
#define VG_DRAW_GMM_U   40
#define VG_DRAW_GMM_EPS 41
int vg_gmm_log_resp(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* mean,
                    const double* prec_chol, const double* log_coef, double* log_prob, double* log_norm, double* resp,
                    void* stream);
int64_t vg_gmm_moments_ws_bytes(int64_t N, int D, int K);
int vg_gmm_moments(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* shift, const double* resp,
                   const double* log_norm, double* nk, double* s1, double* s2, double* loglik_sum, void* ws,
                   int64_t ws_bytes, void* stream);
int vg_gmm_sample(const double* cdf, const double* mean, const double* cov_chol, int K, int D, int64_t n, const double* u,
                  const float* eps, const uint64_t* rng, int32_t* comp, float* z32, void* z, int ZP, int dtype,
                  void* stream);
/* ------------------------------------------------------------------------------------------
 * K-means (not in the reference; ABI 30; csrc/kmeans.hip): Lloyd's two phases and the k-means++ seeding over rows that
 * already sit in HBM -- the k-means start of the mixture prior above (scikit-learn's init_params="kmeans") and the bins of
 * the NDB metric (Richardson & Weiss 2018, "On GANs and GMMs").  Conventions of the Gaussian-mixture section: x f32 [N][D],
 * rows `row_stride` elements apart (row_stride >= D); centres and every sum f64, 8-byte aligned (else VG_EALIGN);
 * 1 <= N <= 2^31 - 1, 1 <= D <= 256, 1 <= K <= 1024.  Outside these limits, on a NULL required pointer or with too small
 * a workspace: VG_EINVAL before any launch.  Deterministic: no floating-point atomics, the same inputs give the same bits
 * on every call.  No launch waits on another workgroup of the same launch.
 *
 * vg_kmeans_assign (one launch, plus a 4-byte memset where `changed` is asked for).  center f64 [K][D].  Per row n:
 *     h_k      = 0.5 * sum_i c_ki^2                       per workgroup, from the centre loads of the product (no workspace)
 *     s_k      = h_k - sum_i (double)x_i * c_ki           the N x K x D product on v_mfma_f64_16x16x4_f64
 *     label[n] = the LOWEST k with minimal s_k            (first strict `<` wins)
 *     dist2[n] = sum_i ((double)x_i - c_label,i)^2        direct form, no cancellation
 * A row with a NaN gets label 0 and a NaN dist2.  Outputs, each optional (NULL), at least one: label int32 [N]; dist2 f64
 * [N]; resp f64 [N][K], the one-hot row vg_gmm_moments consumes; changed int32 [1] TOGETHER WITH prev_label int32 [N] (one
 * without the other: VG_EINVAL): the number of rows whose label differs from prev_label, zeroed by the entry and counted
 * with an integer atomic.  The order of the additions inside a sum is the kernel's (the product: columns in groups of 16,
 * D padded with zeros, inside a group i = 4 q + s with q the MFMA's k index and s ascending; h: per q over the groups, then
 * (q0 + q1) + (q2 + q3); dist2: 256 / rows lanes per row, lane q the columns q, q + lanes, ..., then a xor tree); where every
 * intermediate is exactly representable the result is exact.  A workgroup owns 64 rows (32 where D > 224), whose x tile
 * stays in LDS for all K centres; the four waves split the 16-centre tiles, or the rows where K <= 48 (vg_km_plan).
 *
 * vg_kmeans_update (three launches: main, reduce, and a one-workgroup launch for stats, which needs every centre; only
 * two where stats is NULL).  From label int32 [N], over a FIXED row split whose partials are added in split order:
 *     count[k]  = #{n : label[n] = k}                                            int64 [K], required
 *     sum[k][i] = sum_{label[n] = k} (double)x_ni                                rows ascending inside a split; f64 [K][D]
 *     center[k] = count[k] > 0 ? sum[k] / count[k] (one IEEE division) : old[k]  f64 [K][D]; must not alias old
 *     stats[0]  = sum_k (sum_i (center_ki - old_ki)^2)                           k, i ascending; 0 where center is NULL
 *     stats[1]  = sum_n dist2[n]                                                 0 where dist2 is NULL
 * Rows whose label is outside [0, K) are skipped (the kernel never indexes with such a label; callers mask rows this way).
 * sum, center, stats, dist2 are optional; old is required with center, stats with dist2.  An empty cluster keeps its old
 * centre (scikit-learn relocates it: a stated deviation).  stats[1]: per split, thread t of 256 adds the rows r0 + t +
 * 256 j, j ascending, the 256 values meet in a halving tree (t += t + 128, t + 64, ...), the splits in split order.
 * Main launch: a workgroup owns (row split, chunk of clusters), chunk = min(K, 49152 / (8 D)) so that the f64 accumulators
 * fit in LDS; thread i owns column i; only the chunk that owns a row's label reads that row of x.
 * ws: vg_kmeans_update_ws_bytes(N, D, K) bytes, 8-byte aligned = 8 * (splits * (K D + K + 1) + K) with chunks =
 * ceil(K / chunk), cap = min(1024, max(128, 16 MiB / (8 K D))) (the partial sums stay at 16 MiB, or at 128 splits),
 * s = max(1, min(cap, 1024 / chunks, ceil(N / 256))), rows_per_split = ceil(N / s) rounded up to a multiple of 256,
 * splits = ceil(N / rows_per_split) (N = 200 000, D = 100, K = 200: chunk 61, 4 chunks, 112 splits of 1 792 rows, 18 MB;
 * K = 10: one chunk, 782 splits of 256 rows, 6 MB).  VG_EINVAL (negative) outside the limits.
 *
 * vg_kmeans_seed: plain k-means++ (Arthur & Vassilvitskii 2007: one trial per step, not scikit-learn's greedy variant),
 * no host sync.  u f64 [K] injected, or (u NULL) drawn from rng = {seed, counter} (device memory) as
 * u_j = u01(word(VG_DRAW_KMEANS_U, j)) (u01, word: "Degraded pairs" above):
 *     idx[0] = min((int64)(u_0 * N), N - 1);          mind2[n] = sum_i ((double)x_ni - (double)x_idx0,i)^2, i ascending
 *     for j = 1 .. K - 1:  total = sum mind2;  idx[j] = first n with cum[n] > u_j * total, N - 1 if there is none;
 *                          mind2 = min(mind2, |x - x_idx[j]|^2)
 * cum is a two-level sum with blocks of 256 rows: a block's total adds its rows in ascending order, total adds the block
 * totals in ascending order, and cum[n] = (the totals of the blocks below n's, added in that order) + (the rows of n's
 * block up to n, added in ascending order from 0): two sums and ONE addition of the two.  Each step is two launches -- the mind2 update with block
 * totals, then a one-workgroup pick that leaves idx[j] in device memory for the next update: 2 K - 1 launches.
 * Outputs: idx int32 [K], center f64 [K][D] (the chosen rows).  ws: vg_kmeans_seed_ws_bytes(N, D, K) = 8 * (N +
 * ceil(N / 256)) bytes, 8-byte aligned; its first N doubles are mind2 after the last step.  A picked row has mind2 = 0
 * only when total = 0 (fewer than K distinct rows): the result then holds duplicate centres.
 *
 * vg_kmeans_plan (host-only, needs no GPU): the record the three launchers above launch from.
 * ---------------------------------------------------------------------------------------- */
#define VG_DRAW_KMEANS_U 42
typedef struct vg_km_plan {
    int32_t assign_rows;          /* rows per workgroup of the assign kernel: 64, or 32 where D > 224 */
    int32_t assign_tile;          /* centres per MFMA tile: 16 */
    int32_t assign_row_split;     /* 1: fewer than four centre tiles, the waves split the rows; 0: they split the tiles */
    int32_t assign_lds_bytes;
    int32_t update_splits, update_chunks, update_chunk;
    int32_t seed_block;           /* rows per block of the seed's cumulative sum: 256 */
    int64_t assign_grid, update_rows_per_split, seed_blocks, update_ws_bytes, seed_ws_bytes;
} vg_km_plan;
int vg_kmeans_plan(int64_t N, int D, int K, vg_km_plan* out);
int vg_kmeans_assign(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* center, int32_t* label,
                     double* dist2, double* resp, const int32_t* prev_label, int32_t* changed, void* stream);
int64_t vg_kmeans_update_ws_bytes(int64_t N, int D, int K);
int vg_kmeans_update(const float* x, int64_t N, int D, int64_t row_stride, int K, const int32_t* label, const double* dist2,
                     const double* old, int64_t* count, double* sum, double* center, double* stats, void* ws,
                     int64_t ws_bytes, void* stream);
int64_t vg_kmeans_seed_ws_bytes(int64_t N, int D, int K);
int vg_kmeans_seed(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* u, const uint64_t* rng,
                   int32_t* idx, double* center, void* ws, int64_t ws_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * Resize (dataset_code.py:26-30, CelebADatasetV0's transforms.Resize(image_size) + transforms.CenterCrop(image_size) on
 * the PIL image default_loader hands them): PIL's ImagingResample for 8-bit images with the triangle (BILINEAR) filter,
 * restated as integer arithmetic.  The output equals Image.resize((w, h), Image.BILINEAR) + crop byte for byte.
 * PB = 22 (PIL's PRECISION_BITS = 32 - 8 - 2).
 *
 * Coefficient table of one axis, in_size -> out_size, computed ON THE HOST in IEEE double, in exactly this order of
 * operations ((int) truncates toward zero):
 *   scale = in_size / out_size;  fs = max(scale, 1.0);  support = 1.0 * fs;  ksize = 2 * ceil(support) + 1;  ss = 1.0 / fs
 *   for each output index xx:
 *     center = (xx + 0.5) * scale
 *     xmin = max((int)(center - support + 0.5), 0)
 *     n    = min((int)(center + support + 0.5), in_size) - xmin
 *     w_x  = max(0, 1 - |(x + xmin - center + 0.5) * ss|)  for x < n
 *     ww   = sum of w_x, summed left to right
 *     p_x  = w_x / ww  (left as w_x if ww == 0)
 *     k_x  = (int)(0.5 + p_x * 2^PB);  for p_x < 0 it is (int)(-0.5 + p_x * 2^PB) (cannot occur for this filter, part of the rule)
 *     taps beyond n are 0;  bounds[xx] = (xmin, n)
 * One pass along an axis, on u8 data, per channel, int32 accumulator:
 *   out = clamp((2^(PB-1) + sum_{x<n} in[xmin + x] * k_x) >> PB, 0, 255)
 * (the largest accumulator is 255 * (2^22 + a few ulps) + 2^21 < 2^31).
 * Resize (Hin, Win) -> (Hr, Wr): the horizontal pass first, then the vertical pass on the U8 result of the horizontal one;
 * a pass whose size does not change is skipped; an unchanged image is a copy.
 * CenterCrop to (ch, cw): top = int(round((Hr - ch) / 2.0)), left = int(round((Wr - cw) / 2.0)) with python's round
 * (ties to even); dst[y][x] = resized[top + y][left + x].  ch > Hr or cw > Wr is an error (torchvision would pad).
 * image_size -> geometry (data.resize_geometry): an int resizes the SHORTER edge to it, the longer edge becomes
 * int(size * long / short), crop size x size; an (h, w) pair resizes to exactly that and the crop is a no-op.
 * RGBA is outside the contract (PIL resizes it with premultiplied alpha); L, RGB, CMYK are channels treated alike.
 *
 * vg_resize_u8: src u8 [N][Hin][Win][C], C <= 4, 4-byte aligned -> dst u8 [B][ch][cw][C] (the resident layout).
 *   idx    int64 [B] source image of each output image, or NULL: images 0 .. B-1 in order (B <= N).  idx outside [0, N)
 *          reads image 0 (the host validates).
 *   kh/bh  int32 [cw][ksize_h] and [cw][2]: the horizontal table ALREADY RESTRICTED to the crop window (rows left ..
 *          left + cw - 1 of the Win -> Wr table), 16-byte aligned device memory; bh_host: the same bounds in HOST memory,
 *          read by this call before the launch: every (xmin, n) is checked against the input (0 <= xmin, 1 <= n <=
 *          ksize, xmin + n <= in_size, windows moving forward) -- a table that reaches outside the image is VG_EINVAL,
 *          nothing is launched.  All three NULL: the pass is skipped and `left` is the first source column.
 *   kv/bv/bv_host, ksize_v, top: the same for rows (rows top .. top + ch - 1 of the Hin -> Hr table).
 *   top, left: used only by a skipped pass (a table carries its own offsets).
 *   band   output rows per workgroup; 0: chosen by the library.  The result does not depend on it.
 * One launch: a workgroup owns one image and a band of output rows; it stages the input rows [bv[y0].xmin,
 * bv[y1-1].xmin + bv[y1-1].n) that band reads -- only the columns [bh[0].xmin, bh[cw-1].xmin + bh[cw-1].n) -- through
 * LDS, keeps the horizontal result there as u8 and stores the band as whole contiguous rows; no intermediate in HBM.
 * Columns and rows of the resized image outside the crop window are never computed.  All byte offsets are 64-bit.
 * vg_resize_u8_lds_bytes: the LDS bytes a launch of this geometry takes (host arguments only), or VG_EINVAL where
 * vg_resize_u8 would return it -- which includes a geometry that cannot be served: an LDS image of one output row's
 * input rows plus four staged input rows beyond 64 KiB (e.g. C * (3 * cw + 4 * cols_read) > 65536 for an enlargement).
 * There is no second path.
 * ---------------------------------------------------------------------------------------- */
int64_t vg_resize_u8_lds_bytes(int Hin, int Win, int C, const int32_t* bh_host, int ksize_h, const int32_t* bv_host,
                               int ksize_v, int top, int left, int ch, int cw, int B, int band);
/* The band height (output rows per workgroup) that launch uses -- `band` itself where it is given and fits; VG_EINVAL as above.
 * With it a caller can count the bytes a launch really reads: adjacent bands re-read about 2 * support input rows. */
int vg_resize_u8_band(int Hin, int Win, int C, const int32_t* bh_host, int ksize_h, const int32_t* bv_host, int ksize_v,
                      int top, int left, int ch, int cw, int B, int band);
int vg_resize_u8(const uint8_t* src, int64_t N, int Hin, int Win, int C, const int64_t* idx, int B, const int32_t* kh,
                 const int32_t* bh, const int32_t* bh_host, int ksize_h, const int32_t* kv, const int32_t* bv,
                 const int32_t* bv_host, int ksize_v, int top, int left, uint8_t* dst, int ch, int cw, int band,
                 void* stream);
/* ------------------------------------------------------------------------------------------
 * Feature-space metrics (vaegan_code.py:143-185, gan_code.py:111-145, main_vae.py:472-512, :540-574: fid.update /
 * fid.compute; README.md:22: Precision / Recall / F1 "computed via manifold distances", Kynkaanniemi et al. 2019).  What
 * comes AFTER a feature vector exists; the feature extractor is the caller's (metrics.py: the project's own Encoder, or
 * any callable).  All three entry points are deterministic: no floating-point atomics, partial results are combined in a
 * fixed order, two calls on the same input give the same bits.
 *
 * vg_feat_stats_accum: the running sums behind FID (torchmetrics keeps features.double() sums): x f32 [n][D], rows
 * `row_stride` elements apart (row_stride >= D, no alignment asked of x), sum f64 [D], outer f64 [D][D] (8-byte aligned):
 *     sum[j] += sum_r x[r][j]          outer[i][j] += sum_r x[r][i] * x[r][j]
 * every product and every addition in f64 on the exactly converted f32 inputs (the product of two f32 is exact in f64, so
 * only the order of the additions is the kernel's: rows in ascending order inside a row split, the splits' partials in
 * split order, then ONE addition to the value already in sum / outer).  outer on v_mfma_f64_16x16x4_f64, 64 x 64 column
 * tiles of the upper triangle, mirrored when the partials are combined: the result is the full symmetric matrix.
 * 0 <= n <= 2^31 - 1 (n == 0: nothing is launched, 0 is returned), 1 <= D <= 2048, any D; else VG_EINVAL.
 * ws: vg_feat_stats_accum_ws_bytes(n, D) bytes, 8-byte aligned = splits * (P * 4096 + T * 64) * 8 with T = ceil(D / 64),
 * P = T (T + 1) / 2, splits = min(max(1, 512 / P), ceil(n / 64)): 17.3 MB at D = 2048 and never more than that.
 * Two launches.
 *
 * Distances, for both functions below: f32 inputs, the GEMM form
 *     d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 * dot(a, b))
 * dot accumulated in f32 on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32, columns of the feature vector in ascending
 * order), |.|^2 in f32 by a pass of its own (per lane a fused multiply-add chain over columns lane, lane + 64, ..., then
 * the wavefront's xor tree); no bf16 anywhere.  Error against exact arithmetic: at most 2 (D + 4) 2^-24 (|a|^2 + |b|^2).
 * Where every intermediate is an integer below 2^24 the result is exact.  The Nq x Nr matrix is never written to memory:
 * a workgroup owns 128 query rows and walks the reference rows 64 at a time with the running result in registers; the
 * reference rows are split over up to 16 workgroups per row tile and the partial results are merged by a second, small
 * launch.  1 <= D <= 2048, at most 2^24 rows; x / q / ref contiguous ([N][D], no row stride) and 16-byte aligned.
 *
 * vg_knn_radius2: x f32 [N][D], 1 <= k <= 8, k < N -> r2 f32 [N]: the k-th smallest d2 from row i to the OTHER rows of
 * x.  Row i is excluded by INDEX, not by value: a duplicate of row i at distance 0 counts.
 * ws: vg_knn_radius2_ws_bytes(N, D, k) = 4 N (rounded up to 256) + 4 N k splits bytes, 16-byte aligned.  Three launches.
 *
 * vg_manifold_cover: q f32 [Nq][D], ref f32 [Nr][D], r2_ref f32 [Nr] -> inside int32 [Nq]: 1 where some j has
 * d2(q_i, ref_j) <= r2_ref[j], else 0; count int64 [1] (device, 8-byte aligned): the number of ones (an integer sum).
 * ws: vg_manifold_cover_ws_bytes(Nq, Nr, D) = 4 Nq + 4 Nr (each rounded up to 256) + 4 Nq splits bytes.  Four launches
 * and one 8-byte memset.
 * The _ws_bytes queries return VG_EINVAL (negative) for sizes outside the contract.
 *
 * vg_kid_scores: the Kernel Inception Distance (Binkowski et al. 2018), an unbiased polynomial-kernel MMD^2 estimate per
 * subset pair.  The reference computes no KID: like precision / recall this goes beyond its code.  real f32 [Nr][D], fake
 * f32 [Nf][D], contiguous and 16-byte aligned; idx_real, idx_fake int32 [S][m] on the device: subset s is the rows
 * x_i = real[idx_real[s][i]] and y_j = fake[idx_fake[s][j]].  A table is just a list of rows: repeated indices are
 * allowed, and every index is clamped into [0, N), so a corrupt table cannot read outside the buffers (callers validate
 * tables before upload; the subsets are the CALLER's draw, metrics.kid_subsets draws them on the host).  With
 * b(a, c) = gamma * dot(a, c) + coef and k = b^degree, per subset s:
 *     sums[s][0] = sum_{i != j} k(x_i, x_j)      i, j are POSITIONS in the subset: the pair is left out by position, not
 *     sums[s][1] = sum_{i != j} k(y_i, y_j)      by value and not by row index (a repeated row still counts)
 *     sums[s][2] = sum_{i, j}   k(x_i, y_j)
 *     scores[s]  = (sums0 + sums1) / (m (m - 1)) - 2 * sums2 / (m * m)          in f64, in exactly that order
 *     stat[0] = (sum_s scores[s], ascending s) / S      stat[1] = sqrt(sum_s (scores[s] - stat[0])^2 / S), the
 *     POPULATION standard deviation; exactly 0 for S == 1.
 * Arithmetic: everything in f64.  dot on v_mfma_f64_16x16x4_f64 over the exactly converted f32 inputs, columns in
 * ascending order (f32 x f32 is exact in f64: only the order of the additions is the kernel's); the affine step in f64;
 * the power as degree - 1 left-to-right multiplications, no pow().  Why f64: the score is a small difference of three
 * large sums, and an f32 dot-product bound (3 D 2^-24 relative per kernel value) is of the size of the score at D = 2048.
 * Deterministic: no floating-point atomics.  One workgroup owns one 64 x 64 tile of one family (xx, yy, xy) of one
 * subset; xx and yy take only the tiles on or above the diagonal, an off-diagonal tile counts twice, a diagonal tile
 * masks i == j.  Positions >= m and columns >= D are staged as zeros and masked, never multiplied in.  Each workgroup
 * writes its one partial into ws; a second launch adds them per family in ascending tile order (xx and yy: pairs
 * (ti, tj), ti <= tj, ti-major; xy: ti * T + tj) and forms scores and stat.  Two calls give the same bits.  The m x m
 * Gram matrix is never written to memory.
 * Range: 1 <= D <= 2048, 2 <= m <= min(Nr, Nf, 32768), 1 <= S <= 4096, 1 <= degree <= 8, gamma and coef finite,
 * S * (2 P + T * T) <= 2^31 - 1 workgroups; else (or for a NULL pointer, or ws_bytes too small) VG_EINVAL.  sums f64
 * [S][3], scores f64 [S], stat f64 [2] and ws 8-byte aligned, the tables 4-byte aligned; else VG_EALIGN.
 * ws: vg_kid_scores_ws_bytes(m, S) = 8 * S * (2 P + T * T) bytes with T = ceil(m / 64), P = T (T + 1) / 2: 422 400 bytes
 * at m = 1000, S = 100.  Exactly two launches; nothing is allocated, nothing synchronises.
 * ---------------------------------------------------------------------------------------- */
int64_t vg_kid_scores_ws_bytes(int64_t m, int S);
int vg_kid_scores(const float* real, int64_t Nr, const float* fake, int64_t Nf, int D, const int32_t* idx_real,
                  const int32_t* idx_fake, int S, int64_t m, int degree, double gamma, double coef,
                  double* sums /* [S][3] */, double* scores /* [S] */, double* stat /* [2] */, void* ws, int64_t ws_bytes,
                  void* stream);
int64_t vg_feat_stats_accum_ws_bytes(int64_t n, int D);
int vg_feat_stats_accum(const float* x, int64_t n, int D, int64_t row_stride, double* sum, double* outer, void* ws,
                        int64_t ws_bytes, void* stream);
int64_t vg_knn_radius2_ws_bytes(int64_t N, int D, int k);
int vg_knn_radius2(const float* x, int64_t N, int D, int k, float* r2, void* ws, int64_t ws_bytes, void* stream);
int64_t vg_manifold_cover_ws_bytes(int64_t Nq, int64_t Nr, int D);
int vg_manifold_cover(const float* q, int64_t Nq, const float* ref, int64_t Nr, int D, const float* r2_ref, int32_t* inside,
                      int64_t* count, void* ws, int64_t ws_bytes, void* stream);
/* hipMemsetAsync(p, 0, nbytes) on the stream: optimizer.zero_grad() (vaegan_code.py:103,131-132) over a flat buffer. */
int vg_memset_zero(void* p, int64_t nbytes, void* stream);
/* bf16 -> OCP e4m3fn, elementwise: y[i] = fp8(x[i] * 2^shift).  The fp8 copies of activations (shift 0) and of the
 * packed bf16 GEMM operands (shift VG_FP8_WSHIFT) that VG_FP8 launches of vg_gather_gemm read.  n % 8 == 0. */
int vg_cast_fp8(const void* x_bf16, void* y_fp8, int64_t n, int shift, void* stream);
/* BatchNorm(+activation) backward in ONE launch (csrc/bn_onepass.hip; bf16, C a power of two in [8, 1024], tensors of up to
 * 65 536 elements per CU): column sums, coefficients and dx = a*dz - b*xhat - c with the x / dy block of a workgroup held in
 * registers across a grid-wide exchange of the partial sums -- replaces vg_bn_act_backward_reduce +
 * vg_bn_backward_finalize_grouped + vg_bn_act_backward_apply (nn.BatchNorm2d / nn.LeakyReLU / nn.ReLU backward behind
 * loss.backward(), vaegan_code.py:104, :133; modules main_vae.py:24-25, gan_code.py:22-82).  coeffs: [groups][4][C] as
 * published by the forward pass (mean | invstd | scale | shift); dgamma / dbeta (+)= per `accumulate`, group after group.
 * slab: vg_bn_backward_onepass_ws_bytes() bytes of scratch; sync: 16 bytes that are ZERO before the first call and are left
 * zero by every call (sync[2] != 0 afterwards: a bounded grid-wide wait gave up -- results of that call are invalid).
 * Returns VG_ENOSUP where _supported() says 0 (the three-launch form then applies). */
int vg_bn_backward_onepass_supported(int64_t rows, int C, int groups, int dtype);
int64_t vg_bn_backward_onepass_ws_bytes(int64_t rows, int C, int groups, int dtype);
int vg_bn_backward_onepass(const void* x, const void* dy, void* dx, const float* coeffs, const float* gamma, float* dgamma,
                           float* dbeta, int accumulate, float* slab, unsigned* sync, int64_t rows, int C, int groups,
                           int act, float slope, int dtype, void* stream);
/* out = a + alpha*b (f32, n elements); used for gradient joins on NCHW images. */
int vg_axpy(const float* a, const float* b, float alpha, float* out, int64_t n, void* stream);
/* PSNR/SSIM support for the denoise path lives in vg_image_metrics. */

/* ------------------------------------------------------------------------------------------
 * Adam (torch.optim.Adam defaults as used at vaegan_code.py:42-44; arithmetic of torch 2.10
 * _single_tensor_adam): one launch over a flat f32 buffer.
 * state[0] = step count as float (incremented on device first), so the call is graph-replayable.
 * grad_scale multiplies g before use (1/world_size after an all-reduce SUM).
 * ---------------------------------------------------------------------------------------- */
int vg_adam_step(float* p, const float* g, float* m, float* v, int64_t n,
                 double lr, double beta1, double beta2, double eps, float grad_scale,
                 float* state /* [4] device */, void* stream);
/* A training iteration that steps several optimizers (vaegan_code.py:105, :134-135) can prepare all of them -- step
 * count + 1, bias corrections -- together with the noise generator's iteration counter (rng may be NULL) in ONE
 * single-thread launch at its top; vg_adam_apply then launches the update alone and uses `state` as it finds it.  Same
 * double arithmetic as the per-optimizer prepare: bit-identical updates.  (vg_adam_step rejects lr < 0: ABI 9 overloaded
 * a negative learning rate as "prepared", which a caller's typo could trigger silently.) */
int vg_adam_apply(float* p, const float* g, float* m, float* v, int64_t n, double beta1, double beta2, double eps,
                  float grad_scale, const float* state /* prepared by vg_step_prologue */, void* stream);
#define VG_PROLOGUE_MAX 4
int vg_step_prologue(uint64_t* rng, float* const* states, const double* lr, const double* beta1, const double* beta2,
                     int n, float* zero /* nzero floats set to 0 (the iteration's loss slots), or NULL */, int nzero,
                     void* stream);
/* The Encoder's and the Generator's optimizer step of one iteration (vaegan_code.py:134-135) in ONE launch: arrays of two
 * (p, g, m, v, n, betas, eps, grad_scale, prepared state); arithmetic and per-element work split of vg_adam_apply. */
int vg_adam_apply2(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                   const double* beta1, const double* beta2, const double* eps, const float* grad_scale,
                   const float* const* state, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight averaging (not in the reference): an exponential moving average of the parameters of up to VG_EMA_MAX flat f32
 * buffers (optim.Adam's flat_p) in ONE launch, meant to follow the optimizer step inside the captured iteration.
 * Arrays of `count` entries, 1 <= count <= VG_EMA_MAX.  For buffer i (ema = ema[i], p = p[i], n = n[i] elements):
 *     t = state[i][0]      the optimizer's step count as vg_step_prologue / vg_adam_step left it on the DEVICE, i.e. already
 *                          incremented for this iteration (read by the kernel: a graph replay sees the current count).
 *                          state[i] may be NULL only when warmup[i] == 0.
 *     d = (float)(warmup[i] ? fmin(decay[i], (1.0 + t) / (10.0 + t)) : decay[i])     evaluated in double, narrowed once
 *     w = 1.0f - d                                                                   an f32 subtraction
 *     ema[j] = ema[j] + w * (p[j] - ema[j])       j in [0, n): three separately rounded f32 operations (subtract, multiply,
 *                                                 add; no contraction into an fma).  Non-finite values propagate as IEEE
 *                                                 arithmetic gives them.
 * Any n >= 1: elements [0, n / 4 * 4) move as 16-byte vectors in a grid-stride loop, the tail past n / 4 * 4 element by
 * element in the buffer's first workgroup.  Buffer i gets clamp(ceil(n / 4 / 256), 1, 2048) workgroups of 256 threads and
 * the buffers' workgroups are concatenated in one grid (as in vg_adam_apply2).  12 bytes of traffic per element.
 * Checked on the host before anything is launched, VG_EINVAL: count outside 1..VG_EMA_MAX; a NULL array or entry (apart
 * from the NULL state[i] allowed above, so: warmup[i] != 0 with state[i] NULL); n[i] <= 0; decay[i] not finite or outside
 * [0, 1]; [ema[i], +n[i]) overlapping [p[i], +n[i]).  Then VG_EALIGN: ema[i] or p[i] not 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
#define VG_EMA_MAX 4
int vg_ema_update(float* const* ema, const float* const* p, const int64_t* n, const float* const* state,
                  const double* decay, const int* warmup, int count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient-norm clipping (not in the reference): torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2,
 * error_if_nonfinite=False) of torch 2.10 over flat f32 gradient buffers (optim.Adam's flat_g), with the coefficient left
 * ON THE DEVICE and applied where Adam reads the gradient.  The gradient buffers are never rewritten.
 *
 * vg_grad_norm_clip: arrays of `count` entries, 1 <= count <= VG_GNORM_MAX; every buffer is clipped to ITS OWN norm.  For
 * buffer i (g = g[i], n = n[i] elements, grad_scale = grad_scale[i], max_norm = max_norm[i]):
 *     S     = sum_j (double)g[j] * (double)g[j]        every product exact in f64; summed in f64 in a FIXED order that depends
 *                                                      on n alone (not on the other buffers of the call or on i)
 *     norm  = fabs((double)grad_scale) * sqrt(S)       f64: the norm of the gradient Adam is actually handed
 *                                                      (grad_scale = 1/world_size after an all-reduce SUM)
 *     c     = max_norm / (norm + 1e-6)                 f64
 *     coef  = (float)(c < 1.0 ? c : (c != c ? c : 1.0))     torch.clamp(max=1): NaN propagates; narrowed once
 *     out[i][0] = (float)norm,  out[i][1] = coef
 * So: a NaN element gives norm = coef = NaN; an infinite one norm = inf and coef = 0 (NaN with max_norm = inf); an all-zero
 * gradient norm 0 and coef 1; max_norm = +inf coef 1 for every finite norm (a norm monitor); max_norm = 0 coef 0.
 * Two launches on `stream`:
 *   A  partial sums.  Buffer i gets nb_i = clamp(ceil(n / 4 / 1024), 1, VG_GNORM_PARTS) workgroups of 256 threads, the
 *      buffers' workgroups concatenated in one grid (as in vg_ema_update).  A workgroup walks sweeps of 1024 16-byte vectors
 *      (sweep s belongs to workgroup s mod nb_i); per sweep a thread issues FOUR independent 16-byte loads (vectors t, t + 256,
 *      t + 512, t + 768 of the sweep) before it consumes any, each into an f64 accumulator of its own.  The tail past
 *      n / 4 * 4 is added element by element in the buffer's first workgroup.  The 256 thread sums are added by an xor
 *      butterfly inside each wave and the four wave sums in wave order through LDS; the workgroup writes ONE f64 to
 *      ws[i * VG_GNORM_PARTS + b].  4 bytes of traffic per element, no write pass.
 *   B  finalize.  `count` workgroups of 256 threads; workgroup i adds buffer i's nb_i partials in the same fixed order,
 *      evaluates the formulas above and writes out[i].
 * No atomics, no fences, no hand-off between workgroups inside a launch: the kernel boundary is the hand-off.  The same
 * inputs give the same bits on every launch, eager or replayed.
 * Checked on the host before anything is launched, VG_EINVAL: count outside 1..VG_GNORM_MAX; a NULL array, entry, out[i] or
 * ws; n[i] <= 0; max_norm[i] NaN or < 0 (+inf is allowed); grad_scale[i] not finite.  Then VG_EALIGN: g[i] not 16-byte
 * aligned.  ws: at least VG_GNORM_MAX * VG_GNORM_PARTS doubles, contents irrelevant before and after the call.
 *
 * vg_adam_apply_clip: vg_adam_apply (count = 1) / vg_adam_apply2 (count = 2, the two grids concatenated) with the gradient
 * scale  s = grad_scale[i] * coef[i][0]  -- ONE rounded f32 product (no contraction), read from the device, uniform per
 * buffer -- wherever those kernels use grad_scale: gr = g * s (rounded), everything after that unchanged.  coef[i] == NULL:
 * s = grad_scale[i].  So coef == 1.0f gives the unclipped launch's bits, and with grad_scale == 1 gr is the very f32 product
 * torch's g.mul_(coef) produces.  Grid per buffer, per-element arithmetic and host checks are vg_adam_apply2's; in addition
 * VG_EINVAL for count outside 1..2 or a NULL coef array.
 * ---------------------------------------------------------------------------------------- */
#define VG_GNORM_MAX   4        /* buffers per call */
#define VG_GNORM_PARTS 512      /* workgroups, = f64 partial sums, per buffer at most */
int vg_grad_norm_clip(const float* const* g, const int64_t* n, const float* grad_scale, const double* max_norm,
                      int count, float* const* out /* out[i]: 2 device floats {norm, coef} */,
                      double* ws /* device, >= VG_GNORM_MAX * VG_GNORM_PARTS doubles */, void* stream);
int vg_adam_apply_clip(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                       const double* beta1, const double* beta2, const double* eps, const float* grad_scale,
                       const float* const* state /* prepared */, const float* const* coef /* device; entry may be NULL */,
                       int count /* 1 or 2 */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Learning-rate schedules and decoupled weight decay (not in the reference; ABI 26): the learning rate of an iteration as a
 * closed-form function of the optimizer's DEVICE-resident step count, evaluated in the prologue launch, so that a captured
 * iteration replays a moving rate without being captured again; and torch.optim.AdamW's decay as one more multiply in the
 * update kernel.
 *
 * vg_lr_sched: plain data, one record per optimizer.  With t = the step count AFTER this iteration's increment (1 for the
 * first step) and lr the base rate, everything in double:
 *     e    = (t - 1) / hold                                  integer division: the scheduler moves once per `hold` steps
 *     w    = e < warmup ? warmup_start + (1 - warmup_start) * ((double)e / warmup) : 1
 *     k    = max(e - decay_start, 0);   u = min(k, decay_len)
 *     d    = VG_LRS_CONST  : 1
 *            VG_LRS_LINEAR : 1 + (decay_param - 1) * ((double)u / decay_len)                  decay_param = the end factor
 *            VG_LRS_COSINE : decay_param + (1 - decay_param) * 0.5 * (1 + cos(pi * u / decay_len))
 *            VG_LRS_EXP    : pow(decay_param, k)                                              decay_param = gamma
 *            VG_LRS_STEP   : pow(decay_param, k / decay_len)                                  integer division
 *     lr_t = lr * (w * d)
 * These are the closed forms of torch.optim.lr_scheduler.LinearLR (as the warm-up: start_factor = warmup_start, total_iters =
 * warmup; as the decay: end_factor = decay_param, total_iters = decay_len), CosineAnnealingLR (T_max = decay_len, eta_min =
 * lr * decay_param), ExponentialLR and StepLR (step_size = decay_len); SequentialLR([warm-up, decay], milestones=[warmup]) is
 * decay_start = warmup; hold = the steps per epoch gives the scheduler stepped once per epoch.  Past decay_start + decay_len
 * the LINEAR and COSINE factors STAY at decay_param (torch's CosineAnnealingLR is periodic there and rises again).
 * The evaluation is compiled without floating-point contraction: every operation above is rounded on its own, so CONST, the
 * warm-up and LINEAR (only + - * /) give on the device the bits the same double expression gives on a host; COSINE, EXP and
 * STEP go through the device's cos / pow, a few double ulps from a host's.
 *
 * vg_step_prologue_sched: vg_step_prologue with one `const vg_lr_sched*` per optimizer; still ONE launch of VG_PROLOGUE_MAX
 * lanes, one lane per optimizer.  For optimizer i with sched[i] != NULL:
 *     state[0] = t, state[2] = sqrt(1 - beta2^t)          as vg_step_prologue writes them
 *     state[1] = (float)(lr_t / (1 - beta1^t))
 *     state[3] = (float)(1.0 - lr_t * weight_decay)       product and difference each rounded in double, narrowed once: the
 *                                                         scalar of torch 2.10's param.mul_(1 - lr * weight_decay)
 * sched[i] == NULL: lr_t = lr, state[3] is NOT written and the other three are vg_step_prologue's bits.
 * Checked on the host before anything is launched, VG_EINVAL: everything vg_step_prologue checks; a NULL sched array with
 * n > 0; in a record: hold < 1, warmup < 0, warmup_start outside [0, 1], an unknown decay_kind, decay_start < 0, decay_len < 1
 * (LINEAR, COSINE, STEP; ignored for CONST and EXP), decay_param outside [0, 1] (LINEAR, COSINE) or outside (0, 1] (EXP,
 * STEP; ignored for CONST), weight_decay negative or not finite (NaN fails every range).
 *
 * vg_adamw_apply: vg_adam_apply_clip -- arrays, grid per buffer, host checks, coef (an entry may be NULL), count 1 or 2 --
 * whose per-element code first forms  p = p * state[i][3]  as ONE rounded f32 product (no contraction into what follows)
 * and then runs the Adam update unchanged: torch 2.10 _single_tensor_adam with decoupled_weight_decay.  state[i][3] == 1.0f
 * (weight_decay == 0) gives vg_adam_apply_clip's bits.  28 bytes of traffic per element, as vg_adam_apply_clip.
 * ---------------------------------------------------------------------------------------- */
#define VG_LRS_CONST  0
#define VG_LRS_LINEAR 1
#define VG_LRS_COSINE 2
#define VG_LRS_EXP    3
#define VG_LRS_STEP   4
typedef struct vg_lr_sched {
    int64_t hold;          /* >= 1: optimizer steps per scheduler step */
    int64_t warmup;        /* >= 0: scheduler steps of linear warm-up */
    int64_t decay_start;   /* >= 0: scheduler step at which the decay begins */
    int64_t decay_len;     /* >= 1: scheduler steps of the decay (LINEAR, COSINE); the step size (STEP) */
    double warmup_start;   /* [0, 1]: the factor at scheduler step 0 */
    double decay_param;    /* the end factor in [0, 1] (LINEAR, COSINE); gamma in (0, 1] (EXP, STEP) */
    double weight_decay;   /* >= 0, finite */
    int32_t decay_kind;    /* VG_LRS_* */
    int32_t reserved;      /* 0 */
} vg_lr_sched;
int vg_step_prologue_sched(uint64_t* rng, float* const* states, const double* lr, const double* beta1, const double* beta2,
                           const vg_lr_sched* const* sched /* entry may be NULL */, int n, float* zero, int nzero,
                           void* stream);
int vg_adamw_apply(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                   const double* beta1, const double* beta2, const double* eps, const float* grad_scale,
                   const float* const* state /* prepared by vg_step_prologue_sched */,
                   const float* const* coef /* device; entry may be NULL */, int count /* 1 or 2 */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Differentiable augmentation (not in the reference; Zhao et al., NeurIPS 2020, "DiffAugment"; ABI 25; csrc/diffaug.hip): a
 * random colour change, translation and cutout per image, applied to everything the Discriminator sees -- exactly where the
 * reference perturbs D's inputs with instance noise (vaegan_code.py:91-92) -- and the exact adjoint that carries the
 * Generator's gradient back through it.
 *
 * x, y (forward) and g, dx (backward): images in the engine layout [N][H][W][CP], dtype VG_F32 or VG_BF16, C real channels,
 * CP - C pad channels (read as anything, written as zero); one pixel is a whole number of 16-byte units (CP % 4 == 0 for f32,
 * CP % 8 == 0 for bf16).  params: f32 [PB][8] = {beta, s, k, ty, tx, cy, cx, unused}; N % PB == 0 and image n uses row n % PB
 * (N = 2 B, PB = B: a real image and its reconstruction share one draw).  cut_h, cut_w: the cutout's size, per launch.
 *
 * Forward.  m(p) = (sum_c x_c(p)) / C, M = (sum_{c,p} x_c(p)) / (C H W) over the whole SOURCE image,
 *     col_c(p) = k s x_c(p) + (k - k s) m(p) + (1 - k) M + beta
 * (brightness x + beta, then saturation about the channel mean by s, then contrast about the image mean by k), and
 *     y_c(h, w) = col_c(h + ty, w + tx)   where (h + ty, w + tx) lies in the image and (h, w) is not in the cutout, else 0.
 * The cutout is cy <= h < cy + cut_h and cx <= w < cx + cut_w, clipped by the image; cut_h == 0 or cut_w == 0: no cutout.
 * Backward, the adjoint.  g'_c(p) = g_c(p - t) where p - t lies in the image and is not in the cutout, else 0;
 *     Gsum = sum_{c,p} g'_c(p);   dx_c(p) = k s g'_c(p) + (k - k s) (sum_c' g'_c'(p)) / C + (1 - k) Gsum / (C H W).
 * So <T x, g> = <x, T' g> with T the linear part (beta = 0).
 *
 * Arithmetic: f32, every product, sum and quotient rounded on its own (no contraction into an fma), ONE rounding to dtype on
 * the store.  With v = x (forward) or g' (backward; zero where masked), both directions evaluate, in this order:
 *     ks = k * s;  b = k - ks;  c = 1 - k                                    per image
 *     S  = the whole-image sum, see below;  mean = S / (float)(C H W);  e = c * mean  (forward: e = c * mean + beta)
 *     sc = ((0 + v_0) + v_1) + ... + v_{C-1};  m = sc / (float)C                per pixel, channels ascending
 *     out_c = ((ks * v_c) + (b * m)) + e
 * and the forward then writes 0 where the destination has no source or lies in the cutout (the backward writes out_c
 * everywhere: a pixel whose g' is zero still receives e).  An identity row {0, 1, 1, 0, 0, ., ., .} with no cutout therefore
 * reproduces its input bit for bit, except that -0 is stored as +0.
 * The whole-image sum S (of x, or of g') does not depend on the grid and uses no atomics: the pixels p = h W + w of an image
 * are cut into parts of 1024; in part q thread t (of 256) owns pixels 1024 q + t + 256 j, j < 4, and forms
 * (sc_0 + sc_1) + (sc_2 + sc_3) (sc_j = 0 past the image's end); each 64-thread wave adds its values by the xor butterfly
 * v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1; the part's sum is ((w_0 + w_1) + w_2) + w_3 over the four waves and goes to
 * ws[n * parts + q]; S = (((0 + ws[n][0]) + ws[n][1]) + ...) in ascending part order.  In the backward the sum runs over dx's
 * pixels p of g'.  ws == NULL: the reduce launch is skipped and S = 0 (for callers whose k is 1 in every row: c = 0).
 *
 * Parameter safety.  ty, tx, cy, cx are integers carried in f32; the kernels truncate them toward zero.  NaN or |value| >= 2^30
 * in ty or tx counts as 0, in cy or cx as "no cutout" for that image.  Every source index is bound-checked in integer
 * arithmetic before an address is formed from it: no content of params can cause an out-of-range access (the promise
 * vg_region_mse_forward_backward makes for rects).  beta, s, k are used as they are (a NaN gives NaN pixels).
 *
 * vg_diffaug_params: out f32 [B][8] drawn from rng = {seed, iteration} (device memory) like every in-kernel draw, draw id
 * VG_DRAW_AUGMENT; with w_i = word(VG_DRAW_AUGMENT, 8 b + i) for image b (u01, rint, word: "Degraded pairs" above), all f32:
 *     beta = u01(w_0) - 0.5;  s = 2 * u01(w_1);  k = u01(w_2) + 0.5  (one rounding)
 *     ty = rint(w_3, -sh_h, sh_h + 1), tx = rint(w_4, -sh_w, sh_w + 1),  sh = floor(size / 8 + 0.5) = (size + 4) / 8
 *     cy = rint(w_5, 0, H + 1 - cut_h % 2) - cut_h / 2,  cx likewise from w_6 and W,  cut = floor(size / 2 + 0.5) = (size + 1) / 2
 * policy bits: 1 brightness, 2 saturation, 4 contrast, 8 translation, 16 cutout; a cleared bit writes the identity value (0,
 * 1, 1, 0 and 0, cy = cx = 0); the caller passes cut_h = cut_w = 0 to the apply launches when bit 16 is clear, else the cut
 * sizes above.  H, W < 2^24.  One launch.
 *
 * vg_diffaug_forward / vg_diffaug_backward: at most two launches each (per-part sums into ws, then the apply pass), one
 * workgroup of 256 threads per part, per thread four independent 16-byte loads in flight; no LDS beyond the block sum.
 * HBM traffic with the reduce: 3 passes over the tensor (read, read, write), 2 without.  ws: at least
 * vg_diffaug_ws_floats(N, H, W) = N * ceil(H W / 1024) floats, ws_capacity its capacity in floats.
 * Checked on the host before anything is launched.  VG_EINVAL: in, out or params NULL, in == out, a size < 1, N % PB != 0,
 * C > CP, cut_h or cut_w outside [0, H] / [0, W], H W >= 2^30, ws given but too small.  VG_ENOSUP: VG_FP8 (any dtype but f32 /
 * bf16).  VG_EALIGN: a pixel that is not whole 16-byte units, or in, out, params or ws not 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
#define VG_DRAW_AUGMENT 48
int64_t vg_diffaug_ws_floats(int N, int H, int W);              /* VG_EINVAL (negative) for sizes outside the contract */
int vg_diffaug_params(const uint64_t* rng, int B, int policy, int H, int W, float* out, void* stream);
int vg_diffaug_forward(const void* in, void* out, const float* params, int N, int PB, int H, int W, int C, int CP, int cut_h,
                       int cut_w, float* ws, int64_t ws_capacity, int dtype, void* stream);
int vg_diffaug_backward(const void* in, void* out, const float* params, int N, int PB, int H, int W, int C, int CP, int cut_h,
                        int cut_w, float* ws, int64_t ws_capacity, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tiled denoising (not in the reference, whose networks only take S x S images; ABI 29; csrc/tiling.hip; host plan: tiling.py):
 * an H x W image is cut into ny x nx overlapping S x S tiles, the tiles go through Encoder -> reparameterise -> Generator in
 * batches, and the reconstructions are blended back with a separable window.  Tile t of the global list N * ny * nx belongs to
 * image n = t / (ny nx) and has k = t % (ny nx), ky = k / nx, kx = k % nx, origin (oy[ky], ox[kx]).  No padding: every tile lies
 * inside the image (0 <= oy <= H - S, 0 <= ox <= W - S).
 *
 * Tables (device memory, 4-byte aligned, uploaded once per plan): oy int32 [ny], ox int32 [nx]; per axis and coordinate p the
 * contiguous range of covering tiles first[p], count[p] (int32 [H] / [W]) and their coefficients coef f32 [H][wy] / [W][wx]
 * (row p, slot j belongs to tile first[p] + j; unused slots 0), 1 <= wy, wx <= VG_TILE_MAX_COVER.  The host normalises:
 * coef[p][j] = w[p - o_k] / sum_k w[p - o_k] in f64, rounded once to f32.  The kernels never divide.
 *
 * vg_tile_gather: tiles [t0, t0 + B) as the Encoder's input, out [B][S][S][CP] in dtype (VG_F32 | VG_BF16), pad channels zero:
 * the layout vg_nchw_to_nhwc writes.  Exactly one source: src_u8 [N][H][W][C], the resident set, with exactly
 * vg_gather_normalize_u8's arithmetic (u/255 - 0.5)/0.5; or src_f32 [N][C][H][W], copied (rounded once to bf16).  A chunk may
 * straddle two images and may be shorter than the engine batch.  One launch.
 *
 * vg_tile_blend: out f32 [N][C][H][W] from tiles f32 [N ny nx][C][S][S] (what vg_nhwc_to_nchw writes per chunk, into slices of
 * one buffer), in gather form -- each output element sums its covering tiles, so there are no atomics, no zero-fill, and the
 * result is the same bits on every launch:
 *     inner_ky     = ((0 + cx_0 * r_0) + cx_1 * r_1) + ...      kx = first_x[x] + j ascending, cx_j = coef_x[x][j],
 *                                                               r_j = tiles[n (ny nx) + ky nx + kx][c][y - oy[ky]][x - ox[kx]]
 *     out[n,c,y,x] = ((0 + cy_0 * inner_0) + cy_1 * inner_1) + ...   ky = first_y[y] + j ascending, cy_j = coef_y[y][j]
 * all f32, every product and sum rounded on its own (no contraction into an fma).  One launch; stores are 16-byte vectors
 * aligned to the output row where W % 4 == 0 and out is 16-byte aligned, single floats otherwise; tile rows are read at
 * whatever x origin they have.
 *
 * Table safety.  The host cannot see the tables at launch, so the kernels range-check every index read from them in integer
 * arithmetic before an address is formed from it: count is clamped to [0, width], a tile index outside [0, ny) / [0, nx) or a
 * local coordinate outside [0, S) drops that term (blend), an origin outside the image writes a zero tile (gather).  No content
 * of a table can cause an out-of-range access.
 *
 * Checked on the host before anything is launched.  VG_EINVAL: a NULL pointer (gather: not exactly one source); N, C, S, ny, nx
 * or B < 1; H < S or W < S; ny > H - S + 1 or nx > W - S + 1; N ny nx or N C >= 2^31; S > 32768, H > 262140 or
 * W > 16776960 (the launch grids); t0 < 0 or t0 + B > N ny nx; CP < C; wy or wx
 * outside [1, VG_TILE_MAX_COVER]; tiles == out.  VG_ENOSUP: a dtype other than f32 / bf16.  VG_EALIGN: a pixel that is not whole
 * 16-byte units (CP % 4 for f32, CP % 8 for bf16), the gather's out not 16-byte aligned, an f32 / int32 pointer not 4-byte aligned.
 * ---------------------------------------------------------------------------------------- */
#define VG_TILE_MAX_COVER 8     /* most tiles covering one coordinate of an axis: ceil(S / stride) + 1 for the plans of tiling.py */
int vg_tile_gather(const uint8_t* src_u8, const float* src_f32, int N, int C, int H, int W, int S, int ny, int nx,
                   const int32_t* oy, const int32_t* ox, int64_t t0, int B, void* out, int CP, int dtype, void* stream);
int vg_tile_blend(const float* tiles, float* out, int N, int C, int H, int W, int S, int ny, int nx,
                  const int32_t* oy, const int32_t* ox, const int32_t* first_y, const int32_t* count_y, const float* coef_y,
                  int wy, const int32_t* first_x, const int32_t* count_x, const float* coef_x, int wx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Non-local means baseline and blind noise estimate (not in the reference; added within ABI 31; csrc/nlm.hip): the classical,
 * parameter-free denoiser the evaluation passes report between the noisy input and the model (denoise.py, baselines.py).
 *
 * vg_nlm_denoise: non-local means (Buades, Coll & Morel 2005), pixelwise, uniform patch kernel.  x f32 NCHW [B][C][H][W],
 * contiguous; y of the same shape, y != x (no overlap).  Patch radius P in 0..3, search radius R in 1..10.
 *   Padding.   x~ is x extended by P + R on every side by reflection without repeating the edge (numpy mode="reflect");
 *              min(H, W) >= P + R + 1 is required, so one reflection suffices.
 *   Distance.  For pixel p and each of the K = (2R+1)^2 offsets t (candidates outside the image are the reflected pixels):
 *              d2(p,t) = (1 / (C (2P+1)^2)) * sum_c sum_{|delta|_inf <= P} (x~_c(p+delta) - x~_c(p+t+delta))^2
 *   Weight.    a = max(d2 - 2 sigma_b^2, 0) / h_b^2,  w = exp(-a).  The centre offset has d2 = 0 and w = 1.
 *   Output.    y_c(p) = (sum_t w x~_c(p+t)) / (sum_t w); the final quotient is ONE correctly rounded f32 division, not a
 *              reciprocal multiply.
 *   Per image. sigma_b = sigma[b * sigma_stride] (a device pointer with an element stride, so the call reads column 1 of the
 *              degraded loader's [B][8] rectangle records in place); sigma == NULL means 0.  h_b = h_factor * sigma_b + h_const.
 *              If h_b is not finite or <= 0, or sigma_b is not finite, image b is copied through bit for bit.
 *   Guarantees. Images are independent of each other.  No atomics: two runs are bit-identical.  Nothing is allocated and
 *              there is no host synchronisation: the launch can be captured into a graph.  One launch.
 *   Non-finite pixels may spread within their own image; every access stays in bounds.
 *   Arithmetic. f32 throughout: squared differences by fma over the channels, the patch sum as a separable box sum (rows,
 *              then columns), d2 = S * fl(1 / (C (2P+1)^2)), the weight as ONE hardware base-2 exponential of
 *              max(d2 - 2 sigma^2, 0) * fl(-log2(e) / h^2) (1 ulp; results below 2^-126 are 0), sums over t in row-major
 *              offset order by fma.  tests/_nlm_ref.py counts the first-order error bound of this sequence.
 * VG_EINVAL, checked on the host before the launch: x or y NULL, or the two buffers overlapping; B, C, H or W < 1; C > 4;
 * P outside 0..3 or R outside 1..10; min(H, W) < P + R + 1; sigma != NULL with sigma_stride < 1; h_factor or h_const not finite
 * or negative, or both zero; B C H W > 2^31 - 1 elements, B > 65535 or ceil(H / 16) > 65535 (the launch grid: 16 x 16 output
 * tiles in x / y, images in z), (B - 1) sigma_stride > 2^31 - 1.  VG_EALIGN: a pointer that is not 4-byte aligned (x may sit
 * anywhere on the 4-byte grid: 16-byte loads are used only where an address allows them).
 *
 * vg_noise_sigma: Immerkaer's (1996) fast noise-variance estimate, per image.  With N = [[1,-2,1],[-2,4,-2],[1,-2,1]]:
 *     S_b     = sum_c sum_{1 <= i <= H-2, 1 <= j <= W-2} |(x_c * N)(i,j)|           (interior only, no padding)
 *     sigma_b = (float)((double)S_b * k),   k = sqrt(pi / 2) / (6 C (H-2) (W-2))   computed in double on the host
 * written to sigma[b * sigma_stride].  The mask response is evaluated and summed in f64 in a fixed order (one workgroup per
 * image: rows to waves, columns to lanes, xor butterfly, waves in order): repeatable bit for bit, no atomics, no workspace, no
 * host synchronisation, one launch.  VG_EINVAL: x or sigma NULL; B or C < 1; H or W < 3; sigma_stride < 1; C (H - 2) or
 * (B - 1) sigma_stride > 2^31 - 1 (B itself is the grid's x dimension).  VG_EALIGN: a pointer not 4-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int vg_nlm_denoise(const float* x, float* y, int B, int C, int H, int W, int patch_radius, int search_radius,
                   const float* sigma, int sigma_stride, float h_factor, float h_const, void* stream);
int vg_noise_sigma(const float* x, int B, int C, int H, int W, float* sigma, int sigma_stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Median baseline (not in the reference; added within ABI 31; csrc/median.hip): the textbook filter against impulse noise,
 * where non-local means with a Gaussian sigma has nothing to hold on to.
 * vg_median_filter: y_c(p) = the median of the (2r+1)^2 values of channel c around p, r = radius in {1, 2}; x f32 NCHW
 * [B][C][H][W] contiguous, y of the same shape, no overlap with x.  Border: x extended by r on every side by reflection
 * without repeating the edge (numpy mode="reflect"); min(H, W) >= r + 1, so one reflection suffices.  The output is one of
 * the window's values, selected by a branch-free min / max network: exact for finite inputs (a NaN in a window gives an
 * unspecified value of that window; +0 and -0 compare equal, either may come out).  Channels and images are independent;
 * one launch, no atomics, no workspace, no host synchronisation.
 * VG_EINVAL: x or y NULL or overlapping; B, C, H or W < 1; radius outside 1..2; min(H, W) < radius + 1; B C H W or B C
 * > 2^31 - 1, ceil(H / 16) or ceil(W / 64) > 65535 (the grid: planes in x, 64 x 16 output tiles in z / y).  VG_EALIGN: a
 * pointer not 4-byte aligned (16-byte stores are used where W % 4 == 0 and y is 16-byte aligned).
 * ---------------------------------------------------------------------------------------- */
int vg_median_filter(const float* x, float* y, int B, int C, int H, int W, int radius, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spectral generation metric (not in the reference for images -- it compares the Welch PSD of real and generated EEG,
 * test_eegglow.py:25-46, :79-95; added within ABI 31; csrc/spectrum.hip): per-image binned power spectra of an f32 NCHW
 * batch, the quantity in which stacks of up-convolutions fail (Durall et al. 2020).  The transform is GENERIC: a separable
 * complex transform whose two matrices, the weight map and the bins are the caller's tables (spectrum.py builds windowed
 * DFT tables, the Hermitian-half weight and radial bins), so integer tables with integer images give integer results
 * bit for bit.  With Wh = W / 2 + 1, per image b and channel c, every input converted to f64 exactly:
 *     m       = center ? (sum of the plane) / (H W) : 0        the sum in f64 in this order: partial[t] = sum of plane[i]
 *               over i = t, t + 256, ... ascending (t = 0 .. 255), then partial[t] += partial[t + s] for s = 128, 64, .., 1;
 *               one division
 *     Y[y][v] = sum_x (x[y][x] - m) tw[x][v]                   tw_re, tw_im f64 [W][Wh]
 *     Z[u][v] = sum_y th[u][y] Y[y][v]   (complex)             th_re, th_im f64 [H][H]
 *     P[u][v] = sum_c (Z_re^2 + Z_im^2), c ascending
 *     prof[b][k] = sum over j in [bin_start[k], bin_start[k+1]) of weight[order[j]] P[order[j]], added in ascending j
 * weight f64 [H][Wh]; order int32 [bin_start[n_bins]] (flat indices u Wh + v), bin_start int32 [n_bins + 1]: CSR.  The
 * matrix products run on v_mfma_f64_16x16x4_f64 (the order of additions inside a product is the hardware's); rows and
 * columns past H, W, Wh are staged as zeros and never multiplied in; the negation of the complex product is applied to an
 * operand.  The bin sum's order is part of the contract: no atomics anywhere, a call is repeatable bit for bit, images are
 * independent of each other.  Three launches (mean -- skipped without center --, transform, bins), nothing allocated, no
 * host synchronisation.
 *   Table safety. An `order` entry outside [0, H Wh) contributes nothing and is never dereferenced.  With nnz =
 *   bin_start[n_bins] clamped into [0, H Wh], a bin whose bounds are not 0 <= bin_start[k] <= bin_start[k+1] <= nnz
 *   contributes nothing (prof = 0): whatever the device tables hold, nothing outside the buffers is read (order must hold
 *   nnz entries) and nothing outside prof / power / ws is written.
 *   power f64 [B][H][Wh] or NULL: the channel-summed map P; with NULL it lives in ws.  prof f64 [B][n_bins].
 *   ws: vg_spectrum_ws_bytes = 8 (B C + B H Wh) bytes (the plane means, then the map), a host-only query.
 * VG_EINVAL, checked on the host before any launch: a NULL pointer (power excepted; `bytes` of the query); an output
 * (prof, power, ws) overlapping an input or another output; B < 1, C outside 1..4, H or W outside 2..256, B C H W or
 * B n_bins > 2^31 - 1; n_bins outside 1..H Wh; center outside {0, 1}; ws_bytes below the query's answer.  VG_EALIGN: x, order
 * or bin_start not 4-byte aligned (x may sit anywhere on the 4-byte grid), an f64 buffer or ws not 8-byte aligned.
 *
 * vg_spectrum_accum: sum[k] += prof[b][k] and sumsq[k] += prof[b][k]^2 for b = 0 .. B - 1 ascending, each bin by one thread
 * (s = sum[k]; s += p_0; s += p_1; ...; the squares enter by a fused multiply-add, q = fma(p_b, p_b, q): one rounding a
 * step): prof f64 [B][n_bins], sum and sumsq f64 [n_bins].  One launch, repeatable.
 * VG_EINVAL: a NULL pointer, overlapping buffers, B < 1, n_bins outside 1..256 * 129, B n_bins > 2^31 - 1.  VG_EALIGN: a
 * pointer not 8-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int vg_spectrum_ws_bytes(int B, int C, int H, int W, int64_t* bytes);
int vg_spectrum_profiles(const float* x, int B, int C, int H, int W, int center, const double* tw_re, const double* tw_im,
                         const double* th_re, const double* th_im, const double* weight, const int32_t* order,
                         const int32_t* bin_start, int n_bins, double* power, double* prof, void* ws, int64_t ws_bytes,
                         void* stream);
int vg_spectrum_accum(const double* prof, int B, int n_bins, double* sum, double* sumsq, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAEGAN_HIP_H */
