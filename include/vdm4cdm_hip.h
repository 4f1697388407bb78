/* vdm4cdm_hip.h - C-ABI of libvdm4cdm_hip.so: the MI355X (gfx950) kernels of the vdm4cdm
 * variational-diffusion denoising hot path.
 *
 * The reference (cfpark00/vdm4cdm) has no FFI layer: its hot path is the Python API between its
 * scripts and the third-party `mltools` package, which bottoms out in ATen ops.  Each entry point
 * below replaces the ATen op family that one reference call reaches (SURVEY.md section 8a rows
 * R1-R12); the reference-side call that would bind it is cited per function as
 * [REF file:line] (files under /root/reference) or [NB ...] (notebook traceback fragment,
 * SURVEY.md section 3.2).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless named host_*.
 *  - the caller owns every buffer (they are torch tensors' data_ptr()s); the library never
 *    allocates device memory and never synchronises: all work is enqueued on `stream`
 *    (a hipStream_t passed as void*; NULL = the null stream).
 *  - activations are NDHWC: x[n][z][y][x][c], dtype VDM_F32 or VDM_BF16 (bf16 = storage only,
 *    arithmetic and accumulation are fp32).  Channel counts of conv inputs must be a multiple of
 *    16 bytes (4 fp32 / 8 bf16 elements); the host zero-pads (e.g. conv_in's 2 channels).
 *  - every function returns VDM_OK (0) or a negative vdm_status; vdm_last_error() returns a
 *    thread-local message.  No exceptions cross the boundary; HIP errors are translated.
 */
#ifndef VDM4CDM_HIP_H
#define VDM4CDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDM_ABI_VERSION 21

typedef enum { VDM_OK = 0, VDM_ERR_ARG = -1, VDM_ERR_HIP = -2, VDM_ERR_UNSUPPORTED = -3 } vdm_status;
typedef enum { VDM_F32 = 0, VDM_BF16 = 1 } vdm_dtype;
typedef enum { VDM_PAD_ZEROS = 0, VDM_PAD_CIRCULAR = 1 } vdm_pad_mode; /* [REF trainVDM3D128_c_c_from_field_name_thick_lowbatch.py:125] conv_padding_mode */
typedef enum { VDM_PACK_FWD = 0, VDM_PACK_DGRAD = 1 } vdm_pack_mode;

/* One 3D convolution (k in {1,3}, stride in {1,2}, optional fused nearest x2 up-sampling of the
 * input).  od/oh/ow are the OUTPUT spatial dims.  Input dims: stride 1: the same; stride 2: 2x
 * (k=3, pad 1); upsample: the source tensor is (od/2, oh/2, ow/2) and is read at (z>>1,y>>1,x>>1). */
typedef struct {
    int32_t n, od, oh, ow;
    int32_t cin, cout;
    int32_t ksize;    /* 1 or 3 */
    int32_t stride;   /* 1 or 2 */
    int32_t upsample; /* 0 or 1 (only with stride 1, ksize 3) */
    int32_t pad_mode; /* vdm_pad_mode */
    int32_t dtype;    /* vdm_dtype of x / residual / out */
    int32_t out_f32;  /* 1: write `out` as fp32 regardless of dtype (conv_out -> eps_hat) */
} vdm_conv_desc;

const char* vdm_last_error(void);
int vdm_abi_version(void);
/* fills cu_count / lds_bytes_per_cu / gcn arch name (buffer of >= 64 bytes) for `device`. */
int vdm_device_info(int device, int* cu_count, int* lds_bytes, char* arch_name);

/* ---- K1/K3/K4/K5: convolution (implicit GEMM on MFMA) -------------------------------------
 * Replaces torch.nn.functional.conv3d as reached from ResNetBlock.net1/net2, ResNetDown and the
 * up path [NB blocks.py:129-132,166-170; networks.py:259-265].
 * Master weights are fp32 [taps][cout][cin] (tap = (dz*3+dy)*3+dx).  They are re-packed into the
 * MFMA fragment order once per optimiser step. */
size_t vdm_conv_packed_bytes(const vdm_conv_desc* d, int pack_mode);
int vdm_conv_pack_weights(const vdm_conv_desc* d, int pack_mode, const float* w_master, void* w_packed, void* stream);
/* All packings of a network in one launch (they are redone after every optimiser step).  vdm_conv_pack_plan fills one work item
 * per (conv, form) on the host; the caller cuts [0, item.elems) of every item into chunks of <= VDM_PACK_CHUNK elements, uploads the
 * item and chunk arrays once, and calls vdm_conv_pack_many on them whenever the master weights changed.  All items of one call
 * share the dtype. */
#define VDM_PACK_CHUNK 16384
typedef struct vdm_pack_item {
    const float* w_master;
    void* w_packed;
    int32_t taps, cout, cin, nc, nchunks, nkb, dgrad, variant, cls_kind, dtype;
    int64_t elems; /* packed elements of this item */
} vdm_pack_item;
typedef struct vdm_pack_chunk {
    int32_t item;  /* index into the item array */
    int32_t count; /* elements in this chunk */
    int64_t first; /* first packed element (inside the item) */
} vdm_pack_chunk;
int vdm_conv_pack_plan(const vdm_conv_desc* d, int pack_mode, const float* w_master, void* w_packed, vdm_pack_item* item);
int vdm_conv_pack_many(const vdm_pack_item* items_device, const vdm_pack_chunk* chunks_device, int nchunks, int dtype, void* stream);
/* out = conv(x, w) + bias[c] + nbias[n*nbias_stride + c] + residual   (bias, nbias, residual may be NULL).
 * nbias is the per-sample conditioning bias table (sum_k Linear_k(cond_k)); nbias_stride is the
 * element distance between samples (the table of all blocks is one [n][sum cout] matrix). */
/* gn_partials (may be NULL): the epilogue also reduces the GroupNorm statistics of the output it stores, per spatial tile:
 * gn_partials[n][tile][cout][2] = (sum, sum of squares) fp32, tile < vdm_conv_gn_tiles(d); feed them to vdm_gn_stats instead of
 * a separate pass over the tensor (the up-sampling conv has one slot per coarse tile and parity class). */
int vdm_conv_gn_tiles(const vdm_conv_desc* d);
int vdm_conv_fwd(const vdm_conv_desc* d, const void* x, const void* w_packed_fwd, const float* bias,
                 const float* nbias, int64_t nbias_stride, const void* residual, void* out, float* gn_partials, void* stream);
/* dx = gradient w.r.t. the conv INPUT: the descriptor is the FORWARD conv's; dout has cout channels and the output
 * dims (od,oh,ow); dx gets cin channels and the input dims (stride 1: same; stride 2: 2x; up-sampling conv: the
 * coarse source grid od/2...).  Stride-2 and up-sampling convs run as per-parity-class convs (no dilated /
 * up-sampled intermediate). */
int vdm_conv_dgrad(const vdm_conv_desc* d, const void* dout, const void* w_packed_dgrad, const void* residual, void* dx,
                   void* stream); /* dx = dgrad (+ residual, same shape as dx, may be NULL) */
/* The same input gradient for a conv whose INPUT was y = dropout(silu(groupnorm(x))) [NB blocks.py:129-132: net1 / net2 =
 * Sequential(GroupNorm, SiLU, (Dropout,) Conv)], with the first half of that GroupNorm's backward folded into the epilogue:
 * instead of dL/dy the kernel stores dyh = dL/dy * keep/(1-p) * silu'(yhat) (same shape and dtype) and reduces, per spatial tile
 * and channel, partials[n][tile][cin][2] = (sum dyh, sum dyh * x), tile < vdm_conv_dgrad_gn_tiles(d) - one read of x instead of
 * a separate two-tensor reduction pass, in a fixed order (no float atomics).  vdm_gn_bwd_finalize + vdm_gn_bwd_apply finish the
 * GroupNorm backward.  Only for ksize 3, stride 1, no up-sampling (every conv behind a GroupNorm on the path). */
typedef struct vdm_gn_fold {
    const void* x1;          /* GroupNorm input, first c1 channels  [n][od][oh][ow][c1] */
    const void* x2;          /* ... remaining c2 channels (skip concat), or NULL */
    int32_t c1, c2, groups;  /* c1 + c2 == cin of the conv */
    const float* stats;      /* [n][groups][2] raw moments of x (vdm_gn_stats) */
    const float* gamma;      /* [cin] */
    const float* beta;       /* [cin] */
    float eps;
    float inv_keep;          /* 1 / (1 - p) when keep_mask is given */
    const uint8_t* keep_mask; /* dropout keep bits written by vdm_gn_silu_fwd, or NULL (no dropout) */
    float* partials;         /* out */
} vdm_gn_fold;
int vdm_conv_dgrad_gn_tiles(const vdm_conv_desc* d);
int vdm_conv_dgrad_gn(const vdm_conv_desc* d, const void* dout, const void* w_packed_dgrad, void* dyh, const vdm_gn_fold* fold,
                      void* stream);
/* Which kernel family vdm_conv_fwd (dgrad = 0) / vdm_conv_dgrad (dgrad = 1) launches for this descriptor (profiling keys,
 * tests): one of the VDM_CONV_VARIANT_* values below.  < 0: bad descriptor. */
#define VDM_CONV_VARIANT_GENERIC 0 /* the generic implicit-GEMM kernel */
#define VDM_CONV_VARIANT_CLASS 1 /* per-parity-class kernel: up-sampling conv and its gradients, stride-2 dgrad */
#define VDM_CONV_VARIANT_KPACK 2 /* <= 8 reduction channels (conv_in, conv_out's input gradient): 4 taps per MFMA K-step */
#define VDM_CONV_VARIANT_SPLIT 3 /* generic kernel, half-chunk workgroups (64-cout chunks on a small grid) */
#define VDM_CONV_VARIANT_KSPLIT 4 /* deepest level: the waves of a workgroup split the K-blocks, one weight fetch per workgroup */
int vdm_conv_kernel_variant(const vdm_conv_desc* d, int dgrad);
/* The host-side plan vdm_conv_fwd (dgrad = 0) / vdm_conv_dgrad (dgrad = 1) follows for this descriptor (csrc/conv_common.h plan_of;
 * host only, no HIP call): kernel family, packed-weight layout, channel blocking, spatial tile, whether the launch rolls up z and how
 * it is segmented, and the launch grid.  Tests and profiling tools read it instead of restating the rules; vdm_conv_kernel_variant,
 * vdm_conv_gn_tiles, vdm_conv_dgrad_gn_tiles and vdm_conv_packed_bytes answer from the same plan.  Returns VDM_OK, or the status the
 * launch would return for the descriptor (VDM_ERR_UNSUPPORTED: an fp32 output of bf16 storage that is not built) with `out` filled. */
#define VDM_CONV_CLS_UP_FWD 0   /* cls_kind of a VDM_CONV_VARIANT_CLASS plan: up-sampling conv forward (8 merged taps per class) */
#define VDM_CONV_CLS_UP_DGRAD 1 /* its input gradient (one workgroup loops over the 8 classes) */
#define VDM_CONV_CLS_S2_DGRAD 2 /* stride-2 conv, input gradient (1 / 2 / 4 / 8 taps per class) */
typedef struct {
    int32_t family;          /* VDM_CONV_VARIANT_*: the kernel */
    int32_t layout;          /* VDM_CONV_VARIANT_GENERIC | _CLASS | _KPACK: the packed-weight layout */
    int32_t cls_kind;        /* VDM_CONV_CLS_* when family is VDM_CONV_VARIANT_CLASS, else 0 */
    int32_t nc;              /* 16-channel output tiles per packed chunk (SPLIT workgroups take half a chunk) */
    int32_t nchunks;         /* output-channel chunks */
    int32_t nkb;             /* reduction-channel blocks (32 channels bf16, 16 fp32) */
    int32_t tz, ty;          /* spatial tile (x extent 16), of the coarse grid for the class kernels */
    int32_t roll;            /* 1: rolling-z kernel (persistent workgroups walk up tile columns) */
    int32_t nseg, zsteps;    /* rolling z: segments per tile column, z steps per segment (the last segment may be shorter); else 0 */
    int32_t tiles;           /* per-sample tiles of the GroupNorm partials (vdm_conv_gn_tiles / vdm_conv_dgrad_gn_tiles) */
    int32_t workgroups;      /* launch grid */
    int32_t reserved;
    size_t packed_bytes;     /* vdm_conv_packed_bytes of this direction */
} vdm_conv_plan_info;
int vdm_conv_plan(const vdm_conv_desc* d, int dgrad, vdm_conv_plan_info* out);

/* dw[taps][cout][cin] (fp32) = sum over voxels; workspace holds per-workgroup partial slabs.
 * dbias (optional, ksize 3 only): dbias[cout] = sum over samples and voxels of dout (the conv bias gradient), computed
 * from the dOut tiles the kernel stages anyway.  accumulate != 0 adds to dw / dbias instead of overwriting. */
/* Workspace: vdm_conv_wgrad needs exactly the `workspace_bytes` of its plan (vdm_conv_wgrad_plan with want_bias = (dbias != NULL)
 * and the same accumulate) and returns VDM_ERR_ARG for less.  vdm_conv_wgrad_workspace_bytes(d) is the largest of them over the four
 * (want_bias, accumulate) combinations - those flags change which kernel serves a descriptor - so it is sufficient for any call
 * with this descriptor; 0 for a bad descriptor. */
size_t vdm_conv_wgrad_workspace_bytes(const vdm_conv_desc* d);
int vdm_conv_wgrad(const vdm_conv_desc* d, const void* x, const void* dout, float* dw, float* dbias, int accumulate,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The host-side plan vdm_conv_wgrad follows for this descriptor (ABI v15; csrc/conv_common.h plan_wgrad; host only, no HIP call):
 * which kernel, its spatial tile, the launch grid and the workspace.  Planning queries, profiling tools and tests read it instead
 * of restating the rules.  Returns VDM_OK or the status vdm_conv_wgrad would return for the descriptor (VDM_ERR_UNSUPPORTED: fused
 * bias gradient with ksize 1). */
#define VDM_WGRAD_THIN_IN 0   /* <= 2 input channels (conv_in): the (tap, channel) pairs are the MFMA's N dimension (csrc/wgrad_thin.hip) */
#define VDM_WGRAD_THIN_OUT 1  /* one output channel (conv_out), same kernel with the roles of x and dout swapped */
#define VDM_WGRAD_ROWS 2      /* bf16 3x3x3 stride 1, whole 32-channel blocks: row-reuse kernel over scattered tiles */
#define VDM_WGRAD_ROWS_ROLL 3 /* the same with a rolling z window: persistent workgroups walk segments of tile columns */
#define VDM_WGRAD_TAPSPLIT 4  /* generic tap-split kernel (fp32, stride 2, ksize 1, single-16-channel-tile forms) */
#define VDM_WGRAD_CLASS 5     /* up-sampling conv: 8 parity classes x 8 merged taps on the coarse grid */
typedef struct {
    int32_t kernel;          /* VDM_WGRAD_* */
    int32_t tz, ty;          /* spatial tile (x extent 16); 0 for the thin-side kernels, which walk chunks of 32 voxels along x */
    int32_t workgroups;      /* launch grid of the main kernel */
    int32_t tiles;           /* tiles (rolling window: column segments) that the P workgroups of one channel-block pair walk; thin-side: 0 */
    int32_t P;               /* partial slabs per channel-block pair (= per-pair workgroups); thin-side: slabs in all */
    size_t workspace_bytes;  /* what vdm_conv_wgrad requires for these (want_bias, accumulate) */
} vdm_wgrad_plan_info;
int vdm_conv_wgrad_plan(const vdm_conv_desc* d, int want_bias, int accumulate, vdm_wgrad_plan_info* out);

/* ---- K2: GroupNorm + SiLU (+ dropout) -----------------------------------------------------
 * Replaces torch.group_norm / F.silu / F.dropout [NB normalization.py:273 frame under blocks.py:130].
 * The input may be the channel-concatenation of two tensors (skip connection), never materialised.
 * stats[n][g] = {sum, sumsq} in fp32 (raw moments; mean/rstd are derived where consumed).
 * workspace: VDM_GN_STATS_WS_BYTES of scratch for the per-workgroup partials (two-stage, fixed-order
 * reduction: the forward pass is bit-reproducible).
 * Limits (VDM_ERR_ARG with a message, before any launch - a refused call writes nothing):
 *  - groups <= 64, c1 + c2 <= 512, c1 + c2 divisible by groups, no group across the concat boundary;
 *  - a source given as conv partials: at most 256 channels per group ((c1 + c2) / groups; one thread per channel folds the tiles);
 *  - a source read in full: the pass writes n * B rows of 2 * groups floats into the workspace, B = workgroups per sample
 *    (<= 2048 / n, a multiple of m = P / gcd(P, 256) with P = 16-byte pieces per voxel of that source, at least m); never more
 *    than VDM_GN_STATS_WS_BYTES - a call whose n * m rows alone exceed it (n > 2048 / m with 64 groups) is refused. */
#define VDM_GN_STATS_WS_BYTES (2048 * 2 * 64 * 4)
/* part1 / part2 (may be NULL): per-tile channel partials of that source written by vdm_conv_fwd (tilesK tiles per sample);
 * the source's groups are then summed from them and xK is not read (xK may be NULL). */
/* chsum (may be NULL; needs every source given as partials): chsum[n][c1+c2] = sum_v x[n][v][c], the per-channel sums. */
int vdm_gn_stats(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups,
                 int dtype, float* stats, float* workspace, const float* part1, int tiles1, const float* part2, int tiles2,
                 float* chsum, void* stream);
/* y[n][v][c1+c2] = dropout(silu(gn(concat(x1,x2)))) ; keep-mask from Philox(seed, element index).
 * linear != 0: no activation - the plain GroupNorm in front of the attention block's qkv projection (mid_attn=True).
 * keep_mask (may be NULL): with dropout_p > 0 the keep bits are also written, one byte per 16-byte piece of y
 * ([n][voxels][(c1+c2) / (4 fp32 | 8 bf16)], bit j = channel j of the piece), for vdm_conv_dgrad_gn.
 * seed_step (may be NULL; also vdm_gn_dyh, vdm_randn, vdm_train_scalars): DEVICE step counter mixed into the seed inside the kernel
 * (seed + *seed_step * 0x9E3779B97F4A7C15) - a hipGraph of the training step bakes the host seed into its kernel arguments; the
 * counter, bumped once per replay (vdm_step_inc), keeps dropout masks, noise fields and the time grid fresh. */
int vdm_gn_silu_fwd(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups,
                    int dtype, const float* stats, const float* gamma, const float* beta, float eps,
                    float dropout_p, uint64_t seed, void* y, uint8_t* keep_mask, int linear, const int32_t* seed_step, void* stream);
/* Backward of the above for a GroupNorm whose gradient did not come out of vdm_conv_dgrad_gn, first of three steps:
 * dyh = dy * keep/(1-p) * silu'(yhat) (linear != 0: dyh = dy); dyh may alias dy.  Then vdm_channel_dot_sums(dyh, x) gives the
 * per-sample (sum dyh, sum dyh * x) = the one-tile-per-sample `partials` of vdm_gn_bwd_finalize, and vdm_gn_bwd_apply writes dx:
 * the same fixed-order (bit-reproducible) arithmetic as the folded path; no float atomics. */
int vdm_gn_dyh(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype, const float* stats,
               const float* gamma, const float* beta, float eps, float dropout_p, uint64_t seed, const void* dy, void* dyh, int linear,
               const int32_t* seed_step, void* stream);

/* Second half of the GroupNorm backward after vdm_conv_dgrad_gn (all in fixed summation order: bit-reproducible).
 * finalize: chan[n][c][2] = sum over tiles of the partials; red[n][g][2] = sum_c gamma_c chan[n][c];
 *           colsum (may be NULL; needs chsum of vdm_gn_stats): colsum[n*colsum_stride + c] = sum_v dx[n][v][c], analytically
 *           (the conditioning-table / conv-bias gradient of the ResNetBlock: h = conv1(..) + bias + sum_k Linear_k(cond_k)).
 * apply:    dx = rstd * (gamma * dyh - m1 - xhat * m2) (+ add1 / add2: residual-path gradients), m = red / (voxels * C/groups);
 *           dgamma[c] = sum_n chan[n][c][1], dbeta[c] = sum_n chan[n][c][0] (written, not accumulated).  dx1 may alias dyh. */
int vdm_gn_bwd_finalize(const float* partials, int tiles, int n, int c, int groups, int64_t voxels, const float* stats,
                        const float* gamma, float eps, const float* chsum, float* red, float* chan, float* colsum,
                        int64_t colsum_stride, void* stream);
int vdm_gn_bwd_apply(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype,
                     const float* stats, const float* gamma, float eps, const void* dyh, const float* red, const float* chan,
                     const void* add1, const void* add2, void* dx1, void* dx2, float* dgamma, float* dbeta, void* stream);

/* ---- ResNetBlock skip path folded into the GroupNorm passes (bf16 storage) ------------------------------------------------
 * [NB blocks.py ResNetBlock: out = net2(net1(x) + cond) + skip(x), skip = Conv3d(cin, cout, 1) when cin != cout; call chain
 * trainVDM3D128_c_c_from_field_name_thick_lowbatch.py:116-127.]  norm1 and the 1x1x1 skip conv read the same block input, and the
 * skip conv's input gradient is added to the result of norm1's backward: one pass each instead of a conv launch of their own.
 *   vdm_gn_skip_supported: bit 0 = the forward kernel, bit 1 = the backward kernel exist for (c1 + c2 -> cout) in `dtype`
 *     (host only; 0 for fp32 storage and for wide layers, which keep vdm_conv_fwd / vdm_conv_dgrad / vdm_conv_wgrad with ksize 1).
 *   vdm_gn_silu_skip_fwd: y = silu(gn(concat(x1, x2)))  [n][voxels][c1+c2]  (vdm_gn_silu_fwd without dropout) AND
 *     skip_out[n][voxels][cout] = w1 x1 + w2 x2 + bias, w1 [cout][c1], w2 [cout][c2] = the fp32 MASTER weights of the two column
 *     blocks of the skip conv (rounded to bf16 in the kernel like vdm_conv_pack_weights does), bias [cout] or NULL.
 *   vdm_gn_bwd_apply_skip: vdm_gn_bwd_apply with add = W^T dout computed in the pass (dout [n][voxels][cout] = the gradient of the
 *     block output), plus the skip weight gradients dw1 [cout][c1], dw2 [cout][c2] = sum_{n,v} dout x (written, not accumulated;
 *     per-workgroup slabs in `workspace` (vdm_gn_skip_ws_floats floats) + a fixed-order reduce: bit-reproducible).  The skip bias
 *     gradient is the column sum of dout, which vdm_conv_wgrad of the block's second conv already returns. */
/* The LAST GroupNorm backward of the network (norm1 of the first block) and the weight gradient of conv_in in one pass (bf16): the
 * tensor vdm_gn_bwd_apply would write there - the gradient at the output of conv_in - has no reader but that weight gradient, so it is
 * formed in registers (dx = rstd (gamma dyh - m1 - xhat m2) + add, rounded to bf16 like the tensor it replaces) and fed straight into
 * dw[27][c][thin_c] = sum_v dx[v] (x) thin_x[v + tap], dbias[c] = sum_v dx[v]; dgamma / dbeta as vdm_gn_bwd_apply.  x / dyh / add:
 * [n][od][oh][ow][c] with c in {16, 32, 64}; thin_x: the conv_in input [n][od][oh][ow][8] (thin_c <= 2 real channels); workspace:
 * vdm_conv_wgrad_workspace_bytes of conv_in.  Replaces a 3-tensor pass + a write and a read of dx on the exposed tail of the
 * backward pass. */
int vdm_gn_bwd_apply_wgrad_thin(const void* x, int c, int n, int od, int oh, int ow, int groups, const float* stats, const float* gamma,
                                float eps, const void* dyh, const float* red, const float* chan, const void* add, const void* thin_x,
                                int thin_c, int circular, float* dgamma, float* dbeta, float* dw, float* dbias, void* workspace,
                                size_t workspace_bytes, void* stream);
int vdm_gn_skip_supported(int c1, int c2, int cout, int dtype);
size_t vdm_gn_skip_ws_floats(int c1, int c2, int cout, int n, int64_t voxels);
int vdm_gn_silu_skip_fwd(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype,
                         const float* stats, const float* gamma, const float* beta, float eps, const float* w1, const float* w2,
                         const float* bias, int cout, void* y, void* skip_out, void* stream);
int vdm_gn_bwd_apply_skip(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype,
                          const float* stats, const float* gamma, float eps, const void* dyh, const float* red, const float* chan,
                          const void* dout, const float* w1, const float* w2, int cout, void* dx1, void* dx2, float* dgamma,
                          float* dbeta, float* dw1, float* dw2, float* workspace, size_t workspace_floats, void* stream);

/* ---- small tensor ops on the path ------------------------------------------------------------ */
/* out[n][v][cpad] <- channels {a[n][v], b[n][v] (b may be NULL)} zero-padded to cpad; a,b fp32. */
int vdm_pack_input(const float* a, const float* b, int64_t nvox, int cpad, int dtype, void* out, void* stream);

/* ---- K6: conditioning embeddings -> additive injection table of all ResNetBlocks [R5; D4/D7] -------------------
 * Replaces the ATen chain behind score_model(zt, t=(gamma_t-gamma_min)/(gamma_max-gamma_min), v_conditionings=[...])
 * [NB vdm_model.py:320-324, networks.py:259-265]: per conditioning  c = GELU(Linear2(GELU(Linear1(in))))  with
 * in = sinusoidal embedding of t (sinusoid != 0: `input` is t[rows]) or the raw vector (input[rows][in_dim]), and
 * table[row][w] = sum_k c_k[row] . wproj_k[w]   over the concatenated output channels w of all blocks.
 * `mlps` is a HOST array of n <= 4 descriptors holding DEVICE pointers.  saved: vdm_cond_saved_floats() floats kept for the
 * backward (may be NULL for inference).  bwd writes dw1/db1/dw2/db2/dwproj of every descriptor (plain stores) and, if dbias is
 * given, dbias[w] = sum_rows dtable[row][w] (the conv1 bias gradients); scratch: >= vdm_cond_bwd_scratch_floats() floats
 * (the per-row (dh1, dh2) vectors + the fixed-order slab partials of dtable . Wproj).  Widths: in_dim, dim <= 256; a weight matrix whose
 * row length is a multiple of 4 must be 16-byte aligned.  rows <= 65535 per call.
 * step: table[b] = table_t[*step_ptr] + table_v[b] (either may be NULL) - the per-step row gather of the captured sampler graph. */
typedef struct vdm_cond_mlp {
    const float* input;
    int32_t in_dim, dim, sinusoid, reserved;
    const float* w1; const float* b1; /* [dim][in_dim], [dim] */
    const float* w2; const float* b2; /* [dim][dim], [dim] */
    const float* wproj;               /* [width][dim] */
    float* dw1; float* db1; float* dw2; float* db2; float* dwproj; /* backward outputs (NULL in forward) */
} vdm_cond_mlp;
size_t vdm_cond_saved_floats(const vdm_cond_mlp* mlps, int n, int rows);
size_t vdm_cond_bwd_scratch_floats(const vdm_cond_mlp* mlps, int n, int rows, int width);
int vdm_cond_table_fwd(const vdm_cond_mlp* mlps, int n, int rows, int width, float* table, float* saved, void* stream);
int vdm_cond_table_bwd(const vdm_cond_mlp* mlps, int n, int rows, int width, const float* dtable, int64_t dtable_stride,
                       const float* saved, float* scratch, float* dbias, void* stream);
int vdm_cond_table_step(const float* table_t, const float* table_v, const int32_t* step_ptr, int rows, int width, float* out,
                        void* stream);
/* K6i (ABI v13): input gradients of the conditioning MLPs, enqueued after vdm_cond_table_bwd with the same mlps / rows / width, saved and
 * scratch (it reads the dh1 rows the backward left there): d input = W1^T dh1 per row.  host_dinputs: a HOST array of n DEVICE pointers
 * (4-byte aligned; NULL = not wanted): a vector conditioning receives [rows][in_dim], the sinusoidal t embedding the chain rule through
 * [sin(1000 t f_i), cos(1000 t f_i)] folded into one dL/dt per row ([rows]).  Guidance / inverse problems / learned noise schedules
 * [NB vdm_model.py:320-324: t = (gamma_t - gamma_min) / (gamma_max - gamma_min)]. */
int vdm_cond_input_grad(const vdm_cond_mlp* mlps, int n, int rows, int width, const float* saved, const float* scratch,
                        float* const* host_dinputs, void* stream);

/* ---- K7/K8: VDM forward diffusion + ELBO pieces [R7; D9/D10] -----------------------------------
 * z_t = alpha[n] x + sigma[n] eps  (fp32, contiguous per sample of `per` elements).  per % 4 == 0.
 * vdm_diffuse, vdm_diffuse_pack and vdm_loss_terms_rng read and write their fields as 16-byte vectors: every non-NULL field pointer
 * (x, eps, z_t; x, s_cond, eps, z_t, packed; x, eps, eps_hat, eps0, d_eps_hat) must be 16-byte aligned, else VDM_ERR_ARG with a message
 * before any launch. */
int vdm_diffuse(const float* x, const float* eps, const float* alpha, const float* sigma, int n, int64_t per,
                float* z_t, void* stream);
/* sums[n][3] += {sum (eps-eps_hat)^2, sum x^2, sum (x - z0r)^2} with z0r = x + (sigma0/alpha0) eps0;
 * d_eps_hat = coef[n] * (eps_hat - eps)   (coef folds bpd * gamma'(t) / B).  Caller zeroes sums. */
/* workspace: VDM_REDUCE_WS_ROWS * 3 floats (per-workgroup partials, one row per block, folded in a fixed order: the loss is
 * bit-reproducible).  Its size is not an argument: the entries that write partials (vdm_loss_terms, vdm_loss_terms_rng,
 * vdm_schedule_grad_sums) launch at most max(1, VDM_REDUCE_WS_ROWS / n) blocks per sample and therefore refuse
 * n > VDM_REDUCE_WS_ROWS. */
#define VDM_REDUCE_WS_ROWS 2048
int vdm_loss_terms(const float* x, const float* eps, const float* eps_hat, const float* eps0, float sigma0_over_alpha0,
                   const float* coef, int n, int64_t per, float* sums, float* d_eps_hat, float* workspace, void* stream);

/* Fused head of the training step (ABI v11) [replaces the randn_like -> alpha x + sigma eps -> cat([z_t, s_conditioning]) chain of
 * VDM.get_loss + CUNet.forward, NB vdm_model.py:309-327 / networks.py:259-265]: z_t = alpha[n] x + sigma[n] eps, written as fp32
 * (z_t, may be NULL) AND as conv_in's NDHWC input packed[n][voxel][16 B] = {z_t, s_cond (0 if NULL), 0 ...} in `dtype` - one pass over
 * x instead of vdm_randn + vdm_diffuse + vdm_pack_input.  eps == NULL: the noise is drawn inside the kernel from the Philox counters
 * (seed, stream_id, element group; seed_step as for vdm_randn) - exactly the field vdm_randn(seed, stream_id) would have written;
 * eps != NULL: supplied noise (parity tests).  per % 4 == 0. */
int vdm_diffuse_pack(const float* x, const float* s_cond, const float* eps, uint64_t seed, uint64_t stream_id, const int32_t* seed_step,
                     const float* alpha, const float* sigma, int n, int64_t per, int dtype, float* z_t, void* packed, void* stream);
/* vdm_loss_terms with eps and / or eps0 regenerated from their Philox counters when NULL (the fields vdm_randn(seed_eps, stream_eps) /
 * vdm_randn(seed_eps0, stream_eps0) would have written): the training step never materialises its noise fields.  per % 4 == 0;
 * workspace as vdm_loss_terms.  With both fields supplied the sums equal this kernel's sums for the regenerated fields bit for bit. */
int vdm_loss_terms_rng(const float* x, const float* eps, uint64_t seed_eps, uint64_t stream_eps, const float* eps_hat, const float* eps0,
                       uint64_t seed_eps0, uint64_t stream_eps0, const int32_t* seed_step, float sigma0_over_alpha0, const float* coef, int n,
                       int64_t per, float* sums, float* d_eps_hat, float* workspace, void* stream);

/* ---- input gradients of the network and the learned schedule (ABI v13) [noise_schedule="learned_linear",
 * REF train3D_c_c_from_field_name.py:124-129] -------------------------------------------------------------------------------------
 * K1t conv_in_dgrad: dz / ds = the gradient w.r.t. conv_in's two input channels (z_t, s_conditioning) from dh = d loss / d conv_in output
 *   (NDHWC [n][d][h][w][c], `dtype`, 16-byte aligned; c in {16, 32, 48, 64}): the transposed 3x3x3 conv with conv_in's fp32 master
 *   weight [27 taps][c][cin] (cin in {1, 2}), zeros or circular padding, fp32 outputs [n][d][h][w] (ds may be NULL; needs cin == 2).
 * K7b schedule_grad_sums: sums[n][2] = {sum dz x, sum dz eps} over the `per` elements of sample n - with alpha' and sigma' the gradient
 *   of z_t = alpha x + sigma eps w.r.t. gamma_t.  eps == NULL: regenerated from its Philox counters (seed_eps, stream_eps, seed_step as
 *   vdm_diffuse_pack: the same field).  Fixed-order two-stage reduction, no atomics (bit-reproducible).  per % 4 == 0; dz / x / eps
 *   16-byte aligned; workspace as vdm_loss_terms (VDM_REDUCE_WS_ROWS * 3 floats, n <= VDM_REDUCE_WS_ROWS). */
int vdm_conv_in_dgrad(const void* dh, int n, int d, int h, int w, int c, int dtype, int pad_mode, const float* weight, int cin,
                      float* dz, float* ds, void* stream);
int vdm_schedule_grad_sums(const float* dz, const float* x, const float* eps, uint64_t seed_eps, uint64_t stream_eps,
                           const int32_t* seed_step, int n, int64_t per, float* sums, float* workspace, void* stream);

/* ---- up to three conditioning fields (ABI v18) [CUNet(s_conditioning_channels = k), k in 1..3: conv_in has cin = 1 + k <= 4 input
 * channels, NB networks.py:259-265 cat([x, s_conditioning], dim=1)] -------------------------------------------------------------------
 * The conditioning tensor is NCDHW fp32, cond[n][k][per] (per = d h w voxels, per % 4 == 0).  conv_in's packed NDHWC input stays ONE
 * 16-byte piece per voxel in both storage types: {z, c_0 .. c_{k-1}, 0 ...} (4 fp32 or 8 bf16 elements), rounded like vdm_pack_input.
 * The entries above keep their contracts (vdm_pack_input / vdm_diffuse_pack: one conditioning field, vdm_conv_in_dgrad: cin <= 2);
 * for k = 1 the entries below give the same bits.  Every argument error (NULL pointer, k outside 1..3, cin outside 1..4, n_ds neither
 * 0 nor cin - 1, ds NULL with n_ds > 0, per % 4 != 0, bad dtype / pad_mode, misalignment) returns VDM_ERR_ARG before any launch.
 *   vdm_pack_fields: out[n][voxel][16 B] from z [n][per] and cond (the sampler's step).  z, cond, out 16-byte aligned.
 *   vdm_diffuse_pack_fields: vdm_diffuse_pack for k planes - the same Philox counters (seed mixed with *seed_step, stream id, element
 *     group), so z_t (may be NULL) and channel 0 of `packed` carry the bits vdm_diffuse_pack gives for the same arguments.
 *   vdm_conv_in_dgrad_fields: K1t with conv_in's fp32 master weight [27][c][cin], cin in 1..4: dz [n][d][h][w] and, with
 *     n_ds == cin - 1, the conditioning gradients ds [n][n_ds][d][h][w]; n_ds == 0: dz alone (ds is not touched).  Fixed summation
 *     order (bit-reproducible); dz does not depend on n_ds. */
int vdm_pack_fields(const float* z, const float* cond, int k, int n, int64_t per, int dtype, void* out, void* stream);
int vdm_diffuse_pack_fields(const float* x, const float* cond, int k, const float* eps, uint64_t seed, uint64_t stream_id,
                            const int32_t* seed_step, const float* alpha, const float* sigma, int n, int64_t per, int dtype, float* z_t,
                            void* packed, void* stream);
int vdm_conv_in_dgrad_fields(const void* dh, int n, int d, int h, int w, int c, int dtype, int pad_mode, const float* weight, int cin,
                             float* dz, float* ds, int n_ds, void* stream);

/* ---- flow matching: fused head and loss of an SFM training step (ABI v21) [sfm_model.LightSFM of the trainSFM3D* scripts, REF
 * trainSFM3D128_c_c_from_field_name_thick_lowbatch.py:112-127; the straight path between the paired fields x0 (source) and x1 (target)] --
 * Fields are fp32, contiguous per sample of `per` elements; per % 4 == 0 and every non-NULL field pointer 16-byte aligned.  Every
 * argument error (a required pointer NULL, n <= 0, per <= 0, per % 4 != 0, misalignment, bad dtype, sigma < 0 or NaN, cond outside
 * {0, 1}, n > VDM_REDUCE_WS_ROWS for the loss) returns VDM_ERR_ARG with a message before any launch.
 *   vdm_sfm_head: x_t = (1 - t[n]) x0 + t[n] x1, plus sigma eps when sigma > 0; written as fp32 (x_t, may be NULL) and, always, as
 *     conv_in's NDHWC input packed[n][voxel][16 B] = {x_t, cond ? x0 : 0, 0 ...} in `dtype`, rounded like vdm_pack_input - one pass
 *     instead of vdm_diffuse (+ vdm_randn + vdm_diffuse) + vdm_pack_input.  eps == NULL with sigma > 0: the noise is drawn inside the
 *     kernel from the Philox counters (seed mixed with *seed_step, stream_id, float4 group index over the batch) - exactly the field
 *     vdm_randn(seed, stream_id, seed_step) writes.  sigma == 0: neither eps nor the generator is touched (seed, stream_id and
 *     *seed_step do not matter).  The bits are those of the chain: 1 - t rounded to fp32, then vdm_diffuse(x = x1, eps = x0, alpha = t,
 *     sigma = 1 - t), then vdm_diffuse(x = x_t, eps, alpha = 1, sigma).
 *   vdm_sfm_loss: sums[n] += sum (v_hat - (x1 - x0))^2 (caller zeroes sums, n floats) and d_v = coef[n] (v_hat - (x1 - x0)); the target
 *     velocity field is never written.  Fixed-order two-stage reduction, no float atomics (bit-reproducible): sums and d_v carry the bits
 *     of vdm_loss_terms_rng's first sum and d_eps_hat for eps = the materialised x1 - x0.  workspace as vdm_loss_terms
 *     (VDM_REDUCE_WS_ROWS * 3 floats, n <= VDM_REDUCE_WS_ROWS). */
int vdm_sfm_head(const float* x0, const float* x1, const float* eps, uint64_t seed, uint64_t stream_id, const int32_t* seed_step,
                 const float* t, float sigma, int cond, int n, int64_t per, int dtype, float* x_t, void* packed, void* stream);
int vdm_sfm_loss(const float* v_hat, const float* x0, const float* x1, const float* coef, int n, int64_t per, float* sums, float* d_v,
                 float* workspace, void* stream);

/* ---- conditioning dropout of classifier-free guidance training (added under ABI v21) [VDM(p_uncond=, cfg_drop=): a random share of
 * the training rows sees the null token (zeros) instead of its conditioning; w_cfg then guides the sampler] ---------------------------
 * Every argument error (a required pointer NULL, rows <= 0, p outside [0, 1] or NaN, misalignment, k outside 1..3, and what
 * vdm_diffuse_pack_fields refuses) returns VDM_ERR_ARG with a message before any launch.
 *   vdm_cond_keep: keep[r] = 1.0f / 0.0f for r < rows, one uniform draw per GLOBAL row `row0 + r`: Philox4x32-10 with the key `seed`
 *     mixed with *seed_step (NULL: the seed as it is) and the counter (row lo, row hi, 0xCFD0, 0); keep = unit(word 0) > p, the rule of
 *     the fp32 dropout byte (p = 0 keeps every row, p = 1 none).  A row's draw does not depend on row0 / rows.
 *   vdm_mask_rows: out[r][j] = keep[r] != 0 ? v[r][j] : +0.0f for r < rows, j < dim - a select: NaN / Inf of a dropped row do not
 *     get through.  out == v is allowed.  float4 accesses when v and out are 16-byte aligned and dim % 4 == 0, scalar otherwise.
 *   vdm_diffuse_pack_fields_keep: vdm_diffuse_pack_fields with a per-row keep of the conditioning planes, keep_s[n] (NULL: every row
 *     kept - the launch of vdm_diffuse_pack_fields).  A dropped row (keep_s[n] == 0) gets +0 in planes 1 .. k of its pieces and its cond
 *     planes are not read; z_t and channel 0 carry the bits of vdm_diffuse_pack_fields for the same arguments, with every row kept the
 *     whole output does, and k = 1 gives the bits of vdm_diffuse_pack. */
int vdm_cond_keep(float p, uint64_t seed, const int32_t* seed_step, uint64_t row0, int64_t rows, float* keep, void* stream);
int vdm_mask_rows(const float* v, const float* keep, int64_t rows, int64_t dim, float* out, void* stream);
int vdm_diffuse_pack_fields_keep(const float* x, const float* cond, int k, const float* eps, uint64_t seed, uint64_t stream_id,
                                 const int32_t* seed_step, const float* alpha, const float* sigma, int n, int64_t per, int dtype,
                                 float* z_t, void* packed, const float* keep_s, void* stream);

/* ---- data path: crop + log-normalise + flip + permute on the device -----------------------------
 * Replaces the per-sample CPU DataLoader work of [REF src/dataset/CAMELS_3D_dataset.py:53-73] (AstroDataset.__getitem__) and
 * [REF src/dataset/augmentation.py:8-127] (Crop, LogTransform, Normalize, Flip, Permutate):
 *   out[c][b][i0][i1][i2] = (log10(raw + alpha) - mean) / std  of  field[c][sim][(anchor_d + c_d) % fullsize],
 *   c_d = flip[d] ? crop-1-f_d : f_d,  f[perm[k]] = i_k   (crop -> log/normalise -> flip -> permute, the reference's order).
 * The two tables are HOST arrays (they travel in the kernel arguments); `field` / `out` inside them are device pointers
 * (field: [n_sims][fullsize]^3 fp32 raw cubes resident in HBM; out: [n_samples][crop]^3 fp32).  n_channels <= 4. */
typedef struct {
    const float* field;
    float* out;
    float alpha, mean, std; /* [REF src/dataset/alphas_3d.json, normalizations_3d.json] */
} vdm_augment_channel;
typedef struct {
    int32_t sim;       /* simulation index into `field` */
    int32_t anchor[3]; /* crop origin incl. the random shift (may exceed fullsize: wrapped) [REF augmentation.py:113-117] */
    int32_t flip[3];   /* != 0: flip this axis [REF augmentation.py:51-52] */
    int32_t perm[3];   /* axis permutation [REF augmentation.py:72] */
} vdm_augment_sample;
int vdm_augment_batch(const vdm_augment_channel* host_channels, int n_channels, int fullsize, int crop,
                      const vdm_augment_sample* host_samples, int n_samples, void* stream);

/* ---- data preparation: trilinear down-gridding of the cube stacks on the device ---------------------------------------------------
 * Replaces the data-preparation notebook [REF scripts/make_down_grids.ipynb cell 3], which turns the 256^3 CAMELS stacks into the
 * 3D_grids_<T> training sets with torch.nn.functional.interpolate(stack[:, None], size=T, mode="trilinear", align_corners=False):
 *   per axis and output index d: coordinate max((d + 1/2) S/T - 1/2, 0), i0 = floor, i1 = min(i0 + 1, S - 1), lambda = frac
 *   (edges clamped, not periodic), out = the 8-corner blend with weights (1 - lambda | lambda) per axis.
 * i0 and lambda are taken from the exact rational ((2d + 1) S - T) / (2T) in integer arithmetic (lambda = remainder / 2T rounded once to
 * fp32); the blend is fp32 in a fixed order (z, y, x) without atomics: equal inputs give equal bits on every call, T == S is a
 * bit-exact copy.  src: [n][S][S][S] fp32, dst: [n][T][T][T] fp32 (x fastest), 1 <= T <= S <= 1024; S, T multiples of 4 and 16-byte
 * aligned pointers take the path with 16-byte loads and stores.  n == 0 is a successful no-op. */
int vdm_downgrid_trilinear(const float* src, float* dst, int64_t n, int S, int T, void* stream);

/* ---- data preparation: the moments of log10(field + alpha) over a resident slab (normalisation constants) --------------------------
 * Replaces the arithmetic of the reference's notebook [REF scripts/calc_normalization.ipynb: data = np.load(path).astype(np.float64);
 * data = np.log10(data + alpha); data.mean(), data.std()] with one streaming pass over device memory.  Per element
 * v = log10((double)x + alpha) in float64; the element is valid when x is finite and x + alpha > 0, otherwise it is counted in n_bad
 * and excluded from everything else.  out (device, 6 doubles) = {n_valid, S1, S2, min, max, n_bad}: S1 = sum(v - pivot),
 * S2 = sum((v - pivot)^2) over the valid elements, min / max over the raw fp32 x of the valid elements (+inf / -inf without any), the
 * counts exact.  With the pivot near the mean, mean = pivot + S1/N and var = S2/N - (S1/N)^2 lose nothing to cancellation; records of
 * different slabs computed with the same pivot add.  x: n fp32 values on the device, any n in 0..2^40 and any (4-byte) alignment;
 * workspace: VDM_LOG_MOMENTS_WS doubles on the device, overwritten.  Two launches (per-workgroup records, then one workgroup adds them
 * in a fixed order), no atomics, a grid that depends on n alone: the same values give the same bits on every call, every device and
 * every pointer alignment.  n == 0 writes the empty record {0, 0, 0, +inf, -inf, 0}.  VDM_ERR_ARG before any launch: NULL x / out /
 * workspace, n < 0 (or above 2^40), a non-finite alpha or pivot. */
#define VDM_LOG_MOMENTS_OUT 6                /* doubles */
#define VDM_LOG_MOMENTS_WS 12288             /* doubles of workspace: 2048 workgroup records of VDM_LOG_MOMENTS_OUT */
int vdm_log_moments(const float* x, int64_t n, double alpha, double pivot, double* out, double* workspace, void* stream);

/* ---- attention block of the mid level (CUNet(mid_attn=True, n_attention_heads)) [REF trainSFM_c_uc_from_field_name.py:61,104-118;
 * NB blocks.py:169-170 `x = self.attention_blocks[i](x)`] ---------------------------------------------------------------------
 * Fused core  out_i = sum_j softmax_j(scale q_i . k_j) v_j  per sample and head on the matrix cores, forward and backward, without
 * the [N, heads, V, V] score tensor (csrc/attention.hip).  Operands in `dtype` (bf16 MFMA / exact fp32 MFMA), softmax and sums fp32.
 *   split_heads: src[n][v][src_stride] (channels src_offset + h*hd ...) -> rowmajor [n][h][v][hd] and / or transposed [n][h][hd][v]
 *                (either may be NULL).  The q, k, v of the block's 1x1x1 qkv conv ([n][v][3][C]: stride 3C, offsets 0, C, 2C).
 *   fwd:   q, k row-major, vt transposed -> out [n][v][heads*hd] (the layout the projection conv reads), lse [n][h][v] (may be NULL).
 *   rowdot: out[n][h][v] = sum_d a[n][v][h*hd+d] b[n][v][h*hd+d]   (dsum = rowsum(dOut * out) of the backward).
 *   bwd:   -> dqkv [n][v][3][heads*hd]; dQ in its own pass over the keys: no float atomics, bit-reproducible.
 * voxels % 4 == 0; head_dim in {16, 32, 64, 96, 128}. */
int vdm_attn_split_heads(const void* src, int64_t src_stride, int64_t src_offset, int n, int64_t voxels, int heads, int head_dim,
                         int dtype, void* rowmajor, void* transposed, void* stream);
int vdm_attn_fwd(const void* q, const void* k, const void* vt, int n, int64_t voxels, int heads, int head_dim, int dtype, float scale,
                 void* out, float* lse, void* stream);
int vdm_attn_rowdot(const void* a, const void* b, int n, int64_t voxels, int heads, int head_dim, int dtype, float* out, void* stream);
int vdm_attn_bwd(const void* q, const void* k, const void* v, const void* qt, const void* kt, const void* do_rowmajor,
                 const void* do_transposed, const float* lse, const float* dsum, int n, int64_t voxels, int heads, int head_dim,
                 int dtype, float scale, void* dqkv, void* stream);
/* out[c] = sum over rows of x[row][c] (x: [rows][c] in `dtype`): bias gradients of the block's two 1x1x1 projections. */
int vdm_channel_sums(const void* x, int64_t rows, int c, int dtype, float* out, void* stream);
/* out[n][c1+c2][2] = (sum_rows a, sum_rows a * b) per sample, a: [n][rows][c1+c2], b = concat(b1 [n][rows][c1], b2 [n][rows][c2] or
 * NULL): with a = dyh and b = x of a GroupNorm these are the "one tile per sample" partials vdm_gn_bwd_finalize / vdm_gn_bwd_apply take. */
int vdm_channel_dot_sums(const void* a, const void* b1, int c1, const void* b2, int c2, int n, int64_t rows_per_sample, int dtype,
                         float* out, void* stream);

/* ---- scalar glue of the training step [R7, R11; D9-D11] (replaces ~60 five-microsecond ATen launches on the critical path) --------
 * train_scalars: out[5][batch] = {t, alpha_t, sigma_t, coef = gamma'(t) bpd / batch, t_norm} of the fixed linear schedule; with u0
 *   (DEVICE pointer to one uniform draw) t_i = (u0 + (rank batch + i) / (world batch)) mod 1 - the antithetic time grid stratified over
 *   the global batch - else t_i = times[i]; with neither, u0 is drawn in the kernel from Philox(seed, *seed_step) (same on every rank).
 *   [REF trainVDM3D128...py:128-132 -> LightVDM.training_step; NB vdm_model.py:320-324]
 * elbo_assemble: out[4] = {elbo, diffusion, latent, reconstruction} in bits/dim from the sums of vdm_loss_terms:
 *   diffusion = 0.5 sum_n coef_n S0_n, latent = mean_n (c_lat0 + c_lat1 S1_n), reconstruction = mean_n (c_rec0 S2_n + c_rec1).
 * clip_scale: x *= min(1, max_norm / (sqrt(*sumsq) + 1e-6)) - gradient_clip_val [REF trainVDM3D128...py:45] on the device. */
int vdm_train_scalars(const float* u0, const float* times, int batch, int rank, int world, float gamma_min, float gamma_max,
                      float bpd_over_batch, float* out, uint64_t seed, const int32_t* seed_step, void* stream);
int vdm_elbo_assemble(const float* sums, const float* coef, int batch, float c_lat0, float c_lat1, float c_rec0, float c_rec1,
                      float* out, void* stream);
int vdm_clip_scale(float* x, int64_t n, const float* sumsq, float max_norm, void* stream);

/* ---- K9: ancestral update [NB vdm_model.py:370-378] ----------------------------------------
 * z <- ratio*(z - c_sigma_t*eps_hat) + scale*noise ; the four scalars are read from the DEVICE table
 * coef[step][4] = {ratio, c*sigma_t, scale, t_norm} at row *step_ptr (so one captured graph serves
 * every step).  noise==NULL: Philox normal from (seed, *step_ptr, element index). */
int vdm_ancestral_step(float* z, const float* eps_hat, const float* noise, const float* coef, const int32_t* step_ptr,
                       uint64_t seed, int64_t n, void* stream);
/* The same update under classifier-free guidance [NB vdm_model.py:318-327, the `w_cfg` branch of VDM.get_pred_noise]:
 * eps_hat = (1 + w_cfg) * eps_cond - w_cfg * eps_uncond, blended inside the update (eps_cond / eps_uncond are the two halves of
 * one batch-doubled UNet forward: given v_conditionings / masked v_conditionings). */
int vdm_ancestral_step_cfg(float* z, const float* eps_cond, const float* eps_uncond, float w_cfg, const float* noise,
                           const float* coef, const int32_t* step_ptr, uint64_t seed, int64_t n, void* stream);
/* Row-keyed form for batched chains: z is [rows][per_row]; row r's noise is the Philox normal of (seeds[r], *step_ptr + 1, float4 group
 * index within the row), so a chain draws the same noise wherever it sits in a batch (rows == 1: the stream of vdm_ancestral_step with
 * seed = seeds[0], bit for bit).  eps_uncond == NULL: plain update; otherwise the w_cfg blend of vdm_ancestral_step_cfg.  seeds is a
 * DEVICE array of `rows` values; per_row must be a positive multiple of 4 and the three fields 16-byte aligned. */
int vdm_ancestral_step_rows(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const float* coef,
                            const int32_t* step_ptr, const uint64_t* seeds, int rows, int64_t per_row, void* stream);
/* ---- K9m: multistep update (DPM-Solver++(2M) on the VDM's data prediction; Adams-Bashforth 2 on the flow-matching velocity) ----
 * Per element, with the scalars of row *step_ptr of the DEVICE table coef[steps][8] = {e_z, e_e, w_z, w_x, w_p, t_net, 0, 0} (so one
 * captured graph serves every step) and rn() one fp32 rounding:
 *   e    = eps_uncond ? rn(rn(rn(1 + w_cfg) * eps_hat) - rn(w_cfg * eps_uncond)) : eps_hat      (the blend of vdm_ancestral_step_cfg)
 *   est  = fma(e_z, z, rn(e_e * e))             data prediction (VDM: e_z = 1/alpha_t, e_e = -sigma_t/alpha_t) or velocity (0, 1)
 *   a    = fma(w_z, z, rn(w_x * est))
 *   z    <- w_p != 0 ? fma(w_p, prev, a) : a
 *   prev <- est
 * The sequence is spelled out in the kernel (fmaf and separately rounded products), so both libraries give the same bits whatever the
 * compiler contracts.  A row with w_p == 0 (a first-order step; always the first one) does NOT read prev: the history does not exist
 * yet and the buffer may hold anything, NaN included; prev is still written.  Any n >= 1; 16-byte aligned fields go through float4
 * loads and stores with a ragged tail.  z, eps_hat, prev, coef or step_ptr NULL, or n <= 0: VDM_ERR_ARG, nothing is launched. */
int vdm_multistep_step(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, float* prev, const float* coef,
                       const int32_t* step_ptr, int64_t n, void* stream);
/* standard-normal fill from Philox(seed, stream_id) (z_1 of the sampler; eps in training). */
int vdm_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, const int32_t* seed_step, void* stream);
/* *step_ptr += 1 (device-side step counter for the captured sampler graph). */
int vdm_step_inc(int32_t* step_ptr, void* stream);

/* ---- K11: DDNM range/null-space update (ABI v14; csrc/ddnm.hip) [REF src/utils.py:277-304] ------
 * x_0t = (z - sigma_t*eps_hat)/alpha_t ; x_r = AT y + x_0t - AT A x_0t ; z <- w_z*z + w_x*x_r + scale*noise, fp32.
 * Common contract: the scalars are read on the DEVICE.  e = *cursor is the index of the current network evaluation (monotonic over
 * a whole DDNM run), sched[e][2] = {k, draw} names the row of coef[n_coef][8] = {1/alpha_t, sigma_t, w_z, w_x, scale, t_norm, 0, 0}
 * and the number of this evaluation's noise draw, so one captured graph serves every evaluation (indices are clamped to the tables).
 * noise == NULL: row r's noise is the Philox normal of (seeds[r], draw + 1, float4 group index within the row) - the field
 * vdm_randn(seeds[r], stream_id = draw + 1) writes for one row, so a chain draws the same noise wherever it sits in a batch;
 * batch_stream != 0: one stream over the whole batch, (seeds[0], draw + 1, float4 group index within the batch).
 * eps_uncond != NULL: the w_cfg blend of vdm_ancestral_step_cfg.  x_r == NULL: the x_r write is skipped (only the last inner
 * evaluation of an outer step is consumed).  Fields are [rows][per_row], per_row % 4 == 0, 16-byte aligned; operands with `*_rows`
 * have 1 row (shared by the batch) or `rows`. */
typedef struct vdm_ddnm_tables {
    const float* coef;         /* DEVICE [n_coef][8] */
    const int32_t* sched;      /* DEVICE [n_sched][2] = {k, draw} */
    const int32_t* cursor;     /* DEVICE evaluation index */
    int32_t n_coef, n_sched;
    const uint64_t* seeds;     /* DEVICE [rows] (may be NULL when every launch gets a noise field) */
    int32_t batch_stream, reserved;
} vdm_ddnm_tables;
/* Generic operator, first half: x0 = x_0t over n elements; the caller runs AT(A(x0)) and then vdm_ddnm_update. */
int vdm_ddnm_x0(const float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const vdm_ddnm_tables* tables, float* x0,
                int64_t n, void* stream);
/* Generic operator, second half: x_r = (aty + x0) - atax0, then the z update. */
int vdm_ddnm_update(float* z, const float* x0, const float* atax0, const float* aty, int aty_rows, const float* noise,
                    const vdm_ddnm_tables* tables, float* x_r, int rows, int64_t per_row, void* stream);
/* A = AT = mask: x_0t, x_r = (mask*y + x_0t) - mask*(mask*x_0t), the z update and the noise in ONE pass (reads z, eps_hat, mask, y;
 * writes z, x_r) - bit for bit the generic pair around the callables x -> mask * x. */
int vdm_ddnm_mask_step(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const float* mask, int mask_rows,
                       const float* y, int y_rows, const float* noise, const vdm_ddnm_tables* tables, float* x_r, int rows,
                       int64_t per_row, void* stream);
/* A = mean over fz x fy x fx blocks of the [d][h][w] cube (factors in {1, 2, 4, 8} that divide it; w % 4 == 0), AT = nearest
 * up-sampling: y is [y_rows][d/fz][h/fy][w/fx]; x_r = (y_block + x_0t) - mean_block(x_0t) and the z update in one launch (the block's
 * rows are read twice by the same thread, the second time from cache). */
int vdm_ddnm_blockmean_step(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const float* y, int y_rows, int d, int h,
                            int w, int fz, int fy, int fx, const float* noise, const vdm_ddnm_tables* tables, float* x_r, int rows,
                            void* stream);
/* Travel back: z <- a*z + b*noise with {a, b} = travel[outer][2] (DEVICE table), noise supplied or Philox draw number `draw` keyed as
 * above (only seeds / batch_stream of `tables` are used). */
int vdm_ddnm_travel(float* z, const float* noise, const vdm_ddnm_tables* tables, const float* travel, int outer, int64_t draw, int rows,
                    int64_t per_row, void* stream);
/* *cursor += 1 ; *k_ptr = sched[*cursor][0] - the row index vdm_cond_table_step reads for the next evaluation. */
int vdm_ddnm_advance(int32_t* cursor, const int32_t* sched, int n_sched, int32_t* k_ptr, void* stream);

/* ---- K10: global gradient norm [REF trainVDM3D128_c_c_from_field_name_thick_lowbatch.py:45] -- */
/* out[0] += sum x^2 (caller zeroes).  workspace: >= 2048 floats (fixed-order fold: bit-reproducible). */
int vdm_sumsq(const float* x, int64_t n, float* out, float* workspace, void* stream);

/* ---- exponential moving average of the weights (added under ABI v21: two new entries, nothing existing changes, so the version stays;
 * csrc/ema.hip) [LightVDM / LightSFM(ema_decay=): the averaged weights a trained model is sampled from] ------
 * ema[i] <- ema[i] + w * (p[i] - ema[i]) over n fp32 elements, w = 1 - d_k, d_k = warmup ? min(decay, (1 + k) / (10 + k)) : decay with
 * k = *num_updates read on the DEVICE (NULL: k = 0).  Every operation is rounded on its own, in this order and never fused:
 *   q = rn((float)(1 + k) / (float)(10 + k)) ; d = min(decay, q) ; w = rn(1 - d) ; e' = rn(e + rn(w * rn(p - e)))
 * so a float32 reference that rounds operation by operation gives the same bits.  The counter is NOT bumped: one step may update several
 * tensors with the same k, the caller enqueues vdm_step_inc after the last one.  Both pointers 16-byte aligned: float4 accesses and a
 * scalar tail; otherwise (4-byte aligned) scalar accesses - the schedule scalars go through here with n = 1.  ema or p NULL, n < 0,
 * decay not a finite number in [0, 1), ema == p: VDM_ERR_ARG, nothing is launched.  n == 0: VDM_OK, nothing is launched. */
int vdm_ema_update(float* ema, const float* p, int64_t n, float decay, int warmup, const int32_t* num_updates, void* stream);
/* a[i] <-> b[i] over n fp32 elements, in place and without a temporary (evaluation under the averaged weights: every pointer a captured
 * graph holds stays valid).  Alignment as above.  NULL pointers, n < 0, overlapping ranges (a == b included): VDM_ERR_ARG. */
int vdm_swap(float* a, float* b, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VDM4CDM_HIP_H */
