/* libmiseg_hip.so -- C ABI of the MI355X (gfx950) hot path for MI-Seg's 3D cross-modality nets.
 *
 * Nothing like this exists in the reference (it is pure Python on torch/cuDNN/cuBLAS);
 * each entry point below names the reference code whose device arithmetic it replaces, as
 * /root/reference-relative file:line.  The Python host in mi-seg_amd/ binds these with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain C symbols, POD structs, raw device pointers; no C++/torch types cross the boundary.
 *   - every call only ENQUEUES work on `stream` and returns; no implicit device synchronisation, no
 *     allocation: all buffers (incl. workspaces, sized by the *_workspace_bytes helpers) are the caller's.
 *   - return 0 on success, a negative MISEG_E_* otherwise; miseg_last_error() gives a thread-local message.
 *   - activations are channels-last rows: element (row r, channel c) lives at base[r * ld + c]; a 3D volume
 *     is rows in (b, d, h, w) row-major order.  dtype is MISEG_F32 or MISEG_BF16 (bf16 storage, fp32 math).
 *   - parameters and their gradients are always fp32.
 *   - the library keeps no state of the caller's and reads NO environment variable (round 5: the tuning switches of earlier rounds'
 *     sweeps are gone); per-process caches are limited to device attributes and kernel attributes set once per device.
 */
#ifndef MISEG_HIP_H
#define MISEG_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* miseg_stream_t; /* hipStream_t */

enum { MISEG_F32 = 0, MISEG_BF16 = 1 };
enum { MISEG_OK = 0, MISEG_E_BADARG = -1, MISEG_E_UNSUPPORTED = -2, MISEG_E_LAUNCH = -3 };
enum { MISEG_ACT_NONE = 0, MISEG_ACT_LEAKY = 1, MISEG_ACT_GELU = 2, MISEG_ACT_PRELU = 3 };
#define MISEG_MAX_STYLES 4

/* bumped on EVERY change of a struct layout or prototype; bindings must refuse a library whose version differs from the header they mirror */
#define MISEG_ABI_VERSION 16
int miseg_abi_version(void);
const char* miseg_last_error(void);
/* writes e.g. "gfx950" for the code objects embedded in the library */
int miseg_device_arch(char* buf, size_t n);

/* ------------------------------------------------------------------------------------------------
 * (Conditional) instance norm over channels-last rows.
 * Replaces networks/norms/conditional_instance_norm.py:59-68 (per-sample style lookup + stack),
 * nn.InstanceNorm{1,3}d in networks/blocks/dynunet_block.py:80-81,98 and F.instance_norm in
 * networks/nets/swin_transformer.py:135-136, plus the LeakyReLU / residual add that follow them in
 * dynunet_block.py:100-126.
 *   x: [B][S][C] rows (ldx), statistics per (b, c) over the S rows, biased variance, eps inside sqrt.
 *   styles: device int32[B] or NULL (=> row 0); gamma/beta[s]: fp32[C] per style or NULL (no affine).
 *   y = act((x - mean) * rstd * gamma[s] + beta[s] + res)
 * ---------------------------------------------------------------------------------------------- */
/* statistics are kept as fp64 (sum x, sum x^2) pairs in R replicas: stat is double[R][B][C][2] with R * B * C * 16 =
 * miseg_instnorm_stat_bytes(B, C) bytes; the CALLER zero-fills it (the host pools all statistics buffers of a step behind
 * one fill), miseg_instnorm_stats adds each workgroup's partial sums to one replica with fp64 atomics (one row of
 * addresses serialises ~900 workgroups of a 96^3 tensor); apply / backward add the replicas up and derive mean and
 * 1/sqrt(var+eps). */
size_t miseg_instnorm_stat_bytes(int B, int C);
typedef struct {
  const void* x; int64_t ldx;
  int B, S, C, dtype;
  void* stat;                      /* in/out: miseg_instnorm_stat_bytes(B, C) bytes, zero on entry */
} miseg_instnorm_stats_params;
int miseg_instnorm_stats(const miseg_instnorm_stats_params* p, miseg_stream_t stream);

typedef struct {
  const void* x; int64_t ldx;
  const void* res; int64_t ldres;  /* optional residual added before the activation */
  void* y; int64_t ldy;
  int B, S, C, dtype;
  const void* stat; float eps;
  const int32_t* styles; int num_styles;
  const float* gamma[MISEG_MAX_STYLES]; const float* beta[MISEG_MAX_STYLES];
  int act; float slope;            /* MISEG_ACT_NONE | MISEG_ACT_LEAKY */
  /* optional: `res` is the raw input of a second instance norm (the block's shortcut branch, dynunet_block.py:118-124) and is normalised
   * on the fly with its own statistics (res_stat, layout as stat) and affine rows: y = act(norm(x) + norm_res(res)).  miseg_instnorm_apply only. */
  const void* res_stat;
  const float* res_gamma[MISEG_MAX_STYLES]; const float* res_beta[MISEG_MAX_STYLES];
  /* optional, with res_stat and res == NULL: the shortcut branch is the 1x1x1 convolution of a ONE-channel image (the stem block,
   * dynunet_block.py:87-97) and is never stored: res[row][c] = round(r1x[row] * r1w[c]) in the compute dtype.  r1x: [B*S] rows of one
   * element (row stride ldr1x), r1w: [C] in the compute dtype; res_stat from miseg_rank1_stats.  miseg_instnorm_apply only. */
  const void* r1x; int64_t ldr1x; const void* r1w;
} miseg_instnorm_apply_params;
int miseg_instnorm_apply(const miseg_instnorm_apply_params* p, miseg_stream_t stream);
/* statistics (into the zero-filled p->stat) + apply in one call; tensors of <= 512 rows per sample take ONE fused launch */
int miseg_instnorm_fwd(const miseg_instnorm_apply_params* p, miseg_stream_t stream);
/* miseg_instnorm_fwd whose input is still the `nslabs` fp32 partial slabs [B*S][C] (slab_stride elements apart) of a split convolution
 * (miseg_conv3_params.defer_slabs): x = round(sum of the slabs) is formed in registers and WRITTEN to p->x (the convolution's output, which
 * the backward pass reads), statistics, normalisation, residual and activation follow in the same launch.  S <= miseg_instnorm_fused_max_rows()
 * (2048) only: one workgroup owns every row of its channels there (dynunet_block.py:100-126 at the 12^3-and-smaller stages). */
int miseg_instnorm_fwd_slabs(const miseg_instnorm_apply_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_stream_t stream);
int miseg_instnorm_fused_max_rows(void);

/* backward of the fused op above.  dy is the gradient w.r.t. y; when act != NONE, y (the saved output)
 * supplies the sign for the activation gradient.  Outputs: dx, optionally dres (= gradient flowing to the
 * residual input), dgamma/dbeta[s] (ACCUMULATED with atomics: caller zero-fills once per step).
 * dstat: scratch double [B][C][2], zero on entry. */
typedef struct {
  const void* dy; int64_t lddy;
  const void* y; int64_t ldy;
  const void* x; int64_t ldx;
  void* dx; int64_t lddx;
  void* dres; int64_t lddres;
  int B, S, C, dtype;
  const void* stat; float eps; void* dstat;
  const int32_t* styles; int num_styles;
  const float* gamma[MISEG_MAX_STYLES];
  float* dgamma[MISEG_MAX_STYLES]; float* dbeta[MISEG_MAX_STYLES];
  int act; float slope;
  const void* gadd; int64_t ldgadd;   /* optional: dx += gadd (the gradient of a skip branch forked off x: the fan-out sum rides here) */
  /* y may be NULL with MISEG_ACT_LEAKY when NO residual entered the activation: the sign is then recomputed from x with the forward's
   * scale / shift (needs beta; saves one read of the tensor in each backward kernel and keeping y alive) */
  const float* beta[MISEG_MAX_STYLES];
} miseg_instnorm_bwd_params;
int miseg_instnorm_bwd(const miseg_instnorm_bwd_params* p, miseg_stream_t stream);
/* miseg_instnorm_bwd whose incoming gradient is still the partial slabs of a split data-gradient convolution (as miseg_instnorm_fwd_slabs):
 * p->dy is ignored (the gradient is summed and rounded in registers and never written).  S <= miseg_instnorm_fused_max_rows() only. */
int miseg_instnorm_bwd_slabs(const miseg_instnorm_bwd_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_stream_t stream);
/* the apply half alone (ABI 8): p->dstat already HOLDS the backward sums (sum dy, sum dy * xhat) - the GEMM that produced dy added them in
 * its epilogue (miseg_gemm_params.stat_mode 2, miseg_mlp_params.bs_dstat).  No activation.  dx, dgamma / dbeta as miseg_instnorm_bwd. */
int miseg_instnorm_bwd_apply(const miseg_instnorm_bwd_params* p, miseg_stream_t stream);
/* the reduction half alone (ABI 5): dstat[r][b][c] += (sum dy, sum dy * xhat) over the rows of sample b, xhat from `stat` - what the group /
 * batch norms of the reference's factory (networks/layers/factories.py:219-257) need besides the kernels above (their means run over channel
 * groups / the whole batch: mi-seg_amd/hip/functional.py::group_norm).  Reads dy, x, stat, eps, styles / gamma / beta only with an activation. */
int miseg_instnorm_bwd_reduce(const miseg_instnorm_bwd_params* p, miseg_stream_t stream);

/* Backward of y = LeakyReLU(norm_a(xa) + norm_b(xb)) (miseg_instnorm_apply with res_stat; dynunet_block.py:118-126): one reduction and one
 * apply pass for both norms.  dstat_a / dstat_b: scratch like miseg_instnorm_bwd's dstat (zero on entry); dgamma / dbeta accumulate. */
typedef struct {
  const void* dy; int64_t lddy;
  const void* y; int64_t ldy;
  const void* xa; int64_t ldxa; const void* xb; int64_t ldxb;
  void* dxa; int64_t lddxa; void* dxb; int64_t lddxb;
  int B, S, C, dtype;
  const void* stat_a; const void* stat_b; float eps; void* dstat_a; void* dstat_b;
  const int32_t* styles; int num_styles;
  const float* gamma_a[MISEG_MAX_STYLES]; const float* gamma_b[MISEG_MAX_STYLES];
  float* dgamma_a[MISEG_MAX_STYLES]; float* dbeta_a[MISEG_MAX_STYLES];
  float* dgamma_b[MISEG_MAX_STYLES]; float* dbeta_b[MISEG_MAX_STYLES];
  float slope;
  /* y == NULL: the activation's sign is recomputed from xa / xb (then the betas of both norms are read; NULL rows = 0) */
  const float* beta_a[MISEG_MAX_STYLES]; const float* beta_b[MISEG_MAX_STYLES];
  /* rank-1 shortcut (the stem block, dynunet_block.py:87-97 with one input channel): xb[row][c] = round(r1x[row] * r1w[c]) is not stored
   * (xb = dxb = y = NULL); r1x: [B*S] rows of one element (row stride ldr1x), r1w: [C] in the compute dtype; the weight gradient of that
   * 1x1x1 convolution, sum over rows of dxb[row][c] * r1x[row], is ADDED to r1dw [C] fp32 */
  const void* r1x; int64_t ldr1x; const void* r1w; float* r1dw;
} miseg_instnorm_pair_bwd_params;
int miseg_instnorm_pair_bwd(const miseg_instnorm_pair_bwd_params* p, miseg_stream_t stream);

/* ---- plans of the instance-norm family ----
 * miseg_instnorm_<call>_plan takes the arguments of miseg_instnorm_<call> with a plan in place of the stream and tells what the call will
 * launch: up to two kernels, each with its template lane width, thread geometry, grid and LDS bytes.  Every launcher dispatches on exactly
 * this plan, and a call that is refused gets the same error code from the plan (n_launches == 0 then).  Pointers are only tested for NULL
 * and alignment, so a host may ask with stand-ins for buffers it has not allocated.  Host only: touches no device.  (New symbols and
 * structs: MISEG_ABI_VERSION stays 16.) */
#define MISEG_IN_NONE 0
#define MISEG_IN_STATS 1             /* streaming: (sum x, sum x^2) per channel, fp64 atomics into the replicas */
#define MISEG_IN_APPLY 2             /* streaming: normalise (+ residual / shortcut norm / rank-1 shortcut) (+ activation) */
#define MISEG_IN_BWD_REDUCE 3        /* streaming: (sum g, sum g * xhat) into dstat */
#define MISEG_IN_BWD_APPLY 4         /* streaming: dx (+ dres, + gadd), dgamma / dbeta */
#define MISEG_IN_PAIR_BWD_REDUCE 5   /* streaming, both norms of the residual pair */
#define MISEG_IN_PAIR_BWD_APPLY 6
#define MISEG_IN_FUSED_FWD 7         /* register-resident, S <= miseg_instnorm_fused_max_rows(): statistics + apply in one launch */
#define MISEG_IN_FUSED_BWD 8
#define MISEG_IN_PAIR_FUSED_BWD 9
typedef struct {
  int32_t kernel;                  /* MISEG_IN_* */
  int32_t vec;                     /* the kernel's template lane width in elements: 16-byte lanes (8 bf16 / 4 fp32), 1, or - fused kernels only - a halving between */
  int32_t from_slabs;              /* 1: the fused kernel's instantiation that sums fp32 partial slabs */
  int32_t cv, tx, ty;              /* channel vectors per row (C / vec); thread grid of a workgroup: tx channel vectors x ty row lanes */
  int32_t rpb, chunks, ctiles;     /* streaming: rows per workgroup, row chunks per sample, channel tiles; 0 for the fused kernels */
  int32_t grid_x, grid_y, grid_z;  /* streaming: (chunks, B, ctiles); fused: (ceil(cv / tx), B, 1) */
  int32_t threads;                 /* 256 */
  int32_t rank1;                   /* 1: the launch forms the rank-1 shortcut from r1x / r1w */
  int32_t lds_bytes;               /* dynamic LDS of the launch */
} miseg_instnorm_launch;
typedef struct {
  int32_t n_launches;              /* 0 (refused), 1 or 2 */
  int32_t aligned;                 /* 1: the 16-byte-lane predicate held for every launch of the call (a launch's own outcome is its vec) */
  miseg_instnorm_launch launch[2];
} miseg_instnorm_plan_info;
int miseg_instnorm_stats_plan(const miseg_instnorm_stats_params* p, miseg_instnorm_plan_info* plan);
int miseg_instnorm_apply_plan(const miseg_instnorm_apply_params* p, miseg_instnorm_plan_info* plan);
int miseg_instnorm_fwd_plan(const miseg_instnorm_apply_params* p, miseg_instnorm_plan_info* plan);
int miseg_instnorm_fwd_slabs_plan(const miseg_instnorm_apply_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_instnorm_plan_info* plan);
int miseg_instnorm_bwd_plan(const miseg_instnorm_bwd_params* p, miseg_instnorm_plan_info* plan);
int miseg_instnorm_bwd_apply_plan(const miseg_instnorm_bwd_params* p, miseg_instnorm_plan_info* plan);
int miseg_instnorm_bwd_slabs_plan(const miseg_instnorm_bwd_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_instnorm_plan_info* plan);
int miseg_instnorm_bwd_reduce_plan(const miseg_instnorm_bwd_params* p, miseg_instnorm_plan_info* plan);
int miseg_instnorm_pair_bwd_plan(const miseg_instnorm_pair_bwd_params* p, miseg_instnorm_plan_info* plan);

/* LayerNorm over the channel dim of channels-last rows (vit_norm_name="layer", the reference default:
 * networks/blocks/swin_transformer_block.py:104-105, transformer_block.py:82-83).  gamma/beta may be NULL. */
typedef struct {
  const void* x; int64_t ldx; void* y; int64_t ldy;
  int64_t rows; int C, dtype; float eps;
  const float* gamma; const float* beta;
  float* mean; float* rstd;        /* out fp32 [rows], saved for backward */
} miseg_layernorm_fwd_params;
int miseg_layernorm_fwd(const miseg_layernorm_fwd_params* p, miseg_stream_t stream);
typedef struct {
  const void* dy; int64_t lddy; const void* x; int64_t ldx; void* dx; int64_t lddx;
  int64_t rows; int C, dtype;
  const float* gamma; const float* mean; const float* rstd;
  float* dgamma; float* dbeta;     /* accumulated (atomics); may be NULL */
} miseg_layernorm_bwd_params;
int miseg_layernorm_bwd(const miseg_layernorm_bwd_params* p, miseg_stream_t stream);

/* a (conditional) instance norm whose apply pass is folded into the operand load of a consumer kernel (ABI 8; one sample): its statistics
 * and affine rows.  stat == NULL: no fold. */
typedef struct {
  const void* stat;                 /* fp64 [16][1][C][2], miseg_instnorm_stats layout: (sum x, sum x^2) of the norm's raw input */
  const int32_t* styles;            /* device [1] (the sample's style id) or NULL = style 0 */
  int32_t num_styles; float eps;
  const float* gamma[MISEG_MAX_STYLES]; const float* beta[MISEG_MAX_STYLES];      /* rows per style; NULL = no affine */
} miseg_norm_ref;

/* ------------------------------------------------------------------------------------------------
 * GEMM on the matrix cores:  C[M][N] = A * B (+ bias[N]) (-> act).
 * Replaces every nn.Linear on the path (window_attention.py:92,94 qkv/proj; MONAI MLPBlock used at
 * swin_transformer_block.py:97; patch_merging.py:48 reduction; transformer_block.py:58-59), the 1x1x1
 * convolutions (dynunet_block.py:87-97,278-289) and, with gather/scatter kernels, ConvTranspose3d k2 s2
 * (unetr_block.py:51-59).
 *   ta == 0: A is [M][K] (lda)   ta == 1: A is stored [K][M] (lda)   -- likewise tb for B: 0 => [N][K], 1 => [K][N]
 *   only (ta,tb) = (0,0) "NT" and (1,1) "TN" are implemented (weights are re-packed once per step).
 *   out_dtype: dtype of C (MISEG_F32 for weight gradients).  accumulate != 0: C += result (fp32 C only).
 *   split_k = 0 lets the library choose kernel and split (TN: tall token streams are reduced through per-workgroup
 *   partial sums in `workspace` and a second kernel, no atomics); split_k > 1 partitions K over workgroups and reduces with
 *   fp32 atomics into a zero-filled or accumulate-mode C (fp32 C only).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* A; int64_t lda; const void* B; int64_t ldb; void* C; int64_t ldc;
  int M, N, K;
  int ta, tb;
  int dtype, out_dtype;
  const float* bias; int act;
  int accumulate, split_k;
  void* workspace;   /* miseg_gemm_workspace_bytes(p) bytes of scratch (uninitialised) or NULL when that is 0 */
  /* NT epilogue extras (all [M][N] row views in out_dtype): C = act(z) + res with z = A*B + bias;
   * epi_mode 1: aux = z (the pre-activation a GELU backward needs), 2: z *= gelu'(aux) (the GELU backward folded into the
   * data-gradient GEMM of the layer behind it).  MLP: swin_transformer_block.py:97, residuals :241-252. */
  const void* res; int64_t ldres;
  void* aux; int64_t ldaux;
  int epi_mode;
  int defer_reduce;  /* TN streaming path only: leave the per-split partial tiles in `workspace`; the caller sums them later with
                      * miseg_gemm_tn_reduce_batch (miseg_gemm_tn_splits(p) tells how many there are) */
  void* stat;        /* NT, optional: fp64 [16][1][N][2] (miseg_instnorm_stat_bytes(1, N), zero on entry): instance-norm statistics of the rounded
                      * output when all M rows are ONE sample and miseg_gemm_fuses_stat(p) says so (the tall-skinny bf16 path, N <= 96) -
                      * the linears / 1x1x1 convs whose output feeds an instance norm (swin_transformer_block.py:241-252, dynunet_block.py:118-124) */
  /* NT, optional (scat_cout > 0): the GEMM of a ConvTranspose3d(k2, s2) (unetr_block.py:80-85) stores straight into the upsampled tensor.
   * Rows are the voxels of a [.., scat_d, scat_h, scat_w] grid, the N = 8 * scat_cout columns are (j, co) with j = 4 jd + 2 jh + jw; element
   * (voxel (d,h,w), j, co) goes to row (2d+jd, 2h+jh, 2w+jw) of the [.., 2 scat_d, 2 scat_h, 2 scat_w] grid, column co, of C (row stride ldc -
   * e.g. the left half of a concat buffer).  Only where miseg_gemm_fuses_scatter(p) says so. */
  int scat_d, scat_h, scat_w, scat_cout;
  /* NT, optional (ABI 8), only where miseg_gemm_fuses_anorm(p) says so: A is the RAW input of a (conditional) instance norm over its M rows
   * (ONE sample) and is normalised as it is loaded - C = act(norm(A) B + bias) + res without the norm's apply pass (the Swin block's
   * norm1 -> qkv and norm2 -> fc1, swin_transformer_block.py:103,176-205).  an.stat: the norm's statistics (miseg_instnorm_stats layout, complete
   * when this launch starts).  an_out (optional): norm(A) [M][K] is stored as well, once, rounded exactly as miseg_instnorm_apply rounds
   * it - the operand of the weight-gradient product of the backward pass. */
  miseg_norm_ref an; void* an_out; int64_t ld_an_out;
  /* NT, optional (ABI 8), only where miseg_gemm_fuses_bstat(p) says so: stat_mode 2 - C [M][N] is the gradient with respect to the OUTPUT of an
   * instance norm (one sample = the M rows) whose raw input is bs_x [M][N] with forward statistics bs_stat: `stat` receives that norm's
   * backward sums (sum C, sum C * xhat) in the dstat layout of miseg_instnorm_bwd (zero on entry), from the rounded C - miseg_instnorm_bwd_apply
   * then needs no reduction launch.  stat_mode 0: `stat` = forward statistics as above. */
  int stat_mode;
  const void* bs_x; int64_t ld_bs_x; const void* bs_stat; float bs_eps;
  /* TN, optional (ABI 9), only where miseg_gemm_tn_fuses_colsum(p) says so (the streaming path): tn_colsum[m] += sum over the K rows of A[k][m]
   * (fp32 [M], atomics: zero or accumulating on entry) - with A = dy the bias gradient of the linear layer whose weight gradient dW = dy^T x
   * this product is (swin_transformer_block.py:97,103), from the A fragments the product already holds. */
  float* tn_colsum;
} miseg_gemm_params;
int miseg_gemm_fuses_stat(const miseg_gemm_params* p);  /* 1: miseg_gemm(p) with p->stat set is supported for this problem */
int miseg_gemm_fuses_anorm(const miseg_gemm_params* p); /* 1: ... with p->an.stat set (whatever an_out) */
int miseg_gemm_fuses_bstat(const miseg_gemm_params* p); /* 1: ... with p->stat, stat_mode 2 and the bs_* fields set */
/* instance-norm statistics (layout of miseg_instnorm_stats, one sample = all M rows, zero on entry) of the rank-1 product
 * round(x[m] * w[n]) WITHOUT storing it: the stem block's shortcut convolution (dynunet_block.py:87-97), consumed through the r1x / r1w
 * fields of miseg_instnorm_apply / miseg_instnorm_pair_bwd.  x: [M] rows of one element (stride ldx), w: [N] (stride ldw), N <= 128 */
int miseg_rank1_stats(const void* x, int64_t ldx, const void* w, int64_t ldw, int M, int N, int dtype, void* stat, miseg_stream_t stream);

/* Fused MLP of the high-resolution Swin blocks (ABI 3): y = W2 gelu(W1 x + b1) + b2 (+ res)  (MONAI MLPBlock as used at
 * networks/blocks/swin_transformer_block.py:97,176-205), one launch, the hidden activations never reach memory: the accumulator tile of the
 * first product is the operand of the second (v_mfma_f32_16x16x16_bf16).  Backward (miseg_mlp_bwd): recomputes the hidden pre-activation
 * from x, writes dz = (dy W2) * gelu'(z) and h = gelu(z) for the two weight-gradient products (miseg_gemm TN) and dx = dz W1.
 * bf16, C = 48, HID = 192, M >= 4096 (miseg_mlp_fused tells); weights in the compute dtype: w1 [HID][C], w2 [C][HID], w2t [HID][C] = w2
 * transposed, w1t [C][HID]; biases fp32 (may be NULL); stat: as miseg_gemm_params::stat (one sample, statistics of the rounded y).
 * Row operands: base 8-byte aligned, row stride a multiple of 4 elements and at least the row's width (C; HID for dz and h); weights
 * 16-byte aligned.  Anything else is refused with MISEG_E_BADARG before a launch. */
typedef struct {
  uint32_t struct_size;
  int32_t M, C, HID, dtype;
  const void* x; int64_t ldx;
  const void* w1; const float* b1; const void* w2; const float* b2;
  const void* res; int64_t ldres;          /* forward, optional */
  void* y; int64_t ldy; void* stat;        /* forward */
  const void* dy; int64_t lddy;            /* backward */
  const void* w2t; const void* w1t;
  void* dz; int64_t lddz; void* h; int64_t ldh; void* dx; int64_t lddx;
  /* ABI 8, optional.  Forward: an.stat != NULL - x is the RAW input of the (conditional) instance norm in front of the MLP (one sample; the
   * Swin block's norm2) and is normalised as it is loaded; an_out (optional) receives norm(x) [M][C] for the backward pass (which takes it
   * as its `x`).  Backward: bs_dstat != NULL - dx is the gradient with respect to that norm's OUTPUT; the norm's backward sums (sum dx,
   * sum dx * xhat; xhat from the raw input bs_x and the forward statistics bs_stat) are added to bs_dstat (dstat layout of miseg_instnorm_bwd,
   * zero on entry): miseg_instnorm_bwd_apply then needs no reduction launch. */
  miseg_norm_ref an; void* an_out; int64_t ld_an_out;
  const void* bs_x; int64_t ld_bs_x; const void* bs_stat; float bs_eps; void* bs_dstat;
} miseg_mlp_params;
int miseg_mlp_fused(int M, int C, int HID, int dtype);      /* 1: the two calls below support this problem */
int miseg_mlp_fwd(const miseg_mlp_params* p, miseg_stream_t stream);
int miseg_mlp_bwd(const miseg_mlp_params* p, miseg_stream_t stream);
int miseg_gemm_fuses_scatter(const miseg_gemm_params* p);  /* 1: miseg_gemm(p) with the scat_* fields set is supported for this problem */
int miseg_gemm_tn_splits(const miseg_gemm_params* p);   /* > 1: partial tiles [splits][M][N] fp32 in the workspace */
int miseg_gemm_tn_fuses_colsum(const miseg_gemm_params* p);   /* 1: this TN product takes the streaming path and can carry tn_colsum */
size_t miseg_gemm_workspace_bytes(const miseg_gemm_params* p);
int miseg_gemm(const miseg_gemm_params* p, miseg_stream_t stream);

/* What miseg_gemm(p) does with these params - the launch dispatches on exactly this plan, and the seven question entry points above read
 * their answers from it.  Pointers are only tested for NULL and alignment, so a host may ask with stand-ins for buffers it has not
 * allocated yet (`workspace` is not looked at).  Host only: touches no device.  Returns what miseg_gemm would return for a refused launch
 * (kernel == MISEG_GEMM_NONE then); the fuses_* / tn_fuses_colsum answers, and for a TN product of the streaming path splits and
 * workspace_bytes, are filled either way.  (A new symbol and struct: MISEG_ABI_VERSION stays 16.) */
#define MISEG_GEMM_NONE 0
#define MISEG_GEMM_NT_RANK1 1           /* K == 1 */
#define MISEG_GEMM_NT_RANK1_STAT 2      /* ... with the statistics of its output */
#define MISEG_GEMM_NT_SMALL 3           /* bf16, M <= 2048: <mtw, ntw, gelu, stat, anorm> */
#define MISEG_GEMM_NT_STREAM 4          /* bf16, M >= 4096, weight resident in LDS: <k16, gelu, nch, stat, scat, anorm> */
#define MISEG_GEMM_NT_GENERIC 5         /* <nt> */
#define MISEG_GEMM_TN_STREAM 6          /* bf16 -> fp32 token streams: wm x wn waves of 48 x 48, partial tiles per split */
#define MISEG_GEMM_TN_GENERIC 7
#define MISEG_GEMM_OUT_STORE 0
#define MISEG_GEMM_OUT_ACCUMULATE 1
#define MISEG_GEMM_OUT_ATOMIC 2
typedef struct {
  int32_t kernel;                        /* MISEG_GEMM_* */
  int32_t mtw, ntw;                      /* NT small: 16-row / 16-column tiles per wave */
  int32_t k16, nch;                      /* NT stream: K / 16, column tiles per accumulator chunk */
  int32_t gelu, stat, scat, anorm;       /* NT small / stream: stat 0 none, 1 forward statistics, 2 norm-backward sums */
  int32_t nt;                            /* NT generic: column tiles per workgroup */
  int32_t wm, wn;                        /* TN stream */
  int32_t grid_x, grid_y, grid_z;
  int32_t row_tiles;                     /* NT small: workgroup rows (grid_x = row_tiles * col_groups) */
  int32_t col_groups, cols_per_group;    /* NT small / stream: column groups of the grid and the columns of one */
  int32_t splits, k_per_split;           /* generic kernels and TN stream: parts of the K range and the length of one */
  int32_t out_mode;                      /* MISEG_GEMM_OUT_* */
  int32_t zero_fill;                     /* 1: C is zero-filled first (before the atomics that meet in it) */
  int32_t reduce_groups, reduce_blocks;  /* TN stream: grid y / x of the sum over the partial tiles (0: no such launch) */
  int32_t al_a, al_b;                    /* A / B rows may be read as 16-byte vectors */
  int32_t fuses_stat, fuses_anorm, fuses_bstat, fuses_scatter, tn_fuses_colsum;      /* what the entry points of these names answer */
  size_t lds_bytes;                      /* dynamic LDS of the launch */
  size_t workspace_bytes;                /* what miseg_gemm_workspace_bytes answers */
} miseg_gemm_plan_info;
int miseg_gemm_plan(const miseg_gemm_params* p, miseg_gemm_plan_info* plan);

/* up to MISEG_GEMM_GROUP independent TN problems C[M][N] += A[K][M]^T B[K][N] (fp32 C, accumulate mode) in ONE launch: the weight
 * gradients of the deep stages are a few dozen workgroups each; the host queues them during the backward pass and issues them
 * together.  `descs` is a HOST array (copied into the kernel arguments). */
/* regroup > 0 (ABI 8): column n = j * regroup + c of the summed product is stored at column c * (N / regroup) + j (see miseg_gemm_tn_desc) */
typedef struct { const float* partial; float* C; int64_t ldc; int32_t M, N, splits, block0, regroup, pad_; } miseg_tn_reduce_desc;
#define MISEG_TN_REDUCE_BATCH 32
/* C[m][n] += sum over splits of partial[s][m][n] for up to MISEG_TN_REDUCE_BATCH deferred reductions in one launch (HOST descriptors) */
int miseg_gemm_tn_reduce_batch(const miseg_tn_reduce_desc* descs_host, int n, miseg_stream_t stream);
#define MISEG_GEMM_GROUP 24
/* zeroed (ABI 5): 1 = C is known to hold zeros (a gradient slot no kernel has written since the step's fill) and no other problem of the
 * launch writes it: a problem whose reduction is not split then STORES its tiles instead of reading C back (the 85 M fp32 weight gradients
 * of C-UNETR's ViT: 340 MB less traffic per step). */
/* regroup > 0 (ABI 8): column n = j * regroup + c of the product is stored at column c * (N / regroup) + j - the weight gradient of a
 * ConvTranspose3d(k2, s2) as x^T dy8 (dy8's columns in (j, co) order, regroup = Cout) lands in the torch layout [Cin][Cout][2][2][2]
 * (unetr_block.py:51-59) without a permute pass */
typedef struct { const void* A; int64_t lda; const void* B; int64_t ldb; float* C; int64_t ldc; int32_t M, N, K, zeroed, regroup, pad_; } miseg_gemm_tn_desc;
int miseg_gemm_tn_group(const miseg_gemm_tn_desc* descs_host, int n, int dtype, miseg_stream_t stream);

/* up to MISEG_TN_STREAM_GROUP TN products of the STREAMING path (bf16 operands, fp32 C, M and N multiples of 48, K >= 2048 rows, 16-byte
 * aligned operands: what miseg_gemm_tn_fuses_colsum says yes to) in ONE launch (ABI 15): the tall weight gradients of one block of the
 * backward pass.  The group as a whole gets the workgroup count a lone product takes for itself, shared between the problems by the bytes
 * they stream (K may differ between them); a problem's plan tells its splits.  splits > 1: the launch leaves partial[split][M][N] fp32 in
 * `partial` (plan.workspace_bytes; required) for miseg_gemm_tn_reduce_batch, which ADDS to C (and regroups); splits == 1: C (+)= the
 * product (accumulate 0 stores) - unless `partial` is set all the same (M * N * 4 bytes): the one tile then goes there, for a sum that regroups.  colsum (optional): as miseg_gemm_params::tn_colsum.  `descs` / `plans` are HOST arrays. */
#define MISEG_TN_STREAM_GROUP 8
typedef struct { const void* A; int64_t lda; const void* B; int64_t ldb; float* C; int64_t ldc; float* partial; float* colsum; int32_t M, N, K, accumulate; } miseg_gemm_tn_stream_desc;
typedef struct { int32_t wm, wn, gx, gy, splits, tps, block0, pad_; int64_t workspace_bytes; } miseg_gemm_tn_stream_plan;
int miseg_gemm_tn_stream_group_plan(const miseg_gemm_tn_stream_desc* descs_host, int n, miseg_gemm_tn_stream_plan* plans_host);   /* host only: launches nothing */
int miseg_gemm_tn_stream_group(const miseg_gemm_tn_stream_desc* descs_host, int n, miseg_stream_t stream);
int miseg_gemm_tn_stream_group_target(void);      /* the workgroup count a whole group is planned for */

/* fp32 re-layout: dst[i0][i1][i2] (+)= src[i0*s0 + i1*s1 + i2*s2]  (weight-gradient unpacking) */
int miseg_permute3(const float* src, float* dst, int n0, int n1, int n2, int64_t s0, int64_t s1, int64_t s2, int accumulate,
                   miseg_stream_t stream);

/* column sums: out[c] (+)= sum_r x[r][c]  (bias gradients) */
typedef struct { const void* x; int64_t ldx; int64_t rows; int C, dtype; float* out; int accumulate; } miseg_colsum_params;
int miseg_colsum(const miseg_colsum_params* p, miseg_stream_t stream);
/* up to MISEG_COLSUM_BATCH accumulate-mode column sums (all in `dtype`) in ONE launch: the bias gradients of a backward pass are
 * small launch-bound reductions, queued by the host and issued together; `descs` is a HOST array (copied into the kernel arguments). */
#define MISEG_COLSUM_BATCH 32
typedef struct { const void* x; int64_t ldx; int64_t rows; float* out; int32_t C, block0; } miseg_colsum_desc;
int miseg_colsum_batch(const miseg_colsum_desc* descs_host, int n, int dtype, miseg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 3x3x3 convolution, stride 1, zero padding 1, no bias, as an implicit GEMM on the matrix cores.
 * Replaces nn.Conv3d built by get_conv_layer (networks/blocks/dynunet_block.py:295-326) as used in
 * UnetResBlock/UnetBasicBlock (dynunet_block.py:55-76,100-126).
 *   x: [B][D][H][W][Cin] rows (ldx)   y: [B][D][H][W][Cout] rows (ldy)
 *   wpk: packed weights [Cout][27][Cin] in `dtype` (miseg_pack_conv3_weight); the data gradient is the
 *   same kernel run on dy with the flipped/transposed pack.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x; int64_t ldx; void* y; int64_t ldy; const void* wpk;
  int B, D, H, W, Cin, Cout, dtype;
  void* workspace;                 /* miseg_conv3_plan_info.workspace_bytes (0 bytes for most shapes: may be NULL then) */
  /* optional epilogue pieces, only on the 96-byte-chunk path (channel rows of `dtype` a multiple of 96 bytes; else MISEG_E_UNSUPPORTED):
   * res (ldres): added to the result before rounding (the other gradient of a forked input when this is the data-gradient pass);
   * stat: fp64 [16][B][Cout][2] (miseg_instnorm_stat_bytes, zero on entry) - per-channel sum / sum of squares of the ROUNDED
   *       output, i.e. what miseg_instnorm_stats would compute from y (dynunet_block.py:105-107: every conv feeds a norm);
   *       with a workspace (split reduction) the second launch, which sums the partial slabs into y, computes them. */
  const void* res; int64_t ldres;
  void* stat;
  /* ABI 4: 1 = background launch (96-byte-chunk path): one workgroup per CU instead of two, so that the kernels of another stream find
   * registers, LDS and wave slots on every CU while this one runs (a branch of the step running beside its latency-bound chain) */
  int32_t background;
  /* ABI 5: 1 = when the launch splits its reduction (miseg_conv3_plan_info.splits > 1) it stops after the partial slabs in `workspace`
   * ([splits][B*D*H*W][Cout] fp32): the caller's next launch sums them (miseg_instnorm_fwd_slabs) - y and stat are NOT written.  No `res`. */
  int32_t defer_slabs;
  /* ABI 9, only where miseg_conv3_plan_info.sc says so (bf16, 96-byte chunks, unsplit launch, 16-byte aligned operands): y += sc_x * sc_w^T, a 1x1x1 term -
   * the data-gradient pass of a residual block's first convolution takes the gradient of the block's 1x1x1 shortcut convolution
   * along (dynunet_block.py:87-97,100-126: dx = dgrad3x3(g1) + g3 W3) instead of reading a [voxels][Cout] tensor that a GEMM wrote.
   * sc_x: [B][D][H][W][sc_C] rows (ld_sc_x), sc_C a multiple of 48; sc_w: [Cout][sc_C] in `dtype` (W3 transposed), contiguous. */
  const void* sc_x; int64_t ld_sc_x; const void* sc_w; int32_t sc_C;
  /* ABI 9, only where miseg_conv3_plan_info.s2c says so (96-byte chunks, unsplit launch, even D / H / W): output channels [0, s2c_C) are NOT
   * written to y but to s2c_out [B][D/2][H/2][W/2][8][s2c_C] - voxel (d, h, w) at block j = 4 (d&1) + 2 (h&1) + (w&1) of its coarse voxel: the
   * layout in which the ConvTranspose3d(k2, s2) in front of a decoder block reads the gradient of its output (unetr_block.py:80-85; the
   * data-gradient pass of that block's first convolution produces it, left half of the concat buffer).  Channels >= s2c_C go to y as usual. */
  void* s2c_out; int32_t s2c_C;
  /* ABI 9, only where miseg_conv3_plan_info.fs says so: fs_y = x * fs_w^T as a SECOND output of the launch - the 1x1x1 shortcut
   * convolution of a residual block beside its first 3x3x3 convolution (dynunet_block.py:87-97: both read the block's input).  fs_w: [Cout][Cin]
   * in `dtype`, contiguous; fs_y: [B][D][H][W][Cout] rows (ld_fs_y); fs_stat (optional): instance-norm statistics of fs_y, as `stat` for y. */
  const void* fs_w; void* fs_y; int64_t ld_fs_y; void* fs_stat;
} miseg_conv3_params;
/* ABI 13: what miseg_conv3_fwd(p) does with these params - the launch dispatches on exactly this plan.  A requested piece that the
 * launch cannot serve comes back 0 (the launch refuses it with MISEG_E_UNSUPPORTED); pointers are only tested for NULL and alignment,
 * so a host may ask with stand-ins for buffers it has not allocated yet.  Host only: touches no device. */
#define MISEG_CONV3_GENERIC 0      /* row-major kernel: no optional piece */
#define MISEG_CONV3_FWD96 1        /* 96-byte channel chunks */
#define MISEG_CONV3_FWD_TINY 2     /* 3^3 / 6^3 volumes, weight streaming, always split */
typedef struct {
  int32_t kernel;                  /* MISEG_CONV3_* */
  int32_t splits;                  /* partial slabs [splits][B*D*H*W][Cout] fp32 in `workspace` (1: y is written directly) */
  size_t workspace_bytes;          /* 0: `workspace` may be NULL */
  int32_t res, stat, sc, s2c, fs, defer_slabs;      /* 1: requested and served (stat: not with defer_slabs served) */
} miseg_conv3_plan_info;
int miseg_conv3_fwd_plan(const miseg_conv3_params* p, miseg_conv3_plan_info* plan);
int miseg_conv3_fwd(const miseg_conv3_params* p, miseg_stream_t stream);
/* ABI 16 (new symbol): the whole FORM of the launch miseg_conv3_fwd(p) makes - a superset of the plan; the launcher dispatches on exactly this
 * struct and computes nothing itself.  Host only, stand-in pointers as for miseg_conv3_fwd_plan.  A field means the same for every kernel:
 * `nt` is the planned tile count for FWD_TINY too (that kernel does not use it); fields of a kernel that is not launched are 0, and none of
 * those is a divisor of the launch that is made. */
typedef struct {
  miseg_conv3_plan_info plan;
  int32_t gpt, nchunks, cps;       /* FWD96 / FWD_TINY: 16-byte channel groups per chunk (6 / 4 / 2), chunks of the K side, chunks per split */
  int32_t nt;                      /* 16-channel output tiles per workgroup: FWD96 / FWD_TINY 1 .. 3 (as planned), GENERIC 1, 2, 3, 4, 6 */
  int32_t wd, epi;                 /* FWD96: conv3_fwd96_kernel<T, nt, wd, epi, gpt> */
  int32_t vec_x, vec_y;            /* 16-byte aligned base and whole vectors per row of x / y, for every kernel (only FWD96 and its second launch use vec_y) */
  int32_t vec_r, vec_fs_y;         /* the same test on res / fs_y: what the epilogues of FWD96 find for their own operands (0 without the operand) */
  int32_t ny;                      /* FWD96: output-channel groups per brick = ceil(Cout / (16 nt)); 0 for the other kernels */
  int32_t nbricks;                 /* bricks over the batch: 4 x 4 x 16 voxels (FWD96; counted for FWD_TINY too), 4 x 8 x 8 (GENERIC) */
  int32_t tiny_mt, tiny_mg;        /* FWD_TINY: conv3_fwd_tiny_kernel<MT, MG>: <2, 1> up to 32 voxels, else <4, 4>; else 0 */
  int32_t chunk_bytes;             /* GENERIC: bytes of a staged channel chunk = the padded row (at most 48) */
  int32_t grid_x, grid_y, grid_z;  /* the main launch */
  int32_t second_launch;           /* 1: a second launch sums the slabs (+ res) into y and takes the statistics (splits > 1, not deferred) */
  int32_t pad_;
  size_t lds_bytes;                /* dynamic LDS of the main launch */
} miseg_conv3_fwd_form_info;
int miseg_conv3_fwd_form(const miseg_conv3_params* p, miseg_conv3_fwd_form_info* form);

/* w: fp32 torch layout [Cout][Cin][3][3][3].  fwd_pack feeds miseg_conv3_fwd on x, bwd_pack (taps mirrored, channels swapped) feeds it
 * on dy; either may be NULL.  The layout is internal (row-major [Cout][27][CinP] or planar [27][CinP/k][CoutP16][k], by channel count);
 * buffers hold miseg_pack_conv3_elems(Cin, Cout, dtype, which) elements of `dtype` (which: 0 = fwd, 1 = bwd). */
size_t miseg_pack_conv3_elems(int Cin, int Cout, int dtype, int which);
/* 16x16 tiles miseg_pack_conv3_batch walks for one layer (the padded K groups of a fast-path pack get tiles of their own) */
int miseg_pack_conv3_tiles(int Cin, int Cout, int dtype);
typedef struct { const float* w; void* fwd_pack; void* bwd_pack; int Cin, Cout, dtype; } miseg_pack_conv3_params;
int miseg_pack_conv3_weight(const miseg_pack_conv3_params* p, miseg_stream_t stream);
/* every 3x3x3 weight of a model in ONE launch: `descs` is a DEVICE array of n descriptors sorted by tile0 = number of 16x16
 * (co, ci) tiles before the descriptor; total_tiles = the sum over descriptors of miseg_pack_conv3_tiles(Cin, Cout, dtype). */
typedef struct { const float* w; void* fwd_pack; void* bwd_pack; int32_t Cin, Cout, tile0, pad_; } miseg_pack_conv3_desc;
/* Versioned refresh (ABI 5; also miseg_param_cast_batch): `params_version` is a DEVICE int64 that counts the changes of the fp32 parameters
 * (miseg_opt_step bumps it through its `params_version` field; after any other change of a parameter the host adds to it with
 * miseg_counter_add), `state` a DEVICE int64[2] owned by this table of copies: state[0] = the version the copies were last made from,
 * state[1] = an arrival counter (zero between launches).  With both non-NULL the launch re-lays-out NOTHING when state[0] equals
 * *params_version (every workgroup reads the two words and exits) and otherwise records the new version when its last workgroup retires -
 * a replayed hipGraph thus refreshes the copies exactly in the steps that follow an optimiser step, with no host involvement.  NULL, NULL:
 * unconditional.  Set state[0] = -1 (miseg_fill32) after the table changed. */
int miseg_pack_conv3_batch(const miseg_pack_conv3_desc* descs_dev, int n, int total_tiles, int dtype, const int64_t* params_version, int64_t* state,
                           miseg_stream_t stream);

/* weight gradient: dw[Cout][Cin][27] (fp32, torch layout) (+)= sum_v dy[v][co] * x[v + tap][ci] */
typedef struct {
  const void* x; int64_t ldx; const void* dy; int64_t lddy; float* dw;
  int B, D, H, W, Cin, Cout, dtype;
  int accumulate;                  /* 0: dw = result; 1: dw += result; 2: dw is known to be zero on entry (no fill, no read-back) */
  void* workspace;                 /* miseg_conv3_wgrad_plan_info.workspace_bytes (0: may be NULL) */
  int32_t max_workgroups;          /* ABI 4: 0 = fill the chip (256); else a cap on the workgroups of the launch (a workgroup owns its CU's registers:
                                    * a background launch leaves the other CUs to the kernels of another stream).  miseg_conv3_wgrad only */
} miseg_conv3_wgrad_params;
/* ABI 13: the kernel miseg_conv3_wgrad(p) takes for these params and the workspace it needs (host only, as miseg_conv3_fwd_plan):
 * fp32 / bf16 slab kernels, NARROW (bf16, 16 / 32 channels on both sides), TINY (bf16, 3^3 / 6^3 voxels, Cin % 16 == 0, Cout % 48 == 0,
 * aligned; no workspace).  Only TINY stores the whole of dw when accumulate is 2, and it is a write-bound launch of its own that a host
 * should not queue for miseg_conv3_wgrad_group */
#define MISEG_CONV3_WGRAD_F32 0
#define MISEG_CONV3_WGRAD_NARROW 1
#define MISEG_CONV3_WGRAD_TINY 2
#define MISEG_CONV3_WGRAD_BF16 3
typedef struct { int32_t kernel; int32_t pad_; size_t workspace_bytes; } miseg_conv3_wgrad_plan_info;
int miseg_conv3_wgrad_plan(const miseg_conv3_wgrad_params* p, miseg_conv3_wgrad_plan_info* plan);
int miseg_conv3_wgrad(const miseg_conv3_wgrad_params* p, miseg_stream_t stream);
/* Up to 24 layers of one dtype in one launch (+ one for the partial sums): the small-grid weight gradients of a backward pass
 * (dynunet_block.py:100-126 at 48^3 and below) fill the chip together instead of one after the other.  `workspace` of the
 * params is ignored; one shared buffer of miseg_conv3_wgrad_group_workspace_bytes is passed instead (may be NULL when that is 0). */
size_t miseg_conv3_wgrad_group_workspace_bytes(const miseg_conv3_wgrad_params* layers, int n);
int miseg_conv3_wgrad_group(const miseg_conv3_wgrad_params* layers, int n, void* workspace, miseg_stream_t stream);
/* ABI 16 (new symbols): the whole FORM of a weight-gradient launch - a superset of the plan; the slab, narrow, tiny and grouped launchers
 * dispatch on exactly this struct.  Host only.  miseg_conv3_wgrad_form: the launch miseg_conv3_wgrad(p) makes.
 * miseg_conv3_wgrad_group_form: forms[i] is what miseg_conv3_wgrad_group(layers, n, ..) does with layers[i] (n entries; every layer runs in
 * the slab kernels there; plan.workspace_bytes is the layer's share of the group's buffer). */
typedef struct {
  miseg_conv3_wgrad_plan_info plan;
  int32_t brick_depth;             /* slab kernels: 2 (fp32) / 4 (bf16); NARROW 4; TINY 0 */
  int32_t piped;                   /* slab kernels: 1 = the software-pipelined loop (bf16, whole 48-channel blocks, aligned, a whole brick per axis) */
  int32_t vec_x, vec_dy;           /* 16-byte aligned base and whole vectors per row */
  int32_t nbricks;                 /* bricks of brick_depth x 8 x 8 voxels over the batch */
  int32_t ncob, ncib;              /* slab kernels: 48-channel blocks on the output / input side */
  int32_t nsplit;                  /* slab kernels: brick ranges = partial slabs per channel-block pair */
  int32_t bricks_per_workgroup;    /* slab kernels / NARROW: the most bricks one workgroup walks (> 1: its brick loop goes round) */
  int32_t direct;                  /* slab kernels: 0 = slabs + reduce launch; 1 = direct epilogue adding to dw; 2 = direct epilogue storing */
  int32_t fill;                    /* 1 = dw is zero-filled first (slab route, accumulate 0) */
  int32_t reduce_groups, spg;      /* slab route: split groups of the reduce launch, splits per group (groups > 1: fp32 atomics) */
  int32_t narrow_nco, narrow_nci;  /* NARROW: conv3_wgrad_narrow_kernel<NCO, NCI> (16-channel tiles a side); else 0 */
  int32_t tiny_s;                  /* TINY: conv3_wgrad_tiny_kernel<S> (3 / 6); else 0 */
  int32_t workgroups;              /* workgroups (grouped: units) of this layer in the main launch */
  int32_t walk;                    /* grouped: 1 = the grid this layer runs in is capped (descs[0].max_workgroups) and walks its units */
  int32_t grid_workgroups;         /* grouped: workgroups of that grid; single launch: = workgroups */
  int32_t group_target;            /* grouped: bricks per workgroup the group aimed at; else 0 */
} miseg_conv3_wgrad_form_info;
int miseg_conv3_wgrad_form(const miseg_conv3_wgrad_params* p, miseg_conv3_wgrad_form_info* form);
int miseg_conv3_wgrad_group_form(const miseg_conv3_wgrad_params* layers, int n, miseg_conv3_wgrad_form_info* forms);

/* ------------------------------------------------------------------------------------------------
 * Fused 3D (shifted-)window attention core: zero pad -> cyclic roll -> window partition -> per-head
 * softmax(q*scale k^T + bias_table[index] + shift mask) v -> window reverse -> roll back -> crop, with the
 * scores never leaving the CU.  Replaces networks/blocks/window_attention.py:99-119 (everything between
 * the qkv and proj Linears) and the data movement of swin_transformer_block.py:116-169 +
 * networks/utils/swin_utils.py:15-143.
 *   qkv: [B][D][H][W][3*C] rows (ldq) holding qkv = Linear(norm1(x)) of the UNPADDED grid; rows of padded
 *        tokens are synthesised in-kernel as the qkv bias (a zero token through the Linear).
 *   out: [B][D][H][W][C] rows (ldo), head-major channels, ready for the proj Linear.
 *   window wd/wh/ww (already clamped), shift sd/sh/sw (0 for un-shifted blocks),
 *   rel-pos index always computed for a `tw`^3 table window (reference quirk: 7^3 index sliced [:n,:n]).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* qkv; int64_t ldq; void* out; int64_t ldo;
  const float* qkv_bias;           /* fp32 [3C] or NULL */
  const float* bias_table;         /* fp32 [(2tw-1)^3][heads] or NULL (global attention) */
  float* lse;                      /* out fp32 [B*nW][heads][n]: log-sum-exp per query row, saved for bwd */
  int B, D, H, W, C, heads, dtype;
  int wd, wh, ww, sd, sh, sw, tw;
  float scale;
  /* ABI 3: dropout on the attention probabilities (attn_drop of WindowAttention, swin_transformer_block.py:56-58,91; the SABlock of the
   * ViT): drop_p in [0, 1), 0 = off.  The mask is the counter-based one of miseg_dropout over the matrix [B*nW*heads*n rows][n columns]
   * (row = ((window * heads + head) * n + query), column = key) with the same (seed, stream_id, step_dev) key, so the backward call
   * re-creates it from the same three values; nothing is stored.  Every kernel family takes it: the matrix-core kernels as a template
   * argument (`drop` of miseg_winattn_plan_info), the one-lane-per-query kernels as a run-time branch. */
  float drop_p; uint64_t drop_seed, drop_stream; const uint64_t* drop_step_dev;
} miseg_winattn_params;
int miseg_winattn_fwd(const miseg_winattn_params* p, miseg_stream_t stream);
/* 1 when miseg_winattn_fwd_plan accepts the call and names a matrix-core kernel (window or global), 0 when it names the one-lane-per-query
 * kernels or refuses the call.  No launch. */
int miseg_winattn_on_matrix_cores(const miseg_winattn_params* p);

typedef struct {
  miseg_winattn_params f;          /* same geometry; f.out is the saved forward output */
  const void* dout; int64_t lddo;  /* gradient w.r.t. out */
  void* dqkv; int64_t lddq;        /* gradient w.r.t. qkv (unpadded grid) */
  float* dqkv_bias;                /* accumulated: contribution of padded tokens; may be NULL */
  float* dbias_table;              /* accumulated fp32 [(2tw-1)^3][heads]; may be NULL */
} miseg_winattn_bwd_params;
/* dbias_table without f.bias_table is refused (MISEG_E_BADARG): there is no table to take the gradient of */
int miseg_winattn_bwd(const miseg_winattn_bwd_params* p, miseg_stream_t stream);
/* 1 when miseg_winattn_bwd_plan accepts the call and names a matrix-core kernel, 0 when it names the one-lane-per-query kernels or refuses
 * the call.  No launch.  (A new symbol: MISEG_ABI_VERSION stays 16.) */
int miseg_winattn_bwd_on_matrix_cores(const miseg_winattn_bwd_params* p);

/* What miseg_winattn_fwd(p) / miseg_winattn_bwd(p) do with these params - the launches dispatch on exactly this plan and the two question
 * entry points above read it.  Pointers are only tested for NULL and alignment, so a host may ask with stand-ins for buffers it has not
 * allocated yet.  Host only: touches no device.  Returns what the launch would return for a refused call, with the same miseg_last_error
 * text (kernel == MISEG_WINATTN_NONE and every field 0 then).  (New symbols and a new struct: MISEG_ABI_VERSION stays 16.) */
#define MISEG_WINATTN_NONE 0
#define MISEG_WINATTN_QUERY_LANE 1      /* either dtype, head_dim 4 .. 64: <T, hd4>, one lane per query, grid (windows, heads) */
#define MISEG_WINATTN_WINDOW_MFMA 2     /* bf16, head_dim 16, a table, <= 352 tokens: forward <mask, waves, drop>, backward <mask, table_grad, waves, drop> */
#define MISEG_WINATTN_GLOBAL_MFMA 3     /* bf16, head_dim 64, one unshifted window of <= 256 tokens, no table: <tiles, drop>, grid (tiles of 64, heads, B) */
typedef struct {
  int32_t kernel;                        /* MISEG_WINATTN_* */
  int32_t mask, drop, table_grad;        /* a shift is set / drop_p quantises to > 0 / dbias_table is given: template arguments of the
                                          * matrix-core kernels, run-time branches of the query-lane ones */
  int32_t waves;                         /* window forward 8, or 11 below 256 units; window backward 8; global 4; query-lane ceil(tokens / 64) */
  int32_t hd4;                           /* query-lane: head_dim / 4 (1, 2, 3, 4, 8, 16); else 0 */
  int32_t tiles;                         /* global: padded tokens / 16 (2, 4 .. 16); else 0 */
  int32_t vec;                           /* window matrix-core: operand rows are read as 16-byte vectors (a run-time flag); else 0 */
  int32_t grid_x, grid_y, grid_z, threads;
  int32_t tokens, table_size;            /* tokens per window; (2 tw - 1)^3 table entries per head, 0 without a table */
  int32_t units;                         /* workgroups: grid_x * grid_y * grid_z */
  size_t lds_bytes;                      /* dynamic LDS of the launch */
} miseg_winattn_plan_info;
int miseg_winattn_fwd_plan(const miseg_winattn_params* p, miseg_winattn_plan_info* plan);
int miseg_winattn_bwd_plan(const miseg_winattn_bwd_params* p, miseg_winattn_plan_info* plan);

/* ------------------------------------------------------------------------------------------------
 * Data-movement / small kernels (all channels-last rows)
 * ---------------------------------------------------------------------------------------------- */
/* y = a + b (elementwise over rows x C), any of the three may alias */
typedef struct { const void* a; int64_t lda; const void* b; int64_t ldb; void* y; int64_t ldy; int64_t rows; int C, dtype; } miseg_add_params;
int miseg_add(const miseg_add_params* p, miseg_stream_t stream);
/* y[b][s][c] = coef[b][c][0] * a[b][s][c] + coef[b][c][1] * x[b][s][c] + coef[b][c][2]   (ABI 5; coef: fp32 [B][C][3] on the device) - the input
 * gradient of a normalisation whose means run over several channels: dx = P dy + R x + Q with per-(sample, channel) coefficients */
typedef struct { uint32_t struct_size; const void* a; int64_t lda; const void* x; int64_t ldx; void* y; int64_t ldy; const float* coef; int B, S, C, dtype; } miseg_affine2_params;
int miseg_affine2(const miseg_affine2_params* p, miseg_stream_t stream);

/* strided 2D copy with dtype conversion: dst[r][c] = src[r][c] */
typedef struct { const void* src; int64_t lds; int sdtype; void* dst; int64_t ldd; int ddtype; int64_t rows; int C; } miseg_copy2d_params;
int miseg_copy2d(const miseg_copy2d_params* p, miseg_stream_t stream);

/* fp32 [R][C] -> dtype, optionally transposed to [C][R]  (weight re-packing for the NT GEMM) */
typedef struct { const float* src; void* dst; int R, C, dtype, transpose; } miseg_cast_params;
int miseg_cast_matrix(const miseg_cast_params* p, miseg_stream_t stream);

/* All per-step parameter re-layouts of a model in ONE launch (the per-call form above costs a ~4 us launch per
 * weight, ~100 per step of C-Swin-UNETR): descriptor i turns the fp32 matrix src [R][C] into dst in `dtype`,
 *   dst[r][m(c)] (transpose = 0)  or  dst[m(c)][r] (transpose = 1),   m(c) = (c % inner) * outer + c / inner
 * (inner = 1: identity; inner = 8, outer = Cout: the (co, tap) -> (tap, co) regrouping of ConvTranspose3d k2s2 weights,
 * unetr_block.py:80).  Descriptors live in device memory, sorted by tile0 = number of 32x32 tiles before them. */
typedef struct {
  const float* src; void* dst;
  int32_t R, C, transpose, inner, outer, tile0;
} miseg_cast_desc;
int miseg_param_cast_batch(const miseg_cast_desc* descs_dev, int ndesc, int total_tiles, int dtype, const int64_t* params_version, int64_t* state,
                           miseg_stream_t stream);      /* params_version / state: see miseg_pack_conv3_batch */

/* GELU (exact, erf): y = gelu(x); backward: dx = dy * gelu'(x)  (MONAI MLPBlock act, swin_transformer_block.py:97) */
typedef struct { const void* x; int64_t ldx; void* y; int64_t ldy; int64_t rows; int C, dtype; } miseg_gelu_fwd_params;
int miseg_gelu_fwd(const miseg_gelu_fwd_params* p, miseg_stream_t stream);
typedef struct { const void* dy; int64_t lddy; const void* x; int64_t ldx; void* dx; int64_t lddx; int64_t rows; int C, dtype; } miseg_gelu_bwd_params;
int miseg_gelu_bwd(const miseg_gelu_bwd_params* p, miseg_stream_t stream);

/* 2x2x2 space<->channel gathers.  `offsets` is 8 (dz,dy,dx) triples (host array): output channel block j of
 * the coarse voxel (d,h,w) is the fine voxel (2d+dz_j, 2h+dy_j, 2w+dx_j)  (zero beyond the fine grid).
 *   gather : fine [B][D][H][W][C] -> coarse [B][D2][H2][W2][8C]     (PatchMerging patch_merging.py:120-128 /
 *            PatchMergingV2 :69-71 slice tables; ConvTranspose k2s2 data gradient)
 *   scatter: coarse -> fine, fine[v] = sum of the blocks that reference v   (PatchMerging backward;
 *            ConvTranspose3d k2 s2 forward unetr_block.py:51-59 after the [Cin]x[8*Cout] GEMM)
 */
typedef struct {
  const void* src; int64_t lds; void* dst; int64_t ldd;
  int B, D, H, W, C, dtype;        /* D,H,W: FINE grid; coarse grid is ceil(./2) */
  int8_t offsets[24];
} miseg_s2c_params;
int miseg_space_to_channel(const miseg_s2c_params* p, miseg_stream_t stream);
int miseg_channel_to_space(const miseg_s2c_params* p, miseg_stream_t stream);

/* ---- plans of the network ends (patch embedding, one- to four-channel stem convolution, output head) ----
 * miseg_<call>_plan(&params, &plan) tells what miseg_<call>(&params, stream) will launch; each launcher dispatches on exactly this plan,
 * and a problem the call refuses gets the same error code from the plan.  Pointers are only tested for NULL and alignment, so a host may
 * ask with stand-ins for buffers it has not allocated.  Host only: touches no device.  (New symbols: MISEG_ABI_VERSION stays 16.) */
#define MISEG_NE_NONE 0                  /* no launch (head_bwd: dx or dw is NULL) */
#define MISEG_NE_STEM_FWD_GENERIC 1      /* thread = voxel: Cin 2..4, ragged Cout, misaligned y */
#define MISEG_NE_STEM_FWD_BRICK 2        /* Cin 1, Cout % 8 == 0 <= 64, 4x4x16 bricks, persistent workgroups (cap 4096) */
#define MISEG_NE_STEM_FWD_MFMA 3         /* bf16, Cin 1, Cout 48, matrix cores (cap 2048) */
#define MISEG_NE_STEM_WGRAD_GENERIC 4    /* one 8x8x8 brick per workgroup, fp32 atomics */
#define MISEG_NE_STEM_WGRAD_BRICK 5      /* Cin 1, persistent workgroups (cap 512), fp32 atomics */
#define MISEG_NE_STEM_WGRAD_MFMA 6       /* bf16, Cin 1, Cout 48, matrix cores (cap 512); partial sums with a workspace and >= 16 workgroups */
#define MISEG_NE_PATCH_FWD 7             /* the one forward kernel; idx32 tells its item arithmetic */
#define MISEG_NE_PATCH_BWD_GENERIC 8     /* 1024 coarse voxels per workgroup, fp32 atomics */
#define MISEG_NE_PATCH_BWD_TEAM 9        /* Cout a whole number of 16-byte vectors, aligned dy; workgroups x Cin; partial sums as above */
#define MISEG_NE_HEAD_FWD_SCALAR 10      /* thread = voxel, element loads */
#define MISEG_NE_HEAD_FWD_TILE 11        /* 256-voxel tiles, 16-byte loads, persistent workgroups (cap 1152) */
#define MISEG_NE_HEAD_DX_SCALAR 12
#define MISEG_NE_HEAD_DX_TEAM 13         /* lane = (voxel, 16-byte channel vector); idx32 tells its item arithmetic */
#define MISEG_NE_HEAD_DX_TILE 14         /* bf16, Cout <= 8, S % 256 == 0, Cin <= 256: 256-voxel tiles (cap 1152) */
#define MISEG_NE_HEAD_DW_GENERIC 15      /* 2048 voxels per workgroup */
#define MISEG_NE_HEAD_DW_TEAM 16         /* lane = (row, channel vector); one pass per 8 output channels */
#define MISEG_NE_HEAD_DW_MFMA 17         /* bf16, Cin 48, S % 256 == 0, matrix cores (cap 512) */
typedef struct {
  int32_t kernel;                  /* MISEG_NE_* */
  int32_t workgroups;              /* gridDim.x of the launch (of each pass) */
  int32_t workgroups_y;            /* gridDim.y: Cin for MISEG_NE_PATCH_BWD_TEAM, else 1 */
  int32_t per_workgroup;           /* items one workgroup takes per trip of its loop: 1 brick or tile, 256 thread items, or its block of rows */
  int64_t items;                   /* bricks, tiles, thread items or rows of the whole problem: > workgroups * per_workgroup means the loops wrap */
  int32_t passes;                  /* launches of this kernel (MISEG_NE_HEAD_DW_TEAM: ceil(Cout / 8)), 0 for MISEG_NE_NONE */
  int32_t partial;                 /* 1: per-workgroup partial sums in `workspace` and a reduce launch (a fixed order of summation); 0: fp32 atomics or no sums */
  int32_t idx32;                   /* 1: 32-bit item arithmetic (MISEG_NE_PATCH_FWD, MISEG_NE_HEAD_DX_TEAM), else 0 */
  int32_t pad_;
} miseg_net_end_launch;
typedef struct { miseg_net_end_launch dx, dw; } miseg_head_bwd_plan_info;

/* PatchEmbed Conv3d(k2,s2)+bias with Cin input channels given as NCDHW fp32 (the network input)
 * (networks/blocks/patch_embedding.py:167-169,204).  w: fp32 [Cout][Cin][2][2][2]. */
typedef struct {
  const float* x; void* y; int64_t ldy; const float* w; const float* bias;
  int B, Cin, D, H, W, Cout, dtype;  /* D,H,W: input grid (even) */
} miseg_patch_embed_params;
int miseg_patch_embed_fwd_plan(const miseg_patch_embed_params* p, miseg_net_end_launch* plan);
int miseg_patch_embed_fwd(const miseg_patch_embed_params* p, miseg_stream_t stream);
typedef struct {
  const float* x; const void* dy; int64_t lddy; float* dw; float* dbias;   /* accumulated */
  int B, Cin, D, H, W, Cout, dtype;
  void* workspace;   /* optional, miseg_patch_embed_bwd_workspace_bytes(p): per-workgroup partial sums + a second small launch instead of
                      * fp32 atomics from every workgroup onto the 9 * Cout outputs (46 of 53 us on the headline patch) */
} miseg_patch_embed_bwd_params;
size_t miseg_patch_embed_bwd_workspace_bytes(const miseg_patch_embed_bwd_params* p);
int miseg_patch_embed_bwd_plan(const miseg_patch_embed_bwd_params* p, miseg_net_end_launch* plan);
int miseg_patch_embed_bwd(const miseg_patch_embed_bwd_params* p, miseg_stream_t stream);

/* First encoder conv: 3x3x3, Cin in {1..4} NCDHW fp32 input -> channels-last Cout (dynunet_block.py:55-64 with
 * in_channels = image channels).  Weight gradient accumulated into dw fp32 [Cout][Cin][27]. */
typedef struct {
  const float* x; void* y; int64_t ldy; const float* w;
  int B, Cin, D, H, W, Cout, dtype;
} miseg_conv3_thin_params;
int miseg_conv3_thin_fwd_plan(const miseg_conv3_thin_params* p, miseg_net_end_launch* plan);
int miseg_conv3_thin_fwd(const miseg_conv3_thin_params* p, miseg_stream_t stream);
typedef struct {
  const float* x; const void* dy; int64_t lddy; float* dw;
  int B, Cin, D, H, W, Cout, dtype;
  void* workspace;   /* optional, miseg_conv3_thin_wgrad_workspace_bytes(p) (0: not used by this shape): per-workgroup partial sums + a second
                      * small launch instead of fp32 atomics from every workgroup onto the 27 * Cout outputs */
} miseg_conv3_thin_wgrad_params;
size_t miseg_conv3_thin_wgrad_workspace_bytes(const miseg_conv3_thin_wgrad_params* p);
int miseg_conv3_thin_wgrad_plan(const miseg_conv3_thin_wgrad_params* p, miseg_net_end_launch* plan);
int miseg_conv3_thin_wgrad(const miseg_conv3_thin_wgrad_params* p, miseg_stream_t stream);

/* Network input (NCDHW fp32, Cin <= 8 image channels) -> channels-last rows of CP channels (CP = 4 for fp32, 8 for bf16:
 * one 16-byte vector per voxel), channels >= Cin zero.  Feeds the first encoder convs (dynunet_block.py:55-64 with
 * in_channels = image channels) to the implicit-GEMM kernels above. */
int miseg_ncdhw_to_rows(const float* x, void* y, int B, int Cin, int64_t S, int CP, int dtype, miseg_stream_t stream);

/* ---- pieces of the MONAI residual UNet (networks/nets/unet.py:169-205, blocks/convolutions.py:173-179,323-329, acti_norm.py:104-110) ----
 * A stride-2 3x3x3 convolution is the stride-1 kernel followed by `resample2` dir 0 (keep the even voxels); ConvTranspose3d k3 s2 p1 op1 is
 * `resample2` dir 1 (zero insertion) followed by the stride-1 kernel on the mirrored / channel-swapped pack -- the two directions are each
 * other's adjoint, so the backward passes are the same two kernels.  D, H, W are the FINE grid; the coarse grid is ceil(./2). */
typedef struct { const void* x; int64_t ldx; void* y; int64_t ldy; int B, D, H, W, C, dtype, dir; } miseg_resample2_params;
int miseg_resample2(const miseg_resample2_params* p, miseg_stream_t stream);
/* ---- decoder step of the conditional UNet (networks/nets/unet_vanilla.py:101-117 nn.Upsample(scale_factor=f) nearest, :162-169
 * torch.concat((skip, up), dim=1)) ----
 * out[b,z,y,x][0:Cs] = skip[b,z,y,x][:], out[b,z,y,x][Cs:Cs+Cu] = x[b, z/f, y/f, x/f][:] in one launch; f = 1 or 2, the FINE grid D, H, W exactly
 * f x x's grid.  Channels-last rows with their own leading dimensions.  The skip's gradient is the left half of the concat's gradient (a view,
 * no kernel); x's gradient is miseg_upsample_cat_bwd below.  Both only enqueue and can be captured. */
typedef struct { const void* skip; int64_t ldskip; const void* x; int64_t ldx; void* out; int64_t ldout; int B, D, H, W, Cs, Cu, factor, dtype; } miseg_upsample_cat_params;
int miseg_upsample_cat(const miseg_upsample_cat_params* p, miseg_stream_t stream);
/* dx[b,z',y',x'][c] = sum over the f^3 fine children, in (dz, dy, dx) order, of dcat[child][c] -- dcat is the right half of the concat's
 * gradient as a row view (its first channel, its leading dimension), D, H, W the fine grid; fp32 accumulation rounded once to dtype, no
 * atomics (bit-reproducible). */
typedef struct { const void* dcat; int64_t lddcat; void* dx; int64_t lddx; int B, D, H, W, C, factor, dtype; } miseg_upsample_cat_bwd_params;
int miseg_upsample_cat_bwd(const miseg_upsample_cat_bwd_params* p, miseg_stream_t stream);
/* y[r][c] = x[r][c] + bias[c]  (Conv3d / ConvTranspose3d bias, convolutions.py:115-139; the gradient is miseg_colsum) */
typedef struct { const void* x; int64_t ldx; const float* bias; void* y; int64_t ldy; int64_t rows; int C, dtype; } miseg_rowbias_params;
int miseg_rowbias_add(const miseg_rowbias_params* p, miseg_stream_t stream);
/* PReLU with ONE learnable slope (torch.nn.PReLU() as built by ADN, acti_norm.py:90-93): y = x > 0 ? x : a x;
 * backward: dx = dy (x > 0 ? 1 : a), dslope += sum dy x [x <= 0]  (dslope accumulated, may be NULL) */
typedef struct { const void* x; int64_t ldx; const float* slope; void* y; int64_t ldy; int64_t rows; int C, dtype; } miseg_prelu_fwd_params;
int miseg_prelu_fwd(const miseg_prelu_fwd_params* p, miseg_stream_t stream);
typedef struct {
  const void* dy; int64_t lddy; const void* x; int64_t ldx; const float* slope; void* dx; int64_t lddx; float* dslope; int64_t rows; int C, dtype;
  double* scratch;   /* DEVICE double[2], zero on entry (with dslope): the one-element slope gradient is a cancelling sum over every voxel - workgroup
                        partials meet here in float64 and the last workgroup adds the total to dslope (fp32 atomics were off by up to 60 %) */
} miseg_prelu_bwd_params;
int miseg_prelu_bwd(const miseg_prelu_bwd_params* p, miseg_stream_t stream);
/* channels-last rows [B][S][C] (ld) in `dtype`  <->  NCDHW fp32 [B][C][S]: dir 0 rows -> NCDHW (network output), dir 1 NCDHW -> rows */
int miseg_layout_ncdhw(const void* rows_, int64_t ld, float* ncdhw, int B, int C, int64_t S, int dtype, int dir, miseg_stream_t stream);

/* Output head: Conv3d 1x1x1 + bias from channels-last rows to NCDHW fp32 logits (dynunet_block.py:273-292),
 * and its backward (dx channels-last, dw/dbias accumulated). */
typedef struct {
  const void* x; int64_t ldx; float* y; const float* w; const float* bias;
  int B, S, Cin, Cout, dtype;
} miseg_head_params;
int miseg_head_fwd_plan(const miseg_head_params* p, miseg_net_end_launch* plan);
int miseg_head_fwd(const miseg_head_params* p, miseg_stream_t stream);
typedef struct {
  const void* x; int64_t ldx; const float* dy; void* dx; int64_t lddx; const float* w; float* dw; float* dbias;
  int B, S, Cin, Cout, dtype;
} miseg_head_bwd_params;
int miseg_head_bwd_plan(const miseg_head_bwd_params* p, miseg_head_bwd_plan_info* plan);
int miseg_head_bwd(const miseg_head_bwd_params* p, miseg_stream_t stream);

/* im2col for 3x3x3/pad 1 on small grids (<= 6^3): col[v][tap][ci]; and its adjoint col2im (dst zero-filled by
 * the kernel).  Used with miseg_gemm where the implicit-GEMM tile would be mostly halo. */
typedef struct { const void* src; int64_t lds; void* dst; int64_t ldd; int B, D, H, W, C, dtype; } miseg_im2col3_params;
int miseg_im2col3(const miseg_im2col3_params* p, miseg_stream_t stream);
int miseg_col2im3(const miseg_im2col3_params* p, miseg_stream_t stream);

/* fill a buffer of n 32-bit words with a value (gradient arenas, accumulators) */
#define MISEG_FILL_RANGES 16
/* dst[off .. off + len) = value for up to MISEG_FILL_RANGES (offset, length) pairs, in 32-bit words, of one 16-byte aligned buffer in ONE launch
 * (ABI 8; ranges_host: HOST array [n][2], copied into the kernel arguments; offsets multiples of 4 words): the per-step zero fill of the gradient
 * arena minus the slots whose weight-gradient kernel overwrites them whole (mi-seg_amd/runtime/arena.py) */
int miseg_fill32_ranges(void* dst, uint32_t value, const uint64_t* ranges_host, int n, miseg_stream_t stream);
int miseg_fill32(void* dst, uint32_t value, size_t n, miseg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * After the path, every training step: segmentation loss + d(loss)/d(logits), Dice metric,
 * multi-tensor optimiser step over the gradient arena, sliding-window stitching.  MONAI 1.1.0 arithmetic restated from its
 * public API (the reference calls it at networks/lightning_monai.py:46-67,68-79,86-93,190-195,255-278; MONAI itself is a
 * pinned dependency that is not vendored: PARITY UNPINNED by any reference test).
 * ---------------------------------------------------------------------------------------------- */
enum { MISEG_LABEL_F32 = 0, MISEG_LABEL_I32 = 1, MISEG_LABEL_I64 = 2, MISEG_LABEL_U8 = 3 };
enum { MISEG_LOSS_DICE_FOCAL = 0, MISEG_LOSS_DICE_CE = 1, MISEG_LOSS_GDICE_FOCAL = 2 };
enum { MISEG_GDICE_W_SQUARE = 0, MISEG_GDICE_W_SIMPLE = 1, MISEG_GDICE_W_UNIFORM = 2 };
/* DiceFocalLoss / DiceCELoss(to_onehot_y=True, softmax=True) on fp32 NCDHW logits [B][C][S] and class-id labels [B][1][S]
 * (lightning_monai.py:48-65, training_step :149-166).
 *   dice_focal, include_background = 0: channel 0 is stripped from logits AND target first, the softmax of the Dice term runs over the C-1
 *     foreground logits, the focal term (sigmoid form on raw logits, gamma) over the same channels;  = 1: all C channels.
 *   dice_ce: softmax over all C channels, Dice over channels >= (include_background ? 0 : 1), cross-entropy over all channels.
 *   Dice per (b, c): 1 - (2 sum(p t) + smooth_nr) / (sum(t) + sum(p^2 or p) + smooth_dr), mean over (b, c); focal: mean over (b, c, s); CE: mean over (b, s).
 *   gdice_focal (ABI 14): GeneralizedDiceFocalLoss(to_onehot_y=True, softmax=True) (utils/training_utils.py:26-33).  Softmax over
 *     ALL C channels, then channel 0 dropped from the Dice and focal terms when include_background = 0.  Per sample b, over the kept classes:
 *     1 - (2 sum_c w I + smooth_nr) / (sum_c w (G + P) + smooth_dr), I = sum(p t), G = sum(t), P = sum(p) (never squared: squared_pred is ignored),
 *     w = 1/G^2 | 1/G | 1 by weight_type, an infinite w replaced by the sample's largest finite one (all infinite: all 0); mean over b.  Focal as dice_focal.
 * miseg_seg_loss_fwd: one pass over logits + labels -> per-workgroup fp64 partial sums in `workspace`, summed in a FIXED order by a
 *   one-workgroup launch (bit-reproducible) into sums[B][C][3] (sum p t, sum p^2|p, sum t) + sums[3 B C] (focal / CE total) and the scalar loss.
 * miseg_seg_loss_bwd: second pass -> dlogits [B][C][S] fp32 = gscale * d(loss)/d(logits) (gscale: device scalar or NULL = 1), from the saved sums. */
typedef struct {
  uint32_t struct_size;            /* sizeof(miseg_seg_loss_params): checked against the library's own */
  int kind;                        /* MISEG_LOSS_* */
  const float* logits; const void* label; int label_dtype;
  int B, C; int64_t S;
  int include_background, squared_pred;
  float smooth_nr, smooth_dr, gamma, lambda_dice, lambda_other;
  void* workspace;                 /* miseg_seg_loss_workspace_bytes(B, C, S) bytes, uninitialised */
  double* sums;                    /* out (fwd) / in (bwd): 3 B C + 1 doubles */
  float* loss;                     /* out (fwd): scalar */
  const float* gscale; float* dlogits;   /* bwd only */
  int weight_type;                 /* MISEG_GDICE_W_*: gdice_focal only, ignored by the other kinds */
} miseg_seg_loss_params;
size_t miseg_seg_loss_workspace_bytes(int B, int C, int64_t S);
int miseg_seg_loss_fwd(const miseg_seg_loss_params* p, miseg_stream_t stream);
int miseg_seg_loss_bwd(const miseg_seg_loss_params* p, miseg_stream_t stream);

/* DiceMetric(include_background=True, get_not_nans=True) after AsDiscrete(argmax=True, to_onehot=C) (lightning_monai.py:68-79,190-195):
 * dice[b][c] = 2 |pred == c & label == c| / (|pred == c| + |label == c|), NaN where |label == c| == 0; argmax takes the FIRST maximum.
 * counts: uint64 [B][C][3] scratch (zeroed by the call; integer atomics: bit-reproducible).
 * gdice (ABI 14, optional): GeneralizedDiceScore(include_background, weight_type) from the SAME counts (tune.py:124-129,208-213; MONAI 1.1.0
 *   compute_generalized_dice, parity unpinned): per sample over the kept classes 2 sum_c w I / sum_c w (G + P) with the weights of
 *   gdice_focal above; where that denominator is 0: 1 if the prediction has no kept-class voxel, else 0.  NULL: Dice alone, as before. */
typedef struct {
  uint32_t struct_size;
  const float* logits; const void* label; int label_dtype;
  int B, C; int64_t S;
  uint64_t* counts; float* dice;   /* out fp32 [B][C] */
  float* gdice;                    /* out fp32 [B] or NULL */
  int include_background, weight_type;   /* of gdice: MISEG_GDICE_W_* */
} miseg_dice_metric_params;
int miseg_dice_metric(const miseg_dice_metric_params* p, miseg_stream_t stream);

/* SurfaceDistanceMetric(include_background, symmetric, distance_metric='euclidean') after AsDiscrete(argmax=True, to_onehot=C) (test.py:145-151;
 * MONAI 1.1.0 metrics/surface_distance.py::compute_average_surface_distance, parity unpinned): per sample b and class c, with P = (pred == c)
 * and G = (label == c), the masks are cropped to the tight box of P | G and squeezed (a box side of one voxel has no neighbours), edges are
 * M ^ erode(M) (cross structure, zero border), and asd[b][c'] is the mean exact Euclidean distance (voxel units) of E_P to the nearest voxel
 * of E_G, concatenated with E_G -> E_P when `symmetric`.  One side's edges empty => inf; both empty (or no foreground) => NaN.
 * The prediction is either fp32 logits [B][C][D][H][W] (argmax, the FIRST maximum wins) or an int32 class map [B][D][H][W]: exactly one of
 * the two.  Label values (and class-map values) outside [0, C) belong to no class.  include_background = 0 leaves out class 0: c' = c - 1.
 * Every side of the volume 1..4096, C 1..64.  The call reads the (b, c) boxes back to the host to size the distance passes, so it synchronises
 * the stream and cannot be captured into a graph.  Results are bit-reproducible (fixed-order double sums). */
typedef struct {
  uint32_t struct_size;
  const float* logits; const int32_t* pred;
  const void* label; int label_dtype;
  int B, C, D, H, W;
  int include_background, symmetric;
  void* workspace;                 /* miseg_surface_distance_workspace_bytes(B, C, D, H, W) bytes, uninitialised */
  double* asd;                     /* out fp64 [B][C - (include_background ? 0 : 1)] */
} miseg_surface_distance_params;
size_t miseg_surface_distance_workspace_bytes(int B, int C, int D, int H, int W);
int miseg_surface_distance(const miseg_surface_distance_params* p, miseg_stream_t stream);

/* The average surface distance above and / or the Hausdorff distance (MONAI 1.1.0 metrics/hausdorff_distance.py::compute_hausdorff_distance,
 * parity unpinned) from ONE launch set: same edge sets, same one-way distance lists d(A -> B).  h(A -> B) is NaN for an empty list, inf for
 * a list of infs (one edge set empty; numpy's percentile would give NaN there), else the maximum of the list
 * (percentile <= 0) or numpy's "linear" percentile of it: v_lo + (v_hi - v_lo) (pos - lo) with pos = percentile / 100 (n - 1), lo = floor(pos),
 * hi = min(lo + 1, n - 1) over the ascending list.  hd[b][c'] = h(P -> G) if `directed`, else max(h(P -> G), h(G -> P)).  The order statistics
 * are taken on the exact integer squared distances with integer counters only: bit-reproducible, like the ASD.  At least one of asd / hd; the
 * ASD written is the one miseg_surface_distance writes, bit for bit.  With hd the volume must hold fewer than 2^32 voxels (32-bit bin counts).
 * Same limits otherwise (C 1..64, every side 1..4096, synchronises the stream, cannot be captured). */
typedef struct {
  uint32_t struct_size;
  const float* logits; const int32_t* pred;
  const void* label; int label_dtype;
  int B, C, D, H, W;
  int include_background, symmetric;   /* symmetric: of the ASD only */
  void* workspace;                 /* miseg_surface_metrics_workspace_bytes(B, C, D, H, W) bytes, uninitialised */
  double* asd;                     /* out fp64 [B][C'] or NULL */
  double* hd;                      /* out fp64 [B][C'] or NULL */
  double percentile;               /* of hd: (0, 100]; <= 0: the maximum; > 100 (or NaN): MISEG_E_BADARG */
  int directed;                    /* of hd */
} miseg_surface_metrics_params;
size_t miseg_surface_metrics_workspace_bytes(int B, int C, int D, int H, int W);
int miseg_surface_metrics(const miseg_surface_metrics_params* p, miseg_stream_t stream);

/* The two metrics above and / or the normalized surface Dice (NSD; MONAI's SurfaceDiceMetric / compute_surface_dice, parity unpinned) from ONE
 * launch set, on the objects of DESIGN.md section 7.1 (rules in section 7.9): the same edge sets E_P, E_G, cropped to the box of P | G and
 * squeezed, and the same one-way lists d(P -> G), d(G -> P).  With tau = thresholds[c'] (voxel units, one per class AFTER include_background):
 *   nsd[b][c'] = (#{d in d(P -> G) : d <= tau} + #{d in d(G -> P) : d <= tau}) / (|d(P -> G)| + |d(G -> P)|)   in double;
 * both lists empty (no foreground, or a union of one voxel) => NaN; one edge set empty => both lists all inf => 0.0.  `d <= tau` is the double
 * comparison on sqrt(d^2); it is made on the exact integer d^2 against the largest integer k with sqrt((double)k) <= tau, so the result is
 * bit-reproducible and equals the CPU restatement's.  `thresholds` is a HOST array, read during the call; every value finite and >= 0.  At
 * least one of asd / hd / nsd; with nsd NULL the call is miseg_surface_metrics (same kernels), and asd / hd are bit for bit those of the two
 * calls above in every case.  Same limits (C 1..64, every side 1..4096, fewer than 2^32 voxels with hd, synchronises, cannot be captured). */
typedef struct {
  uint32_t struct_size;
  const float* logits; const int32_t* pred;
  const void* label; int label_dtype;
  int B, C, D, H, W;
  int include_background, symmetric;   /* symmetric: of the ASD only */
  void* workspace;                 /* miseg_surface_dice_workspace_bytes(B, C, D, H, W) bytes, uninitialised */
  double* asd;                     /* out fp64 [B][C'] or NULL */
  double* hd;                      /* out fp64 [B][C'] or NULL */
  double percentile;               /* of hd: (0, 100]; <= 0: the maximum; > 100 (or NaN): MISEG_E_BADARG */
  int directed;                    /* of hd */
  double* nsd;                     /* out fp64 [B][C'] or NULL */
  const double* thresholds;        /* of nsd: HOST array of C' = C - (include_background ? 0 : 1) tolerances */
} miseg_surface_dice_params;
size_t miseg_surface_dice_workspace_bytes(int B, int C, int D, int H, int W);
int miseg_surface_dice(const miseg_surface_dice_params* p, miseg_stream_t stream);

/* One optimiser step for every parameter of a model in ONE launch (lightning_monai.py:255-278: AdamW / Adam / SGD-nesterov), over the flat
 * fp32 gradient arena the weight-gradient kernels accumulate into.  Descriptor i: parameter tensor `param` of n elements whose gradient, and
 * whose two state slots, live at element offset `off` of grad / state1 / state2 (state2 unused by SGD).  used[i] == 0 => the parameter had no
 * gradient this step (`grad is None`: an absent style's norm rows) and is skipped entirely - no update, no weight decay, no step count -
 * exactly like torch.optim skips `p.grad is None`.  steps[i] (int32, device) counts the updates of parameter i (Adam bias correction).
 * Descriptors live in device memory sorted by block0 = number of 4096-element blocks before them. */
enum { MISEG_OPT_ADAMW = 0, MISEG_OPT_ADAM = 1, MISEG_OPT_SGD_NESTEROV = 2 };
typedef struct { float* param; int64_t off; int32_t n, block0; } miseg_opt_desc;
typedef struct {
  uint32_t struct_size;
  int kind;
  const miseg_opt_desc* descs_dev; int ndesc, total_blocks;
  const float* grad; float* state1; float* state2;
  const int32_t* used; int32_t* steps;
  float lr, beta1, beta2, eps, weight_decay, momentum;
  const float* lr_dev;             /* optional device scalar overriding lr (schedulers under hipGraph replay) */
  int64_t* params_version;         /* optional DEVICE int64, incremented once per launch: the parameters changed (miseg_pack_conv3_batch) */
  /* ABI 8, a step in TWO launches over disjoint descriptor tables (the parameters whose gradients are final early - the big tiny-volume conv
   * weights of the headline net - are updated on a side stream beside the end of the backward pass, the rest after it):
   * index (optional, DEVICE int32 [ndesc]): descriptor d of THIS table is parameter index[d] of used / steps (NULL: d itself);
   * count_n: > 0 = after the update, steps[i] += used[i] for i < count_n and params_version is bumped (the LAST launch of a step, over all
   * parameters); 0 = an early launch: neither (every launch of a step must see the step counts of before it); < 0 = ndesc (one-launch step). */
  const int32_t* index; int32_t count_n;
} miseg_opt_step_params;
int miseg_opt_step(const miseg_opt_step_params* p, miseg_stream_t stream);

/* ABI 9.  The optimiser step of every 3x3x3 conv weight of a model TOGETHER WITH its re-layout (lightning_monai.py:255-278 + what the next
 * forward pass needs of dynunet_block.py:295-326): the launch walks the 16 x 16 (co, ci) tiles of the miseg_pack_conv3_batch table, updates a
 * tile's weights / state from their gradients (same arithmetic as miseg_opt_step, element offsets of `grad` / `state1` / `state2` = map[i].off
 * + the element's index in the weight) and writes the tile's forward and data-gradient packs from the NEW values.  The refresh launch of the
 * next step then has nothing to do for these weights: with `pack_state` (the `state` words of that table's versioned refresh) the launch
 * records the new parameter version there.  map[i] belongs to descs[i]; param_index = the weight's row in used / steps.  A tensor with
 * used[param_index] == 0 is left alone (weights, state, packs).  `p`: descs_dev / ndesc / total_blocks / index are ignored; count_n > 0 = this is
 * the LAST launch of the step (steps[i] += used[i] for i < count_n, version bump - see miseg_opt_step); 0 = another launch follows. */
typedef struct { int64_t off; int32_t param_index, pad_; } miseg_opt_pack_map;
int miseg_opt_step_pack_conv3(const miseg_opt_step_params* p, const miseg_pack_conv3_desc* descs_dev, const miseg_opt_pack_map* map_dev, int n, int total_tiles,
                              int dtype, int64_t* pack_state, miseg_stream_t stream);

/* Gradient clipping and the non-finite step guard of the fused optimiser (Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm,
 * track_grad_norm), which the reference's train.py takes through Trainer.add_argparse_args; new symbols: MISEG_ABI_VERSION stays 16).
 *
 * miseg_grad_norm: the global L2 norm of the gradient arena over the parameters with used[i] != 0, in two launches and without atomics.
 *   1. one workgroup per 4096-element block of the descriptor table (the table of miseg_opt_step over ALL parameters: used[] is indexed by the
 *      descriptor) squares and sums its elements in double - per thread its 16 elements in ascending order, then a shuffle tree over the 64
 *      lanes, then the four waves in order - and stores the block's partial; a block of an unused parameter reads nothing and stores 0.
 *   2. one workgroup of 16 waves: a tensor's partials are added by one wave (which one does not matter to the sum): lane l adds partials
 *      l, l + 64, ... in ascending order, then the shuffle tree (offsets 32, 16, .., 1); thread t then adds the tensor sums t, t + 1024, ...
 *      in ascending order, the shuffle tree again, and thread 0 adds the 16 wave sums in ascending order.  The order depends on the table
 *      alone: equal bits every run.
 * The launch fills `record`:  norm = (float)sqrt(S);  coef = fminf(1, max_norm / (norm + 1e-6f)), every operation rounded in fp32
 * (torch.nn.utils.clip_grad_norm_) in MISEG_CLIP_NORM mode, 1 otherwise;  finite = isfinite(norm);  skip = skip_nonfinite && !finite;  and the
 * running counters seen (+1 per call), clipped (+1 when coef < 1), skipped (+1 when skip) - the caller zeroes the record once.
 * per_param (optional, fp32 [ndesc]): every tensor's own L2 norm, 0 for an unused one.  used: optional (NULL = every parameter).
 * workspace: miseg_grad_norm_workspace_bytes(total_blocks, ndesc) bytes, 8-byte aligned.  max_norm is read in MISEG_CLIP_NORM mode only.
 *
 * miseg_opt_step_clipped / miseg_opt_step_pack_conv3_clipped: miseg_opt_step / miseg_opt_step_pack_conv3 on the clipped gradient
 *   MISEG_CLIP_NORM : g' = g * rec->coef, the product rounded on its own (never contracted into the update's multiply-adds): the result is
 *                     bit-identical to the plain step on gradients multiplied by coef beforehand;  clip_value is ignored
 *   MISEG_CLIP_VALUE: g' = g < -clip_value ? -clip_value : (g > clip_value ? clip_value : g)  (a NaN stays a NaN, as in torch.clamp)
 *   MISEG_CLIP_NONE : g' = g (the guard alone)
 * The gradient arena itself is never written.  With rec_dev->skip set every workgroup returns before its first store: parameters, moments,
 * conv packs, steps, params_version and pack_state keep their bits.  rec_dev may be NULL only in MISEG_CLIP_VALUE mode (no guard).
 * Refused before any launch: a wrong struct_size, a null pointer, an unknown mode, a max_norm / clip_value that is not finite or <= 0,
 * MISEG_CLIP_NORM or MISEG_CLIP_NONE without a record. */
enum { MISEG_CLIP_NONE = 0, MISEG_CLIP_NORM = 1, MISEG_CLIP_VALUE = 2 };
typedef struct {
  float norm, coef;
  int32_t finite, skip;
  uint32_t seen, clipped, skipped, reserved;
} miseg_grad_clip_record;
typedef struct {
  uint32_t struct_size;
  int mode;                        /* MISEG_CLIP_* */
  const miseg_opt_desc* descs_dev; int ndesc, total_blocks;
  const float* grad;
  const int32_t* used;
  float max_norm;
  int skip_nonfinite;
  void* workspace;
  miseg_grad_clip_record* record;
  float* per_param;
} miseg_grad_norm_params;
size_t miseg_grad_norm_workspace_bytes(int total_blocks, int ndesc);
int miseg_grad_norm(const miseg_grad_norm_params* p, miseg_stream_t stream);
int miseg_opt_step_clipped(const miseg_opt_step_params* p, const miseg_grad_clip_record* rec_dev, int mode, float clip_value, miseg_stream_t stream);
int miseg_opt_step_pack_conv3_clipped(const miseg_opt_step_params* p, const miseg_pack_conv3_desc* descs_dev, const miseg_opt_pack_map* map_dev, int n,
                                      int total_tiles, int dtype, int64_t* pack_state, const miseg_grad_clip_record* rec_dev, int mode, float clip_value,
                                      miseg_stream_t stream);

/* Gradient accumulation over the micro-batches of a window (the reference's --iters_to_accumulate, utils/trainer.py:33-78, and Lightning's
 * --accumulate_grad_batches; a new symbol and struct: MISEG_ABI_VERSION stays 16).  Every micro-batch runs its forward and backward pass as a
 * step of its own (zero fill, storing weight-gradient kernels); miseg_grad_fold then streams once over the gradient arena `grad` and a second
 * flat fp32 buffer `acc` laid out like it, in miseg_opt_step's geometry (the same descriptor table over ALL parameters; `param` is not
 * looked at).  ops[i] (device int32 [ndesc]) says what happens to parameter i:  u (bit 0) = it has a gradient in this micro-batch,
 * a (bit 1) = it had one in an earlier micro-batch of this window, F (bit 2) = this micro-batch closes the window.  Per element, every
 * operation rounded on its own in fp32 (no contraction):
 *   0, 2, 4      nothing: neither buffer's slot is read or written (it may hold anything)
 *   1 (u)        acc = g                          acc is not read
 *   3 (u, a)     acc = fl(acc + g)
 *   5 (F, u)     grad = fl(g * scale)             acc is not touched
 *   6 (F, a)     grad = fl(acc * scale)           the arena slot is not read
 *   7 (F, u, a)  grad = fl(fl(acc + g) * scale)
 * After the closing call the ARENA holds scale x the window's sum in micro-batch order (scale = fl(1 / window length): the mean), and
 * miseg_grad_norm / miseg_opt_step* run on it unchanged with used[] = the union of the window.  No atomics; equal bits every run.
 * Refused before any launch: a wrong struct_size, a null pointer, ndesc / total_blocks / arena_elems < 1, a scale that is not finite or
 * <= 0, grad / acc not 16-byte aligned, [grad, grad + arena_elems) and [acc, acc + arena_elems) overlapping. */
typedef struct {
  uint32_t struct_size;
  const miseg_opt_desc* descs_dev; int ndesc, total_blocks;
  float* grad; float* acc;
  const int32_t* ops;
  int64_t arena_elems;             /* elements of each of the two buffers (the overlap check) */
  float scale;
} miseg_grad_fold_params;
int miseg_grad_fold(const miseg_grad_fold_params* p, miseg_stream_t stream);

/* An average of the weights over the optimisation steps, kept on the device (EMA of the weights as nnU-Net-style / MONAI bundles ship it;
 * Lightning's StochasticWeightAveraging / torch.optim.swa_utils.AveragedModel, which the reference's train.py takes through
 * Trainer.add_argparse_args; new symbols and structs: MISEG_ABI_VERSION stays 16).  `avg` is a flat fp32 buffer laid out like the gradient
 * arena (parameter i at element offset descs[i].off), walked in miseg_opt_step's geometry (the same descriptor table over ALL parameters).
 *
 * miseg_weight_average: one averaging call, in two launches.
 *   1. the tick, one thread, reads and writes `record` (the caller zeroes it once; its counters run on).  If clip_record (optional: the
 *      record miseg_grad_norm filled for this step) has skip set, the step wrote no weight and the call changes NOTHING - no counter, no
 *      element of avg.  Otherwise, with t = calls before this call (calls then counts this one) and n = n_averaged before it:
 *        apply = t >= start && (t - start) % every == 0;  first = n == 0;  n_averaged = n + apply;  and, when apply, coef = c:
 *        MISEG_AVG_MEAN              c = 1.0f / (float)(n + 1)                                   (SWA: the running mean; correctly rounded)
 *        MISEG_AVG_EMA               c = 1.0f - decay
 *        MISEG_AVG_EMA, warmup != 0  c = 1.0f - fminf(decay, (1.0f + (float)n) / (10.0f + (float)n))   (the timm / TF warm-up: without it an
 *                                    EMA stays biased towards the initial weights for about 1 / (1 - decay) steps)
 *      every operation rounded on its own in fp32.  A call that does not apply leaves coef as it was.
 *   2. the stream, one workgroup per 4096-element block, only READS the two records (no workgroup reads a word another workgroup of its
 *      launch writes: that is why the tick is a launch of its own):  skip or apply == 0: every workgroup returns before its first load;
 *      first: avg = w (avg is NOT read and may hold anything);  otherwise avg = fl(avg + fl(c * fl(w - avg))), no contraction.
 *      ALL parameters, whatever their `used` flags (as AveragedModel: a parameter without a gradient simply did not move).  The
 *      parameters are never written; the padding between the slots of avg keeps its bits.  No atomics, no LDS: equal bits every run.
 * Refused before any launch: a wrong struct_size, a null descs_dev / avg / record, ndesc / total_blocks < 1, an unknown mode, a decay that
 * is not finite or outside [0, 1) (whatever the mode), every < 1, start < 0, an avg that is not 16-byte aligned.
 *
 * miseg_weight_swap: ONE launch that exchanges param[i][e] <-> avg[off_i + e] for every descriptor (validation / export on the averaged
 * weights): a pure exchange - a second call restores every bit of both sides; padding is not touched.  params_version (optional DEVICE
 * int64, miseg_opt_step's field) is incremented once per launch: the refresh launches of the next step re-cast and re-pack every weight.
 * Refused before any launch: a wrong struct_size, a null descs_dev / avg, ndesc / total_blocks < 1, an avg that is not 16-byte aligned. */
enum { MISEG_AVG_EMA = 0, MISEG_AVG_MEAN = 1 };
typedef struct {
  int32_t apply, first;            /* of the last call that was not skipped */
  float coef;                      /* of the last applying call */
  uint32_t calls, n_averaged, reserved[3];
} miseg_weight_average_record;
typedef struct {
  uint32_t struct_size;
  int mode;                        /* MISEG_AVG_* */
  const miseg_opt_desc* descs_dev; int ndesc, total_blocks;
  float* avg;
  miseg_weight_average_record* record;
  const miseg_grad_clip_record* clip_record;      /* optional */
  float decay;
  int warmup, start, every;
} miseg_weight_average_params;
typedef struct {
  uint32_t struct_size;
  const miseg_opt_desc* descs_dev; int ndesc, total_blocks;
  float* avg;
  int64_t* params_version;         /* optional */
} miseg_weight_swap_params;
int miseg_weight_average(const miseg_weight_average_params* p, miseg_stream_t stream);
int miseg_weight_swap(const miseg_weight_swap_params* p, miseg_stream_t stream);

/* Sliding-window stitching (MONAI sliding_window_inference, mode="constant", as used at lightning_monai.py:86-93,187): every window's logits
 * stay resident (win: fp32 [nd*nh*nw][C][rd][rh][rw], window (id, ih, iw) at index (id*nh + ih)*nw + iw, origin (start_d[id], start_h[ih],
 * start_w[iw]); 700 windows x 6 x 96^3 = 14.9 GB of the 288), and ONE gather pass writes out[c][d][h][w] = (sum over the windows covering the
 * voxel, in window-index order = the order MONAI accumulates them) / count.  No atomics, no read-modify-write of the 2.3 GB accumulator.
 * starts: HOST int32 arrays (copied into the kernel arguments; at most MISEG_STITCH_MAX_WINDOWS per axis); count (optional): uint16 [D][H][W].
 * Slab form (ABI 5; volumes whose window logits do not fit in memory at once): d_count > 0 writes only the depths [d_begin, d_begin + d_count)
 * of `out` / `count` (which still address the whole [C][D][H][W] volume) from the nd RESIDENT depth layers whose starts are start_d[0..nd):
 * every depth of the slab must be covered by resident layers only, i.e. start_d[0] <= d_begin, no gaps, and the layer after the last
 * resident one starts at or behind d_begin + d_count (the caller's promise; MONAI's accumulation order is kept inside the slab).
 * Weighted form (the struct's last two fields; the leading struct_size tells the layouts apart - a caller built against the shorter struct
 * is refused, MISEG_ABI_VERSION stays 16; MONAI's mode="gaussian" or any roi_weight_map): `weight` is the dense importance map of one window.  The same
 * ONE gather pass writes out = (sum of fl(weight[voxel in window] * win), windows in index order, product and add rounded separately - no
 * FMA) / (sum of the weights in the same order), a true division: bit-identical to MONAI's `out[win] += map * pred; wsum[win] += map`
 * loop.  weight == NULL is the constant form above, unchanged. */
#define MISEG_STITCH_MAX_WINDOWS 64
typedef struct {
  uint32_t struct_size;
  const float* win; float* out; uint16_t* count;
  int C, D, H, W, rd, rh, rw, nd, nh, nw;
  const int32_t* start_d; const int32_t* start_h; const int32_t* start_w;
  int d_begin, d_count;            /* d_count == 0: the whole volume */
  const float* weight;             /* fp32 [rd][rh][rw] importance map of a window (device); NULL: every window weighs 1 (mode="constant") */
  float* wsum;                     /* optional, only with `weight`: fp32 [D][H][W], the summed weights of a voxel (the weighted `count`) */
} miseg_stitch_params;
int miseg_stitch_windows(const miseg_stitch_params* p, miseg_stream_t stream);

/* GPU-resident training augmentation (the random part of the MONAI chain at data/multi_modal.py:50-65, after the cached deterministic
 * part): for each of n <= MISEG_AUG_MAX_SAMPLES samples ONE gather pass produces a roi-sized image + label patch from the resident volume:
 *   RandCropByPosNegLabeld (crop origin, chosen by the host from cached foreground / background voxel lists), RandFlipd x3 (flip[a] on
 *   the PATCH axis a), RandRotate90d (rot_k quarter turns in the (0, 1) plane, roi_d == roi_h when rot_k is odd), RandScaleIntensityd
 *   (image * (1 + scale)), RandShiftIntensityd (image + shift) - applied in that order, intensity ops on the image only.
 * image: fp32 [C][D][H][W]; label: [D][H][W] elements of label_bytes (1, 4 or 8) bytes, copied verbatim; out_image fp32 [n][C][rd][rh][rw];
 * out_label [n][rd][rh][rw].  Sample descriptors are a HOST array (copied into the kernel arguments). */
#define MISEG_AUG_MAX_SAMPLES 16
typedef struct { int32_t origin[3]; int32_t flip[3]; int32_t rot_k; float scale, shift; } miseg_aug_sample;
typedef struct {
  uint32_t struct_size;
  const float* image; const void* label; int label_bytes;
  int C, D, H, W, rd, rh, rw, n;
  float* out_image; void* out_label;
  const miseg_aug_sample* samples_host;
} miseg_augment_params;
int miseg_augment_crop(const miseg_augment_params* p, miseg_stream_t stream);

/* miseg_augment_crop plus a free affine resample, gamma contrast and Gaussian noise (MONAI RandAffined / RandAdjustContrastd /
 * RandGaussianNoised, restated; parity unpinned - DESIGN.md section 7.11; csrc/augment.hip).  A new symbol and new structs:
 * MISEG_ABI_VERSION stays 16.  Per sample, in this order: crop -> affine resample about the crop centre -> flip 0, 1, 2 -> rot90 (the
 * gather inverts the last two exactly as miseg_augment_crop does); on the image only: -> gamma -> fma(v, fl(1 + scale), shift), one fused
 * multiply-add as in miseg_augment_crop -> noise.
 *   Coordinates, all fp32, every operation rounded on its own (no FMA): q = the pre-flip patch coordinate of the output voxel,
 *     c = (roi - 1) / 2 per axis, d = q - c (exact), r_a = (m[3a] * d_0 + m[3a+1] * d_1) + m[3a+2] * d_2,
 *     s_a = (r_a + t[a]) + (origin[a] + c_a)     - a position in the RESIDENT VOLUME, not in the crop: a rotated patch reads real
 *     neighbouring tissue; only positions outside the volume see padding_mode (BORDER clamps every index; ZEROS contributes 0 / label 0).
 *   image: trilinear, i = floor(s), f = s - i per axis, seven lerps a + f * (b - a): along W, then H, then D.
 *   label: nearest, index floor(s + 0.5) per axis (halves round up), the element copied verbatim (1, 4 or 8 bytes).
 *   A sample whose m is exactly the identity and whose t is exactly 0 takes miseg_augment_crop's integer gather: without gamma and
 *     noise its output is that call's, bit for bit.
 *   gamma > 0 (MONAI AdjustContrast, per sample over all channels of the resampled patch): lo = min, range = max - lo,
 *     v' = powf((v - lo) / (range + 1e-7f), gamma) * range + lo.  min / max: wave shuffles -> LDS -> one integer atomicMax per workgroup on
 *     an order-preserving uint32 code of the float (the minimum as the maximum of the complemented code) - order independent, so the
 *     result is bit-reproducible.  `minmax` is the caller's device scratch of MISEG_AUG_AFFINE_SCRATCH_BYTES: ZERO before its first use;
 *     every call that completes leaves it zero again (the last workgroup of a sample to arrive clears that sample's words).
 *   noise_std > 0: v += noise_mean + noise_std * z.  z is a pure function of (seed, draw, sample index i, element index e of the sample's
 *     [C][rd][rh][rw] block), nothing is stored, and sample i's noise does not depend on n:
 *       key = seed * 0x9E3779B97F4A7C15 + draw * 0xC2B2AE3D27D4EB4F + 0x165667B19E3779F9          (mod 2^64; dropout's host key)
 *       ks  = mix64(key ^ (i * 0x9E3779B97F4A7C15)),   h = mix64(ks + e * 0xD1342543DE82EF95)
 *       mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *       u1 = ((h >> 40) + 1) * 2^-24 in (0, 1]   (bits 63..40),      u2 = ((h >> 16) & 0xFFFFFF) * 2^-24 in [0, 1)   (bits 39..16)
 *       z  = sqrtf(-2 * logf(u1)) * cosf(fl(6.2831855f * u2))        (Box-Muller; the accurate logf / cosf / sqrtf / powf, never the fast forms)
 *   One launch when no sample has gamma; two otherwise (resample + reduce, then the samples with gamma are finished in place - the
 *   others were finished by the first launch, so they carry the bits of a call without gamma).  Only enqueues; can be captured.
 * Refused before any launch: a wrong struct_size, a null image / out_image / samples_host, a label without out_label, a non-finite
 * m / t / scale / shift / gamma / noise value, a crop that leaves the volume (MISEG_E_BADARG); n outside 1..MISEG_AUG_MAX_SAMPLES,
 * label_bytes not 1 / 4 / 8, an unknown padding_mode (MISEG_E_UNSUPPORTED); an odd rot_k with rd != rh, a sample with gamma and no
 * minmax (MISEG_E_BADARG). */
enum { MISEG_AUG_PAD_BORDER = 0, MISEG_AUG_PAD_ZEROS = 1 };
#define MISEG_AUG_AFFINE_SCRATCH_BYTES 256     /* uint32 [MISEG_AUG_MAX_SAMPLES][4]: ~code(min), code(max), arrivals, unused */
typedef struct {
  int32_t origin[3]; int32_t flip[3]; int32_t rot_k;
  float m[9];                      /* row-major 3x3: output offsets -> input offsets (a sampling grid) */
  float t[3];                      /* voxels */
  float scale, shift;
  float gamma;                     /* <= 0: off */
  float noise_mean, noise_std;     /* std <= 0: off */
} miseg_aug_affine_sample;
typedef struct {
  uint32_t struct_size;
  const float* image; const void* label; int label_bytes;
  int C, D, H, W, rd, rh, rw, n;
  float* out_image; void* out_label;
  const miseg_aug_affine_sample* samples_host;
  int padding_mode;                /* MISEG_AUG_PAD_* */
  uint64_t seed, draw;             /* the noise key */
  uint32_t* minmax;                /* device, MISEG_AUG_AFFINE_SCRATCH_BYTES; may be NULL when no sample has gamma */
} miseg_augment_affine_params;
int miseg_augment_affine(const miseg_augment_affine_params* p, miseg_stream_t stream);

/* Separable Gaussian filter on a batch of patches: the smoothing and sharpening end of the augmentation chain (MONAI RandGaussianSmoothd /
 * RandGaussianSharpend and nnU-Net's GaussianBlurTransform, restated; parity unpinned - DESIGN.md section 7.16; csrc/gaussian.hip).  A new
 * symbol and new structs: MISEG_ABI_VERSION stays 16.  One call is ONE filter application over n <= MISEG_AUG_MAX_SAMPLES samples of C
 * channels: src, dst fp32 [n][C][D][H][W], contiguous, distinct and not overlapping; every channel volume is filtered on its own.
 *   Taps (the host's, MONAI gaussian_1d(sigma, truncated = 4, approx = "erf"), not normalised; data/augment.py::gaussian_taps):
 *     r = int(max(4 sigma, 0.5) + 0.5),  t = 0.70710678 / |sigma|,  w[k] = max(0.5 (erf(t (k + 0.5)) - erf(t (k - 0.5))), 0) for k = -r..r,
 *     in float64, rounded once to fp32.  taps[a][k + r] is w[k] of axis a; a = 0, 1, 2 = D, H, W.  r <= MISEG_GAUSS_MAX_RADIUS.
 *     radius[a] == 0 (sigma == 0) skips axis a: the exact identity, bit for bit - no tap is read.
 *   The filter: three 1-D passes in the fixed order W, then H, then D; each reads the previous pass's fp32 result with ZEROS outside the
 *     volume (MONAI filters the cropped patch with zero padding).  Per output element
 *       acc = 0;  for k = -r..r:  acc = fl(acc + fl(w[k] * v[x + k]))
 *     in fp32, every product and every sum rounded on its own (no FMA: contraction is off for the whole file).  A tap outside the volume
 *     contributes exactly 0.  Inputs are finite; what an inf or a NaN gives is unspecified, except for the verbatim copy below.
 *   sharpen != 0: the epilogue  dst = fl(src + fl(alpha * fl(src - filtered)))  in place of  dst = filtered  (three separate roundings).
 *     Sharpening x is two calls: b1 = G(sigma1)(x), then G(sigma2) on b1 with the epilogue and alpha - out = b1 + alpha (b1 - G(sigma2)(b1)) -
 *     and no third elementwise pass.
 *   A sample whose radii are all 0 and whose sharpen is 0 is copied verbatim (NaN payloads and signed zeros included).
 *   One workgroup per MISEG_GAUSS_TILE_D x _H x _W output tile of one channel volume: tile + halo staged into LDS a few planes at a time
 *   (16-byte loads when src is 16-byte aligned and W % 4 == 0, 4-byte loads otherwise), W and H passes in LDS, the H results of all planes
 *   kept for the D pass, stores with W fastest.  The passes are unrolled for even radii: an odd radius runs as the next even one with a
 *   zero tap at either end, which adds fl(0 * v) = +-0 to an acc that is never -0 and so changes no bit (v is finite).  The descriptors
 *   travel in the kernel arguments: one launch, no allocation, no host synchronisation, no atomics; only enqueues, can be captured.
 * Refused before any launch (MISEG_E_BADARG): a wrong struct_size, a null src / dst / samples_host, src and dst that overlap, n outside
 * 1..MISEG_AUG_MAX_SAMPLES, C, D, H or W below 1, a radius outside 0..MISEG_GAUSS_MAX_RADIUS, a non-finite tap among the 2 r + 1 of an axis,
 * a non-finite alpha; MISEG_E_UNSUPPORTED: C above 65535 or more than 2^31 - 1 tiles in a channel volume. */
#define MISEG_GAUSS_MAX_RADIUS 8
#define MISEG_GAUSS_TILE_D 8
#define MISEG_GAUSS_TILE_H 16
#define MISEG_GAUSS_TILE_W 32
typedef struct {
  int32_t radius[3];                               /* D, H, W; 0: the axis is skipped */
  float taps[3][2 * MISEG_GAUSS_MAX_RADIUS + 1];   /* taps[a][0 .. 2 radius[a]] */
  float alpha;
  int32_t sharpen;                                 /* != 0: the sharpen epilogue */
} miseg_gaussian_filter_sample;
typedef struct {
  uint32_t struct_size;
  const float* src; float* dst;
  int n, C, D, H, W;
  const miseg_gaussian_filter_sample* samples_host;
} miseg_gaussian_filter_params;
int miseg_gaussian_filter3d(const miseg_gaussian_filter_params* p, miseg_stream_t stream);

/* Dropout / stochastic depth on channels-last rows (the `drop` / `dropout_path_rate` arguments of the reference's Swin stack:
 * networks/blocks/swin_transformer_block.py:90-97,205,247; MONAI Dropout / DropPath semantics): y = x * keep / (1 - p).
 *   rows_per_sample == 0: one Bernoulli(1 - p) draw per ELEMENT (nn.Dropout); > 0: one draw per SAMPLE (DropPath: rows r belong to
 *   sample r / rows_per_sample).  The mask is a pure function of (seed, stream_id, *step_dev, element / sample index) - a counter-based
 *   hash, nothing is stored: the backward pass is the same call on the gradient.  stream_id tells call sites apart within a step; step_dev
 *   (device uint64, may be NULL) tells steps apart under hipGraph replay, where seed and stream_id are baked into the graph
 *   (advance it once per step with miseg_counter_add). */
typedef struct {
  uint32_t struct_size;
  const void* x; int64_t ldx; void* y; int64_t ldy;
  int64_t rows; int C, dtype;
  int64_t rows_per_sample;
  float p;
  uint64_t seed, stream_id;
  const uint64_t* step_dev;
} miseg_dropout_params;
int miseg_dropout(const miseg_dropout_params* p, miseg_stream_t stream);
int miseg_counter_add(uint64_t* counter_dev, uint64_t value, miseg_stream_t stream);
/* *dst = *src on the device (a plain kernel: device-to-device copies recorded as memcpy nodes crashed hipStreamEndCapture on ROCm 7.2).
 * A dropout call snapshots the step counter so that its backward pass re-creates the same mask after the counter moved on. */
int miseg_counter_copy(uint64_t* dst_dev, const uint64_t* src_dev, miseg_stream_t stream);
/* (measurement and experiment entry points - miseg_debug_stamp, miseg_prof_*, miseg_flag_wait, miseg_graph_split_* - are declared in
 * include/miseg_hip_debug.h: no product path calls them) */

/* The resampling step of the cached, deterministic head of the data chain (Spacingd at data/multi_modal.py:41-44: image "bilinear", label
 * "nearest"): in [C][Di][Hi][Wi] -> out [C][Do][Ho][Wo], voxel centres aligned (src = (dst + 0.5) * in / out - 0.5), coordinates clamped to
 * the border.  mode 0: trilinear (fp32), mode 1: nearest (round half up).  elem_bytes 4: fp32 for mode 0; 1 / 4 / 8 for mode 1 (labels are
 * copied verbatim).  MONAI's own grid construction is not restated (parity unpinned). */
typedef struct {
  uint32_t struct_size;
  const void* in; void* out;
  int C, Di, Hi, Wi, Do, Ho, Wo, mode, elem_bytes;
} miseg_resample3d_params;
int miseg_resample3d(const miseg_resample3d_params* p, miseg_stream_t stream);

/* The prediction export (predict_whs.py:92-114: AsDiscrete(argmax=True), the inverse of SpatialPadd / Spacingd / Orientationd through the
 * label key in nearest mode, the class remap): out[z][y][x] = lut[argmax_c logits[c][i_D][i_H][i_W]], where the logits index along axis_a
 * (0 = D, 1 = H, 2 = W) is table_a[coordinate a] for each output axis a of X, Y, Z.  The tables fold the flips, the pad crop and the nearest
 * resampling rule into one lookup per axis (the host builds them), so the kernel is a pure gather.  Argmax takes the FIRST maximum with a
 * strict `>` (dice_count / surface_classify): a NaN in channel 0 gives class 0, a NaN in a later channel never wins.  Two launches: the argmax of
 * the box [box_*0, box_*0 + box_n*) the tables index into a uint8 class map in the workspace, then the gather + LUT through LDS tiles.  Table
 * values are clamped into the box (the host wrapper refuses values outside it).  out is C-contiguous [nz][ny][nx] (the NIfTI file's own
 * Fortran order) of out_bytes = 1, 2 or 4-byte unsigned elements (lut values truncated to that width).  C 1..64, every side 1..65535, the box
 * below 2^31 voxels.  The call only enqueues and reads nothing back: it can be captured into a graph. */
typedef struct {
  uint32_t struct_size;
  const float* logits;             /* fp32 [C][D][H][W] */
  int C, D, H, W;
  int box_d0, box_h0, box_w0, box_nd, box_nh, box_nw;
  int nx, ny, nz;
  int axis_x, axis_y, axis_z;      /* logits axis indexed by output axis X / Y / Z: a permutation of 0, 1, 2 */
  const int32_t* table_x; const int32_t* table_y; const int32_t* table_z;   /* device int32 [nx] / [ny] / [nz]: logits index along that axis */
  const int32_t* lut;              /* device int32 [C]: the value written for each class */
  void* workspace;                 /* miseg_label_export_workspace_bytes(box_nd, box_nh, box_nw) bytes, uninitialised */
  void* out; int out_bytes;
  /* a class map [D][H][W] of cls_bytes = 1 (uint8) or 4 (int32) instead of logits, e.g. miseg_keep_largest's out; exactly one of logits / cls.
   * The argmax launch is skipped and the gather reads the map in place (the workspace is not touched); a value outside [0, C) is written as 0. */
  const void* cls; int cls_bytes;
} miseg_label_export_params;
size_t miseg_label_export_workspace_bytes(int box_nd, int box_nh, int box_nw);
int miseg_label_export(const miseg_label_export_params* p, miseg_stream_t stream);

/* The soft prediction export: class scores are resampled to the file's grid BEFORE the argmax (nnU-Net's resample-the-softmax rule, MONAI's
 * Invertd(nearest_interp=False) + AsDiscreted(argmax=True)), and the resampled scores can be written beside the labels (DESIGN.md section
 * 7.15).  The reference's own way back (predict_whs.py:92-114) is miseg_label_export above; this call replaces its nearest gather by a
 * trilinear blend.  For each output axis a of X, Y, Z, three device tables of the file side's length give the two taps lo[a][i] <= hi[a][i]
 * <= lo[a][i] + 1 along logits axis axis[a] (0 = D, 1 = H, 2 = W) and the weight t[a][i] of the hi tap.  The host builds them (flips, pad
 * crop and the centre-aligned rule of miseg_resample3d folded in); the kernel computes no coordinate of its own.  lo_host / hi_host are the
 * host's copies of lo / hi: every limit below, the table contents included, is checked on them before any launch (the kernel still clamps the
 * device values into the box, so every gathered address lies inside the scores whatever the device tables hold).
 *   Arithmetic, every operation rounded to fp32 on its own (no FMA contraction), so that a numpy restatement gives the same bits:
 *   1. softmax != 0: every voxel of the box first becomes e_c = expf(x_c - max_c x), p_c = e_c / sum_c e_c, the maximum by a strict `>` scan
 *      from channel 0 and the sum taken in channel order; one pass into the workspace.
 *   2. per channel the 8 taps (lo | hi) of the three logits axes are blended along W first, then H, then D:
 *      lerp(a, b, t) = t == 0 ? a : fl(fl(a * fl(1 - t)) + fl(b * t)).  Where t == 0 the hi tap is not used, so an inf or NaN there does not
 *      leak in; with all three t zero the call is the nearest gather, bit for bit.
 *   3. the first-maximum argmax of the blended values under miseg_label_export's strict `>` rule (a NaN in channel 0 gives class 0, a NaN in
 *      a later channel never wins), through lut, truncated to out_bytes.
 * Outputs, either may be NULL but not both: out, labels [nz][ny][nx] of out_bytes = 1, 2 or 4; prob, the blended scores [C][nz][ny][nx] (the
 * Fortran order of an [X, Y, Z, C] NIfTI) of prob_bytes = 4 (fp32) or 1: q = min(255, (int)floorf(p * 255.f + 0.5f)), a NaN gives 0.  The
 * 1-byte form needs softmax != 0 or unit_range != 0 (the caller declares the scores to lie in [0, 1]).
 *   One workgroup blends a 64 (X) x 64 output tile channel after channel from an LDS image of the source voxels under the tile (read with the
 * lanes along logits W whichever output axis maps to it, shared by the neighbouring outputs of an upsampling); a tile whose source span does
 * not fit the image reads its taps from memory.  Stores are whole lines along X.  C 1..64, every side 1..65535, the box below 2^31 voxels.
 * The call only enqueues, allocates nothing and reads nothing back: it can be captured into a graph. */
typedef struct {
  uint32_t struct_size;
  const float* scores;             /* fp32 [C][D][H][W] */
  int C, D, H, W;
  int box_d0, box_h0, box_w0, box_nd, box_nh, box_nw;   /* the box of the scores the tables index */
  int nx, ny, nz;
  int axis_x, axis_y, axis_z;      /* logits axis indexed by output axis X / Y / Z: a permutation of 0, 1, 2 */
  const int32_t* lo[3]; const int32_t* hi[3]; const float* t[3];   /* device [nx] / [ny] / [nz], per output axis X, Y, Z */
  const int32_t* lo_host[3]; const int32_t* hi_host[3];            /* host copies of lo / hi, read during the call only */
  const int32_t* lut;              /* device int32 [C]; may be NULL when out is */
  int softmax, unit_range;
  void* workspace;                 /* miseg_soft_export_workspace_bytes(C, box_nd, box_nh, box_nw, softmax) bytes, uninitialised; NULL when 0 */
  void* out; int out_bytes;
  void* prob; int prob_bytes;
} miseg_soft_export_params;
size_t miseg_soft_export_workspace_bytes(int C, int box_nd, int box_nh, int box_nw, int softmax);
int miseg_soft_export(const miseg_soft_export_params* p, miseg_stream_t stream);

/* Keep-largest-connected-component post-processing (MONAI 1.1.0 transforms/post/array.py::KeepLargestConnectedComponent with
 * num_components = 1, restated; parity unpinned - DESIGN.md section 7.7).  The class map is `cls` (cls_bytes 1: uint8, 4: int32), or the
 * first-maximum argmax of fp32 `logits` under miseg_label_export's strict `>` rule; exactly one of the two.  `applied`: bit c set = class c is
 * filtered.  independent != 0: of every applied class the largest component of {cls == c} stays and its other voxels become 0.  independent
 * == 0: the components are those of {cls in applied} (adjacent applied voxels of different classes are connected), the largest stays with
 * its classes, every other applied voxel becomes 0.  connectivity 1 / 2 / 3: the 6- / 18- / 26-neighbourhood; neighbours never wrap around
 * a row, slice or sample end.  Among components of equal largest size the one holding the smallest linear voxel index stays.  Unapplied classes
 * are never changed and connect nothing; a map value outside [0, C) belongs to no class and is copied through (truncated to out_bytes).
 *   One union-find labelling serves all classes (csrc/components.hip): classify, tile-local union-find in LDS, unions across tile borders with
 * atomicMin on an int32 parent volume, a flatten launch, one 64-bit atomicMax per root, apply.  Parents only ever decrease and every root is
 * its component's smallest linear index, so the result does not depend on scheduling; integer atomics only.  The call only enqueues and reads
 * nothing back: it can be captured into a graph.  C 1..64, every side 1..65535, each sample below 2^31 voxels, B >= 1.
 *   stats (optional): int64 [B][C][3] = voxels of class c before, voxels of class c kept, roots whose voxel has class c (components of an
 * applied class; in joint mode their sum over c is the component count; 0 for an unapplied class). */
typedef struct {
  uint32_t struct_size;
  const float* logits;             /* fp32 [B][C][D][H][W], or NULL */
  const void* cls; int cls_bytes;  /* [B][D][H][W] uint8 / int32, or NULL */
  int B, C, D, H, W;
  uint64_t applied;
  int independent, connectivity;
  void* workspace;                 /* miseg_keep_largest_workspace_bytes(B, D, H, W) bytes, uninitialised */
  void* out; int out_bytes;        /* [B][D][H][W] of 1 (uint8) or 4 (int32) byte elements; may be `cls` itself when cls_bytes == out_bytes */
  int64_t* stats;                  /* [B][C][3] or NULL */
} miseg_keep_largest_params;
size_t miseg_keep_largest_workspace_bytes(int B, int D, int H, int W);
int miseg_keep_largest(const miseg_keep_largest_params* p, miseg_stream_t stream);

/* Fill-holes post-processing (MONAI 1.1.0 transforms/utils.py::fill_holes / transforms/post/array.py::FillHoles, restated; parity unpinned -
 * DESIGN.md section 7.8).  The class map is `cls` (cls_bytes 1: uint8, 4: int32), or the first-maximum argmax of fp32 `logits` as in
 * miseg_keep_largest; exactly one of the two.  `applied`: bit L set = label L is filled; bit 0 (the background) is ignored.  The applied labels
 * are processed in ascending order, each on the map as the previous one left it.  Pass L: a voxel is passable iff its value is not L (values
 * outside [0, C) included); passable voxels are connected through the 6- / 18- / 26-neighbourhood of connectivity 1 / 2 / 3, never across a row,
 * slice or sample end; a component holding a voxel on one of the six faces of the volume is open; every voxel of every other component becomes
 * L, whatever it held.  A volume with a side of 1 is all face: nothing is filled.  Untouched voxels are copied through (a value outside [0, C)
 * truncated to out_bytes).
 *   csrc/components.hip: per label the keep-largest labelling (tile-local union-find in LDS, atomicMin unions across tile borders, flatten) on
 * the passable voxels of the label's bounding box grown by one voxel, a flag on the root of every passable voxel on that box's faces, and a
 * rewrite of the unflagged passable voxels; a uint8 working map is updated in place between the passes.  Integer atomics only, the result does
 * not depend on scheduling, an absent label's launches return on a device-side empty box; the call only enqueues and reads nothing back: it
 * can be captured into a graph.  C 1..64, every side 1..65535, each sample below 2^31 voxels, B >= 1.
 *   stats (optional): int64 [B][C] = voxels whose value pass L changed to L (0 for an unapplied label). */
typedef struct {
  uint32_t struct_size;
  const float* logits;             /* fp32 [B][C][D][H][W], or NULL */
  const void* cls; int cls_bytes;  /* [B][D][H][W] uint8 / int32, or NULL */
  int B, C, D, H, W;
  uint64_t applied;
  int connectivity;
  void* workspace;                 /* miseg_fill_holes_workspace_bytes(B, D, H, W) bytes, uninitialised */
  void* out; int out_bytes;        /* [B][D][H][W] of 1 (uint8) or 4 (int32) byte elements; may be `cls` itself when cls_bytes == out_bytes */
  int64_t* stats;                  /* [B][C] or NULL */
} miseg_fill_holes_params;
size_t miseg_fill_holes_workspace_bytes(int B, int D, int H, int W);
int miseg_fill_holes(const miseg_fill_holes_params* p, miseg_stream_t stream);

/* Flip test-time augmentation / model ensembling (MONAI 1.1.0 transforms/post/array.py::MeanEnsemble / VoteEnsemble and nnU-Net's mirror
 * TTA, restated; parity unpinned - DESIGN.md section 7.10): folds ONE member's stitched logits into a running accumulator.
 *   src: fp32 [B][C][D][H][W], the member's logits in the frame of the flipped volume; acc: fp32, same shape, in the volume's own frame.
 *   flip: bit 0 / 1 / 2 = the member was predicted on the volume mirrored along D / H / W: the source voxel of acc[b][c][d][h][w] is
 *     src[b][c][bit 0 ? D-1-d : d][bit 1 ? H-1-h : h][bit 2 ? W-1-w : w].
 *   kind: the term t a voxel contributes - MEAN_LOGITS: t_c = x_c.  MEAN_PROB: t = softmax_c(x): the maximum subtracted (fmaxf from -inf),
 *     expf, summed in channel order, times 1 / sum.  VOTE: t_c = 1 for the first-maximum argmax (a strict `>` scan from channel 0: a NaN in
 *     channel 0 gives class 0, a NaN in a later channel never wins), 0 elsewhere; weight is ignored (every vote weighs 1).
 *   acc' = fl(fl(acc + fl(weight[c] * t_c)) * out_scale[c]), fp32, every operation rounded on its own (no FMA); first != 0: "acc +" is absent
 *     and acc is not read (it may be uninitialised memory); scaled == 0: "* out_scale[c]" is absent (the host sets it on the last member).
 * One streaming pass: src is read once (C <= 16; more channels are read once per pass over them), acc is read unless first and written once.
 * Refused before any launch (MISEG_E_BADARG): a null pointer, C outside 1..64, a dimension below 1, an unknown kind, flip outside 0..7, a
 * non-finite or negative weight[c < C] (or out_scale[c < C] when scaled), src and acc ranges that overlap; MISEG_E_UNSUPPORTED: B * D * H *
 * ceil(W / 4) of 2^32 or more (every element offset is 64-bit: a tensor may exceed 2^31 bytes).  The call only enqueues and reads nothing
 * back: it can be captured into a graph. */
enum { MISEG_ENSEMBLE_MEAN_LOGITS = 0, MISEG_ENSEMBLE_MEAN_PROB = 1, MISEG_ENSEMBLE_VOTE = 2 };
typedef struct {
  uint32_t struct_size;
  const float* src; float* acc;
  int B, C, D, H, W;
  int flip, kind, first, scaled;
  float weight[64];                /* per class; a scalar member weight is the same value repeated */
  float out_scale[64];             /* per class, read when scaled != 0 */
} miseg_ensemble_params;
int miseg_ensemble_accumulate(const miseg_ensemble_params* p, miseg_stream_t stream);

/* sizeof() of a params struct as this library was compiled ("miseg_gemm_params", ...), 0 for an unknown name: bindings compare it with
 * their own mirror at load time (together with miseg_abi_version) so that header and binding cannot drift silently. */
size_t miseg_abi_struct_size(const char* struct_name);
/* sha256 (hex) over the sources this library was compiled from (csrc/build.py); a binding that finds the sources beside the library
 * compares and refuses a stale build */
const char* miseg_source_digest(void);
/* MISEG_OK when HIP device `device` runs the code objects embedded in this library (gcnArchName starts with miseg_device_arch) */
int miseg_device_check(int device);

#ifdef __cplusplus
}
#endif
#endif
