/* lemevit_hip.h -- C ABI of liblemevit_hip.so, the MI355X (gfx950) kernels behind the LeMeViT
 * backbone hot path.
 *
 * The reference (ViTAE-Transformer/LeMeViT) has no FFI: its hot path is PyTorch calls inside
 * models/lemevit.py, dispatched through the attention-backend seam at models/lemevit.py:32-52.
 * Each entry point below replaces the torch calls of the cited reference lines; the Python
 * binding a maintainer would add is shown in INTEGRATION.md (ctypes, as lemevit_amd/_lib.py).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (PyTorch's caching allocator) and must stay alive until `stream` reaches the kernel;
 *   - tensors are contiguous row-major, token-major [B, L, C]; 16-byte aligned;
 *   - dtype: LMV_F32 = 0, LMV_BF16 = 1 (activations and matrix weights); vectors (bias, LayerNorm
 *     affine, statistics, DropPath scales) and gradient accumulators are always fp32;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, never synchronised;
 *   - return 0 on success, else LMV_ERR_* (message via lmv_last_error()); nothing throws;
 *   - re-entrant: entry points may be called from several host threads and on any streams; the device is whatever the caller made current.
 *     Per-call state lives in the caller's buffers.  What the library keeps per PROCESS, and is therefore not "stateless", is listed here:
 *       * the tuning switches (lmv_config_set: process-wide, unsynchronised -- set them between launches);
 *       * one sticky error word per device (pinned host memory) that the persistent stage kernels raise (lmv_stage_error_count);
 *       * the measurement aids lmv_debug_launch_timing / lmv_stem_debug_timing (single host thread, never in production);
 *       * per-device caches of occupancy queries and of the hipFuncSetAttribute calls (write-once, atomics).
 */
#ifndef LEMEVIT_HIP_H
#define LEMEVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMV_ABI_VERSION 14

enum { LMV_F32 = 0, LMV_BF16 = 1, LMV_U8 = 2 /* images handed to lmv_mix_images only */ };
enum {
  LMV_OK = 0,
  LMV_ERR_SHAPE = -1,      /* bad shape / alignment */
  LMV_ERR_DTYPE = -2,      /* unsupported dtype / arch */
  LMV_ERR_WORKSPACE = -3,  /* workspace too small */
  LMV_ERR_LAUNCH = -4      /* HIP launch error (hipGetLastError) */
};

int lmv_abi_version(void);
const char* lmv_last_error(void);
/* Run-time switches of alternative code paths (the GPU parity tests run both sides): these two change / read one.  Keys: "gemm_rs", "gemm_wn",
 * "mlp_rw96", "mlp_tm", "mlp_dx_fused", "stage_ticket_skew" (test switch) (lemevit_amd/csrc/common.h: LmvConfig); an unknown key is LMV_ERR_SHAPE.  None is read from the
 * environment.  Process-wide, not synchronised: set them between launches. */
int lmv_config_set(const char* key, int value);
int lmv_config_get(const char* key, int* value);

/* ------------------------------------------------------------------------------------------
 * Linear layers (nn.Linear calls of models/lemevit.py:200,205,289,291,299,302,478-479,486 and
 * the MLP :526-530).  One launch runs up to two independent "problems" that share N and K (the
 * image-token matrix and the meta-token matrix of a block share LN/MLP -- and in S-blocks
 * attention -- weights, :560-564,:632-635).
 *
 *   fwd : out[r, n] = res[r, n] + row_scale[r / rows_per_sample] * act(sum_k a[r,k] w[n,k] + bias[n])
 *         (act == LMV_ACT_GELU_GRAD: out[r, n] = row_scale * (sum_k a[r,k] w[n,k] + bias[n]) * gelu'(aux[r, n]), no residual: a dX through
 *          a TRANSPOSED weight copy;
 *          act == LMV_ACT_GELU_BWD: out[r, n] = aux[r, n] * gelu'(sum_k a[r,k] w[n,k] + bias[n]) -- the GELU backward of a forward that kept no pre-activation
 *          (lmv_linear_fwd(.., LMV_ACT_GELU) with out_pre = NULL): z is recomputed from the saved rows, aux is the incoming gradient.  A kernel of its own
 *          (csrc/convbn.hip): N <= 128, K a multiple of 32, no residual / row_scale / out_pre)
 *   dx  : out[r, k] = (sum_n a[r,n] w[n,k]) (* gelu'(aux[r,k]) if act == LMV_ACT_GELU_GRAD)
 *   dw  : dw[n, k] += sum_r dy[r,n] x[r,k] ;  db[n] += sum_r dy[r,n]      (fp32; split-K partial slabs in
 *         `workspace` + a reduce kernel: deterministic, no atomics)
 * ------------------------------------------------------------------------------------------ */
enum { LMV_ACT_NONE = 0, LMV_ACT_GELU = 1, LMV_ACT_GELU_GRAD = 2, LMV_ACT_GELU_BWD = 3 };

typedef struct {
  const void* a;           /* fwd: x [rows, K]; dx: dy [rows, N]; dw: dy [rows, N]            */
  const void* w;           /* fwd/dx: weight [N, K];               dw: x  [rows, K]            */
  const float* bias;       /* fwd: [N] or NULL                                                  */
  const void* res;         /* fwd: residual [rows, N] or NULL (dx: [rows, K] added to out)      */
  const float* row_scale;  /* per-sample DropPath scale [rows / rows_per_sample] or NULL        */
  const void* aux;         /* dx with GELU_GRAD: pre-activation u [rows, K]; fwd with GELU_BWD: incoming gradient [rows, N] */
  void* out;               /* fwd: [rows, N]; dx: [rows, K]; dw: fp32 dW [N, K] (accumulated)   */
  void* out_pre;           /* fwd: optional copy of the pre-activation (training) or NULL       */
  float* bias_grad;        /* dw: fp32 db [N] (accumulated) or NULL                             */
  int64_t rows;
  int32_t rows_per_sample; /* tokens per image for row_scale (ignored when row_scale == NULL)   */
  int32_t _pad;
} lmv_linear_problem;

int lmv_linear_fwd(const lmv_linear_problem* p, int nproblems, int N, int K, int act, int dtype, void* stream);
int lmv_linear_dx(const lmv_linear_problem* p, int nproblems, int N, int K, int act, int dtype, void* stream);
size_t lmv_linear_dw_workspace_bytes(const lmv_linear_problem* p, int nproblems, int N, int K, int dtype);
int lmv_linear_dw(const lmv_linear_problem* p, int nproblems, int N, int K, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* Deferred form: only the split-K GEMM is launched; the partial slabs stay in `workspace` (which must then stay untouched until
 * they are summed) and up to 2 reduce segments describing them are written to segs[0 .. *nsegs).  lmv_reduce_batch sums the slabs
 * of any number of segments -- the weight gradients of a whole block -- into their out_w / out_b (accumulating, fixed summation
 * order: bit-identical to lmv_linear_dw) in ONE launch per LMV_REDUCE_MAX_SEGS segments. */
#define LMV_REDUCE_MAX_SEGS 12
#define LMV_REDUCE_SLABS 0   /* split-K slabs of a weight-gradient GEMM (summation tree of lmv_linear_dw)                              */
#define LMV_REDUCE_ROWS  1   /* per-workgroup partial rows of a column reduction: LayerNorm dgamma | dbeta (lmv_layernorm_bwd_partial,  */
                             /* mode 0) or the depth-wise convolution's [10][C] tap sums (lmv_dwconv3x3_bwd_weight_partial, mode 1:     */
                             /* partial column tap * C + c -> out_w[c * 9 + tap], tap 9 -> out_b[c]); summation tree of the stand-alone */
                             /* reduce of those ops, so the merged launch is bit-identical to them                                       */
typedef struct {
  const float* ws;        /* first slab of the segment: [nslabs][slab_stride] fp32, a slab = [nw weights | nb bias sums]   */
  float* out_w;           /* fp32 [nw], accumulated                                                                          */
  float* out_b;           /* fp32 [nb], accumulated; NULL = no bias gradient                                                  */
  int64_t slab_stride;    /* floats between consecutive slabs (LMV_REDUCE_ROWS: row width = nw + nb, or 10 * nw in mode 1)    */
  int64_t nw;
  int32_t nslabs, nb;
  int32_t kind, mode;     /* LMV_REDUCE_SLABS (mode ignored) or LMV_REDUCE_ROWS with the output mapping `mode`                */
} lmv_reduce_seg;
int lmv_linear_dw_partial(const lmv_linear_problem* p, int nproblems, int N, int K, void* workspace, size_t workspace_bytes, int dtype, void* stream,
                          lmv_reduce_seg* segs, int* nsegs);
int lmv_reduce_batch(const lmv_reduce_seg* segs, int nsegs, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused block entry points (`ln_linear`, `mlp_fused`, `attn_out_proj_residual`).
 *
 * LayerNorm folded into the Linear that consumes it (norm1 -> qkv / q / kv, models/lemevit.py:560,599,632,634; norm2 -> mlp.0,
 * :563-564,:633,635).  With x_hat = (x - mean) rstd:
 *     LN(x) W^T + b  =  rstd (x W'^T - mean colsum(W'))  +  b',      W' = gamma . W  (rounded to `dtype`),  b' = b + W beta
 * so the GEMM reads the RAW residual-stream rows and the normalised copy never exists in HBM.
 *   lmv_ln_fold       : (W fp32 [N, K], bias [N] or NULL, gamma [K], beta [K]) -> wf [N, K] in `dtype`, colsum [N], bf [N] (fp32);
 *                       colsum is taken over the ROUNDED wf, so the mean term cancels exactly.  Run once per weight version.
 *   lmv_ln_linear_fwd : out[r, n] = act(LN(x[r, :]) . W[n, :] + b[n]) from the folded operands; the row statistics are accumulated
 *                       from the MFMA operand fragments inside the k-loop (one-pass, fp32).  p[i].a = x, p[i].w = wf, p[i].bias = bf,
 *                       p[i].aux = colsum (fp32 [N]); res / row_scale / out_pre as in lmv_linear_fwd.
 *   lmv_mlp_fused_fwd : out = x + row_scale * fc2(GELU(fc1(LN(x))))  -- the whole MLP half of a LeMeBlock in ONE kernel: a workgroup
 *                       keeps 128 token rows in LDS, streams the weights, and the 4C-wide hidden activations never leave the chip
 *                       (C in + C out per token instead of 17 C).  bf16, C in {64, 96, 128, 192, 256, 320, 384}, hidden % 128 == 0
 *                       (lmv_mlp_fused_supported); inference form: nothing is saved for a backward pass.
 *   lmv_attn_out_proj_residual : out = res + row_scale * (attn_out W^T + b) -- the output projection of an attention module with the
 *                       block's residual add and DropPath folded into the GEMM epilogue (:205 + :562 / :601 / :632,634).
 * ------------------------------------------------------------------------------------------ */
int lmv_ln_fold(const float* w, const float* bias, const float* gamma, const float* beta, int N, int K, void* wf, float* colsum, float* bf,
                int dtype, void* stream);
int lmv_ln_linear_fwd(const lmv_linear_problem* p, int nproblems, int N, int K, float eps, int act, int dtype, void* stream);
typedef struct {
  const void* x;            /* [rows, C]: input of the MLP half (= its residual)                 */
  void* out;                /* [rows, C]                                                          */
  const float* row_scale;   /* per-sample DropPath scale [rows / rows_per_sample] or NULL        */
  int64_t rows;
  int32_t rows_per_sample;
  int32_t _pad;
} lmv_mlp_problem;
typedef struct {
  const void* w1f; const float* colsum1; const float* b1f;   /* lmv_ln_fold(mlp.0, norm2): [hidden, C], [hidden], [hidden] */
  const void* w2; const float* b2;                           /* mlp.3: [C, hidden] in `dtype`, [C] fp32                    */
} lmv_mlp_weights;
int lmv_mlp_fused_supported(int C, int hidden, int dtype);
/* Test hook: y[i] = the activation lmv_mlp_fused_fwd applies to the hidden values (a degree-7 minimax fit of GELU in packed fp32,
 * |y - GELU_erf(x)| <= 1.9e-4 absolute, exact 0 / identity beyond |x| >= 4), for x, y fp32 [n] on the device. */
int lmv_gelu_poly_eval(const float* x, float* y, int64_t n, void* stream);
int lmv_mlp_fused_fwd(const lmv_mlp_problem* p, int nproblems, const lmv_mlp_weights* w, int C, int hidden, float eps, int dtype, void* stream);
/* The data gradient of the same MLP half in ONE launch (csrc/fused.hip, a variant of the forward kernel; bf16, the shapes of lmv_mlp_fused_supported):
 *     dn2 = ((g fc2) * GELU'(u)) fc1      g [rows, C]: gradient of the MLP output, already DropPath-scaled; u [rows, hidden]: the saved fc1
 *     pre-activations; fc2_wt = mlp.3.weight TRANSPOSED [hidden, C], fc1_wt = mlp.0.weight TRANSPOSED [C, hidden] (lmv_transpose_batch); dn2 [rows, C]:
 *     gradient of norm2's output (no bias, no residual).  GELU' is the one LMV_ACT_GELU_GRAD evaluates, and du = (g fc2) * GELU'(u) is rounded to bf16
 *     where lmv_linear_fwd(.., LMV_ACT_GELU_GRAD) rounds it -- but it stays on the chip: the two-launch form writes and re-reads rows x hidden x 2 B.
 * Up to two problems per launch (image and meta rows).  For a backward pass that wants no weight gradient (nothing else reads du). */
typedef struct { const void* g; const void* u; void* dn2; int64_t rows; } lmv_mlp_dx_problem;
int lmv_mlp_dx_fused_supported(int C, int hidden, int dtype);
int lmv_mlp_dx_fused(const lmv_mlp_dx_problem* p, int nproblems, const void* fc2_wt, const void* fc1_wt, int C, int hidden, int dtype, void* stream);
int lmv_attn_out_proj_residual(const lmv_linear_problem* p, int nproblems, int C, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (nn.LayerNorm, models/lemevit.py:513,525 eps 1e-6; :731-743,774
 * eps 1e-5).  One launch normalises up to TWO row segments with the same (gamma, beta): the image-token
 * and the meta-token matrix of a block share norm1 / norm2 (:560-564,:632-635).
 *   fwd: y = LN(x); stats = [rows, 2] fp32 (mean, rstd), written when non-NULL.
 *   bwd: dx = dres + LN'(dy)   (dres may be NULL);  dgamma/dbeta are ACCUMULATED (fp32; per-workgroup partials
 *        in `workspace` + a reduce kernel, no atomics).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* x;      /* [rows, C] input of the forward pass                               */
  void* y;            /* fwd: output [rows, C]                                              */
  float* stats;       /* [rows, 2] (mean, rstd): written by fwd (may be NULL), read by bwd  */
  const void* dy;     /* bwd: gradient of y                                                 */
  const void* dres;   /* bwd: optional residual-path gradient added to dx (or NULL)         */
  void* dx;           /* bwd: output [rows, C]                                              */
  int64_t rows;
  /* bwd, optional (all three or none): a second output dx_scaled[r, :] = dx[r, :] * dx_scale[r / rows_per_sample] -- the
   * DropPath-scaled gradient the NEXT backward stage consumes (saves a separate lmv_row_scale pass over dx) */
  const float* dx_scale;
  void* dx_scaled;
  int64_t rows_per_sample;
} lmv_ln_segment;

int lmv_layernorm_fwd(const lmv_ln_segment* seg, int nseg, const float* gamma, const float* beta, int C, float eps,
                      int dtype, void* stream);
/* y = GELU(LayerNorm(x)) in one pass and its backward (dy is multiplied by GELU'(LayerNorm(x)), recomputed from x, gamma, beta):
 * the Linear -> LayerNorm -> GELU -> Linear -> LayerNorm meta-token MLP of every stage (models/lemevit.py:731-743). */
int lmv_layernorm_gelu_fwd(const lmv_ln_segment* seg, int nseg, const float* gamma, const float* beta, int C, float eps,
                           int dtype, void* stream);
int lmv_layernorm_gelu_bwd(const lmv_ln_segment* seg, int nseg, const float* gamma, const float* beta, float* dgamma, float* dbeta, int C,
                           void* workspace, size_t workspace_bytes, int dtype, void* stream);      /* dgamma == dbeta == workspace == NULL: dx only */
size_t lmv_layernorm_bwd_workspace_bytes(int64_t total_rows, int C, int dtype);
int lmv_layernorm_bwd(const lmv_ln_segment* seg, int nseg, const float* gamma, float* dgamma, float* dbeta, int C,
                      void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* The same in two calls: _partial writes dx and leaves `*partial_rows` per-workgroup rows of (dgamma | dbeta) partial sums in
 * `workspace`; _reduce accumulates them into dgamma / dbeta -- on any stream that is ordered behind _partial (the block scheduler
 * keeps it off the critical path).  Results are bit-identical to lmv_layernorm_bwd.
 * dx-only mode: workspace == NULL and partial_rows == NULL -- the same launch writes dx (and dx_scaled) and no partial rows (frozen affine). */
int lmv_layernorm_bwd_partial(const lmv_ln_segment* seg, int nseg, const float* gamma, int C, void* workspace, size_t workspace_bytes,
                              int* partial_rows, int dtype, void* stream);
int lmv_layernorm_bwd_reduce(const void* workspace, int partial_rows, int C, float* dgamma, float* dbeta, void* stream);
/* The dX of a Linear fused with the LayerNorm backward of the Linear's INPUT (models/lemevit.py:560,563: norm -> Linear; csrc/wngemm.hip,
 * bf16, C = 384, N % 64 == 0: lmv_linear_dx_ln_bwd_supported):
 *     dy = dY wt^T   (wt = the Linear's weight TRANSPOSED, [C, N]: lmv_transpose_batch),     dx = dres + LN'(dy),     dx_scaled = dx * dx_scale[sample]
 * p[i].a = dY [rows, N], p[i].w = wt; seg[i] as for lmv_layernorm_bwd_partial (x, stats, dres, dx, rows, dx_scale / dx_scaled /
 * rows_per_sample; seg[i].dy is ignored -- dy never reaches memory, the LayerNorm sees it in fp32).  `*partial_rows` rows of (dgamma | dbeta)
 * partial sums are left in `workspace` for lmv_layernorm_bwd_reduce / an LMV_REDUCE_ROWS segment of lmv_reduce_batch.
 * dx-only mode: workspace == NULL and partial_rows == NULL -- dx (and dx_scaled) only, no partial rows. */
/* The forward mirror: a Linear with the residual epilogue followed by the LayerNorm of its output (proj + norm2, models/lemevit.py:562-563,
 * 632-635) in one launch:  out = res + row_scale (a W^T + bias);  seg[i].y = LN(out) (of the ROUNDED out, as a separate launch would read
 * it), seg[i].stats = (mean, rstd) when non-NULL.  bf16, N = 384, K % 64 == 0 (lmv_linear_res_ln_fwd_supported). */
/* LayerNorm -> Linear with the EXACT LayerNorm in front (no folding), for the C = 96 layers (norm1 -> qkv1 / qkv2 / kv / q,
 * models/lemevit.py:560,599; csrc/rswgemm.hip: the whole weight matrix resident in LDS, every wave streams 32-row panels through registers):
 *     seg[i].y = LN(p[i].a)  (written when non-NULL: training keeps it for the weight gradient),  seg[i].stats = (mean, rstd) (when non-NULL),
 *     p[i].out = seg[i].y W^T + bias.      gamma == NULL: plain Linear.   bf16, K = 96, N % 32 == 0, N <= 384 (lmv_ln_linear_exact_fwd_supported). */
int lmv_ln_linear_exact_fwd_supported(int N, int K, int dtype);
int lmv_ln_linear_exact_fwd(const lmv_linear_problem* p, const lmv_ln_segment* seg, int nproblems, int N, int K, const float* gamma, const float* beta,
                            float eps, int dtype, void* stream);
int lmv_linear_res_ln_fwd_supported(int N, int K, int dtype);
int lmv_linear_res_ln_fwd(const lmv_linear_problem* p, const lmv_ln_segment* seg, int nproblems, int N, int K, const float* gamma, const float* beta,
                          float eps, int dtype, void* stream);
int lmv_linear_dx_ln_bwd_supported(int C, int N, int dtype);
size_t lmv_linear_dx_ln_bwd_workspace_bytes(int64_t total_rows, int C);
int lmv_linear_dx_ln_bwd(const lmv_linear_problem* p, const lmv_ln_segment* seg, int nproblems, int C, int N, const float* gamma,
                         void* workspace, size_t workspace_bytes, int* partial_rows, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode BatchNorm2d (+ exact GELU) over a channels-last feature map viewed as [rows = B*H*W][C]: the BatchNorm2d
 * (-> GELU) of the stem and of every stage transition (models/lemevit.py:698-704, 714-717) and the final `norm` (:773, 822).
 * Replaces torch.nn.BatchNorm2d.forward in training mode (+ the nn.GELU after the first stem BatchNorm) and their autograd.
 *   fwd: batch mean / biased variance per channel (fp32 partial sums, fp64 combine); y = (x - mean) * rstd * gamma + beta
 *        (act = LMV_ACT_GELU: GELU of that); stats[0:C] = mean, stats[C:2C] = rstd (saved for the backward);
 *        running_mean / running_var (may be NULL) updated with `momentum` and the UNBIASED variance, as torch.
 *   bwd: dgamma / dbeta are WRITTEN (not accumulated); dx = gamma * rstd * (dy' - mean(dy') - xhat * mean(dy' * xhat)),
 *        dy' = dy * GELU'(xhat * gamma + beta) when act = LMV_ACT_GELU.
 * C % 8 == 0 (bf16) / C % 4 == 0 (fp32), C <= 2048 / 1024; workspace: lmv_batchnorm_workspace_bytes(C).
 * ------------------------------------------------------------------------------------------ */
size_t lmv_batchnorm_workspace_bytes(int C);
int lmv_batchnorm_train_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                            float eps, int act, void* y, float* stats, int64_t rows, int C, void* workspace, size_t workspace_bytes,
                            int dtype, void* stream);
int lmv_batchnorm_train_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats, int act, void* dx,
                            float* dgamma, float* dbeta, int64_t rows, int C, void* workspace, size_t workspace_bytes, int dtype,
                            void* stream);
/* The apply step of lmv_batchnorm_train_fwd alone, from statistics it returned: y = (x - stats[0:C]) * stats[C:2C] * gamma + beta
 * (-> GELU), with the forward's launch geometry, so y is bit-equal to the y of the lmv_batchnorm_train_fwd call that produced `stats`.
 * Running statistics are not touched and no workspace is needed.  A checkpointed stem / transition recomputes its BatchNorm with it in
 * the backward pass (the running statistics were updated once, in the forward pass). */
int lmv_batchnorm_apply_fwd(const void* x, const float* gamma, const float* beta, const float* stats, int act, void* y, int64_t rows, int C,
                            int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Conditional position embedding: y = x + dwconv3x3(x) + bias, NHWC (models/lemevit.py:510,546).
 * weight is the reference's [C, 1, 3, 3] fp32 tensor.
 *   bwd_data  : dx = dy + dwconv3x3^T(dy)
 *   bwd_weight: dw[C,1,3,3] += ..., db[C] += ...     (fp32; per-workgroup partials in `workspace` + reduce)
 * ------------------------------------------------------------------------------------------ */
int lmv_dwconv3x3_residual_fwd(const void* x, const float* weight, const float* bias, void* y,
                               int B, int H, int W, int C, int dtype, void* stream);
int lmv_dwconv3x3_residual_bwd_data(const void* dy, const float* weight, void* dx,
                                    int B, int H, int W, int C, int dtype, void* stream);
size_t lmv_dwconv3x3_bwd_weight_workspace_bytes(int B, int H, int W, int C, int dtype);
int lmv_dwconv3x3_bwd_weight(const void* dy, const void* x, float* dweight, float* dbias,
                             int B, int H, int W, int C, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* Deferred form: only the tap-sum kernel runs; `*partial_rows` rows of [10][C] partial sums stay in `workspace` and are accumulated into
 * dweight / dbias later by lmv_reduce_batch (segment kind LMV_REDUCE_ROWS, mode 1, nw = C, nb = C, slab_stride = 10 C, nslabs = rows). */
int lmv_dwconv3x3_bwd_weight_partial(const void* dy, const void* x, int B, int H, int W, int C, void* workspace, size_t workspace_bytes,
                                     int* partial_rows, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention cores, head dim 32 (all registered variants, models/lemevit.py:851,881,911).
 * q/k/v/o are addressed as  ptr + b * batch_stride + l * row_stride + head * 32  (strides in
 * ELEMENTS), so the packed projections of the reference (qkv [B,L,3C] :200-202, kv [B,N,2C]
 * :479-482) are consumed in place -- no 'x B h N d' re-pack (:201,290,292,481).
 *   o[b,l,h,:] = softmax_j(scale * q[b,l,h,:] . k[b,j,h,:]) v[b,j,h,:]       (:54-63)
 *   lse[b,h,l] = log sum_j exp(scale * q.k)   (fp32, kept for the backward pass)
 * Lq <= 16 (meta-token queries over image-token keys, :300,:484) takes the split-key path and
 * needs `workspace` (lmv_attn_workspace_bytes).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* q; const void* k; const void* v;  /* inputs                                       */
  void* o;                                      /* fwd: output; bwd: the saved forward output    */
  float* lse;                                   /* [B, H, Lq] fp32                               */
  const void* d_o;                              /* bwd: grad of o (strides of o)                 */
  void* dq; void* dk; void* dv;                 /* bwd: grads (strides of q / k / v)             */
  int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;
  int32_t B, H, Lq, Lk;
  float scale;
  int32_t _pad;
} lmv_attn_desc;

size_t lmv_attn_workspace_bytes(int B, int H, int Lq, int Lk, int backward);
int lmv_attn_fwd(const lmv_attn_desc* d, void* workspace, size_t workspace_bytes, int dtype, void* stream);
int lmv_attn_bwd(const lmv_attn_desc* d, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* Two independent problems d[0], d[1] with the same B and H -- the image-token and the meta-token self-attention of an "S" block
 * (models/lemevit.py:632,634) -- in ONE launch where the shapes allow (bf16, 196 / 49 + 16 tokens), otherwise as two launches.
 * The workspace must be large enough for either problem (max of lmv_attn_workspace_bytes). */
int lmv_attn_fwd_pair(const lmv_attn_desc* d, void* workspace, size_t workspace_bytes, int dtype, void* stream);
int lmv_attn_bwd_pair(const lmv_attn_desc* d, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* The probabilities the forward never materialises (csrc/attnmap.hip), recomputed from the forward's log-sum-exp:
 *   P[b,h,i,j] = exp(scale * q[b,i,h,:].k[b,j,h,:] - lse[b,h,i]).
 * d: the descriptor of the lmv_attn_fwd call whose probabilities are wanted (q, k, their strides, B, H, Lq, Lk, scale, lse are read;
 * v, o and the gradient fields are ignored).  head_mean = 0: p is [B, H, Lq, Lk] fp32; 1: p is [B, Lq, Lk] = (1/H) sum_h, summed in
 * the fixed order h = 0 .. H-1.  Every element of p is written exactly once; no workspace, no atomics, no pre-zeroed buffer.
 * p must be 16-byte aligned; one (b, h) plane Lq * Lk must stay below 2^31 elements. */
int lmv_attn_probs(const lmv_attn_desc* d, float* p, int head_mean, int dtype, void* stream);

/* Named cores of the reference seam; thin wrappers that fill an lmv_attn_desc.
 *   sa : StandardAttention      qkv [B,L,3C] -> o [B,L,C]                        (:199-205)
 *   ca : CrossAttention         q [B,M,C], kv [B,N,2C] -> o [B,M,C]              (:477-486)
 *   dca: DualCrossAttention     qkv1 [B,N,3C], qkv2 [B,M,3C] -> ox [B,N,C], oc [B,M,C]
 *        with scale_x = log_N(M) C^-1/2, scale_c = C^-1/2                        (:235,255-256,288-302) */
int lmv_sa_core_fwd(const void* qkv, void* o, float* lse, int B, int L, int C, void* ws, size_t ws_bytes, int dtype, void* stream);
int lmv_ca_core_fwd(const void* q, const void* kv, void* o, float* lse, int B, int M, int N, int C,
                    void* ws, size_t ws_bytes, int dtype, void* stream);
int lmv_dca_core_fwd(const void* qkv1, const void* qkv2, void* ox, void* oc, float* lse_x, float* lse_c,
                     int B, int N, int M, int C, void* ws, size_t ws_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small utilities used by the host side
 * ------------------------------------------------------------------------------------------ */
/* dst[i] = (dtype_dst) src[i]   (fp32 master weights -> bf16 compute copies and back) */
int lmv_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* y[r, :] = x[r, :] * scale[r / rows_per_sample]   (DropPath on a gradient) */
/* Stem, first convolution (models/lemevit.py:713, Conv2d(3, C/2, kernel 3, stride 2, padding 1)) lowered to a GEMM:
 * patches[(b, ho, wo)][ci * 9 + ky * 3 + kx] = x[b][ci][2 ho - 1 + ky][2 wo - 1 + kx] (zero outside the image), columns
 * 27..31 zero -> a [B * ceil(H/2) * ceil(W/2), 32] matrix in `dtype`.  x is read through its element strides
 * (sb, sc, sh, sw), so NCHW and channels-last batches of fp32 or bf16 images are accepted as they are.
 * lmv_linear_fwd(patches, W[Cout, 32]) is then the convolution (NHWC output), lmv_linear_dw its weight gradient. */
int lmv_im2col3x3s2_c3(const void* x, int x_dtype, void* patches, int dtype, int B, int H, int W, int64_t sb, int64_t sc, int64_t sh,
                       int64_t sw, void* stream);
/* The same convolution for ANY channel count, and its data gradient (csrc/conv1.hip; the Cin == 3 launches of the model stay on lmv_im2col3x3s2_c3):
 *   lmv_im2col3x3s2_nchw: patches[(b, ho, wo)][ci * 9 + ky * 3 + kx] = x[b][ci][2 ho - 1 + ky][2 wo - 1 + kx] (zero outside the image), columns 9 Cin .. KP - 1 zero,
 *     KP >= 9 Cin a multiple of 32 -> [B * ceil(H/2) * ceil(W/2), KP] in `dtype`; x ([B, Cin, H, W], fp32 or bf16) is read through its element strides.
 *   lmv_conv3x3s2_nchw_dx: dx[b, ci, h, w] = sum over co and the taps (ky, kx) with h + 1 - ky = 2 ho, w + 1 - kx = 2 wo, ho < Ho, wo < Wo of
 *     dy[(b, ho, wo), co] * wm[co, ci * 9 + ky * 3 + kx] -- ONE launch, no patch-gradient matrix.  dy [B Ho Wo, Co] and wm [Co, KP] in `dtype` (16-byte aligned, Co % 8 == 0,
 *     Co <= 128 for bf16 / 64 for fp32), fp32 accumulation (MFMA), dx in `dx_dtype` written through the element strides (sb, sc, sh, sw) of a [B, Cin, H, W] image: every
 *     element exactly once (no pre-zeroed buffer, no atomics), every sum in one fixed order -- two launches agree bit for bit. */
int lmv_im2col3x3s2_nchw(const void* x, int x_dtype, void* patches, int dtype, int B, int Cin, int H, int W, int KP, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                         void* stream);
int lmv_conv3x3s2_nchw_dx(const void* dy, const void* wm, void* dx, int dx_dtype, int B, int Cin, int H, int W, int Co, int KP, int64_t sb, int64_t sc, int64_t sh,
                          int64_t sw, int dtype, void* stream);
int lmv_row_scale(const void* x, const float* scale, void* y, int64_t rows, int C, int rows_per_sample, int dtype, void* stream);
/* The same for up to two row segments in ONE launch (the x and c gradients of a block, each with its own DropPath vector). */
typedef struct lmv_row_scale_segment {
  const void* x; const float* scale; void* y;
  int64_t rows; int rows_per_sample;
} lmv_row_scale_segment;
int lmv_row_scale_multi(const lmv_row_scale_segment* seg, int nseg, int C, int dtype, void* stream);
/* dst[c][r] = src[r][c] for any number of bf16 matrices (src [rows, cols] -> dst [cols, rows]) in one launch per LMV_TRANSPOSE_MAX_SEGS:
 * the transposed weight copies that let a dX run as a forward-form GEMM (lmv_block_desc.fc2_wt). */
#define LMV_TRANSPOSE_MAX_SEGS 48
typedef struct { const void* src; void* dst; int32_t rows, cols; } lmv_transpose_seg;
int lmv_transpose_batch(const lmv_transpose_seg* segs, int nsegs, int dtype, void* stream);
/* Dense 3x3 / stride-2 / padding-1 convolutions on channels-last maps -- the second stem convolution and the stage transitions
 * (models/lemevit.py:701-703, :714-717) -- lowered to the block GEMM:
 *   patches[(b, ho, wo)][(ky * 3 + kx) * C + ci] = x[b, 2 ho - 1 + ky, 2 wo - 1 + kx, ci]  (zero outside the map and in the padding
 *   columns 9 C .. KP - 1), x = [B, H, W, C] NHWC, patches = [B * ceil(H/2) * ceil(W/2), KP], C % 8 == 0, KP >= 9 C, KP % 8 == 0.
 * lmv_linear_fwd(patches, Wm[Cout, KP]) is the convolution (NHWC output), lmv_linear_dw its weight gradient, and
 * lmv_col2im3x3s2_nhwc(lmv_linear_dx(dY, Wm)) its data gradient (a gather over the <= 4 output pixels that read an input pixel). */
int lmv_im2col3x3s2_nhwc(const void* x, void* patches, int B, int H, int W, int C, int KP, int dtype, void* stream);
int lmv_col2im3x3s2_nhwc(const void* dpatches, void* dx, int B, int H, int W, int C, int KP, int dtype, void* stream);
/* The same convolution WITHOUT the patch matrix (round 6; bf16): an implicit GEMM -- the LDS-DMA loads of the GEMM kernels gather the patch elements straight from the
 * NHWC map x [B, H, W, Cin] (zeros for the padding taps and for the columns behind 9 Cin), so the forward pass and the weight gradient read the map instead of writing and
 * re-reading a [B Ho Wo, KP] matrix 2.25 x its size.  wm / dwm: [Cout, KP] in lmv_im2col3x3s2_nhwc's column order ((ky * 3 + kx) * Cin + ci), KP >= 9 Cin a multiple of 64;
 * B Ho Wo must be a multiple of 64 (whole k-tiles of the weight gradient); y [B Ho Wo, Cout] = patches wm^T + bias (act: LMV_ACT_NONE / LMV_ACT_GELU);
 * dwm += dy^T patches, dbias += column sums of dy (fp32, accumulated; split-K slabs in `workspace`, fixed summation order as lmv_linear_dw).  The data gradient stays
 * lmv_linear_dx + lmv_col2im3x3s2_nhwc.  Replaces models/lemevit.py:701-703, :714-717 (nn.Conv2d(.., 3, 2, 1)). */
int lmv_conv3x3s2_fwd(const void* x, const void* wm, const float* bias, void* y, int B, int H, int W, int Cin, int Cout, int KP, int act, int dtype, void* stream);
size_t lmv_conv3x3s2_dw_workspace_bytes(int B, int H, int W, int Cin, int Cout, int KP, int dtype);
int lmv_conv3x3s2_dw(const void* dy, const void* x, float* dwm, float* dbias, int B, int H, int W, int Cin, int Cout, int KP, void* workspace, size_t workspace_bytes, int dtype,
                     void* stream);
/* A frozen (eval-mode) BatchNorm2d behind one of these convolutions, under autograd (csrc/convbn.hip): the BatchNorm is folded into the GEMM operand, with gradients.
 * With r = 1 / sqrt(var + eps) and s = gamma r (all vectors fp32 [Co], w the fp32 master weight [Co, Cin, 3, 3], b its bias or NULL):
 *   lmv_conv_bn_fold (one launch): wm[co, col] = w[co, ci, tap] s[co] in `dtype` with the columns 9 Cin .. KP - 1 zero -- col = ci * 9 + tap for LMV_FOLD_CI_TAP
 *     (the operand of lmv_im2col3x3s2_c3 / _nchw), col = tap * Cin + ci for LMV_FOLD_TAP_CI (lmv_im2col3x3s2_nhwc / lmv_conv3x3s2_fwd) --,
 *     bf = (b - mean) s + beta and sc = s.  Co % 8 == 0, KP >= 9 Cin a multiple of 8.
 *   lmv_conv_bn_fold_bwd (one launch) from the folded gradients dwm [Co, KP] / dbf [Co] (fp32) that lmv_linear_dw / lmv_conv3x3s2_dw produced:
 *     dW = dwm s in the weight's own [Co, Cin, 3, 3] layout, db = dbf s, dgamma = r (sum_k dwm[co, k] w[co, k] + dbf (b - mean)), dbeta = dbf -- WRITTEN, not
 *     accumulated; each of the four may be NULL.  The per-channel sums run in one fixed order: two launches agree bit for bit. */
enum { LMV_FOLD_CI_TAP = 0, LMV_FOLD_TAP_CI = 1 };
int lmv_conv_bn_fold(const float* w, const float* b, const float* gamma, const float* beta, const float* mean, const float* var, float eps, int Co, int Cin, int KP,
                     int layout, void* wm, float* bf, float* sc, int dtype, void* stream);
int lmv_conv_bn_fold_bwd(const float* dwm, const float* dbf, const float* w, const float* b, const float* gamma, const float* mean, const float* var, float eps, int Co,
                         int Cin, int KP, int layout, float* dW, float* db, float* dgamma, float* dbeta, void* stream);
/* Classifier tail (models/lemevit.py:815-835, `x.flatten(2).mean(-1) + c.mean(1)`): out[b, :] = mean_l x[b, l, :] + mean_m c[b, m, :]
 * for token-major x [B, L, C] and c [B, M, C] (c may be NULL), out [B, C] in `dtype`; and its backward, the broadcast
 * dx[b, l, :] = g[b, :] / L, dc[b, m, :] = g[b, :] / M (dc may be NULL). */
int lmv_token_mean2_fwd(const void* x, int L, const void* c, int M, int C, int B, void* out, int dtype, void* stream);
int lmv_token_mean2_bwd(const void* g, void* dx, int L, void* dc, int M, int C, int B, int dtype, void* stream);
/* Inference tail (models/lemevit.py:815, 825 with the final BatchNorm in eval mode): BatchNorm with running statistics is affine per channel and
 * commutes with the spatial mean, so out[b, :] = xscale * mean_l x[b, l, :] + xshift + mean_m c[b, m, :] with
 * xscale = gamma / sqrt(running_var + eps), xshift = beta - running_mean * xscale (fp32 [C]). */
int lmv_token_mean2_affine_fwd(const void* x, int L, const void* c, int M, int C, int B, const float* xscale, const float* xshift, void* out, int dtype,
                               void* stream);
/* Fused multi-tensor AdamW over a flat fp32 parameter / gradient / moment buffer
 * (decoupled weight decay, bias correction as torch.optim.AdamW; benchmark.py:559-561,587).
 * wd_mask (nullable): per-element 0/1 factor on weight_decay.  shadow_bf16 (nullable): bf16 copy of the updated parameters,
 * written in the same pass (the operand copy the block kernels read; no separate cast launches).  step_dev (nullable):
 * device int holding the 1-based step count -- read by the kernel instead of `step`, so a captured hipGraph replays with
 * the right bias correction. */
int lmv_adamw_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* wd_mask, void* shadow_bf16,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                   void* stream);
/* Global L2 norm of a list of fp32 gradient segments, and the clipping coefficient derived from it, all on the device (engine.py:82-95
 * dispatch_clip_grad / utils/__init__.py:311-331 NativeScalerWithGradNormCount; torch.nn.utils.clip_grad_norm_ with norm_type 2).
 * Any number of segments, each of any length >= 0 and 4-byte alignment (a segment whose start is 16-byte aligned is read with 16-byte loads).
 * Stage 1: every segment is cut into chunks of LMV_NORM_CHUNK elements, one workgroup sums the squares of one chunk in fp32 and writes one partial
 * into `ws` (the table goes to the kernel by value, one launch per run of segments that fits it); stage 2 (one more launch, one workgroup) adds the partials in a fixed order in double.
 * Which element meets which accumulator depends on the segment lengths alone -- not on the grid, the device, the stream or a pointer's
 * alignment -- and there are no floating-point atomics: two calls, and all ranks of a data-parallel job, agree bit for bit.
 * stat (device, 16-byte aligned, LMV_GRAD_STAT_FLOATS floats):
 *   [0] norm   [1] coef = min(1, max_norm / (norm + 1e-6)), 1 when max_norm <= 0 (measure only)   [2] 1 / coef
 *   [3] found_inf: 1.0 when the norm is inf or NaN, else 0.0   [4] running count of skipped steps (read, then written: zero it once)
 *   [5..7] reserved, written as 0.
 * flags & LMV_NORM_SKIP_NONFINITE: when found_inf is set, [1] = 0 and [4] += 1 (lmv_adamw_flat_clip then leaves everything alone); without
 * the flag a non-finite norm flows through as in torch (coef 0 for inf, NaN for NaN).
 * step_dev (nullable): device int step count, advanced by one here unless the step is skipped.
 * ws: lmv_grad_norm_workspace_bytes(segs, nsegs) bytes (one float per chunk), 4-byte aligned; no pre-zeroing. */
typedef struct { const float* ptr; int64_t n; } lmv_norm_seg;
#define LMV_GRAD_STAT_FLOATS 8
#define LMV_NORM_CHUNK 16384
enum { LMV_NORM_SKIP_NONFINITE = 1 };
size_t lmv_grad_norm_workspace_bytes(const lmv_norm_seg* segs, int nsegs);
int lmv_grad_norm(const lmv_norm_seg* segs, int nsegs, float max_norm, int flags, float* stat, int* step_dev, void* ws, size_t ws_bytes,
                  void* stream);
/* lmv_adamw_flat with the gradient scaled or clamped on the fly -- the gradients in memory are not rewritten:
 * stat (nullable; what lmv_grad_norm wrote): g * stat[1] enters the update; stat[3] != 0 && stat[1] == 0 is a skipped step -- nothing is written
 * (parameters, both moments and the bf16 copy stay as they are).  clip_value > 0: g is clamped to [-clip_value, clip_value] (clip mode 'value'). */
int lmv_adamw_flat_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* wd_mask, void* shadow_bf16,
                        int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                        const float* stat, float clip_value, void* stream);
/* lmv_adamw_flat_clip with the learning rate and the weight decay of every element read from DEVICE memory by the running kernel: element i takes
 * groups[group_of_unit[i / LMV_ADAMW_UNIT]] (layer-wise rate decay, lr_mult by prefix), and a captured hipGraph replays with whatever the table holds
 * at replay time (a scheduled rate; lemevit_amd.optim.FlatAdamW(layer_decay= / lr_scale= / device_lr=), sync_hyper()).  There is no wd_mask: a group
 * that does not decay has weight_decay = 0.  group_of_unit: device, n / LMV_ADAMW_UNIT bytes; a byte >= ngroups reads the last entry.  groups: device,
 * 8-byte aligned, ngroups entries (1 .. LMV_ADAMW_MAX_GROUPS).  n % LMV_ADAMW_UNIT == 0.  stat (nullable) / clip_value (0: none) / step / step_dev:
 * as lmv_adamw_flat_clip; with neither stat nor clip_value the launch is lmv_adamw_flat's arithmetic.  On a sub-range whose elements share one group
 * the result equals, bit for bit, what lmv_adamw_flat (neither stat nor clip_value) or lmv_adamw_flat_clip (either) computes there with that group's
 * lr and weight_decay.  Refused with LMV_ERR_SHAPE before any launch: n % LMV_ADAMW_UNIT, ngroups outside 1 .. LMV_ADAMW_MAX_GROUPS, a null or
 * misaligned buffer (the fp32 buffers to 16 bytes, groups to 8), step < 1 without step_dev, clip_value < 0 or NaN. */
#define LMV_ADAMW_UNIT 8
#define LMV_ADAMW_MAX_GROUPS 256
typedef struct { float lr; float weight_decay; } lmv_adamw_group;
int lmv_adamw_flat_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t n,
                          const uint8_t* group_of_unit, const lmv_adamw_group* groups, int ngroups, float beta1, float beta2, float eps, int step,
                          const int* step_dev, const float* stat, float clip_value, void* stream);
/* Exponential moving average of the weights over the same flat buffer (timm.utils.ModelEmaV2: main.py:316, engine.py model_ema.update(model)):
 * ema[i] = decay * ema[i] + (1 - decay) * param[i], n % 4 == 0, one launch (lemevit_amd.optim.ModelEma). */
int lmv_ema_flat(float* ema, const float* param, int64_t n, float decay, void* stream);

/* ------------------------------------------------------------------------------------------
 * The two ends of the reference's training step (csrc/recipe.hip): batch mixing in front of the forward pass and the loss behind it.
 *
 * lmv_mix_record: one per image, in DEVICE memory -- the running kernels read it, so a captured hipGraph mixes (and weighs its targets) with whatever the
 * table holds at replay time.  A pixel inside [yl, yh) x [xl, xh) takes the partner's value; elsewhere out = w * self + (1 - w) * partner.  Mixup: empty box,
 * w = lam.  Cutmix: w = 1 and a box.  No mixing: w = 1, empty box.  lam_t is the weight of the image's OWN label in its target (mixup: lam; cutmix: the
 * corrected 1 - area / (H W)); lmv_soft_ce reads nothing else of a record.
 *
 * lmv_mix_images (timm.data.Mixup._mix_batch / _mix_elem / _mix_pair on the images: main.py:375-389, engine.py:61-62; with scale / shift also the
 * PrefetchLoader normalisation): x [B, C, H, W], LMV_U8 / LMV_F32 / LMV_BF16, ELEMENT strides sb, sc, sh, sw (any: NCHW, channels-last, a sliced view) ->
 * out, contiguous NCHW, LMV_F32 / LMV_BF16, in ONE launch.  Image b is mixed with image B - 1 - b (x.flip(0)); an odd B pairs the middle image with
 * itself.  One workgroup serves both images of a pair: every input element is loaded once, every output element stored once (no atomics: bit-identical
 * from run to run); 16-byte stores where C H W is a multiple of the 16-byte element count and `out` is 16-byte aligned (with element stores for the head
 * and tail of a row), loads as wide as the addresses allow when sw == 1.  x is not modified and must not overlap out.
 * scale / shift (nullable, together; fp32 [C], device): out = mixed * scale[c] + shift[c] in fp32.  Without them, with equal dtypes, a pixel that takes
 * one image as it is (inside the box, or w == 1) is a bit-exact copy.
 * host_records (nullable): a HOST copy of the table, validated before the launch.  Refused with LMV_ERR_SHAPE and a message, before any launch: a null
 * image buffer or table, B / C / H / W < 1, a dtype pair other than the above, scale without shift, a misaligned buffer, and -- given host_records -- a
 * box outside the image, yl > yh, xl > xh, a NaN factor.  (A box outside the image in the DEVICE table cannot cause an access outside the buffers: the
 * box is only ever compared with pixel coordinates.)
 *
 * lmv_soft_ce (timm.loss.SoftTargetCrossEntropy / LabelSmoothingCrossEntropy, F.cross_entropy: main.py:456-466; the target of timm.data.mixup.mixup_target
 * without building it): logits [B, N] fp32 / bf16, row stride `row_stride` elements (>= N: the [:, :N] view of padded logits is legal), any N >= 1.
 *   sparse form (labels != NULL, target == NULL): labels int64 [B]; t = lam_t oh(labels[b]) + (1 - lam_t) oh(labels[B - 1 - b]), oh = 1 - s + s / N on
 *     the label and s / N elsewhere, s = smoothing in [0, 1); table == NULL: lam_t = 1 (plain / label-smoothed cross-entropy; the partner is not read).
 *     A label outside [0, N) carries no one-hot mass and is never used as an index.  Labels are NOT validated (that would need a host synchronisation).
 *   dense form (target != NULL, labels == NULL): target [B, N] fp32 / bf16 (target_dtype), row stride target_stride.
 *   row_loss[b] = -sum_j t_j log softmax(x)_j (fp32 [B], always written); *mean_loss = (sum_b row_loss[b]) / B (fp32 device scalar);
 *   dlogits (nullable: loss only; else contiguous [B, N] in the logits dtype) = d mean_loss / d logits = (p_j sum(t) - t_j) / B, sum(t) = 1 for a proper target.
 * Two launches: one wave per row (max, log-sum-exp and sums in fp32, three sweeps over the cached row), then ONE wave that adds the B row losses in a
 * fixed order -- no floating-point atomics, two calls agree bit for bit.  Refused with LMV_ERR_SHAPE before any launch: B < 1, N < 1, a dtype code other
 * than LMV_F32 / LMV_BF16, null logits / row_loss / mean_loss, both or neither of labels and target, a table with the dense form, row strides < N,
 * smoothing outside [0, 1), a misaligned buffer.
 * ------------------------------------------------------------------------------------------ */
typedef struct lmv_mix_record { float w; int32_t yl, yh, xl, xh; float lam_t; } lmv_mix_record;
int lmv_mix_images(const void* x, int x_dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* out, int out_dtype, int B, int C, int H, int W,
                   const lmv_mix_record* table, const lmv_mix_record* host_records, const float* scale, const float* shift, void* stream);
int lmv_soft_ce(const void* logits, int dtype, int64_t row_stride, int B, int N, const int64_t* labels, const lmv_mix_record* table, float smoothing,
                const void* target, int target_dtype, int64_t target_stride, float* row_loss, float* mean_loss, void* dlogits, void* stream);

/* ------------------------------------------------------------------------------------------
 * Random erasing fused into the batch-mixing launch (csrc/recipe.hip; timm.data.random_erasing.RandomErasing as timm's PrefetchLoader runs it behind the
 * normalisation: configs/lemevit.yaml:74-76 reprob 0.25, remode pixel, recount 1; main.py:406-409).  An addition to ABI 14: callers detect it by symbol.
 *
 * lmv_erase_record: one per image, in DEVICE memory: up to LMV_ERASE_MAX_BOXES boxes box[i] = {yl, yh, xl, xh}, i.e. [yl, yh) x [xl, xh); 16 int32 words.  An
 * empty box (yl >= yh or xl >= xh, e.g. all zero) erases nothing.  The boxes are only ever compared with pixel coordinates: a bad box in the DEVICE table
 * cannot cause an access outside the buffers.  The noise key is two 32-bit words in DEVICE memory.  The running kernel reads table and key, so a captured
 * hipGraph erases with whatever they hold at replay time.
 *
 * lmv_augment_images: x, the strides, out, B, C, H, W, the dtypes, host_records, scale / shift and stream as in lmv_mix_images.  Per pixel: mix under
 * mix_table (NULL: every image stays as it is), then * scale[c] + shift[c], then erase: a pixel (y, x) of image b inside any box of erase_table[b] is the
 * FILL VALUE instead (rounded to the output dtype; what the mix would have given there is not used), so the boxes of image b apply to OUTPUT image b, after
 * the mixing -- collate-time mixup, normalise, erase: the reference's order.  erase_table == NULL: the output equals lmv_mix_images' bit for bit; both tables
 * NULL: the plain PrefetchLoader normalise-and-cast.  One launch, the kernel of lmv_mix_images with the fill behind it: every input element loaded once, every
 * output element stored once, 16-byte stores where the phase allows, no atomics, no workspace; two launches with one key agree bit for bit.
 *
 * Fill values, erase_mode (timm's `mode`):
 *   LMV_ERASE_CONST  0.
 *   LMV_ERASE_PIXEL  one standard normal per element, a pure function of (key, b, c, y, x) -- not of the layout of x, the alignment of out or the path the
 *                    kernel takes.  (r0, r1, r2, r3) = Philox4x32-10 (Salmon et al., SC'11; Random123 philox4x32_R(10, ctr, key)) with the counter words
 *                    ctr = (x >> 2, y, c, b) and the key words (erase_key[0], erase_key[1]): ten rounds of
 *                      (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  M0 = 0xD2511F53, M1 = 0xCD9E8D57,
 *                    hi / lo the halves of the 64-bit product, with (k0, k1) += (0x9E3779B9, 0xBB67AE85) (mod 2^32) between rounds; known answer:
 *                    ctr = 0, key = 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  Two Box-Muller pairs: from words (ra, rb) = (r0, r1) the lanes x & 3 = 0, 1 and
 *                    from (r2, r3) the lanes 2, 3: u1 = ((ra >> 9) + 1) 2^-23 in (0, 1], u2 = (rb >> 8) 2^-24 in [0, 1) (both exact in fp32),
 *                    rad = sqrt(-2 ln u1), the even lane rad cos(2 pi u2), the odd lane rad sin(2 pi u2); |value| <= sqrt(46 ln 2) = 5.6467.  Evaluated in
 *                    fp32 with the accurate logarithm and sincospi(2 u2): within 1e-5 of the exact value.  Overlapping boxes write the same noise.
 *   LMV_ERASE_RAND   one normal per (box i, channel c): lane 0 of the counter (i, 0xffffffff, c, b).  Where boxes overlap, the box of the highest index wins.
 * Noise is generated only by threads whose chunk meets a box: a launch with an all-empty table runs no Philox round.
 *
 * host_erase_records (nullable): a HOST copy of erase_table, validated before the launch.  Refused with LMV_ERR_SHAPE and a message, before any launch:
 * everything lmv_mix_images refuses (except a null mix_table), an unknown erase_mode, an erase_table without erase_key in the RAND / PIXEL mode, a
 * misaligned table or key, and -- given host_erase_records -- a box outside the image or with yl > yh, xl > xh.
 * ------------------------------------------------------------------------------------------ */
#define LMV_ERASE_MAX_BOXES 4
enum { LMV_ERASE_CONST = 0, LMV_ERASE_RAND = 1, LMV_ERASE_PIXEL = 2 };
typedef struct lmv_erase_record { int32_t box[LMV_ERASE_MAX_BOXES][4]; } lmv_erase_record;
int lmv_augment_images(const void* x, int x_dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* out, int out_dtype, int B, int C, int H, int W,
                       const lmv_mix_record* mix_table, const lmv_mix_record* host_records, const lmv_erase_record* erase_table, const uint32_t* erase_key,
                       int erase_mode, const lmv_erase_record* host_erase_records, const float* scale, const float* shift, void* stream);

/* ------------------------------------------------------------------------------------------
 * Validation metrics (csrc/metrics.hip; the metrics tail of the reference's evaluation loop, engine.py:177-247 validate and validate.py:330-377:
 * nn.CrossEntropyLoss, utils.accuracy(output, target, topk=(1, 5)), the --tta reduction, three reduce_tensor, a synchronize and three .item() per batch).
 * An addition to ABI 14: callers detect it by symbol.  Neither call synchronises the host; both can be captured in a hipGraph.
 *
 * lmv_eval_logits: logits [B, N] fp32 / bf16, unit column stride, row stride `row_stride` elements (>= N: the [:, :N] view of padded logits is read in place;
 * what lies behind column N is never read), any N >= 1 (every class value is recomputed per sweep, nothing is staged).  reduce_factor r >= 1, B % r == 0 (the
 * reference's --tta: output.unfold(0, r, r).mean(dim=2), target[0::r]); labels int64 [B / r].  Output row g, g < B / r, evaluates the values
 *     v_j = (((x[g r, j] + x[g r + 1, j]) + ...) + x[g r + r - 1, j]) * (1.0f / r)        in fp32, in this order, the product never fused into its consumer;
 * r == 1: v_j = x[g, j], no arithmetic touches it.  Per output row, each element written by exactly one thread, no atomics, two launches agree bit for bit:
 *   row_loss[g] (fp32) = lse - v_y, lse = max_j v_j + log(sum_j exp(v_j - max)), y = labels[g]: plain cross-entropy.  A NaN logit makes the row's loss NaN.
 *   rank[g] (int32)    = the number of classes ordered BEFORE class y in this total order: class j is before class i iff v_j > v_i, or v_j == v_i and j < i;
 *                        NaN orders before every number (as torch.topk does) and NaNs among themselves by index; -0.0 == +0.0.  The comparison at j == y is
 *                        decided by the index, never by the value.  rank < k  <=>  the label is among the first k classes: top-k accuracy.
 *   pred[g, 0 .. K)    (int32 [B / r, K], K <= LMV_EVAL_MAX_PRED, K <= N; K == 0: pred may be NULL) = the first K classes of the same order.
 * The order is that of the 64-bit word (key(v_j), ~j), key = the value's bits flipped on sign, every NaN the top key, -0 the key of +0.
 * A row whose label is outside [0, N) is IGNORED: row_loss = 0, rank = -1, pred still written; the label is never used as an index.  A padded last batch or a
 * distributed sampler's duplicates are marked so (label -1).  This differs ON PURPOSE from lmv_soft_ce, where such a label merely carries no one-hot mass and
 * the row still contributes lse * (remaining mass): there the row is a training sample with a partner, here it is not a sample at all.
 * One wave per output row, 2 + K sweeps over the cached row.  Refused with LMV_ERR_SHAPE and a message, before any launch: null logits / labels / row_loss /
 * rank, B < 1, N < 1, reduce_factor < 1 or not a divisor of B, row_stride < N, a dtype code other than LMV_F32 / LMV_BF16, K outside 0 .. 16, K > N, K > 0
 * with a null pred, a misaligned buffer.
 *
 * lmv_meter_add: ONE wave adds a batch into the persistent DEVICE accumulator `state`, float64 [2 + nk] = {loss_sum, rows_counted, hits(ks[0]), ...,
 * hits(ks[nk - 1])}, nk <= LMV_METER_MAX_K; the thresholds ks are read on the HOST and passed to the kernel by value.
 *   per-row mode (row_loss, rank != NULL, loss == NULL): over the `rows` results of lmv_eval_logits, rows with rank < 0 (ignored) adding nothing:
 *     state[0] += sum row_loss, state[1] += number of rows, state[2 + i] += number of rows with 0 <= rank < ks[i].  Lane l adds rows l, l + 64, ... in order,
 *     then a butterfly, all in double -- a fixed tree; one thread then updates the state.
 *   scalar mode (loss != NULL, row_loss == rank == NULL): state[0] += (double)*loss * n, state[1] += n (loss: fp32 DEVICE scalar; the train loop's
 *     losses_m.update(loss.item(), n) without the .item()); the hit entries are not touched.
 * Stream order serialises successive updates: two runs give the same bits.  Doubles hold the counts exactly (< 2^53) and one dtype keeps the merge across
 * ranks to ONE sum all-reduce of the state.  Refused with LMV_ERR_SHAPE before any launch: a null state, nk outside 0 .. 8, null ks with nk > 0, a threshold
 * < 1, both or neither mode's operands, row_loss without rank, rows < 1 (per-row mode), n < 1 (scalar mode), a misaligned buffer.
 * ------------------------------------------------------------------------------------------ */
#define LMV_EVAL_MAX_PRED 16
#define LMV_METER_MAX_K 8
int lmv_eval_logits(const void* logits, int dtype, int64_t row_stride, int B, int N, const int64_t* labels, int reduce_factor, float* row_loss, int32_t* rank,
                    int32_t* pred, int K, void* stream);
int lmv_meter_add(double* state, const float* row_loss, const int32_t* rank, int rows, const int32_t* ks, int nk, const float* loss, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense-prediction losses and metrics (csrc/dense.hip; the reference's change_detection/utils/metrics.py FocalLoss / dice_loss / jaccard_loss, utils/losses.py
 * hybrid_loss, the per-batch torch.max / eq / sum of train.py:154-260, sklearn's confusion_matrix of eval.py:39-66, and the segmentation heads' per-pixel
 * cross-entropy with an ignore index and mIoU histogram).  An addition to ABI 14: callers detect it by symbol.  No call synchronises the host; all can be captured.
 *
 * Inputs.  logits [B, K, H, W] fp32 / bf16: pixel stride 1, ELEMENT strides batch_stride and class_stride (a class-sliced view buf[:, 1:K+1] is read in place;
 * nothing outside the K planes of H W pixels is read), 2 <= K <= LMV_DENSE_MAX_CLASSES, B H W < 2^31 (HW = H W).  labels [B, H W], contiguous,
 * LMV_DENSE_LABEL_I64 or LMV_DENSE_LABEL_U8.  A pixel is IGNORED when its label equals ignore_index or lies outside [0, K): it is never used as an index and
 * contributes to no sum, count or gradient -- the rule of lmv_eval_logits (a row that is not a sample at all), not that of lmv_soft_ce.  Pass ignore_index = -1
 * for "none".  alpha: float32 DEVICE vector [K] or NULL (= all ones); float32 by definition (the reference builds it with torch.Tensor([...])).
 *
 * Per valid pixel i, in fp32 with the maximum subtracted (logits of +-80 work): p = softmax(z_i), y = label,
 *     f_i = alpha[y] (1 - p_y)^gamma        a CONSTANT of the backward pass (the reference detaches pt, utils/metrics.py:35); gamma == 0: f_i = alpha[y].
 * Per class k over the valid pixels of the call:  I_k = sum p_k [y = k],  P_k = sum p_k,  T_k = sum [y = k].
 *     ce      = (sum_i f_i (-log p_{i,y})) / D,   D by avg_mode:  LMV_DENSE_AVG_VALID  the number of valid pixels (F.cross_entropy(ignore_index=));
 *                                                                 LMV_DENSE_AVG_ALL    B H W (the reference's .mean());
 *                                                                 LMV_DENSE_AVG_WEIGHT sum_k alpha_k T_k (F.cross_entropy(weight=));      D == 0: ce = 0, gradient 0
 *     dice    = 1 - (1 / K) sum_k 2 I_k / (P_k + T_k + eps)
 *     jaccard = 1 - (1 / K) sum_k I_k / (P_k + T_k - I_k + eps)
 *     loss    = w_ce ce + w_dice dice + w_jac jaccard
 * Gradient: with C_k = P_k + T_k + eps, U_k = P_k + T_k - I_k + eps,
 *     u_k = -w_dice 2 / (K C_k) - w_jac (1 / U_k + I_k / U_k^2) / K,     v_k = w_dice 2 I_k / (K C_k^2) + w_jac I_k / (K U_k^2),     g_ik = u_k [y_i = k] + v_k,
 *     dz_ik = gout ( p_ik (g_ik - sum_j p_ij g_ij) + w_ce f_i (p_ik - [y_i = k]) / D );          an ignored pixel gets exact zeros.
 *
 * lmv_dense_loss_fwd -- two launches.  (a) a grid-stride pass: a thread owns chunks of 16 bytes of consecutive pixels of one image (4 fp32 / 8 bf16) and reads one
 * 16-byte word per class plane when the logits pointer is 16-byte aligned and both strides are multiples of the chunk, element loads otherwise -- the chunks, the
 * arithmetic and every summation order are the same on both paths, so the result does not depend on which ran.  Each thread keeps fp32 partial sums; they are added
 * by a butterfly within the wave and over the waves in order, and each workgroup writes one row of 3 K + 3 floats into `workspace`
 * (lmv_dense_loss_workspace_bytes(B, K, HW)).  pred (nullable): uint8 [B, H W], the argmax of EVERY pixel, ignored ones included: the first index of the maximum,
 * a NaN greater than every number (the first NaN wins), -0 == +0.  conf (nullable): a persistent int64 [K, K] DEVICE matrix, conf[y, pred] += 1 per valid pixel
 * (an LDS histogram per workgroup, then integer atomics: integer adds commute).  No floating-point atomic anywhere: two calls agree bit for bit.
 * (b) ONE workgroup adds the rows in double in a fixed order and writes `stats`, float32 [LMV_DENSE_STATS_FLOATS(K)]:
 *     stats[0 .. 6) = loss, ce, dice, jaccard, n_valid, 1 / D (0 when D == 0);  then u[K], v[K], I[K], P[K], T[K]
 * (n_valid and T_k are exact below 2^24).  meter (nullable): a persistent float64 [2] DEVICE accumulator, meter[0] += sum_valid -log p_y (unweighted),
 * meter[1] += n_valid, both exact in double; stream order serialises successive calls.
 *
 * lmv_dense_loss_bwd -- one launch: re-reads logits and labels, reads u, v and 1 / D from `stats` in DEVICE memory and gout through a DEVICE pointer to a float
 * (NULL = 1), and writes dlogits, contiguous [B, K, H, W] in the logits dtype, every element exactly once (no pre-zeroed buffer).  gamma, the weights, alpha,
 * ignore_index and avg_mode are the arguments of the forward call that produced `stats`.
 *
 * Refused with LMV_ERR_SHAPE and a message that starts "dense_loss", before any launch: null logits / labels / workspace / stats / dlogits; a misaligned buffer
 * (logits and dlogits to their element, int64 labels, conf and meter to 8 bytes, workspace, stats, alpha and gout to 4); K outside 2 .. 64; B < 1, H W < 1 or
 * B H W >= 2^31; a dtype code other than LMV_F32 / LMV_BF16 or a label dtype code other than the two above; class_stride < H W or
 * batch_stride < (K - 1) class_stride + H W (strides smaller than the extent they skip); a workspace smaller than lmv_dense_loss_workspace_bytes; a negative (or
 * NaN) w_ce / w_dice / w_jac, gamma < 0, eps <= 0; an unknown avg_mode.
 * ------------------------------------------------------------------------------------------ */
#define LMV_DENSE_MAX_CLASSES 64
#define LMV_DENSE_STATS_HEAD 6
#define LMV_DENSE_STATS_FLOATS(K) (LMV_DENSE_STATS_HEAD + 5 * (K))
enum { LMV_DENSE_LABEL_I64 = 0, LMV_DENSE_LABEL_U8 = 1 };
enum { LMV_DENSE_AVG_VALID = 0, LMV_DENSE_AVG_ALL = 1, LMV_DENSE_AVG_WEIGHT = 2 };
size_t lmv_dense_loss_workspace_bytes(int B, int K, int64_t HW);
int lmv_dense_loss_fwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int64_t HW, const void* labels, int label_dtype,
                       int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps, int avg_mode, void* workspace,
                       size_t workspace_bytes, float* stats, uint8_t* pred, int64_t* conf, double* meter, void* stream);
int lmv_dense_loss_bwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int64_t HW, const void* labels, int label_dtype,
                       int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps, int avg_mode, const float* stats,
                       const float* gout, void* dlogits, void* stream);

/* ------------------------------------------------------------------------------------------
 * The dense losses on LOW-RESOLUTION logits: the bilinear upsampling in front of every dense loss of the reference (change_detection/models/Models.py:221
 * F.interpolate(scale_factor=4, align_corners=True); the segmentation heads' resize(seg_logit, size=seg_label.shape[2:], mode='bilinear'), 4x / 16x) is evaluated
 * inside the pass, so the [B, K, H, W] map and its gradient never exist.  An addition to ABI 14: callers detect it by symbol.  Everything of the block above holds
 * unless stated: the formulas, the ignore rule, the argmax rule, the `stats` layout, the workspace row layout, launch (b), no floating-point atomics, capture.
 *
 * Geometry.  logits [B, K, h, w] fp32 / bf16 (pixel stride 1, rows of a plane contiguous, ELEMENT strides batch_stride / class_stride as above), labels [B, H W],
 * H >= h, W >= w, B H W < 2^31.  The logit of output pixel (Y, X) is PyTorch's upsample_bilinear2d in its `size=` form (the scale comes from the sizes; equal to
 * scale_factor=s for an integer s), per axis, in fp32:
 *     align_corners = 0:  src = max(0, (dst + 0.5) in / out - 0.5)          align_corners = 1:  src = dst (in - 1) / (out - 1),  0 when out == 1
 *     i0 = floor(src),  i1 = min(i0 + 1, in - 1),  l = src - i0
 *     z = (1 - ly) ((1 - lx) z00 + lx z01) + ly ((1 - lx) z10 + lx z11)          per class
 * A bf16 input is NOT rounded back to bf16 after the interpolation (the stock path rounds the map it stores): this path is the more accurate one.  One device
 * function computes (i0, i1, l) for every kernel, and the backward pass finds the output pixels that touch an input pixel by bisection on that same function.
 *
 * lmv_dense_up_loss_fwd -- what lmv_dense_loss_fwd computes, on the interpolated logits.  A thread owns chunks of 4 consecutive output pixels of ONE output row
 * (a chunk never crosses a row); the labels of a chunk are loaded as one word where the address allows, element-wise otherwise (the same bits); the four input
 * values per class come from the 16 x smaller, cache-resident logits.  workspace: lmv_dense_up_loss_workspace_bytes(B, K, H, W).  pred: uint8 [B, H W].
 * labels == NULL with pred != NULL is PREDICTION ONLY (resize + argmax at inference): no sums, launch (b) is skipped, workspace / stats / conf / meter are not
 * touched and may be NULL.
 *
 * lmv_dense_up_loss_bwd -- one launch.  dlogits, contiguous [B, K, h, w] in the logits dtype:
 *     d z_low[b, k, y, x] = sum over (Y, X) of wy(Y, y) wx(X, x) dz_high[b, k, Y, X],          dz_high: the closed form above (exact zero at an ignored pixel)
 * accumulated in fp32, rounded once, every element written exactly once (no pre-zeroed buffer, no floating-point atomic in global memory or LDS): a workgroup owns a
 * tile of input pixels, evaluates the softmax of every output pixel of the tile's footprint once per block of the footprint, and gathers per class from an LDS
 * plane in a fixed order.  Two calls agree bit for bit.
 *
 * Refused with LMV_ERR_SHAPE and a message that starts "dense_up_loss", before any launch: everything the block above refuses (with h w in the place of H W for
 * the strides); h < 1, w < 1, H < h or W < w; B H W >= 2^31; an align_corners other than 0 / 1; labels == NULL with pred == NULL (backward: labels == NULL).
 * ------------------------------------------------------------------------------------------ */
size_t lmv_dense_up_loss_workspace_bytes(int B, int K, int H, int W);
int lmv_dense_up_loss_fwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int h, int w, int H, int W, int align_corners,
                          const void* labels, int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac,
                          float eps, int avg_mode, void* workspace, size_t workspace_bytes, float* stats, uint8_t* pred, int64_t* conf, double* meter, void* stream);
int lmv_dense_up_loss_bwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int h, int w, int H, int W, int align_corners,
                          const void* labels, int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac,
                          float eps, int avg_mode, const float* stats, const float* gout, void* dlogits, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sliding-window dense inference (mmseg's EncoderDecoder.slide_inference, which all three segmentation configs of the reference select:
 * test_cfg=dict(mode='slide', stride=(384, 384), crop_size=(512, 512))): stitch, resize and argmax in ONE pass.  An addition to ABI 14: callers detect it by
 * symbol.  The stock loop resizes every window's logits to the crop, pads them to a full [B, K, H, W] fp32 map, adds that into `preds`, bumps a count map, and
 * divides at the end; here none of those maps exists.  Everything of the two blocks above holds unless stated: the interpolation formulas, the ignore rule, the
 * argmax rule, the `stats` and workspace row layouts, launch (b), no floating-point atomics (two calls agree bit for bit), capture.
 *
 * Geometry.  logits [G, B, K, h, w] fp32 / bf16: the stack of window logits, G = gy gx windows in mmseg's order (window iy gx + ix), ELEMENT strides
 * window_stride / batch_stride / class_stride, the h x w planes contiguous.  The window set is separable: window (iy, ix) covers the wh x ww image pixels at
 * origin (ys[iy], xs[ix]); ys [gy] and xs [gx] are HOST int arrays, copied into the kernel arguments (1 <= gy, gx <= LMV_DENSE_SLIDE_MAX_GRID).  The image is
 * H x W, labels [B, H W], B H W < 2^31; h <= wh, w <= ww.  Per image pixel (Y, X) and class k, in fp32:
 *     z_k = (v_1 + v_2 + ... ) / (float)count        over the windows with ys[iy] <= Y < ys[iy] + wh and xs[ix] <= X < xs[ix] + ww, in ascending (iy, ix) order,
 *     v   = the bilinear interpolation of that window's class plane, h x w -> wh x ww (the scales from those sizes), at (Y - ys[iy], X - xs[ix])
 * which is `preds += F.pad(resize(logits))` in window order followed by `preds / count_mat`; the division is carried out.  From z on it is the pixel of
 * lmv_dense_up_loss_fwd; the loss terms are fixed to plain cross-entropy averaged over the valid pixels (w_ce = 1, no alpha, gamma = 0, LMV_DENSE_AVG_VALID).
 *
 * Outputs, each nullable: pred uint8 [B, H W]; mean_logits fp32 [B, K, H, W], contiguous (the stitched map, for callers that average over augmentations
 * themselves); conf int64 [K, K] and meter float64 [2], persistent; stats float32 [LMV_DENSE_STATS_FLOATS(K)].  labels == NULL is PREDICTION ONLY (pred and / or
 * mean_logits; workspace / stats / conf / meter are not touched and may be NULL).  workspace: lmv_dense_slide_workspace_bytes(B, K, H, W).
 *
 * Refused with LMV_ERR_SHAPE and a message that starts "dense_slide", before any launch: everything lmv_dense_up_loss_fwd refuses (with wh x ww in the place of
 * its H x W: h > wh or w > ww is downsampling); gy or gx outside 1 .. 64, null origins; origins that are not strictly increasing; ys[0] != 0 or xs[0] != 0; a last
 * window that does not end at the image's edge (ys[gy - 1] + wh != H, xs[gx - 1] + ww != W); neighbouring origins further apart than the window (an uncovered
 * pixel: mmseg's assert (count_mat == 0).sum() == 0); H < 1, W < 1 or B H W >= 2^31; a window stride smaller than the B images it skips; a misaligned
 * mean_logits; labels == NULL with pred == NULL and mean_logits == NULL.
 * ------------------------------------------------------------------------------------------ */
#define LMV_DENSE_SLIDE_MAX_GRID 64
size_t lmv_dense_slide_workspace_bytes(int B, int K, int H, int W);
int lmv_dense_slide_fwd(const void* logits, int dtype, int64_t window_stride, int64_t batch_stride, int64_t class_stride, int B, int K, int h, int w,
                        const int* ys, int gy, const int* xs, int gx, int wh, int ww, int H, int W, int align_corners, const void* labels, int label_dtype,
                        int64_t ignore_index, void* workspace, size_t workspace_bytes, float* stats, uint8_t* pred, float* mean_logits, int64_t* conf,
                        double* meter, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rotated RoIAlign over a feature pyramid (csrc/rroi.hip; csrc/roi_frame.h has what it shares with csrc/roi.hip): the RoI layer of the reference's three Oriented R-CNN configs
 * (object_detection/configs/obb/oriented_rcnn/: roi_layer=dict(type='RoIAlignRotated', out_size=7, sample_num=2) inside an OBB single-level extractor over
 * featmap_strides=[4, 8, 16, 32] with extend_factor=(1.4, 1.2)), which the reference has as a CUDA extension only (mmdet/ops/roi_align_rotated/src; the CPU source
 * there is the specification of the arithmetic).  An addition to ABI 14: callers detect it by symbol.  One plan launch, one forward launch and one backward launch
 * serve ALL levels; no floating-point atomics, no pre-zeroed buffer, no host synchronisation: two calls agree bit for bit, and every entry point can be captured.
 *
 * Geometry.  rois: fp32 [R, 6], rows (batch_index, cx, cy, w, h, theta), theta in RADIANS (the reference's sources have the degree conversion commented out).
 * levels[l], l < L <= LMV_RROI_MAX_LEVELS: a map [B, C, H_l, W_l] in fp32 or bf16 read through its own ELEMENT strides sb, sc, sh, sw (NCHW, channels-last, a view;
 * all levels share B, C and the dtype), and spatial_scale_l = 1 / stride_l.  out_size (oh, ow), sample_num s in 1 .. LMV_RROI_MAX_SAMPLE_NUM (s = 0, the
 * reference's adaptive grid, is refused), aligned in {0, 1}.  The output is [R, C, oh, ow], contiguous, in the maps' dtype, accumulated in fp32.
 *
 * Level rule (upstream mmdet's map_roi_levels; the OBB extractor's source is not part of the reference tree, so the order below restates upstream):
 *     lvl = clamp(floor(log2(sqrt(w h) / finest_scale + 1e-6)), 0, L - 1)          from the UN-extended w, h
 *     then  w *= extend_w,  h *= extend_h
 * `level_index` (nullable int32 [R]) overrides the rule RoI by RoI (the extension still applies), so either order is expressible.
 *
 * Per RoI at its level, in fp32 with accurate sinf / cosf / log2f / sqrtf:
 *     off = aligned ? 0.5 : 0;   cw = cx scale - off,  ch = cy scale - off;   rw = w scale,  rh = h scale  (aligned == 0: both clamped to >= 1)
 *     bin_h = rh / oh,  bin_w = rw / ow;   sample (ph, pw, iy, ix):   yy = -rh / 2 + ph bin_h + (iy + .5) bin_h / s,   xx = -rw / 2 + pw bin_w + (ix + .5) bin_w / s
 *     y = yy cos(theta) - xx sin(theta) + ch,   x = yy sin(theta) + xx cos(theta) + cw
 *     y < -1, y > H, x < -1 or x > W: the sample contributes 0.  Otherwise y, x are clamped to >= 0; y_low = (int)y; y_low >= H - 1: y_low = y_high = H - 1, y = y_low;
 *     else y_high = y_low + 1 (the same for x); ly = y - y_low, hy = 1 - ly:  w1 = hy hx, w2 = hy lx, w3 = ly hx, w4 = ly lx  on (y_low, x_low), (y_low, x_high),
 *     (y_high, x_low), (y_high, x_high).
 *     out[r, c, ph, pw] = (sum over the bin's s s samples, iy outer, of w1 v1 + w2 v2 + w3 v3 + w4 v4) / (s s)          (empty samples count in the divisor)
 * A RoI whose batch_index truncates to a value outside [0, B) (a NaN batch_index included), whose level_index lies outside [0, L), or whose cx, cy, w, h or theta
 * is not finite (the rule of lmv_roi_plan; the reference lets the NaN through), is not a sample: its output row is zero and it reaches no gradient (the rule of
 * lmv_eval_logits and of the dense label maps).  Finite negative w / h are not validated (that would synchronise): the formulas apply as they are.
 *
 * lmv_rroi_plan -- one launch, one workgroup per RoI.  plan (lmv_rroi_plan_bytes(R, oh, ow, s) bytes, 8-byte aligned): R headers of LMV_RROI_HEADER_BYTES
 * {level, batch, valid, y0, y1, x0, x1, n: the rows / columns of the pixels its samples touch and the number of non-empty samples}, then R x (oh ow s s) sample
 * records of LMV_RROI_SAMPLE_BYTES {y_low | y_high << 16, x_low | x_high << 16, w1 .. w4}; 4.7 KB per RoI at 7 x 7 x 2 x 2.  The `data` and stride fields of
 * `levels` are not read.  The forward and the backward pass take ALL geometry from the plan, which makes the backward the adjoint of the forward to the bit; they
 * must be given the R, L, B, H_l, W_l, oh, ow, s of the plan call (the forward skips a sample whose indices lie outside the map it is given, the backward only ever
 * writes inside its own tile: a foreign plan gives wrong numbers, not a wild access).
 *
 * lmv_rroi_fwd -- one launch, one workgroup per (RoI, 64 channels).  Every output element is written exactly once, rows of invalid RoIs as zeros; no pre-zeroed
 * buffer.  Lanes run along the memory-contiguous axis of each level's strides: along the bins over NCHW maps, along the channels over channels-last maps (whose
 * chunk is transposed through LDS so that the store is contiguous too).
 *
 * lmv_rroi_bwd -- one launch, gather form.  dx[l]: [B, C, H_l, W_l] in `dtype` through its own strides (the layout of the forward's map, or any other);
 * dy: [R, C, oh, ow], contiguous, in `dtype`.  dX is the exact adjoint:  dx[b, c, y, x] = sum of w_k dy[r, c, ph, pw] / (s s)  over the corners that land on (y, x),
 * added in fp32 in a FIXED order (RoI index ascending, then sample order, then corner order w1 .. w4) and rounded once.  A workgroup owns an 8 x 16 pixel tile of
 * one (level, image) and 64 channels, with the accumulator [pixel][channel] in LDS (33 KB, + 260 B per bin and 24 B per sample for the staged dY rows and sample
 * records: 50 KB at 7 x 7 x 2 x 2, at most 122 KB); a wave owns two pixel rows and a lane a channel, so no accumulator is shared.  EVERY element of every level is written exactly once -- zeros where no sample lands, on a level that
 * received no RoI, and at R = 0 -- without a memset and without an atomic.  The result over L levels equals the L single-level results bit for bit.
 * There is no gradient for the RoIs, and no double backward.  The strides of dx[l] must give every element its own address (the library cannot tell an expanded
 * view from its arguments' meaning and does not refuse it: several workgroups would store to one address); lemevit_amd/ops.py refuses such a buffer.
 *
 * Refused with LMV_ERR_SHAPE (a plan buffer that is too small: LMV_ERR_WORKSPACE) and a message that starts "rroi", before any launch: a null level table, a null
 * map, null rois / plan / out / dy with R > 0; L outside 1 .. 5; s outside 1 .. 4; oh < 1, ow < 1, oh ow > LMV_RROI_MAX_BINS or oh ow s s > LMV_RROI_MAX_SAMPLES
 * (what a plan record holds); R < 0, B < 1, C < 1; H_l or W_l outside 1 .. LMV_RROI_MAX_EXTENT (the 16-bit indices); a dtype code other than LMV_F32 / LMV_BF16;
 * R oh ow s s, R C oh ow or B C H_l W_l >= 2^31; a negative stride, a misaligned buffer, an `aligned` other than 0 / 1, finest_scale <= 0.  R = 0 is legal: the
 * plan and the forward launch nothing, the backward writes zeros everywhere.  lmv_rroi_plan_bytes returns 0 for arguments the plan call refuses (and for R = 0).
 * ------------------------------------------------------------------------------------------ */
#define LMV_RROI_MAX_LEVELS 5
#define LMV_RROI_MAX_SAMPLE_NUM 4
#define LMV_RROI_MAX_BINS 256
#define LMV_RROI_MAX_SAMPLES 1024
#define LMV_RROI_MAX_EXTENT 65535
#define LMV_RROI_HEADER_BYTES 32
#define LMV_RROI_SAMPLE_BYTES 24
typedef struct lmv_rroi_level {
  void* data;                 /* the level's map (forward) or gradient (backward); not read by the plan */
  int64_t sb, sc, sh, sw;     /* ELEMENT strides of [B, C, H, W] */
  int32_t H, W;
  float spatial_scale;        /* read by the plan only */
  int32_t _pad;
} lmv_rroi_level;
size_t lmv_rroi_plan_bytes(int R, int oh, int ow, int sample_num);
int lmv_rroi_plan(const float* rois, const int32_t* level_index, int R, const lmv_rroi_level* levels, int L, int B, int oh, int ow, int sample_num, int aligned,
                  float finest_scale, float extend_w, float extend_h, void* plan, size_t plan_bytes, void* stream);
int lmv_rroi_fwd(const void* plan, int R, const lmv_rroi_level* levels, int L, int B, int C, int oh, int ow, int sample_num, int dtype, void* out, void* stream);
int lmv_rroi_bwd(const void* plan, int R, const void* dy, const lmv_rroi_level* dx, int L, int B, int C, int oh, int ow, int sample_num, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rotated IoU and rotated NMS (csrc/obb.hip; the NMS frame is csrc/nms_frame.h): the two remaining custom operators of the reference's Oriented R-CNN configs -- iou_calculator=dict(type='OBBOverlaps')
 * (mmdet/ops/box_iou_rotated: obb_overlaps) in both assigners, and nms_pre / nms_thr=0.8 of the oriented RPN and nms=dict(type='obb_nms', iou_thr=0.1) of the test
 * config (mmdet/ops/nms_rotated: obb_nms, arb_batched_nms).  An addition to ABI 14: callers detect it by symbol.  No host round trip, no atomics: two calls agree bit
 * for bit and every entry point can be captured.
 *
 * Boxes.  fp32 rows (cx, cy, w, h, theta) with a ROW STRIDE in floats (>= 5: a [N, 6] dets tensor is read in place), theta in RADIANS; the width axis is
 * (cos theta, -sin theta), the height axis (sin theta, cos theta) -- the reference's convention.
 *
 * The pair rule (single_box_iou_rotated and the wrapper's "too small" rule), in fp32 with cos / sin evaluated once per box (accurate cosf / sinf):
 *     a box with a non-finite entry, or with w < 0.001 or h < 0.001 (which covers the reference's w h < 1e-14), gives 0 against everything;
 *     I = area of the intersection;   iou = I / (w1 h1 + w2 h2 - I);   iof = I / (w1 h1);   a non-finite quotient gives 0.
 * I is computed from the centre DIFFERENCE (a pair's value does not depend on where it sits in the image) with one box expressed in the other's frame, as the
 * boundary integral of clamp(u, -W, W) dv over the four edges restricted to |v| <= H (csrc/obb.hip): no polygon is built, so exactly degenerate pairs (a duplicate,
 * its theta + pi twin, its theta + pi / 2 twin with w and h swapped, shared edges, containment) are ordinary inputs.  Which box supplies the frame follows a total
 * order on the boxes: iou(p, q) and iou(q, p) agree bit for bit.  Pairs whose bounding circles are apart give exactly 0.
 * Deliberate differences from the reference: (1) its 24-point / Graham-scan routine breaks down on such pairs (0.25 instead of 1.0 for (100, 100, 40, 20, 0.3)
 * against (100, 100, 40, 20, 0.3 + pi) in its float32 CPU build); this one does not.  (2) classes are separated by `groups`, not by adding class_id *
 * (max_coordinate + 1) to the centres in fp32, which moves an IoU by about 1e-5 at 15 classes on a 1024^2 crop.
 *
 * lmv_obb_overlaps -- one launch.  out: fp32 [N, M] (aligned == 0) or [N] from the N pairs (b1[n], b2[n]) (aligned == 1, N == M); every element is written exactly
 * once, stores run along M.  A workgroup owns a 16 x 64 tile and stages the tile's box records in LDS.  N == 0 or M == 0 launches nothing.
 *
 * lmv_obb_nms -- two launches.  order: int64 [N], the STABLE descending sort of the scores (the caller's; boxes, scores and groups are gathered through it, an
 * entry outside [0, N) names no box: that rank is never kept and suppresses nothing).  The launches rank by `order` ALONE -- entry r is rank r; the scores are read
 * only for the candidate rule -- so a permutation that is not the score sort is a legal ranking of the caller's own (tests/test_det_limits_gpu.py runs all three:
 * the default sort passed in, entries that name no box, another permutation).  groups: nullable int32 [N].  A box is a CANDIDATE iff score > score_thr (-inf: every score that is not NaN or -inf) and
 * w >= 0.001 and h >= 0.001 (and all five entries are finite).  Non-candidates are never kept and never suppress.  A kept box suppresses every lower-ranked
 * candidate of its group with IoU > iou_thr (strict, as the reference's CUDA kernel).
 *     mask launch    64 x 64 tiles of the rank-ordered boxes, upper triangle; a wave64 owns rows of the tile, lane j evaluates (row, column j) and the ballot is
 *                    the row's 64-bit word: workspace[rank * ceil(N / 64) + column_block], written for column_block >= row_block (the rest is never read).
 *     reduce launch  one workgroup; thread c keeps word c of the `removed` bit vector.  Per block of 64 ranks the diagonal word is resolved serially and the rows
 *                    of the kept ranks are ORed into `removed` in parallel.  keep: int64 [cap], cap = max_num > 0 ? max_num : N: the original indices of the kept
 *                    boxes in rank order, then -1; count: one int64, the number written (at most max_num).  Every element of both is written exactly once.
 * phases: 3 for both launches; 1 / 2 run one of them alone (probes: the reduce launch then reads a workspace that a mask launch has filled).
 * N == 0 launches nothing: count = 0 and keep = -1 are set by memset nodes.  workspace: lmv_obb_nms_workspace_bytes(N) = N ceil(N / 64) 8 bytes, 8-byte aligned.
 *
 * Refused with LMV_ERR_SHAPE (a workspace that is too small: LMV_ERR_WORKSPACE) and a message that starts "obb", before any launch: null pointers, a row stride
 * below 5, misaligned pointers, negative sizes, more than LMV_OBB_MAX_BOXES boxes on a side (overlaps) or N > LMV_OBB_NMS_MAX (nms), max_num < 0, a NaN threshold,
 * an unknown mode, aligned / phases out of range.  lmv_obb_nms_workspace_bytes returns 0 for an N the call refuses (and for N = 0).
 * ------------------------------------------------------------------------------------------ */
#define LMV_OBB_IOU 0
#define LMV_OBB_IOF 1
#define LMV_OBB_MAX_BOXES 1048576
#define LMV_OBB_NMS_MAX 16384
int lmv_obb_overlaps(const float* boxes1, int stride1, int N, const float* boxes2, int stride2, int M, int mode, int aligned, float* out, void* stream);
size_t lmv_obb_nms_workspace_bytes(int N);
int lmv_obb_nms(const float* boxes, int stride, const float* scores, const int64_t* order, const int32_t* groups, int N, float iou_thr, float score_thr, int max_num,
                int phases, void* workspace, size_t workspace_bytes, int64_t* keep, int64_t* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Horizontal RoIAlign over a feature pyramid, adaptive sampling grid included (csrc/roi.hip; csrc/roi_frame.h has what it shares with csrc/rroi.hip): the RoI layers of the reference's Mask R-CNN config
 * (object_detection/configs/mask_rcnn/: RoIAlign with out_size 7 in the box head and 14 in the mask head, sample_num=0, aligned=True, over featmap_strides
 * [4, 8, 16, 32]), which the reference has as a CUDA extension (mmdet/ops/roi_align/src; cpu/roi_align_v2.cpp there is the specification of the arithmetic).  An
 * addition to ABI 14: callers detect it by symbol.  One plan launch, one forward launch and one backward launch serve ALL levels; no floating-point atomics, no
 * pre-zeroed buffer, no host synchronisation: two calls agree bit for bit, and every entry point can be captured.
 *
 * Geometry.  rois: fp32 [R, 5], rows (batch_index, x1, y1, x2, y2) in image coordinates.  levels[l], l < L <= LMV_ROI_MAX_LEVELS: a map [B, C, H_l, W_l] in fp32 or
 * bf16 read through its own ELEMENT strides (lmv_roi_level is lmv_rroi_level), and spatial_scale_l = 1 / stride_l.  out_size (oh, ow) with oh ow <= LMV_ROI_MAX_BINS;
 * sample_num s in 0 .. LMV_ROI_MAX_GRID, 0 being the reference's default, the adaptive grid.  Only aligned = true exists here (the reference's "v2" arithmetic).
 * The output is [R, C, oh, ow], contiguous, in the maps' dtype, accumulated in fp32.
 *
 * Level rule (upstream mmdet's SingleRoIExtractor.map_roi_levels; its source is not part of the reference tree, so this restates upstream):
 *     lvl = clamp(floor(log2(sqrt((x2 - x1) (y2 - y1)) / finest_scale + 1e-6)), 0, L - 1)          (NaN: level 0)
 * `level_index` (nullable int32 [R]) overrides the rule RoI by RoI.
 *
 * Per RoI at its level, in fp32, operation by operation as roi_align_v2.cpp with aligned = true:
 *     start_w = x1 scale - 0.5,  start_h = y1 scale - 0.5;   roi_w = (x2 scale - 0.5) - start_w,  roi_h likewise;   bin_h = roi_h / oh,  bin_w = roi_w / ow
 *     g_h = s > 0 ? s : ceil(roi_h / oh),   g_w = s > 0 ? s : ceil(roi_w / ow)
 *     sample (ph, pw, iy, ix), iy < g_h, ix < g_w:   y = start_h + ph bin_h + (iy + .5) bin_h / g_h,   x = start_w + pw bin_w + (ix + .5) bin_w / g_w
 *     y < -1, y > H, x < -1 or x > W: the sample contributes 0.  Otherwise y, x <= 0 become 0; y_low = (int)y; y_low >= H - 1: y_low = y_high = H - 1, y = y_low;
 *     else y_high = y_low + 1 (the same for x); ly = y - y_low, hy = 1 - ly: the weights hy hx, hy lx, ly hx, ly lx on the four corners (the rotated operator's rule).
 *     out[r, c, ph, pw] = (sum over the bin's samples) / max(g_h g_w, 1)          (empty samples count in the divisor)
 * y depends on (ph, iy) only and x on (pw, ix) only, and so does the empty rule: with A_y [oh x H], row ph = the sum over iy of (hy at y_low, ly at y_high), and
 * A_x [ow x W] likewise,  out[r, c] = A_y f[c] A_x^T / count  and  dX[c] += A_y^T dY[r, c] A_x / count.  This is what the kernels evaluate; a row of A touches a
 * run of consecutive pixels, and the runs of neighbouring bins share at most two pixels, so a RoI's record is bounded by the map (H_l + 2 oh and W_l + 2 ow
 * weights), whatever the grid, and so is the cost of the forward and the backward pass.
 *
 * Data rules (none can be validated without a synchronisation; the oracle, lemevit_amd.detection.reference_roi_align, applies the same ones).  A RoI is INVALID --
 * its output row is zero and it reaches no gradient -- when its batch_index truncates to a value outside [0, B); its level_index lies outside [0, L); a
 * coordinate is not finite; roi_w < 0 or roi_h < 0 (the reference asserts); or its grid exceeds LMV_ROI_MAX_GRID = 128 on either axis (a RoI of more than 896
 * pixels OF ITS LEVEL at oh = 7; one clipped to a 1333-pixel image on stride 4 needs 48).  A RoI of zero width or height is valid and gives zeros (grid 0, divisor 1).
 *
 * lmv_roi_plan -- one launch, one workgroup per RoI.  plan (lmv_roi_plan_bytes(R, levels, L, oh, ow) bytes, 16-byte aligned): per RoI a record of
 * LMV_ROI_HEADER_BYTES {level, batch, valid, y0, y1, x0, x1: the pixels its samples touch, g_h, g_w, ny, nx: weights in use}, oh + ow bin entries of
 * LMV_ROI_BIN_BYTES {first pixel, run length, offset of the run's weights}, then max_l H_l + 2 oh weights of A_y and max_l W_l + 2 ow of A_x, rounded up to 16 bytes
 * (2.5 KB per RoI at 7 x 7 on the levels of an 800 x 1344 image).  The `data` and stride fields of `levels` are not read.  The forward and the backward pass take ALL
 * geometry from the plan, which makes the backward the adjoint of the forward; they must be given the R, L, B, H_l, W_l, oh, ow of the plan call (a bin entry that
 * does not fit the map or the record it is read with counts as an empty run: a foreign plan gives wrong numbers, not a wild access).
 *
 * lmv_roi_fwd -- one launch, one workgroup per (RoI, 64 channels), the RoI's bin table and weights staged in LDS.  Every output element is written exactly once,
 * rows of invalid RoIs as zeros.  Lanes run along the bins over NCHW maps, along the channels over channels-last maps (transposed through LDS for the store).
 *
 * lmv_roi_bwd -- one launch, gather form.  dx[l]: [B, C, H_l, W_l] in `dtype` through its own strides; dy: [R, C, oh, ow], contiguous, in `dtype`.  A workgroup owns
 * an 8 x 16 pixel tile of one (level, image) and 64 channels with the accumulator in LDS; per RoI that reaches the tile it stages dY / count and the tile's slices
 * of A_y and A_x, and a pixel adds sum over (ph, pw) of A_y[ph, y] A_x[pw, x] dY[ph, pw] in a FIXED order (RoI index ascending, ph, pw).  EVERY element of every
 * level is written exactly once -- zeros where no sample lands, on a level that received no RoI, and at R = 0.  The result over L levels equals the L
 * single-level results bit for bit.  No gradient for the RoIs, no double backward.  The strides of dx[l] must give every element its own address
 * (lemevit_amd/ops.py refuses a buffer that does not).
 *
 * Refused with LMV_ERR_SHAPE (a plan buffer that is too small: LMV_ERR_WORKSPACE) and a message that starts "roi", before any launch: a null level table, a null
 * map, null rois / plan / out / dy with R > 0; L outside 1 .. 5; s outside 0 .. LMV_ROI_MAX_GRID; oh < 1, ow < 1, oh ow > LMV_ROI_MAX_BINS; R < 0, B < 1, C < 1; H_l or
 * W_l outside 1 .. LMV_ROI_MAX_EXTENT; a dtype code other than LMV_F32 / LMV_BF16; R C oh ow or B C H_l W_l >= 2^31; a negative stride, a misaligned buffer,
 * finest_scale <= 0; a forward whose staged record and tile exceed the 160 KB of LDS.  R = 0 is legal: the plan and the forward launch nothing, the backward writes
 * zeros everywhere.  lmv_roi_plan_bytes returns 0 for arguments the plan call refuses (and for R = 0).
 * ------------------------------------------------------------------------------------------ */
#define LMV_ROI_MAX_LEVELS 5
#define LMV_ROI_MAX_GRID 128
#define LMV_ROI_MAX_BINS 256
#define LMV_ROI_MAX_EXTENT 8192
#define LMV_ROI_HEADER_BYTES 48
#define LMV_ROI_BIN_BYTES 16
typedef lmv_rroi_level lmv_roi_level;
size_t lmv_roi_plan_bytes(int R, const lmv_roi_level* levels, int L, int oh, int ow);
int lmv_roi_plan(const float* rois, const int32_t* level_index, int R, const lmv_roi_level* levels, int L, int B, int oh, int ow, int sample_num, float finest_scale,
                 void* plan, size_t plan_bytes, void* stream);
int lmv_roi_fwd(const void* plan, int R, const lmv_roi_level* levels, int L, int B, int C, int oh, int ow, int dtype, void* out, void* stream);
int lmv_roi_bwd(const void* plan, int R, const void* dy, const lmv_roi_level* dx, int L, int B, int C, int oh, int ow, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Horizontal NMS (csrc/nms.hip; csrc/nms_frame.h has what it shares with csrc/obb.hip): mmdet/ops/nms (nms, batched_nms) of the reference's Mask R-CNN config -- the RPN proposals (nms_thr 0.7) and the test-time
 * multiclass NMS (iou_thr 0.5, score_thr 0.05, max_per_img 100).  An addition to ABI 14: callers detect it by symbol.  The interface and the two launches are
 * those of lmv_obb_nms above (order: the caller's STABLE descending sort; groups; candidates; keep padded with -1; count; phases; nothing synchronised; capturable),
 * with boxes fp32 rows (x1, y1, x2, y2) read in place through a ROW STRIDE >= 4 floats and the pair rule of cpu/nms_cpu.cpp in fp32, operation by operation:
 *     area = (x2 - x1)(y2 - y1);   inter = max(0, min(x2) - max(x1)) max(0, min(y2) - max(y1));   suppress iff inter / (area_i + area_j - inter) > iou_thr
 * The comparison is strict, and a NaN quotient suppresses nothing: two zero-area duplicates are both kept, as in the reference.  A box is a CANDIDATE iff
 * score > score_thr (-inf: every score that is not NaN or -inf) and its four coordinates are finite.  Deliberate difference from the reference: classes are
 * separated by `groups` (exact), not by adding class_id (max_coordinate + 1) to the coordinates in fp32.
 * Refused with LMV_ERR_SHAPE (LMV_ERR_WORKSPACE) and a message that starts "nms", before any launch: what lmv_obb_nms refuses, with N <= LMV_NMS_MAX.
 * ------------------------------------------------------------------------------------------ */
#define LMV_NMS_MAX 16384
size_t lmv_nms_workspace_bytes(int N);
int lmv_nms(const float* boxes, int stride, const float* scores, const int64_t* order, const int32_t* groups, int N, float iou_thr, float score_thr, int max_num,
            int phases, void* workspace, size_t workspace_bytes, int64_t* keep, int64_t* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Max-IoU target assignment without the [boxes x ground truths] matrix, and horizontal overlaps (csrc/assign.hip): what the reference's Oriented R-CNN configs do
 * twice per image with MaxIoUAssigner -- at the RPN on horizontal boxes (0.7 / 0.3 / 0.3, match_low_quality, gpu_assign_thr=200) and at the R-CNN head with
 * iou_calculator=dict(type='OBBOverlaps') (0.5 / 0.5 / 0.5, no low-quality matches).  The sources of MaxIoUAssigner and bbox_overlaps are NOT part of the reference
 * tree (only mmdet/ops and the backbone are): the rules below restate upstream mmdet 2.x.  An addition to ABI 14: callers detect it by symbol.  No host round trip,
 * no floating-point atomics (integer maxima only, which do not depend on arrival order): two calls agree bit for bit, and every entry point can be captured.
 *
 * lmv_bbox_overlaps -- the horizontal counterpart of lmv_obb_overlaps, with its arguments and properties: boxes fp32 rows (x1, y1, x2, y2) read in place through a
 * ROW STRIDE >= 4 floats; out fp32 [N, M] (aligned == 0) or [N] from the pairs (b1[n], b2[n]) (aligned == 1, N == M); modes LMV_OBB_IOU / LMV_OBB_IOF; one launch,
 * every element written exactly once, stores run along M, N == 0 or M == 0 launches nothing.  The pair rule (upstream bbox_overlaps, which has no "+ 1"), in fp32:
 *     w = max(min(x2, x2') - max(x1, x1'), 0),  h likewise;   I = w h;   a = (x2 - x1)(y2 - y1)
 *     iou = I / max(a + a' - I, 1e-6);   iof = I / max(a, 1e-6)
 * A box with a non-finite coordinate gives 0 against everything (the data rule of the rotated operator), and so does a non-finite quotient.  iou(p, q) and iou(q, p)
 * agree bit for bit.
 *
 * lmv_max_iou_assign -- at most two launches and one memset node; the [N, G] values are never stored.  kind: LMV_ASSIGN_HORIZONTAL (k = 4 columns, the pair rule
 * above) or LMV_ASSIGN_ROTATED (k = 5, the pair function of lmv_obb_overlaps: v[j, n] below equals lmv_obb_overlaps(boxes, gts)[n, j] bit for bit, pairs whose
 * bounding circles are apart are exactly 0).
 *     boxes        fp32 [N, k] shared by all images (box_batch_stride == 0) or [B, N, k] (box_batch_stride: floats from one image's boxes to the next's), rows read
 *                  through box_stride >= k
 *     gts          fp32 [B, Gmax, k], rows through gt_stride >= k (an image's rows are Gmax gt_stride floats apart)
 *     gt_counts    nullable int32 [B] ON THE DEVICE: the valid rows per image, clamped to 0 .. Gmax by the kernel; null: Gmax everywhere.  Rows past the count are
 *                  never read
 *     gt_labels    nullable int64 [B, Gmax];   ignore: nullable uint8 [B, N] (non-zero: the box is ignored)
 *     gt_inds      int64 [B, N];   max_overlaps fp32 [B, N];   labels (nullable) int64 [B, N], written only when gt_labels is given (with Gmax = 0 gt_labels may
 *                  be null: every label is then -1).  Every element is written exactly once.
 * Nothing is synchronised and every size the host needs is an argument: capturable after one eager call per shape.
 * Rules, for one image with g valid ground truths and v[j, n] the pair value (IoU) of ground truth j and box n:
 *     an ignored box gets gt_inds = -1, max_overlaps = -1, labels = -1 and takes no part in any ground truth's maximum (upstream's ignore_iof_thr outcome, and
 *         allowed_border filtering without a boolean-index copy); deliberately also when g = 0
 *     g = 0: every other box gets gt_inds = 0, max_overlaps = 0
 *     otherwise max_overlaps[n] = max_j v[j, n], argmax[n] = the LOWEST j that attains it;   gt_max[j] = max over the boxes n that are not ignored of v[j, n]
 *     base rule: gt_inds[n] = argmax[n] + 1 if max_overlaps[n] >= pos_iou_thr, else 0 if neg_lo <= max_overlaps[n] < neg_hi, else -1  (upstream's float
 *         neg_iou_thr is neg_lo = 0, neg_hi = neg_iou_thr; its tuple form gives both)
 *     match_low_quality overrides it as upstream's loop over j ascending does: with gt_max_assign_all = 1, gt_inds[n] = the LARGEST j + 1 with
 *         gt_max[j] >= min_pos_iou and v[j, n] == gt_max[j] (fp32 equality of the kernel's own values); with gt_max_assign_all = 0, ground truth j is held by the
 *         lowest n that attains gt_max[j], and a box takes the largest j + 1 it holds.  Upstream's literal consequence stays: with min_pos_iou <= 0 a ground truth
 *         that overlaps nothing matches every box at value 0 (gt_max_assign_all = 1) or the image's first box that is not ignored (= 0)
 *     labels[n] = gt_labels[gt_inds[n] - 1] where gt_inds[n] > 0, else -1
 * Mapping: a workgroup owns 256 boxes of one image, a record per thread, and stages the ground-truth records through LDS in chunks of LMV_ASSIGN_GT_CHUNK.
 * Launch 1 (only with match_low_quality): IoU >= 0, so its bit pattern orders as an unsigned integer; lanes with v > 0 issue an LDS integer max on the key
 * (bits of v << 32) | ~n, the workgroup one global integer atomicMax per ground truth with a non-zero key, into a table [B, Gmax + 1] of 8-byte keys that a memset
 * node zeroed (workspace: lmv_max_iou_assign_workspace_bytes(B, Gmax) = B (Gmax + 1) 8 bytes, 8-byte aligned, always required).  Launch 2 recomputes v with the same
 * function and writes every output.
 * Refused with LMV_ERR_SHAPE (a workspace that is too small or null: LMV_ERR_WORKSPACE) and a message that starts "assign", before any launch: null pointers with
 * non-zero sizes, gt_labels without labels or labels without gt_labels (Gmax > 0), a row stride below k, B outside 1 .. LMV_ASSIGN_MAX_BATCH, negative sizes, N > LMV_OBB_MAX_BOXES, Gmax > LMV_ASSIGN_MAX_GT, a NaN threshold,
 * neg_lo > neg_hi, an unknown kind, flags other than 0 / 1, misaligned buffers.  lmv_bbox_overlaps refuses what lmv_obb_overlaps refuses (row stride below 4), with
 * a message that starts "bbox_overlaps".  lmv_max_iou_assign_workspace_bytes returns 0 for a B or Gmax the call refuses.
 * ------------------------------------------------------------------------------------------ */
#define LMV_ASSIGN_HORIZONTAL 0
#define LMV_ASSIGN_ROTATED 1
#define LMV_ASSIGN_GT_CHUNK 64
#define LMV_ASSIGN_MAX_GT 16384
#define LMV_ASSIGN_MAX_BATCH 4096
int lmv_bbox_overlaps(const float* boxes1, int stride1, int N, const float* boxes2, int stride2, int M, int mode, int aligned, float* out, void* stream);
size_t lmv_max_iou_assign_workspace_bytes(int B, int Gmax);
int lmv_max_iou_assign(int kind, const float* boxes, int box_stride, int64_t box_batch_stride, int N, const float* gts, int gt_stride, int B, int Gmax,
                       const int32_t* gt_counts, const int64_t* gt_labels, const uint8_t* ignore, float pos_iou_thr, float neg_lo, float neg_hi, float min_pos_iou,
                       int match_low_quality, int gt_max_assign_all, void* workspace, size_t workspace_bytes, int64_t* gt_inds, float* max_overlaps, int64_t* labels,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Box coders of the Oriented R-CNN configs (csrc/coder.hip): MidpointOffsetCoder (the RPN head: anchors (x1, y1, x2, y2), ground truths / proposals
 * (cx, cy, w, h, theta), D = 6 deltas, target_stds (1, 1, 1, 1, 0.5, 0.5)) and OBB2OBBDeltaXYWHTCoder (the R-CNN head: both sides (cx, cy, w, h, theta), D = 5 deltas,
 * target_stds (0.1, 0.1, 0.2, 0.2, 0.1)).  Their sources are NOT part of the reference tree (only their names in the configs are): the rules below restate upstream
 * (OBBDetection on mmdet 2.x) and are the specification.  An addition to ABI 14: callers detect it by symbol.  One launch per call, one thread per output row, 256
 * threads per workgroup, operands read in place through their strides, no atomics, nothing synchronised, capturable; every output element is written exactly once.
 * There is ONE device function per rule and every entry point inlines it (fp contraction off): the plain and the gathering form of an operation agree bit for bit,
 * and so do two calls.
 *
 * kind: LMV_CODER_MIDPOINT (k = 4 box columns, D = 6) or LMV_CODER_OBB2OBB (k = 5, D = 5).  means / stds: HOST arrays of D floats, read during the call and passed
 * to the kernel by value (nothing of them is read later: a captured call keeps the values it was captured with).
 *
 * Conventions (theta in radians, fp32 throughout, IEEE arithmetic):
 *     regular_theta(t) = t + pi/2 - pi floor((t + pi/2) / pi) - pi/2          a floored modulo: the result is in [-pi/2, pi/2)
 *     regular_obb(x, y, w, h, t): if w > h keep (w, h, t), else (h, w, t + pi/2); then t = regular_theta(t)
 *     corners of (cx, cy, w, h, t) with c = cos t, s = sin t, v1 = (w/2 c, -w/2 s), v2 = (-h/2 s, -h/2 c):
 *         p1 = ctr + v1 + v2,  p2 = ctr + v1 - v2,  p3 = ctr - v1 - v2,  p4 = ctr - v1 + v2
 *     hull: ctr -+ (|w/2 c| + |h/2 s|, |w/2 s| + |h/2 c|)
 *     normalisation: encode ends with (delta - mean) / std, decode begins with delta std + mean
 *     size clamp: decode clamps dw, dh to +-|log(wh_ratio_clip)| (upstream's default wh_ratio_clip = 16 / 1000)
 * Midpoint encode (anchor (x1, y1, x2, y2), ground truth obb): px, py the anchor's centre, pw, ph its sides; gx, gy, gw, gh the centre and sides of the ground
 *     truth's hull; ga = max{ x_i : |y_i - min_j y_j| <= 0.1 } over the four corners (the x of the top vertex; the rightmost of two on a level top edge);
 *     gb = max{ y_i : |x_i - max_j x_j| <= 0.1 };   deltas = ((gx - px)/pw, (gy - py)/ph, log(gw/pw), log(gh/ph), (ga - gx)/gw, (gb - gy)/gh)
 * Midpoint decode: gw = pw exp(dw), gh = ph exp(dh), gx = px + pw dx, gy = py + ph dy;  x1, y1, x2, y2 = gx -+ gw/2, gy -+ gh/2;  da, db clamped to [-0.5, 0.5];
 *     the four vertices (gx + da gw, y1), (x2, gy + db gh), (gx - da gw, y2), (x1, gy - db gh); each is moved along its ray from (gx, gy) to the largest of the four
 *     distances to (gx, gy) (the parallelogram becomes a rectangle); theta = atan2(-(y_2 - y_1), x_2 - x_1) on the first two moved vertices; the centre is the mean
 *     of the four; with c = cos theta, s = sin theta each centred vertex (ux, uy) goes to (ux c - uy s, ux s + uy c); w, h are the extents (max - min) of the first
 *     and second rotated coordinate; the result is regular_obb(centre, w, h, theta).  Rotated proposals are not clipped to an image shape.
 * OBB2OBB encode (proposal p, ground truth g): d1 = regular_theta(gt - pt), d2 = regular_theta(gt - pt + pi/2); if |d1| < |d2| then (gw', gh', dt) = (gw, gh, d1)
 *     else (gh, gw, d2); with c = cos(-pt), s = sin(-pt): dx = (c (gx - px) + s (gy - py)) / pw, dy = (-s (gx - px) + c (gy - py)) / ph, dw = log(gw'/pw),
 *     dh = log(gh'/ph);   deltas = (dx, dy, dw, dh, dt)
 * OBB2OBB decode: gx = dx pw c - dy ph s + px, gy = dx pw s + dy ph c + py (the same c, s), gw = pw exp(dw), gh = ph exp(dh), gt = regular_theta(dt + pt); the
 *     result is regular_obb(gx, gy, gw, gh, gt)
 * Data rules: a degenerate anchor or a non-finite input gives whatever the formulas give (inf / NaN), as upstream; nothing traps, nothing is read out of bounds.
 * Only the non-live rows of the encode are defined to be zero.
 *
 * lmv_box_encode -- targets and weights of B images in one launch.
 *     boxes        fp32 [N, k] shared by all images (box_batch_stride == 0) or [B, N, k] (box_batch_stride: floats between the images' box sets), rows through
 *                  box_stride >= k
 *     gts          fp32 [B, Gmax, 5], rows through gt_stride >= 5 (an image's rows are Gmax gt_stride floats apart)
 *     gt_counts    nullable int32 [B] ON THE DEVICE, clamped to 0 .. Gmax by the kernel; null: Gmax everywhere.  No row at or past the count is ever read
 *     gt_inds      nullable int64 [B, N] (what lmv_max_iou_assign writes): row (b, n) is encoded against gts[b, gt_inds[b, n] - 1].  Null: the ALIGNED form, row n
 *                  is paired with ground-truth row n (as if gt_inds[b, n] = n + 1; needs Gmax == N)
 *     sampled      nullable uint8 [B, N]: a sampler's mask
 *     targets      fp32 [B, N, D];   weights fp32 [B, N]
 * Row (b, n) is LIVE if, and only if, 1 <= gt_inds[b, n] <= count[b] and (sampled given) sampled[b, n] != 0: its weight is 1 and its D targets the normalised
 * deltas.  Every other row has weight 0 and D targets of exactly +0.0.
 *
 * lmv_box_decode -- boxes fp32 [N, k] through box_stride; deltas fp32 [N, D C] through delta_stride >= D C floats per row, C >= 1 delta sets per row (upstream's
 * 0::D striding, class-specific regression: set c of row n is deltas[n, c D .. c D + D - 1] and is decoded against box n); out fp32 [N, 5 C] contiguous.  One
 * thread per (row, set).
 *
 * lmv_box_decode_map -- the proposals of one level from a head's regression output read in place: map fp32 [A D, H, W] with arbitrary channel / row / column
 * strides (in floats, map_stride_c / _h / _w), index int64 [K] on the device.  Row r = (h W + w) A + a of the level has delta d at channel a D + d, position (h, w)
 * -- the order of permute(1, 2, 0).reshape(-1, D).  Output row i decodes row r = index[i]: out fp32 [K, 5] contiguous.  boxes: [K, k], row i (gathered == 1: already
 * gathered), or [H W A, k], row index[i] (gathered == 0).  An index outside 0 .. H W A - 1 writes a row of zeros and reads nothing.
 *
 * Limits: N, K (and Gmax) <= LMV_OBB_MAX_BOXES, B in 1 .. LMV_ASSIGN_MAX_BATCH, 1 <= C <= LMV_CODER_MAX_SETS, H W A <= 2^31 - 1.
 * Refused with LMV_ERR_SHAPE and a message that starts "box_encode" / "box_decode" / "box_decode_map", before any launch: an unknown kind, sizes outside the limits,
 * negative sizes, row strides below k / 5 / D C, a negative batch stride, the aligned form with Gmax != N, null means / stds, a NaN mean or std, a wh_ratio_clip
 * that is not a positive finite number, a gathered flag other than 0 / 1, null pointers with non-zero sizes, misaligned buffers.  N == 0 / K == 0 launches nothing.
 * ------------------------------------------------------------------------------------------ */
#define LMV_CODER_MIDPOINT 0
#define LMV_CODER_OBB2OBB 1
#define LMV_CODER_MAX_SETS 128
int lmv_box_encode(int kind, const float* boxes, int box_stride, int64_t box_batch_stride, int N, const float* gts, int gt_stride, int B, int Gmax,
                   const int32_t* gt_counts, const int64_t* gt_inds, const uint8_t* sampled, const float* means, const float* stds, float* targets, float* weights,
                   void* stream);
int lmv_box_decode(int kind, const float* boxes, int box_stride, const float* deltas, int64_t delta_stride, int N, int C, const float* means, const float* stds,
                   float wh_ratio_clip, float* out, void* stream);
int lmv_box_decode_map(int kind, const float* boxes, int box_stride, int gathered, const float* map, int A, int H, int W, int64_t map_stride_c, int64_t map_stride_h,
                       int64_t map_stride_w, const int64_t* index, int K, const float* means, const float* stds, float wh_ratio_clip, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The samplers of both heads of the Oriented R-CNN configs (csrc/sampler.hip): train_cfg.rpn.sampler = RandomSampler(num=256, pos_fraction=0.5, neg_pos_ub=-1,
 * add_gt_as_proposals=False) over the anchors and train_cfg.rcnn.sampler = OBBRandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
 * over the proposals plus the ground truths -- what sits between lmv_max_iou_assign and lmv_box_encode.  Their sources are NOT part of the reference tree (only
 * their names in the configs are): the rules below restate upstream mmdet 2.x and are the specification.  An addition to ABI 14: callers detect it by symbol.  No
 * host round trip, no floating-point atomics (integer counters only; no value depends on the order in which an atomic lands): two calls agree bit for bit, the
 * number of launches is fixed by the arguments, and both entry points can be captured.
 *
 * lmv_random_sample -- B images; two launches and one memset node.
 *   Element space of one image: M = (add_gt ? Gmax : 0) + N.  With add_gt, element e < Gmax is ground truth e: a candidate only if e < count[b], and then a
 *     POSITIVE with assigned index e + 1; element Gmax + n is box n.  Without add_gt element n is box n (Gmax and gt_counts are not used).  This is upstream's
 *     cat([gt_bboxes, bboxes]) + AssignResult.add_gt_ without the copies; the padding rows (count[b] <= e < Gmax) are never candidates.
 *   Classes, from gt_inds int64 [B, N] (what lmv_max_iou_assign writes; nullable with N == 0): box n is positive if gt_inds > 0, negative if gt_inds == 0; anything
 *     else (e.g. -1, ignored) is never sampled.  gt_counts: nullable int32 [B] ON THE DEVICE, clamped to 0 .. Gmax by the kernel; null: Gmax everywhere.
 *   Quotas (upstream's arithmetic), with c_pos / c_neg the candidates of the image:  P = int(num * pos_fraction) is computed by the HOST and passed as an integer;
 *     n_pos = min(c_pos, P);   E = num - n_pos;   if neg_pos_ub >= 0: E = min(E, (int)floor((double)neg_pos_ub * max(1, n_pos)));   n_neg = min(c_neg, E)
 *     (neg_pos_ub is a float; negative: no bound; +inf: no bound either).
 *   Choice: among the c candidates of a class the k = n_pos / n_neg chosen are those with the smallest 64-bit word (priority << 32) | e -- the smallest 32-bit
 *     priority first, the lower element index on a tie; with c <= k all are taken.  The priority of element e of image b is
 *       (a) priorities[b, e], a nullable uint32 [B, M] supplied by the caller (a test hook, and how a caller builds a score-ordered or IoU-balanced sampler), or
 *       (b) with priorities null: word r0 of Philox4x32-10 (the generator of lmv_augment_images above) with the counter (e, b, 0, 0x53414d50) and the key words
 *           (key[0], key[1]), key a uint32 [2] in DEVICE memory.  The running kernel reads the key: a captured call samples anew at every replay once the key has
 *           been rewritten.  Every k-subset of a class is equally likely up to the generator's quality (ties of 32-bit priorities fall to the lower index).
 *     With both given, priorities is used and the key is not read.
 *   Outputs -- every element is written exactly once, on every call (nothing is assumed about what the buffers hold):
 *     inds      int64 [B, num]: the chosen positives in ascending element order, then the chosen negatives in ascending element order, then -1
 *     num_pos, num_neg   int32 [B]
 *     mask      nullable uint8 [B, M]: 0 not sampled, 1 sampled positive, 2 sampled negative.  Without add_gt it is exactly what lmv_box_encode takes as `sampled`,
 *               and mask != 0 is the RPN's label_weights.
 *   Upstream draws a torch.randperm; the subset here is as uniform, but not the same draw, and inds is ordered.
 *   Workspace: lmv_random_sample_workspace_bytes(B, M) = B (2048 + 5 ceil16(M)) bytes, 16-byte aligned, always required; 0 for a B or M the call refuses.  It
 *     holds the [B, 2, 256] histograms of the priority's top byte per class and, per element, the priority and a class byte (rows padded to 16 elements).
 *   Mapping: launch 1, grid-wide over 1024 elements x B, classifies, computes the priorities, stores both and counts the top bytes in LDS, flushed with integer
 *     global atomics into the table the memset node zeroed; the bin totals are c_pos / c_neg.  Launch 2, one workgroup of 1024 threads per image, computes the
 *     quotas, finds for an oversubscribed class only (c > k > 0) the threshold priority t and the number of elements equal to t to take (lowest index first) with
 *     three more 8-bit radix-select sweeps over the workspace, and writes every output in one ordered sweep with block prefix scans.
 *
 * lmv_sample_gather -- the R-CNN head's inputs from inds in one launch, one thread per output row (upstream's bbox2roi, pos_assigned_gt_inds, pos_gt_labels).
 *     inds         int64 [B, num] (what lmv_random_sample writes) into the element space above (add_gt, Gmax, N as in that call)
 *     boxes        fp32 [N, k] shared by all images (box_batch_stride == 0) or [B, N, k], rows through box_stride >= k;  k = 4 or 5
 *     gts          fp32 [B, Gmax, k], rows through gt_stride >= k; read only with add_gt, and never at or past count[b]
 *     gt_inds      int64 [B, N];   gt_labels nullable int64 [B, Gmax];   gt_counts as above;   bg_label: the label of a negative
 *     rois         fp32 [B, num, 1 + k]: row (b, s) = (b, the box's k columns)
 *     s_gt_inds    int64 [B, num]: the assigned index j + 1 (a ground-truth element e: e + 1), 0 for a negative
 *     s_labels     nullable int64 [B, num]: gt_labels[b, j] (-1 without gt_labels or with j >= Gmax), bg_label for a negative
 *   A PADDING row -- inds = -1, or any index that names no candidate: outside 0 .. M - 1, a ground-truth element at or past count[b], a box with gt_inds < 0 --
 *   reads nothing and is (-1, 0 ...) with s_gt_inds = -1 and s_labels = -1: lmv_rroi_fwd / lmv_roi_fwd give a zero row for batch index -1, and lmv_box_encode
 *   with boxes = rois + 1 (box_stride = 1 + k), gt_inds = s_gt_inds gives weight 0.  Every output element is written exactly once.
 *
 * Limits: M <= LMV_OBB_MAX_BOXES, 1 <= num <= LMV_SAMPLE_MAX_NUM, 0 <= P <= num, B in 1 .. LMV_ASSIGN_MAX_BATCH.
 * Refused with LMV_ERR_SHAPE (a workspace that is too small or null: LMV_ERR_WORKSPACE) and a message that starts "random_sample" / "sample_gather", before any
 * launch: sizes outside the limits, negative sizes, add_gt other than 0 / 1, a NaN neg_pos_ub, both key and priorities null, k other than 4 / 5, a row stride below
 * k, a negative batch stride, s_labels without gt_labels (Gmax > 0), null pointers with non-zero sizes, misaligned buffers.  lmv_random_sample with M == 0
 * launches nothing and writes nothing.
 * ------------------------------------------------------------------------------------------ */
#define LMV_SAMPLE_MAX_NUM 16384
size_t lmv_random_sample_workspace_bytes(int B, int M);
int lmv_random_sample(const int64_t* gt_inds, int N, int B, const int32_t* gt_counts, int Gmax, int add_gt, int num, int P, float neg_pos_ub,
                      const uint32_t* priorities, const uint32_t* key, void* workspace, size_t workspace_bytes, int64_t* inds, int32_t* num_pos, int32_t* num_neg,
                      uint8_t* mask, void* stream);
int lmv_sample_gather(const int64_t* inds, int num, const float* boxes, int box_stride, int64_t box_batch_stride, int N, int k, const float* gts, int gt_stride,
                      int B, int Gmax, const int64_t* gt_inds, const int64_t* gt_labels, const int32_t* gt_counts, int add_gt, int64_t bg_label, float* rois,
                      int64_t* s_gt_inds, int64_t* s_labels, void* stream);

/* ------------------------------------------------------------------------------------------
 * The head losses of the Oriented R-CNN configs (csrc/headloss.hip), forward and backward -- what follows lmv_random_sample / lmv_sample_gather in a training step.
 * RPN head: CrossEntropyLoss(use_sigmoid=True) + SmoothL1Loss(beta=1/9); R-CNN head: CrossEntropyLoss(use_sigmoid=False) + SmoothL1Loss(beta=1.0) with
 * reg_class_agnostic=True, num_classes=15.  Their sources are NOT part of the reference tree (only their names in the configs are): the rules below restate upstream
 * (OBBDetection on mmdet 2.x) and are the specification.  An addition to ABI 14: callers detect it by symbol.
 *
 * Common to the four entry points: fp32 arithmetic, exponentials taken with the maximum subtracted, fp contraction off; NO floating-point atomics; every summation
 * order is fixed by the arguments (two calls agree bit for bit); nothing is synchronised with the host and every call can be captured; every output element is
 * written exactly once (a zero is +0.0) and no buffer needs pre-zeroing.  Maps and predictions are fp32 or bf16 (`dtype`: LMV_F32 / LMV_BF16, one for all of a
 * call), read in place through ELEMENT strides; gradients are written in that dtype through their own strides.  The regression targets are never stored: a live row
 * computes its target with the coder's device rule (the function lmv_box_encode inlines), so it has the bits that call would have written.
 * means / stds: HOST arrays of D floats, passed by value as in lmv_box_encode.  beta, w_cls, w_bbox: the smooth-L1 threshold and the two loss weights.
 *     smoothL1(d) = 0.5 d^2 / beta if |d| < beta, else |d| - 0.5 beta;   its derivative: d / beta if |d| < beta, else sign(d)
 *
 * lmv_rpn_loss_fwd / lmv_rpn_loss_bwd -- B images, L <= LMV_RPN_LOSS_MAX_LEVELS levels of (H_l, W_l) positions, A anchors per position.
 *   Element space of one image: anchor r = (h W_l + w) A + a of level l is element off_l + r, off_l = sum_{l' < l} H_l' W_l' A -- the row order of
 *     lmv_box_decode_map and of upstream's permute(0, 2, 3, 1).reshape; N = sum_l H_l W_l A.
 *   levels       HOST table of L lmv_rpn_loss_level, read during the call: cls the class map [B, A, H, W] (channel a: the logit of anchor a), reg the regression
 *                map [B, A D, H, W] (channel a D + d: delta d of anchor a), each with its four strides (batch, channel, row, column); dcls / dreg and their strides:
 *                the two gradient maps, used by the backward call only
 *   mask         uint8 [B, N], what lmv_random_sample writes (add_gt = 0): 0 not sampled, 1 sampled positive, anything else sampled negative
 *   anchors      fp32 [N, 4] shared by all images (anchor_batch_stride == 0) or [B, N, 4], rows through anchor_stride >= 4
 *   gts          fp32 [B, Gmax, 5] through gt_stride >= 5;  gt_counts nullable int32 [B] ON THE DEVICE, clamped to 0 .. Gmax by the kernel (null: Gmax)
 *   gt_inds      int64 [B, N], what lmv_max_iou_assign writes
 *   kind         LMV_CODER_MIDPOINT (D = 6); nothing else is wired up
 *   Rules: a sampled anchor (mask != 0) with logit z and t = [mask == 1] has the class term max(z, 0) - z t + log1p(exp(-|z|)) (weight 1).  A row is LIVE for
 *     the regression if mask == 1 and 1 <= gt_inds <= count[b] (the rule of lmv_box_encode); its term is sum_d smoothL1(reg_d - target_d), target = the midpoint
 *     encode of the anchor against gts[b, gt_inds - 1].  With n_pos_b / n_neg_b the number of mask bytes == 1 / other non-zero bytes of image b:
 *         avg = sum_b (max(n_pos_b, 1) + max(n_neg_b, 1))          (upstream's num_total_samples)
 *         loss_cls[l] = w_cls sum_{level l} class terms / avg;   loss_bbox[l] = w_bbox sum_{level l} regression terms / avg
 *   stats        fp32 [LMV_RPN_LOSS_STATS(L) = 2 L + 3]: loss_cls[L], loss_bbox[L], n_pos, n_neg (all images), 1 / avg
 *   Forward: two launches.  The sweep gives one wave to every 1024 consecutive mask bytes of an image, 16 bytes per lane -- one 16-byte load when N % 16 == 0 and
 *     the mask is 16-byte aligned, byte loads otherwise, the same arithmetic in the same order either way -- and only a non-zero byte does work; a lane adds its
 *     terms in element order, the wave adds its lanes with a fixed butterfly and stores one partial row.  One reduce workgroup adds the rows in double in a fixed
 *     order.  workspace: lmv_rpn_loss_workspace_bytes(B, N) = 48 B ceil(N / 1024) bytes, 16-byte aligned; 0 for a B or N the call refuses.
 *   Backward: one launch, one thread per (image, anchor).  It re-reads the mask, the maps and the assignment, reads 1 / avg from `stats` (what the forward call
 *     wrote) and gout, a nullable DEVICE float [2 L] -- the upstream gradient of loss_cls[0 .. L-1], loss_bbox[0 .. L-1]; null: ones -- and writes EVERY element of
 *     the 2 L gradient maps once: dcls = gout[l] w_cls (sigmoid(z) - t) / avg at a sampled anchor, dreg = gout[L + l] w_bbox smoothL1'(reg - target) / avg on a
 *     live row, +0.0 everywhere else (also on a level without a sampled anchor).  A gradient map must not alias itself (injective strides).
 *
 * lmv_rcnn_loss_fwd / lmv_rcnn_loss_bwd -- R sampled RoIs of B images, K classes plus the background class K.
 *   cls_score    [R, K + 1] through cls_stride >= K + 1 elements;   bbox_pred [R, D C] through bbox_stride >= D C, C = 1 (class-agnostic) or C = K
 *   rois         fp32 [R, 1 + 5] through roi_stride >= 6, what lmv_sample_gather writes: column 0 is the image index b; b outside 0 .. B - 1 (or NaN): padding
 *   s_gt_inds, s_labels   int64 [R];   gts, gt_counts as above;   kind LMV_CODER_OBB2OBB (D = 5); nothing else is wired up
 *   Rules: a row is VALID if 0 <= label <= K and its b is in range, LIVE if valid, label < K and 1 <= s_gt_inds <= count[b]; n_valid = the number of valid rows.
 *         loss_cls  = w_cls sum_valid (log sum_c exp(z_c - max z) - (z_label - max z)) / max(n_valid, 1)
 *         loss_bbox = w_bbox sum_live sum_d smoothL1(bbox_pred[set D + d] - target_d) / n_valid, 0 if n_valid == 0; set = 0 if C == 1, else the label; target =
 *                     the OBB2OBB encode of rois[r, 1 .. 5] against gts[b, s_gt_inds - 1].  (The divisor is upstream's bbox_targets.size(0): all sampled RoIs.)
 *         acc       = 100 #(valid rows with argmax == label) / n_valid, 0 if n_valid == 0; argmax: the first index of the maximum, NaN greatest (lmv_dense_loss_fwd)
 *   stats        fp32 [LMV_RCNN_LOSS_STATS = 7]: loss_cls, loss_bbox, acc, n_valid, n_live, 1 / max(n_valid, 1), 1 / n_valid (0 if n_valid == 0)
 *   Forward: two launches (one lane per row, one partial row per wave; one reduce workgroup, in double, in a fixed order); workspace
 *     lmv_rcnn_loss_workspace_bytes(R) = 32 ceil(R / 64) bytes, 16-byte aligned.  R == 0 writes zero stats (all seven) and nothing else.
 *   Backward: one launch, one thread per row; gout: nullable DEVICE float [2] (loss_cls, loss_bbox).  It writes all of dcls [R, K + 1] (dcls_stride) and dbbox
 *     [R, D C] (dbbox_stride): dcls = gout[0] w_cls (softmax(z) - onehot(label)) / max(n_valid, 1) on a valid row, a zero row elsewhere; dbbox = gout[1] w_bbox
 *     smoothL1'(.) / n_valid in the chosen set of a live row, +0.0 everywhere else.  R == 0 launches nothing.
 *
 * Limits: N <= LMV_OBB_MAX_BOXES, H_l W_l <= LMV_OBB_MAX_BOXES, 1 <= A <= LMV_CODER_MAX_SETS, R and Gmax <= LMV_OBB_MAX_BOXES, B in 1 .. LMV_ASSIGN_MAX_BATCH,
 * 1 <= K <= LMV_CODER_MAX_SETS - 1.  The reduce launch of a forward call is ONE workgroup over all partial rows (RPN: B ceil(N / 1024); R-CNN: ceil(R / 64)): 2 048 /
 * 64 rows at the configs' shapes; at the limits (B = 4096 with N = 2^20: 4 M rows) its time grows with the row count and it, not the sweep, sets the call's time.
 * Refused with LMV_ERR_SHAPE and a message that starts "rpn_loss" / "rcnn_loss", before any launch: an unknown kind or dtype, sizes outside the limits, null
 * pointers, buffers not aligned to their element (the workspace: 16 bytes), a map stride below 1 or a batch stride below the extent of one image, row strides below
 * the row, a beta that is not a positive finite number, a negative or NaN loss weight, null means / stds or a NaN among them, a workspace that is too small.
 * ------------------------------------------------------------------------------------------ */
#define LMV_RPN_LOSS_MAX_LEVELS 5
#define LMV_RPN_LOSS_STATS(L) (2 * (L) + 3)
#define LMV_RCNN_LOSS_STATS 7
typedef struct lmv_rpn_loss_level {
  const void* cls; const void* reg;          /* [B, A, H, W] and [B, A D, H, W] */
  void* dcls; void* dreg;                    /* their gradients (backward only) */
  int64_t cls_stride[4], reg_stride[4], dcls_stride[4], dreg_stride[4];          /* batch, channel, row, column; in elements */
  int32_t H, W;
} lmv_rpn_loss_level;
size_t lmv_rpn_loss_workspace_bytes(int B, int64_t N);
int lmv_rpn_loss_fwd(const lmv_rpn_loss_level* levels, int L, int A, int dtype, int B, const uint8_t* mask, const float* anchors, int anchor_stride,
                     int64_t anchor_batch_stride, const float* gts, int gt_stride, int Gmax, const int32_t* gt_counts, const int64_t* gt_inds, int kind,
                     const float* means, const float* stds, float beta, float w_cls, float w_bbox, void* workspace, size_t workspace_bytes, float* stats, void* stream);
int lmv_rpn_loss_bwd(const lmv_rpn_loss_level* levels, int L, int A, int dtype, int B, const uint8_t* mask, const float* anchors, int anchor_stride,
                     int64_t anchor_batch_stride, const float* gts, int gt_stride, int Gmax, const int32_t* gt_counts, const int64_t* gt_inds, int kind,
                     const float* means, const float* stds, float beta, float w_cls, float w_bbox, const float* stats, const float* gout, void* stream);
size_t lmv_rcnn_loss_workspace_bytes(int R);
int lmv_rcnn_loss_fwd(const void* cls_score, int64_t cls_stride, const void* bbox_pred, int64_t bbox_stride, int dtype, int R, int K, int C, const float* rois,
                      int roi_stride, const int64_t* s_gt_inds, const int64_t* s_labels, const float* gts, int gt_stride, int B, int Gmax, const int32_t* gt_counts,
                      int kind, const float* means, const float* stds, float beta, float w_cls, float w_bbox, void* workspace, size_t workspace_bytes, float* stats,
                      void* stream);
int lmv_rcnn_loss_bwd(const void* cls_score, int64_t cls_stride, const void* bbox_pred, int64_t bbox_stride, int dtype, int R, int K, int C, const float* rois,
                      int roi_stride, const int64_t* s_gt_inds, const int64_t* s_labels, const float* gts, int gt_stride, int B, int Gmax, const int32_t* gt_counts,
                      int kind, const float* means, const float* stds, float beta, float w_cls, float w_bbox, const float* stats, const float* gout, void* dcls,
                      int64_t dcls_stride, void* dbbox, int64_t dbbox_stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * The proposal stage of the oriented RPN head of the Oriented R-CNN configs (csrc/proposal.hip): upstream's OrientedRPNHead.get_bboxes / _get_bboxes_single with
 * train_cfg.rpn_proposal = test_cfg.rpn = (nms_across_levels=False, nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.8, min_bbox_size=0) -- what turns the
 * head's maps into the proposals that lmv_max_iou_assign, lmv_random_sample and lmv_rroi_plan take.  The head's source is NOT part of the reference tree (only its
 * name in the configs is): the rules below restate upstream (OBBDetection on mmdet 2.x) and are the specification.  An addition to ABI 14: callers detect it by
 * symbol.  No host round trip, no floating-point atomics (integer counters only; no value depends on the order in which an atomic lands): two calls agree bit for
 * bit, the number of launches is fixed by the arguments, and both entry points can be captured.
 *
 * lmv_rpn_select -- B images, L <= LMV_RPN_LOSS_MAX_LEVELS levels; three launches and one memset node.
 *   levels       HOST table of L lmv_rpn_loss_level, read during the call: cls [B, A, H, W] and reg [B, 6 A, H, W] with their four ELEMENT strides (batch, channel,
 *                row, column), fp32 or bf16 (`dtype`, one for all of a call), read in place: contiguous, channels-last or a channel slice.  dcls / dreg are not read.
 *   anchors      fp32 [N, 4] shared by all images, rows through anchor_stride >= 4; N = sum_l n_l, n_l = H_l W_l A.  Row r = (h W_l + w) A + a of level l is anchor
 *                off_l + r, off_l = sum_{l' < l} n_l' -- the element space of lmv_rpn_loss_fwd and the row order of lmv_box_decode_map.
 *   The selection rule:
 *     The rank of a row is decided by its LOGIT, not by the rounded sigmoid (the sigmoid is monotone, and fp32 saturation would invent ties).  key = the
 *     order-preserving 32-bit image of the fp32 logit (bits | 0x80000000 for a non-negative value, ~bits for a negative one; a bf16 logit widens exactly; -0.0
 *     ranks equal to +0.0; +inf / -inf are ordinary values).  The greater logit first; on a tie the smaller row index first: level l's slots are its rows in
 *     ascending order of the 64-bit word (~key << 32) | r.  A row with a NaN logit is NOT a candidate -- a deliberate difference from upstream, whose sort puts NaN
 *     first; it is lmv_obb_nms's own "a NaN score is no candidate".  Upstream's sort is unstable, so its choice among tied scores differs from run to run; this one
 *     is fixed.  Level l contributes K_l = min(nms_pre, n_l) slots (upstream skips the sort when n_l <= nms_pre; here such a level is ranked all the same); the
 *     slots past the number of candidates are EMPTY: index -1, a box of zeros, score -inf.  Ktot = sum_l K_l; slot s of level l is element koff_l + s of an image.
 *   Outputs -- every element is written exactly once, on every call:
 *     index      int64 [B, Ktot]: the row r within the slot's level, -1 for an empty slot
 *     groups     int32 [B, Ktot]: the slot's level l (lmv_obb_nms's `groups`: nms_across_levels=False)
 *     scores     fp32 [B, Ktot]: 1 / (1 + exp(-z)) in fp32; -inf for an empty slot and, with min_bbox_size > 0, for a box that fails (w >= min_bbox_size and
 *                h >= min_bbox_size) -- lmv_obb_nms then does not take it as a candidate
 *     boxes      fp32 [B, Ktot, 5]: the midpoint decode (the rule above, kind LMV_CODER_MIDPOINT; means / stds HOST arrays of 6 floats by value; wh_ratio_clip)
 *                of anchor off_l + r with the six deltas at channels 6 a .. 6 a + 5 of position (h, w): the device function lmv_box_decode_map inlines, so a row has
 *                the bits that call writes for the same index
 *     order      int64 [B, Ktot]: the image's slots, as elements 0 .. Ktot - 1, by ascending (~key, level, slot number), empty slots last in element order -- the
 *                stable descending order of the concatenated levels by logit, and what lmv_obb_nms takes as `order` (with boxes + b Ktot 5, scores + b Ktot,
 *                groups + b Ktot and N = Ktot, per image).  A slot whose score min_bbox_size turned into -inf keeps its rank; it is no candidate there.
 *   Workspace: lmv_rpn_select_workspace_bytes(sizes, L, A, B, nms_pre), sizes a HOST array (H_0, W_0, H_1, W_1, ...) = B (5120 + 4 sum_l ceil16(n_l) + 4 Ktot) bytes,
 *     16-byte aligned, always required; 0 for sizes the call refuses.  It holds the [B, 5, 256] histograms of the top byte of ~key per level, ~key of every row
 *     (a level's row padded to 16 entries) and ~key of every slot.  It may hold anything on entry.
 *   Mapping: launch 1, grid-wide over 2 048 rows x B, computes ~key of every row, stores it and counts the top bytes in LDS, flushed with integer global atomics
 *     into the table the memset node zeroed; the bin total is the number of candidates.  Launch 2, one workgroup of 1 024 threads per (image, level), finds for an
 *     oversubscribed level only the threshold and the number of rows equal to it to take (lowest index first) with three more 8-bit radix-select sweeps over the
 *     workspace, collects the chosen words in one ordered sweep with a block prefix scan, sorts the at most 2 048 words in LDS (16 KB) and writes the slots.
 *     Launch 3, one thread per slot: rank = slot number + by binary search the number of slots of every other level in front (on equal keys the lower level).
 *
 * lmv_rpn_gather -- the fixed-shape results of B images in one launch, from what lmv_obb_nms wrote per image: keep int64 [B, max_num] (ranks order, then -1) and
 * count int64 [B].  boxes fp32 [B, Ktot, 5] and scores fp32 [B, Ktot] as above.  With c_b = clamp(count[b], 0, max_num):
 *     proposals  fp32 [B, max_num, 5]: the kept boxes in rank order, then rows of zeros
 *     out_scores fp32 [B, max_num]: their scores, -inf on padding
 *     num        int32 [B]: c_b
 *     ignore     uint8 [B, max_num]: 1 on padding, 0 on a proposal -- lmv_max_iou_assign's `ignore`: a padding row gets gt_inds = -1 and no sampler draws it
 * A keep entry outside 0 .. Ktot - 1 in front of the count reads nothing and is padding.  Every output element is written exactly once.
 *
 * Limits: 1 <= nms_pre <= LMV_RPN_MAX_PRE, L <= LMV_RPN_LOSS_MAX_LEVELS (so Ktot <= 10 240 <= LMV_OBB_NMS_MAX; the configs' shape, 1024 x 1024 with strides 4 .. 64
 * and A = 3: 2000 x 4 + 768 = 8 768), N <= LMV_OBB_MAX_BOXES, 1 <= A <= LMV_CODER_MAX_SETS, B in 1 .. LMV_ASSIGN_MAX_BATCH, 1 <= max_num <= LMV_OBB_NMS_MAX.
 * Refused with LMV_ERR_SHAPE (a workspace that is too small or null: LMV_ERR_WORKSPACE) and a message that starts "rpn_select" / "rpn_gather", before any launch:
 * sizes outside the limits, an unknown dtype, null pointers, buffers not aligned to their element (the workspace: 16 bytes), a map stride below 1 or a batch
 * stride below the extent of one image, an anchor row stride below 4, a negative or NaN min_bbox_size, a wh_ratio_clip that is not a positive finite number, null
 * means / stds or a NaN among them, Ktot (rpn_gather) outside 1 .. LMV_OBB_NMS_MAX.
 * ------------------------------------------------------------------------------------------ */
#define LMV_RPN_MAX_PRE 2048
size_t lmv_rpn_select_workspace_bytes(const int32_t* sizes, int L, int A, int B, int nms_pre);
int lmv_rpn_select(const lmv_rpn_loss_level* levels, int L, int A, int dtype, int B, const float* anchors, int anchor_stride, int nms_pre, float min_bbox_size,
                   const float* means, const float* stds, float wh_ratio_clip, void* workspace, size_t workspace_bytes, int64_t* index, int32_t* groups, float* scores,
                   float* boxes, int64_t* order, void* stream);
int lmv_rpn_gather(const float* boxes, const float* scores, int Ktot, const int64_t* keep, const int64_t* count, int B, int max_num, float* proposals,
                   float* out_scores, int32_t* num, uint8_t* ignore, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-block schedules: ONE call enqueues every launch of a LeMeBlock (models/lemevit.py:500-660) on token-major tensors
 * x [B, H*W, C], c [B, M, C] -- `LeMeBlock.forward_with_x` ("S", :615-650), `forward_with_xc` ("D", :542-582), `forward_with_c`
 * ("C", :584-613; x is returned untouched by the caller, x_out / dx_out may be NULL).  Replaces the ~12 / ~30 per-op calls a Python
 * scheduler makes per block and pass (lemevit_amd/blocks.py keeps that schedule for the variants not covered here).
 *   params: matrices (attn_w, fc1_w, fc2_w) in `dtype`, vectors (biases, LayerNorm affine, pos_embed weight [C, 9] and bias) fp32.
 *     attn_w / attn_b by kind:  S: {qkv, proj}   D: {qkv1, qkv2, proj_x, proj_c}   C: {q, kv, proj}
 *   masks: per-sample DropPath scale vectors [B] fp32 or NULL, in the reference's draw order (S / D: x-attn, x-mlp, c-attn, c-mlp; C: c-attn, c-mlp).
 *   g_*: fp32 gradient accumulators of the same shapes (backward only; accumulated, split reductions: deterministic).
 * Memory: the library allocates nothing.  `arena` (lmv_block_arena_bytes) receives every forward intermediate and IS the saved state
 * of the backward pass when save != 0 (keep it until lmv_block_bwd; with save == 0 it is scratch).  `scratch`
 * (lmv_block_bwd_scratch_bytes) holds the backward temporaries; one buffer may serve all blocks.  side_stream (nullable): the
 * weight-gradient launches are enqueued there behind an event on `stream`, and `stream` waits for them before the call returns.
 * Inference (save == 0) with flags & LMV_BLOCK_FUSED takes the fused entry points above (LayerNorm folded into qkv / q / kv, the MLP
 * half in one kernel); the training form keeps the per-layer launches, whose intermediates the backward pass reads.
 * ------------------------------------------------------------------------------------------ */
enum { LMV_BLOCK_S = 0, LMV_BLOCK_D = 1, LMV_BLOCK_C = 2 };
enum { LMV_BLOCK_NO_JOIN = 1, LMV_BLOCK_FUSED = 2, LMV_BLOCK_DATA_ONLY = 4 };
typedef struct lmv_block_desc {
  int32_t kind, dtype, B, H, W, M, C, hidden;      /* hidden: MLP width (0 = 4 C) */
  float eps;                                       /* LayerNorm eps of norm1 / norm2 (1e-6, models/lemevit.py:513,525) */
  int32_t flags;                                   /* LMV_BLOCK_NO_JOIN: lmv_block_bwd leaves the side stream un-joined (the caller records an
                                                      event on it and makes `stream` wait later; scratch and arena must then outlive that wait) */
  const float* pos_w; const float* pos_b; const float* n1_w; const float* n1_b;
  const void* attn_w[4]; const float* attn_b[4];
  const float* n2_w; const float* n2_b; const void* fc1_w; const float* fc1_b; const void* fc2_w; const float* fc2_b;
  const float* masks[4];
  float* g_pos_w; float* g_pos_b; float* g_n1_w; float* g_n1_b;
  float* g_attn_w[4]; float* g_attn_b[4];
  float* g_n2_w; float* g_n2_b; float* g_fc1_w; float* g_fc1_b; float* g_fc2_w; float* g_fc2_b;
  /* LMV_BLOCK_FUSED (lmv_block_fwd with save == 0, bf16): lmv_ln_fold operands (folded weight, colsum, folded bias) of the Linears that
   * consume norm1 -- S: {qkv, -}, D: {qkv1, qkv2}, C: {q, kv} -- and of mlp.0 (norm2).  The block then runs lmv_ln_linear_fwd instead of
   * LayerNorm + Linear where that is the faster form and lmv_mlp_fused_fwd for the MLP half where lmv_mlp_fused_supported. */
  const void* fold_attn_w[2]; const float* fold_attn_s[2]; const float* fold_attn_b[2];
  const void* fold_fc1_w; const float* fold_fc1_s; const float* fold_fc1_b;
  /* optional (NULL = absent): mlp.3.weight TRANSPOSED, [hidden, C] in `dtype` (lmv_transpose_batch of fc2_w).  With it lmv_block_bwd runs the dX
   * of fc2 -- du = (dOut W2) * GELU'(u) -- as the forward-form GEMM  dOut [rows, C] x fc2_wt^T  with the GELU' epilogue, which the
   * register-stationary kernel (csrc/rsgemm.hip) takes for C = 192 / 384.  Must hold the same values as fc2_w. */
  const void* fc2_wt;
  /* optional (NULL = absent), S blocks: mlp.0.weight TRANSPOSED [C, hidden] and the attention weights attn_w[0] (qkv) / attn_w[1] (proj)
   * TRANSPOSED [C, 3C] / [C, C] in `dtype`.  With them lmv_block_bwd runs the dX of fc1 / qkv / proj as forward-form GEMMs
   * dY [rows, N] x wt^T -> [rows, C], which the whole-width kernel (csrc/wngemm.hip) takes for C = 384.  Same values as the weights. */
  const void* fc1_wt; const void* attn_wt[2];
} lmv_block_desc;
size_t lmv_block_arena_bytes(const lmv_block_desc* d);
size_t lmv_block_bwd_scratch_bytes(const lmv_block_desc* d);
int lmv_block_fwd(const lmv_block_desc* d, const void* x, const void* c, void* x_out, void* c_out, void* arena, size_t arena_bytes, int save, void* stream);
/* The images [image0, image0 + nimages) of the same call: `d`, the tensors and the arena are those of the WHOLE batch (every tensor is
 * [rows, width] with the images outermost, so a range of images is a contiguous slice of each; the attention workspace of the arena is
 * sliced the same way).  The images of a batch do not interact inside a LeMeBlock (models/lemevit.py:500-650: LayerNorm, per-image
 * attention, per-row Linears), so calls over disjoint ranges that cover the batch, on ANY streams and in any order, leave the outputs and
 * the arena in the state one lmv_block_fwd call leaves them in (up to the kernel selection, which follows the row count) -- the training
 * forward runs them on concurrent streams so that the ramp and the tail of each launch are covered by another range's kernels;
 * lmv_block_bwd then consumes the arena as a whole. */
int lmv_block_fwd_range(const lmv_block_desc* d, const void* x, const void* c, void* x_out, void* c_out, void* arena, size_t arena_bytes, int save,
                        int image0, int nimages, void* stream);
/* x, c: the block inputs of the forward call; dx_out / dc_out: gradients of x_out / c_out; dx / dc: gradients of x / c (written). */
int lmv_block_bwd(const lmv_block_desc* d, const void* x, const void* c, const void* arena, size_t arena_bytes, const void* dx_out, const void* dc_out,
                  void* dx, void* dc, void* scratch, size_t scratch_bytes, void* stream, void* side_stream);
/* flags & LMV_BLOCK_DATA_ONLY: the block's parameters are frozen, only dx / dc are wanted.  (Additions of ABI 14: detect them by symbol.)
 *   - lmv_block_arena_bytes returns the reduced saved set xp, st1, pj, ao, lse, t2, st2, u + the attention workspace: the LayerNorm outputs n1 / n2 and the
 *     GELU output h, which only weight-gradient launches read, are not kept (10 C instead of 16 C per token of an S / D block);
 *   - a forward call still needs n1 / n2 / h while it runs: lmv_block_fwd_range_scratch takes them from `scratch` (lmv_block_fwd_scratch_bytes; one buffer
 *     may serve every block).  The buffer is laid out for the whole batch and sliced by image like the arena, so calls over disjoint image ranges share no
 *     byte of it.  lmv_block_fwd / lmv_block_fwd_range refuse the flag (no transient buffer); without the flag `scratch` is ignored;
 *   - lmv_block_bwd ignores the g_* pointers (they may be NULL) and enqueues no lmv_linear_dw or slab reduce, no lmv_reduce_batch, no
 *     lmv_dwconv3x3_bwd_weight_partial and nothing on side_stream -- `x`, which that launch alone reads, may be NULL, so the caller need not keep the
 *     block's input for the backward pass; the LayerNorm backward launches run in their dx-only mode; with both fc2_wt and fc1_wt
 *     present, bf16 and lmv_mlp_dx_fused_supported, the MLP half's two dX launches become one lmv_mlp_dx_fused where the "mlp_dx_fused" switch selects it
 *     (0 off, 1 where it measured faster -- no shape so far --, 2 wherever it applies).  dx / dc are those of the full backward (bit for bit when
 *     the same dX kernels are selected).
 * Without the flag none of these functions changes what it enqueues. */
size_t lmv_block_fwd_scratch_bytes(const lmv_block_desc* d);
int lmv_block_fwd_range_scratch(const lmv_block_desc* d, const void* x, const void* c, void* x_out, void* c_out, void* arena, size_t arena_bytes, int save,
                                int image0, int nimages, void* scratch, size_t scratch_bytes, void* stream);
/* Weight-gradient launches (lmv_linear_dw calls), reduces (lmv_reduce_batch) and side-stream forks that lmv_block_bwd has enqueued since the library was
 * loaded, plus its lmv_dwconv3x3_bwd_weight_partial launches: a host-side counter, a measurement aid like lmv_debug_launch_timing -- it makes "a data-only
 * backward launched no weight-gradient work" testable. */
long long lmv_debug_wgrad_launches(void);

/* ------------------------------------------------------------------------------------------
 * A whole run of "S" blocks as ONE persistent launch (csrc/sstage.hip; inference form, bf16): stage 3 of LeMeViT-Base -- 18 x
 * LeMeBlock.forward_with_x (models/lemevit.py:615-650, live :631-635; StandardAttention :185-205; MLP :526-530) on x [B, 196, 384] and
 * c [B, 16, 384].  The token rows stay on chip for the whole stage (two workgroups per image, residual stream in registers); only the
 * block weights stream from L2.  Replaces nblocks lmv_block_fwd(kind = S, save = 0) calls; same math, the residual stream is kept in
 * fp32 between the blocks instead of being rounded to bf16 after every residual add.
 *   lmv_sstage_supported: 1 where the kernel applies: C = 384 / 12 heads / hidden 1536 (LeMeViT-Base, Small-v2: 8 waves per workgroup) or C = 192 / 6 heads /
 *     hidden 768 (LeMeViT-Tiny: 4 waves, two workgroups per CU), 14 x 14 image tokens, 16 meta tokens, bf16.
 *   lmv_sstage_pack: one block's parameters (matrices bf16, vectors fp32, the reference's layouts: attn.qkv [3C, C], attn.proj [C, C],
 *     mlp.0 [4C, C], mlp.3 [C, 4C], pos_embed.weight [C, 9]) -> `wpk_out` (lmv_sstage_wpk_bytes: the matrices in MFMA-fragment order) and
 *     `vec_out` (lmv_sstage_vec_floats fp32).  The packed blocks of a stage are consecutive: block j at wpk + j * wpk_bytes, vec + j * vec_floats.
 *   lmv_sstage_fwd: x_out / c_out may alias x / c.  `workspace` (lmv_sstage_workspace_bytes(min(B, lmv_sstage_max_images(C)), C)) holds the K / V fragments and the
 *     grid rows the two halves of an image exchange, the parked residual registers, and the flags (reset by the call on `stream`).  The launch needs 2 * min(B, max images)
 *     co-resident workgroups (512 threads / 147 KB LDS, one per CU; C = 192: 256 threads / 74 KB, two per CU): concurrent calls on different streams are safe up to lmv_sstage_max_concurrent() at a time (each with its own workspace).
 * ------------------------------------------------------------------------------------------ */
typedef struct lmv_sstage_block_params {
  int32_t C, heads, hidden, _pad;
  const void* qkv_w; const void* proj_w; const void* fc1_w; const void* fc2_w;
  const float* n1_w; const float* n1_b; const float* qkv_b; const float* proj_b;
  const float* n2_w; const float* n2_b; const float* fc1_b; const float* fc2_b;
  const float* pos_w; const float* pos_b;
} lmv_sstage_block_params;
typedef struct lmv_sstage_desc {
  int32_t B, H, W, M, C, heads, hidden, nblocks, dtype;
  float eps;                                       /* LayerNorm eps of norm1 / norm2 (1e-6) */
  const void* wpk; const float* vec;               /* nblocks packed blocks (lmv_sstage_pack) */
  void* timing; int32_t timing_block, kind;        /* optional (NULL): uint64 s_memtime stamps [workgroup][8 waves][24] of block `timing_block` (tools/sstage_timeline.py); kind: 0 (lmv_dstage_fwd: 0 = "D" blocks, 1 = "C" blocks) */
} lmv_sstage_desc;
int lmv_sstage_supported(int C, int heads, int hidden, int H, int W, int M, int dtype);
size_t lmv_sstage_wpk_bytes(int C, int hidden);
size_t lmv_sstage_vec_floats(int C, int hidden);
size_t lmv_sstage_workspace_bytes(int B, int C);
int lmv_sstage_max_images(int C);                 /* images one launch takes: (workgroups of the instance the device holds) / 2, whole groups of 8 -- 128 at C = 384, 256 at C = 192 on an MI355X; size the workspace for min(B, this) */
int lmv_sstage_max_concurrent(int C);             /* lmv_sstage_fwd calls that may be in flight on different streams of a device at once (see lmv_dstage_max_concurrent); 0: none */
int lmv_sstage_pack(const lmv_sstage_block_params* p, void* wpk_out, float* vec_out, void* stream);
int lmv_sstage_fwd(const lmv_sstage_desc* d, const void* x, const void* c, void* x_out, void* c_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A whole run of "D" blocks as ONE persistent launch (csrc/dstage.hip; inference form, bf16): stages 1 and 2 of LeMeViT-Base -- 4 x
 * LeMeBlock.forward_with_xc (models/lemevit.py:542-582, live :560-564; DualCrossAttention :220-324, live :288-302; MLP :526-530) on
 * x [B, 784, 192] and c [B, 16, 192].  An image is 7 workgroups of 112 image tokens (4 grid rows) plus one workgroup for the 16 meta tokens,
 * all resident together; per block they exchange, through L2, the grid rows next to a cut, the meta tokens' K2 / V2 / (q2 W_k1) operand
 * fragments, and the per-workgroup softmax partials of the meta queries over the image keys.  Replaces nblocks lmv_block_fwd(kind = D, save = 0)
 * calls; same math (the image tokens' k projection is folded into the meta queries; its bias cancels in the softmax), residual stream fp32
 * between the blocks.
 *   lmv_dstage_supported: 1 for C = 192 (LeMeViT-Base / -Small stage 2) or 128 (LeMeViT-Tiny stage 2) at 28 x 28 image tokens (7 + 1 workgroups of 4 waves per image) and for
 *     C = 96 (Base / Small stage 1) or 64 (Tiny stage 1) at 56 x 56 (28 + 1 workgroups of 2 waves); heads = C / 32, hidden = 4 C, 16 meta tokens, bf16.
 *   lmv_dstage_pack: one block's parameters (matrices bf16, vectors fp32, the reference's layouts: attn.qkv1 / attn.qkv2 [3C, C], attn.proj_x /
 *     attn.proj_c [C, C], mlp.0 [4C, C], mlp.3 [C, 4C], pos_embed.weight [C, 9]) -> wpk_out / vec_out; blocks of a stage consecutive as for lmv_sstage_pack.
 *   lmv_dstage_fwd: x_out / c_out must NOT alias x / c.  `workspace`: lmv_dstage_workspace_bytes(B, C) (exchange buffers and flags of the image
 *     slots; flags reset by the call on `stream`; one workspace per concurrent call).  All 8 (29) workgroups of an image slot must be co-resident (256 threads / 74 KB LDS each, two per CU;
 *     128 / 37 KB, four per CU).  Concurrent calls on different streams are safe up to lmv_dstage_max_concurrent() at a time (lemevit_amd.graph.split_forward issues up to 4): slots are assigned by ticket
 *     (see "Residency" below), so every call holds at most 8 incomplete slots and the rest of the chip always runs complete ones, whatever the dispatch order.
 * ------------------------------------------------------------------------------------------ */
typedef struct lmv_dstage_block_params {
  int32_t C, heads, hidden, _pad;
  const void* qkv1_w; const void* qkv2_w; const void* projx_w; const void* projc_w; const void* fc1_w; const void* fc2_w;
  const float* n1_w; const float* n1_b; const float* qkv1_b; const float* qkv2_b; const float* projx_b; const float* projc_b;
  const float* n2_w; const float* n2_b; const float* fc1_b; const float* fc2_b;
  const float* pos_w; const float* pos_b;
} lmv_dstage_block_params;
/* kind = 2: a run of "S" blocks on a long sequence (LeMeBlock.forward_with_x, models/lemevit.py:615-650; C = 384, 24 x 24 image tokens: stage 3 of LeMeViT-Base at 384 x 384), packed as a D
 * block with qkv1 = qkv2 = attn.qkv and proj_x = proj_c = attn.proj (lemevit_amd/ops.py::s2stage_pack): 6 image-row workgroups + 1 meta workgroup per image, the image's keys and values cross
 * its workgroups through L2. */
typedef lmv_sstage_desc lmv_dstage_desc;          /* same fields; timing: uint64 stamps [workgroup][waves][16]; kind = 1: a run of "C" blocks (stage 0: LeMeBlock.forward_with_c,
                                                   * models/lemevit.py:584-612 -- only the meta tokens change: c += proj(softmax(q(n1 c) k(n1 x')^T / sqrt(32)) v(n1 x')), c += mlp(n2 c) with x' = x + dwconv(x);
                                                   * x passes through, x_out is not written and may be NULL-equivalent = x).  Packed as a D block with qkv1 = [0 | attn.kv], qkv2 = [attn.q | 0 | 0],
                                                   * proj_c = attn.proj, proj_x unused (lemevit_amd/ops.py::cstage_pack) */
int lmv_dstage_supported(int C, int heads, int hidden, int H, int W, int M, int dtype);
size_t lmv_dstage_wpk_bytes(int C, int hidden);
size_t lmv_dstage_vec_floats(int C, int hidden);
size_t lmv_dstage_workspace_bytes(int B, int C);
int lmv_dstage_max_concurrent(int C, int H, int kind);   /* lmv_dstage_fwd calls that may be in flight on different streams of the device at once (0: unsupported shape): 8 / 4 at 28 x 28 / 56 x 56,
                                                           * 2 / 1 at 48 x 48 / 96 x 96 -- the caller must not exceed it (lemevit_amd.model falls back to the per-block schedule) */
int lmv_dstage_pack(const lmv_dstage_block_params* p, void* wpk_out, float* vec_out, void* stream);
int lmv_dstage_fwd(const lmv_dstage_desc* d, const void* x, const void* c, void* x_out, void* c_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The stem as ONE launch (csrc/stem.hip; inference form, BatchNorm folded into the convolutions by the caller):
 *   Conv2d(3, Cm, 3, 2, 1) -> BN -> GELU -> Conv2d(Cm, Co, 3, 2, 1) -> BN   (models/lemevit.py:698-704, called at :713)
 * on images x [B, 3, H, W] (element strides sb, sc, sh, sw: NCHW or channels-last, fp32 or bf16) -> y [B, H/4, W/4, Co] bf16 (= the token
 * matrix [B, H/4 * W/4, Co]).  Replaces lmv_im2col3x3s2_c3 + lmv_linear_fwd(GELU) + lmv_im2col3x3s2_nhwc + lmv_linear_fwd: no patch matrix and
 * no Cm-channel map in HBM (an 8 x 8 output tile's 17 x 17 x Cm intermediate lives in LDS).
 *   lmv_stem_supported: (Cm, Co) = (48, 96) (LeMeViT-Base / -Small) or (32, 64) (LeMeViT-Tiny), H and W multiples of 32, bf16 compute.
 *   lmv_stem_pack: w1m [Cm, 32] bf16 (column ci * 9 + ky * 3 + kx, 27..31 zero: the operand of lmv_im2col3x3s2_c3's GEMM), w2m [Co, ld2] bf16
 *     (column (ky * 3 + kx) * Cm + ci: the operand of lmv_im2col3x3s2_nhwc's GEMM) -> wpk_out (lmv_stem_wpk_bytes, MFMA-fragment order).
 *   lmv_stem_fwd: b1 [Cm], b2 [Co] fp32 (the folded biases).
 * ------------------------------------------------------------------------------------------ */
int lmv_stem_supported(int H, int W, int Cm, int Co, int dtype);
size_t lmv_stem_wpk_bytes(int Cm, int Co);
int lmv_stem_pack(const void* w1m, const void* w2m, int ld2, int Cm, int Co, void* wpk_out, void* stream);
int lmv_stem_fwd(const void* x, int x_dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int B, int H, int W, int Cm, int Co, const void* wpk, const float* b1,
                 const float* b2, void* y, void* stream);
/* Residency of the persistent stage kernels.  The workgroups of a slot (the two halves of an image in lmv_sstage_fwd, the image-row workgroups + the meta workgroup of an image in
 * lmv_dstage_fwd) wait for each other inside the launch, so a slot advances only while all of them are resident.  The kernels do NOT rely on a dispatch order or a workgroup -> XCD
 * map for that (HIP promises neither): every workgroup takes a ticket when it starts (csrc/stage_common.h: stage_ticket) and becomes role t % NWG of slot t / NWG, so the started workgroups
 * always form complete slots plus at most 8 incomplete ones per launch, and the next workgroups to start complete those.  Progress needs room for the incomplete slots of ALL launches in
 * flight plus one workgroup: n * 8 (NWG - 1) + 1 <= (workgroups the device holds) -- lmv_sstage_max_concurrent / lmv_dstage_max_concurrent return that n for a shape (launches of
 * different shapes mix under the same per-shape bound), lmv_*stage_supported is 0 on a device too small for n = 1, and the host mirror (lemevit_amd/model.py) takes the per-block
 * schedule where a bound is exceeded.  The bounds count the launches of ONE process; processes sharing a device add up (one process per GPU is the deployment contract).
 * Every in-launch wait is bounded all the same: a spin that runs out (a lost hand-off -- a bug, or more launches in flight than the bound) sets a sticky per-device error word in pinned
 * host memory instead of hanging the GPU.  lmv_stage_error_count returns it without synchronising anything: 0 = every hand-off of every COMPLETED launch arrived (synchronise the streams
 * of interest first for a verdict on them); < 0: LMV_ERR_*; reset != 0 clears it.  lmv_debug_stage_error_set stores a value there from the host (tests of the callers' error paths). */
int lmv_stage_error_count(int reset);
int lmv_debug_stage_error_set(int value);

/* Launch timing probe: lmv_debug_launch_timing(capacity > 0) creates `capacity` event pairs and from then on brackets every lmv_linear_fwd / lmv_linear_res_ln_fwd /
 * lmv_ln_linear_exact_fwd call -- from any schedule, the native block schedule (lmv_block_fwd) included -- with HIP events on the stream it launches on; after a device
 * synchronisation lmv_debug_launch_timing_read returns the number of calls and fills their durations [ms], FLOPs and algorithmic HBM bytes; capacity = 0 frees the events.
 * Not for use inside a stream capture; single host thread.  (bench.py's roofline object.) */
int lmv_debug_launch_timing(int capacity);
int lmv_debug_launch_timing_read(float* ms, double* flops, double* bytes, int* kinds, int capacity);   /* kinds: 0 forward-form Linear, 1 lmv_sstage_fwd, 2 lmv_dstage_fwd, 3 lmv_stem_fwd, ..., 12 lmv_mlp_dx_fused */
void lmv_stem_debug_timing(void* buf);   /* tools/stem_timeline.py: NULL, or a device buffer of [workgroups][4 waves][8] uint64 s_memtime stamps filled by the next lmv_stem_fwd calls */

#ifdef __cplusplus
}
#endif
#endif /* LEMEVIT_HIP_H */
