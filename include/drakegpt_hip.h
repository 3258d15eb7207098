/*
 * drakegpt_hip.h -- C ABI of libdrakegpt_hip.so, the MI355X (gfx950) kernels behind
 * DrakeGPT's transformer training hot path.
 *
 * The reference (ChrisTho23/DrakeGPT) has no native code and no FFI: every number is produced
 * by stock ATen ops called from src/model.py and src/model_component.py (SURVEY.md section 2b
 * lists the call sites K1..K19).  Each entry point below therefore names the reference call
 * site(s) whose arithmetic it replaces; the Python layer in drakegpt_amd/ binds these symbols
 * with ctypes and presents the reference's nn.Module surface on top.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host; the library allocates
 *    nothing and owns nothing: workspaces are passed in by the caller;
 *  - `stream` is a hipStream_t; calls only enqueue work and return immediately, so they may be
 *    captured into a hipGraph;
 *  - all matrices are row-major with an explicit leading dimension in ELEMENTS;
 *  - dtype codes: DG_F32 = 0 (float), DG_BF16 = 1 (bfloat16, round-to-nearest-even);
 *  - return value: 0 on success, a negative DG_ERR_* for a rejected argument, or a positive
 *    hipError_t from the launch; dg_error_string() explains either;
 *  - no global mutable state: safe to call from the autograd worker thread and the main
 *    thread concurrently (forward runs on one, backward on the other).
 *
 * Dropout stream: a keep decision is a stateless hash of (seed, step, site, element index)
 * (csrc/common.h: dg_keep): elements 2i and 2i + 1 read the low / high 16 bits of one 32-bit
 * word hash(key, i) and are kept iff that field >= floor(p * 65536).
 * `rng_state` points at 4 device uint32: {seed_lo, seed_hi, step, 0 (scratch of dg_adamw_step's advance)}; the step word is
 * advanced on the device (dg_state_advance, or inside dg_adamw_step) so a captured graph replays with fresh masks.  A NULL rng_state or p == 0 disables dropout (eval mode).
 */
#ifndef DRAKEGPT_HIP_H
#define DRAKEGPT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_F32 0
#define DG_BF16 1
#define DG_FP8_E4M3 2      /* OCP e4m3fn (gfx950's fp8; NOT MI300's fnuz encoding), max 448 */
#define DG_FP8_E5M2 3      /* OCP e5m2, max 57344 */
#define DG_F32X3 4         /* fp32 operands in memory, contracted as split bf16 (hi.hi + hi.lo + lo.hi, hi = bf16(x),
                              lo = bf16(x - hi), fp32 accumulation): in_dtype of dg_gemm_nt (out_dtype DG_F32) and dtype of
                              dg_gemm_tn only; every other entry point rejects it with DG_ERR_DTYPE */

#define DG_OK 0
#define DG_ERR_ARG (-1)       /* bad size / null pointer / unsupported combination */
#define DG_ERR_ALIGN (-2)     /* pointer or leading dimension not 16-byte aligned */
#define DG_ERR_DTYPE (-3)

#define DG_ABI_VERSION 21   /* bump whenever a signature or struct of this header changes: the Python binding refuses a stale library */

int dg_version(void);
const char* dg_error_string(int code);

/* {seed_lo, seed_hi, step, 0}: step += 1.  One launch of one thread. */
int dg_state_advance(uint32_t* rng_state, void* stream);

/* ---------------------------------------------------------------------------------------
 * get_batch -- ref: src/preprocessing.py:43-45.  The corpus stays resident in HBM; the B window
 * offsets are still drawn by the host CPU generator (torch.randint) for parity and passed in.
 * x[b, t] = corpus[off[b] + t], y[b, t] = corpus[off[b] + t + 1].  All int64. */
int dg_batch_gather(const int64_t* corpus, int64_t n_corpus, const int64_t* offsets,
                    int64_t* x, int64_t* y, int B, int T, void* stream);

/* ---------------------------------------------------------------------------------------
 * Token + position embedding -- ref: src/model.py:595-597 (K1-K3).
 * x[b,t,:] = tok[idx[b,t],:] + pos[t,:]   (pos == NULL: BigramLM-style plain gather, :96).
 * T <= rows of pos is the caller's job to check.  idx values are clamped to [0, V) on the device so that a bad id can
 * never fault the GPU; torch raises IndexError instead, and so does the Python layer, at the points where ids enter
 * (drakegpt_amd.ops.check_ids: module forward / generate, TrainEngine.set_corpus / set_batch) -- never inside the step. */
int dg_embed_fwd(const int64_t* idx, const float* tok, const float* pos, float* x,
                 int B, int T, int C, int V, void* onehot, int64_t ld_onehot, void* stream);
/* onehot (nullable): bf16 [B*T, ld_onehot >= V, multiple of 8], row m = e_{idx[m]}.  With it the token-table gradient
 * is dg_gemm_tn_grouped problem (A = onehot, B = bf16 dx): deterministic, no atomics. */
/* get_batch and the embedding in ONE launch (ref: src/preprocessing.py:43-45 + src/model.py:595-597): the ids are gathered
 * from the resident corpus at this step's window offsets and x_ids / y_ids [B, T] (the batch and its targets) are written
 * beside x.  `offsets` is a staged block [n_rows, B] of host-drawn offsets; the row is step_state[2] - ctl[0], clamped to
 * ctl[1] rows (ctl: 2 device uint32 {step word at staging time, n_rows}; step_state as in the header comment), so a captured
 * step walks through the block without any per-step host copy.  ctl == step_state == NULL: row 0. */
int dg_batch_embed_fwd(const int64_t* corpus, int64_t n_corpus, const int64_t* offsets, const uint32_t* step_state,
                       const uint32_t* ctl, int64_t* x_ids, int64_t* y_ids, const float* tok, const float* pos, float* x,
                       int B, int T, int C, int V, void* onehot, int64_t ld_onehot, void* stream);
/* Backward of dg_embed_fwd (embedding_dense_backward).  dtok [V,C] (nullable) is zero-filled here and then
 * accumulated with fp32 atomics; dpos [T,C] (nullable) is overwritten with sum over b. */
int dg_embed_bwd(const int64_t* idx, const void* dx, int dx_dtype, float* dtok, float* dpos,
                 int B, int T, int C, int V, void* stream);
/* dx_dtype: DG_F32, or DG_BF16 (the bf16 gradient stream of the engine's bf16 / fp8 modes) */

/* ---------------------------------------------------------------------------------------
 * LayerNorm over the last dim, eps inside the sqrt, biased variance -- ref: nn.LayerNorm at
 * src/model_component.py:488-489 applied at :505-506 (K4).  x is the fp32 residual stream;
 * y is written in y_dtype (the next GEMM's operand type). mean/rstd [M] are saved for bwd. */
int dg_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype,
                     float* mean, float* rstd, int M, int C, float eps, void* stream);
/* precision fp8 (round 3): the same LayerNorm with its output as OCP e4m3 (q8 [M][C] bytes: the operand of the fp8 GEMM that
 * follows and of the fp8 dW launch) with delayed per-tensor scaling -- the value is first rounded to bf16, as the separate cast
 * launch saw it -- one partial maximum per workgroup: parts2 [2][n_parts] floats with n_parts = dg_layernorm_fwd_fp8_parts(M)
 * (slot step_state[2] & 1 written, the other read), *scale_inv the factor the consumer multiplies back.  y_bf16 nullable (nobody
 * reads the bf16 form in the engine's fp8 step).  C % 4 == 0, C <= 1024. */
int dg_layernorm_fwd_fp8_parts(int M);
int dg_layernorm_fwd_fp8(const float* x, const float* gamma, const float* beta, void* y_bf16, void* q8, float* mean, float* rstd,
                         int M, int C, float eps, float* parts2, int n_parts, const uint32_t* step_state, float* scale_inv,
                         void* stream);
/* dx = dresid (nullable, the residual branch's gradient) + LN'(dy).  dgamma/dbeta are emitted
 * as n_partials row-chunk partial sums: partial g at dgamma_part + g*part_stride (same for
 * dbeta_part); finish with dg_reduce_partials.  dy_dtype: DG_F32, or DG_BF16 (C % 4 == 0 only) when dy comes
 * straight out of a bf16-output dX GEMM. */
int dg_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                     const float* rstd, const float* dresid, float* dx,
                     float* dgamma_part, float* dbeta_part, int64_t part_stride, int n_partials,
                     int M, int C, void* stream);

/* The same, and additionally g[m,c] = (g_dtype)(dx[m,c] * keep/(1-p)) with its column-sum partials in
 * gbias_part (same stride / count as dgamma_part): the operand and the bias gradient that the sub-layer
 * which runs next in backward would otherwise get from dg_dropout_bwd_cast(dx, site) -- one 38 MB pass and
 * one launch less per sub-layer (gbias_part may be NULL).  Returns DG_ERR_ARG for shapes the fused kernel does not cover
 * (C % 4 != 0 or C > 1024): call dg_layernorm_bwd + dg_dropout_bwd_cast then.
 * resid_dtype: type of dresid and dx, DG_F32 or (bf16 dy and bf16 g only) DG_BF16: the engine's bf16 / fp8 modes keep the
 * residual-branch gradient stream in bf16 (25 MB less per launch at the scaled configuration). */
int dg_layernorm_bwd_fused(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                           const float* rstd, const void* dresid, void* dx, int resid_dtype,
                           float* dgamma_part, float* dbeta_part, int64_t part_stride, int n_partials,
                           int M, int C,
                           void* g, int g_dtype, float dropout_p, const uint32_t* rng_state, uint32_t site,
                           float* gbias_part, void* stream);
/* fp8 mode: the same with g in bf16 AND a second time as OCP e5m2 (g8 [M][C] bytes: the gradient operand of the dX GEMM that
 * runs next) with delayed per-tensor scaling as in dg_fp8_quantize_delayed (g8_parts2 [2][DG_FP8_AMAX_PARTS], step_state,
 * *g8_scale_inv); the cast sees the bf16 value of g, as a separate cast launch would.  n_partials must be DG_FP8_AMAX_PARTS: every
 * workgroup leaves one partial maximum. */
int dg_layernorm_bwd_fused_fp8(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                               const float* rstd, const void* dresid, void* dx, int resid_dtype,
                               float* dgamma_part, float* dbeta_part, int64_t part_stride, int n_partials,
                               int M, int C,
                               void* g, float dropout_p, const uint32_t* rng_state, uint32_t site, float* gbias_part,
                               void* g8, float* g8_parts2, const uint32_t* step_state, float* g8_scale_inv, int g8_only, void* stream);
/* g8_only != 0: the bf16 form of g is not written (its consumers read the e5m2 copy); g must still be a valid pointer. */

/* ---------------------------------------------------------------------------------------
 * GEMM "NT": C[M,N] = epilogue(A[M,K] . B[N,K]^T), MFMA with fp32 accumulation.
 * Replaces every nn.Linear forward (y = x W^T + b; W is [out,in]) -- ref:
 * src/model_component.py:392-393,404 (packed q/k/v), :454 (proj), :321-323 (FFN),
 * src/model.py:599 (lm_head) -- and, with B = W^T, every Linear's dX = dY . W.
 * Epilogue, in this order (each optional):
 *    v = acc + bias[n];  v = max(v,0) if relu;  v = 0 where relu_mask[m,n] <= 0 (or its sign_bits bit is clear);
 *    v = dropout(v; p, site);  v += residual[m,n];  C[m,n] = (out_dtype) v
 * in_dtype: type of A, B and relu_mask.  K and lda/ldb must be multiples of 16 bytes' worth of
 * elements (8 bf16 / 4 f32) and A, B 16-byte aligned.  DG_F32X3: fp32 A, B and relu_mask, split-bf16 contraction, fp32
 * output; no sign_bits / colsum / fp8 outputs.
 * sign_bits_out / sign_bits: the ReLU mask as one BIT per element (C[m,n] > 0).  The forward Linear+ReLU of
 * FeedForward (ref: src/model_component.py:321-322) emits it next to C; the dX GEMM of the second Linear consumes it
 * instead of re-reading the 16x larger activation.  The buffer (dg_gemm_nt_sign_bits_bytes(M, N) bytes) is OPAQUE: bits
 * are stored in the order the kernel's lanes own the output tile, so it is only meaningful between a producing and a
 * consuming dg_gemm_nt call with the same M and N.  Supported when dg_gemm_nt_sign_bits_supported(args) is non-zero
 * (bf16 operands, N % 8 == 0, K % 64 == 0, K >= 128); DG_ERR_ARG otherwise. */
typedef struct dg_gemm_nt_args {
    const void* A; int64_t lda;
    const void* B; int64_t ldb;
    void* C; int64_t ldc;
    int32_t M, N, K;
    int32_t in_dtype, out_dtype;
    const float* bias;
    int32_t relu;
    const void* relu_mask; int64_t ldmask;
    const float* residual; int64_t ldr;
    float dropout_p;
    const uint32_t* rng_state;
    uint32_t site;
    uint8_t* sign_bits_out;        /* nullable */
    const uint8_t* sign_bits;      /* nullable; excludes relu_mask */
    int64_t sign_bits_bytes;       /* size of either buffer, >= dg_gemm_nt_sign_bits_bytes(M, N) */
    float* colsum_part;            /* nullable: [colsum_rows][colsum_ld] fp32, see below */
    int64_t colsum_ld;
    int32_t colsum_rows;           /* rows of colsum_part, >= dg_gemm_nt_colsum_rows(args) */
    /* fp8 operands (in_dtype = DG_FP8_E4M3 for forward activations or DG_FP8_E5M2 for gradients; b_dtype = DG_FP8_E4M3, the
     * weight operand): one byte per element, K % 128 == 0, K >= 256, block-scaled MFMA (v_mfma_f32_16x16x128_f8f6f4) with unit
     * block scales; the per-tensor dequantisation factors *scale_a and *scale_b (device scalars written by dg_fp8_quantize)
     * multiply the fp32 accumulator before the epilogue.  b_dtype 0 = same as in_dtype (every non-fp8 call). */
    int32_t b_dtype;
    const float* scale_a;
    const float* scale_b;
    /* fp8_out (nullable): the output is ALSO written as OCP e4m3, [M][ld_fp8_out] bytes -- the operand of the next fp8 GEMM,
     * without a cast launch that re-reads C -- with delayed per-tensor scaling exactly as dg_fp8_quantize_delayed does it:
     * fp8_out_parts2 = [2][DG_FP8_AMAX_PARTS] partial maxima of the call site (slot rng_state-style step & 1 written, the other
     * read; fp8_out_step = the device step word array), *fp8_out_scale_inv = the factor the consumer multiplies back.  The cast
     * sees the fp32 value (before the rounding to out_dtype).  Only where dg_gemm_nt_fp8_out_supported(args) is non-zero
     * (fp8 e4m3 operands, bf16 out, bias + ReLU + sign_bits_out epilogue, whole tiles, exactly DG_FP8_AMAX_PARTS workgroups:
     * the first FFN Linear of the engine's step); DG_ERR_ARG otherwise. */
    void* fp8_out; int64_t ld_fp8_out;
    float* fp8_out_parts2;
    const uint32_t* fp8_out_step;
    float* fp8_out_scale_inv;
    /* fp8_out_only != 0 (with fp8_out): C is NOT written -- the fp8 copy (and the sign bits / column sums) is all the callers of
     * this output read (the engine's fp8 step: the FFN hidden layer and its gradient feed an fp8 GEMM and the fp8 dW launch only);
     * C must still be a valid pointer (shape / alignment checks). */
    int32_t fp8_out_only;
} dg_gemm_nt_args;
int dg_gemm_nt(const dg_gemm_nt_args* args, void* stream);
int dg_gemm_nt_sign_bits_supported(const dg_gemm_nt_args* args);
int dg_gemm_nt_fp8_out_supported(const dg_gemm_nt_args* args);
/* colsum_part: the epilogue also leaves the column sums of C (fp32, of the values before rounding to out_dtype) as
 * dg_gemm_nt_colsum_rows(args) partial rows: sum them with dg_reduce_partials.  Which rows of C a partial row covers is
 * the kernel's business (one per 32 rows of C, or one per workgroup and wave row when a workgroup's tiles share their
 * columns); every partial row is written by every call.  With C = d(pre-activation) of FeedForward's first Linear this is
 * that Linear's bias gradient (ref: autograd of src/model_component.py:321), for which the step used to re-read all of C
 * (dg_colsum).  Only for the sign_bits-consuming form with whole tiles: dg_gemm_nt_colsum_supported(args) non-zero,
 * DG_ERR_ARG otherwise. */
int dg_gemm_nt_colsum_supported(const dg_gemm_nt_args* args);
int dg_gemm_nt_colsum_rows(const dg_gemm_nt_args* args);
int64_t dg_gemm_nt_sign_bits_bytes(int M, int N);

/* fp8 operand preparation (per-tensor scaling, just in time) for dg_gemm_nt's fp8 form -- precision = "fp8".
 * dg_fp8_amax: DG_FP8_AMAX_PARTS partial maxima of |x| per segment of the flat buffer x (n elements) into amax_parts
 * [n_seg * DG_FP8_AMAX_PARTS] (no atomics, nothing to zero).  seg = NULL: one segment; else a device table of n_seg x 2 int64
 * {first element, element count}, both multiples of 8 (all weight matrices of the step in one launch).
 * dg_fp8_quantize: q[i] = fp8(clamp(x[i] * FMAX / amax[s])) in format fmt (DG_FP8_E4M3 / DG_FP8_E5M2), one byte per element,
 * with amax[s] = the maximum of segment s's partial maxima, and scale_inv[s] = amax[s] / FMAX (1 when amax is 0), the factor
 * dg_gemm_nt multiplies back.  The scale FMAX / amax is capped at 2^126 (an amax below FMAX * 2^-126, where the quotient runs
 * towards +Inf in fp32: zeros stay zeros and scale_inv stays a normal 2^-126); every fp8 producer of the library shares the rule.
 * n % 8 == 0. */
#define DG_FP8_AMAX_PARTS 256
int dg_fp8_amax(const void* x, int dtype, int64_t n, const int64_t* seg, int n_seg, float* amax_parts, void* stream);
int dg_fp8_quantize(const void* x, int dtype, void* q, int fmt, int64_t n, const int64_t* seg, int n_seg,
                    const float* amax_parts, float* scale_inv, void* stream);
/* Delayed scaling in ONE pass (the training engine's activations and gradients: the amax pass is what made just-in-time
 * scaling slower than the bf16 GEMMs it replaced): q = fp8(clamp(x * FMAX / amax_prev)), amax_prev = what this call site
 * recorded one step ago, and this tensor's own partial maxima are recorded for the next step.  parts2: [2][DG_FP8_AMAX_PARTS]
 * floats owned by the call site; slot (rng_state[2] & 1) is written, the other one read (rng_state[2] is the step word that
 * dg_state_advance increments).  Seed both slots with dg_fp8_amax before the first use.  scale_inv[0] = amax_prev / FMAX. */
int dg_fp8_quantize_delayed(const void* x, int dtype, void* q, int fmt, int64_t n, float* parts2,
                            const uint32_t* rng_state, float* scale_inv, void* stream);

/* GEMM "TN": weight gradients, dW[P,Q] = sum_r A[r,P] * B[r,Q]  (A = dY [R,P], B = X [R,Q]).
 * The contraction over the R = B*T rows is split n_splits ways across workgroups; split s
 * writes its fp32 partial to out + s*split_stride (finish with dg_reduce_partials).
 * P and Q need no alignment; lda/ldb must be multiples of 8 bf16 / 4 f32 and every 16-byte
 * chunk that starts left of P (resp. Q) must be readable.  dtype DG_BF16, DG_F32, or DG_F32X3 (fp32
 * operands, split-bf16 contraction). */
int dg_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb,
               float* out, int64_t ldo, int64_t split_stride, int n_splits,
               int R, int P, int Q, int dtype, void* stream);

/* Grouped form of dg_gemm_tn: n independent weight-gradient problems in ONE launch, each over its whole
 * contraction (no split, no partial slabs, no reduction pass): out_i[P_i,Q_i] = sum_r A_i[r,P_i] * B_i[r,Q_i].
 * The 128x128 output tiles of all problems are dealt to persistent workgroups, so the step's ~25 small dW
 * GEMMs (ref: autograd of every nn.Linear, src/model_component.py:321-323,392-393,454, src/model.py:599) fill
 * the chip together at the end of backward.  dtype DG_BF16: bf16 operands, R_i a multiple of 64, alignment as for dg_gemm_tn.
 * dtype DG_FP8_E5M2 (precision "fp8"): A = dY as OCP e5m2, B = X as OCP e4m3 -- the very copies the fp8 dX / forward GEMMs
 * consumed -- one byte per element, R_i a multiple of 128, lda / ldb multiples of 16, scale_a / scale_b the dequantisation
 * factors dg_fp8_quantize* left for them; fp32 accumulation, v_mfma_f32_16x16x128_f8f6f4.
 * The operands must stay alive until this call (the caller keeps dY of every Linear). */
typedef struct dg_tn_problem {
    const void* A; int64_t lda;     /* dY [R,P] */
    const void* B; int64_t ldb;     /* X  [R,Q] */
    float* out; int64_t ldo;        /* dW [P,Q] fp32, overwritten */
    int R, P, Q, reserved;
    const float* scale_a;           /* fp8 operands only: device scalars, dW = scale_a[0] * scale_b[0] * sum_r qA qB */
    const float* scale_b;
} dg_tn_problem;
int dg_gemm_tn_grouped(const dg_tn_problem* problems, int n, int dtype, void* workspace, int64_t workspace_bytes, void* stream);
/* Optional workspace (device memory of dg_gemm_tn_grouped_workspace_bytes(problems, n) bytes, zero-filled ONCE by the
 * caller and then left to the library between calls on one stream): lets the kernel cut every tile's contraction into
 * two halves run by different workgroups when that shortens the schedule (381 tiles on 256 CUs: 3 rounds of half
 * tiles instead of 2 rounds of whole ones).  The halves are summed first + second, a fixed order.  NULL = no split.
 * A second half waits (spins on a flag) for the first half of its tile.  The launch rules make the producer an earlier item
 * of a LOWER-numbered workgroup that never waits itself: every tile is cut only when each workgroup gets one item (2 * tiles
 * <= #CUs: workgroup tiles + t waits for workgroup t); otherwise only the leftover tiles of the last round are cut, their
 * first halves run FIRST on even XCDs and their second halves LAST on the next-numbered workgroup.  Under in-order workgroup
 * dispatch the wait therefore resolves whatever part of the grid is resident.  It is bounded all the same (~1 s): a wave
 * that runs out sets the sticky error word in the LAST 16 BYTES of the workspace (uint32, non-zero = some result of some
 * launch since the workspace was zeroed is invalid) instead of hanging the GPU; the host may read it at any sync point.
 * Layout.  A call of more than 64 (bf16) or 48 (fp8) problems is several launches on the one workspace.  With T = the tiles
 * (256 x 128) of the call's largest launch under EITHER chunking -- the size function has no dtype argument --
 *   [0, T * 128 KB)                  partials, tile t of a launch at t * 128 KB (8 waves x 16 KB);
 *   [T * 128 KB, T * 128 KB + 32 T)  hand-over flags, 8 words per tile, at the SAME place for every launch of the call;
 *   the last 16 bytes                the sticky error word,
 * so dg_gemm_tn_grouped_workspace_bytes = T * (128 KB + 32) + 16, "the last 16 bytes" are those of that size whatever
 * workspace_bytes says, and no launch's flags lie where another launch of the call keeps partials.  DG_ERR_ARG, before
 * anything is launched, if workspace_bytes is less than any launch of the call needs. */
int64_t dg_gemm_tn_grouped_workspace_bytes(const dg_tn_problem* problems, int n);

/* out[i] = sum_{g < n_partials} partials[g*stride + i], i < n.  Deterministic order. */
int dg_reduce_partials(const float* partials, int64_t stride, int n_partials,
                       float* out, int64_t n, void* stream);

/* Column sums (bias gradients): partial g (< n_partials) of sum_m A[m, n], fp32. */
int dg_colsum(const void* A, int64_t lda, int dtype, float* part, int64_t part_stride,
              int n_partials, int M, int N, void* stream);

/* g = (dtype)(dy * keep/(1-p)) -- backward of the nn.Dropout after proj / FFN
 * (ref: src/model_component.py:454,324); with p == 0 a plain cast.  relu_mask (nullable, fp32
 * [M,N]): additionally g = 0 where relu_mask <= 0 (backward of the ReLU that ends FeedForward,
 * ref: src/model_component.py:118-121).  Optionally also emits the column-sum partials of g (the
 * bias gradient of the Linear in front). g may be NULL when only the column sums are wanted. */
int dg_dropout_bwd_cast(const void* dy, int dy_dtype /* DG_F32; DG_BF16 with a bf16 g and no relu_mask */, int64_t lddy, void* g, int64_t ldg, int dtype,
                        int M, int N, float p, const uint32_t* rng_state, uint32_t site,
                        const float* relu_mask, int64_t ldmask,
                        float* colsum_part, int64_t part_stride, int n_partials, void* stream);

/* out = (out_dtype) in, n elements: f32 -> bf16 (shadow copies), bf16 -> f32, f32 -> f32. */
int dg_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, void* stream);
/* out[c, r] = (dtype) in[r, c] for r < R, c < Cc; out has leading dim ldo >= R and columns
 * R..ldo-1 are zero-filled (W^T operands for the dX GEMMs, K padded to the MFMA granule). */
int dg_transpose_cast(const float* in, int64_t ldi, void* out, int64_t ldo, int dtype,
                      int R, int Cc, void* stream);

/* The same for n_desc matrices in ONE launch.  desc: device array of n_desc x 8 int64
 * {in ptr, out ptr, ldi, ldo, R, Cc, first_tile, tiles_x} where a matrix owns tiles_x * ceil(ldo/64)
 * consecutive 64x64 tiles starting at first_tile (tiles_x = ceil(Cc/64)); total_tiles = their sum.
 * in_dtype: DG_F32 (the fp32 masters) or, for bf16 output, DG_BF16 (the bf16 shadow copy: same values, half the read). */
int dg_transpose_cast_batched(const int64_t* desc, int n_desc, int total_tiles, int in_dtype, int out_dtype, void* stream);
/* The same for one-byte elements (precision fp8: the e4m3 copy of every W^T from the e4m3 copy of W, scales unchanged), tiles of
 * 128 x 128: first_tile / tiles_x of the desc rows count 128-wide tiles (tiles_x = ceil(Cc / 128), a matrix owns tiles_x *
 * ceil(ldo / 128) of them).  Rows of `out` beyond R (ldo > R: padding) are written as zeros. */
int dg_transpose_u8_batched(const int64_t* desc, int n_desc, int total_tiles, void* stream);

/* ---------------------------------------------------------------------------------------
 * Causal multi-head attention -- ref: Head2.forward src/model_component.py:392-405 for every
 * head of MultiHeadAttention3 (:453), i.e. K5's output to K11:
 *   S = (Q K^T) * scale; mask j > i to -inf; P = softmax(S); P = dropout(P) (no renorm); O = P V.
 * qkv: [B*T, 3*NH*H] with column blocks [Q heads | K heads | V heads]; out: [B*T, NH*H], head h
 * at columns h*H.. (the torch.cat of :453 disappears).  lse [B,NH,T] = log-sum-exp of the scaled
 * masked scores, saved for backward.  Dropout element index = ((b*NH+h)*T+i)*T+j. */
/* keep_bits (nullable; round 3): dg_attn_keep_bits_bytes(...) bytes in which the forward pass leaves its dropout keep decisions
 * (16 wave masks per unmasked 32 x 32 tile, opaque layout); handed to dg_attn_bwd the dQ pass selects with them instead of
 * hashing every score again (same decisions either way: the masks are the hash's compare results).  0 bytes = the shape takes
 * the generic kernels, which have no such path: pass NULL. */
int64_t dg_attn_keep_bits_bytes(int B, int T, int NH, int H, int dtype);
int dg_attn_fwd(const void* qkv, void* out, float* lse, int B, int T, int NH, int H,
                float scale, float dropout_p, const uint32_t* rng_state, uint32_t site,
                int dtype, void* keep_bits, int64_t keep_bits_bytes, void* stream);
/* dqkv [B*T, 3*NH*H] from dout.  workspace: at least B*NH*T floats (delta = rowsum(dO * O)); with
 * dg_attn_bwd_workspace_bytes(...) bytes the dQ pass also leaves the dropped-out probabilities and dS of every
 * unmasked 32 x 32 tile behind it and the dK/dV pass consumes them instead of recomputing scores, exp and the
 * dropout hash (bf16, head size 64; 55 MB at the scaled config). */
int64_t dg_attn_bwd_workspace_bytes(int B, int T, int NH, int H, int dtype);
int dg_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                void* dqkv, void* workspace, int64_t workspace_bytes, int B, int T, int NH, int H,
                float scale, float dropout_p, const uint32_t* rng_state, uint32_t site,
                int dtype, const void* keep_bits, int64_t keep_bits_bytes, void* stream);

/* Precision "fp8" (round 3): the attention kernels leave their outputs a second time as fp8, so that the cast launches in front of
 * the projection (o as e4m3: the x operand of `proj` and of its weight gradient -- ref: MultiHeadAttention3.proj,
 * src/model_component.py:454) and in front of the QKV dX GEMM (dqkv as e5m2: its gradient operand and the dY of the QKV weight
 * gradient -- ref: autograd through the packed query / key / value Linears, :392-393) disappear.  Delayed per-tensor scaling as in
 * dg_fp8_quantize_delayed, with a history format of the kernels' own: hist3 = DG_ATTN_FP8_HIST floats per call site (16-byte
 * aligned; three slots of 64 partial maxima, each partial on a 128-byte line of its own -- partial i of slot s is word
 * (s * 64 + i) * 32) -- slot step % 3 (step = step_state[2]) collects this step's maxima by atomic max, slot (step + 2) % 3 holds
 * last step's (the scale of this launch, *scale_inv = its inverse), slot (step + 1) % 3 is cleared for the next step; seed every
 * partial with a just-in-time maximum.  q8: [B*T, NH*H] (forward) / [B*T, 3*NH*H] (backward), one byte per element, 16-byte aligned.  only8 (backward only): the
 * bf16 dqkv is not written.  dg_attn_fp8_out_supported: 1 when the shape takes the MFMA kernels (else cast). */
#define DG_ATTN_FP8_HIST (3 * 64 * 32)
typedef struct dg_attn_fp8_out {
    void* q8; float* hist3; const uint32_t* step_state; float* scale_inv; int only8;
} dg_attn_fp8_out;
int dg_attn_fp8_out_supported(int B, int T, int NH, int H, int dtype);
int dg_attn_fwd_fp8(const void* qkv, void* out, float* lse, int B, int T, int NH, int H,
                    float scale, float dropout_p, const uint32_t* rng_state, uint32_t site,
                    int dtype, void* keep_bits, int64_t keep_bits_bytes, const dg_attn_fp8_out* fp8, void* stream);
int dg_attn_bwd_fp8(const void* qkv, const void* out, const void* dout, const float* lse,
                    void* dqkv, void* workspace, int64_t workspace_bytes, int B, int T, int NH, int H,
                    float scale, float dropout_p, const uint32_t* rng_state, uint32_t site,
                    int dtype, const void* keep_bits, int64_t keep_bits_bytes, const dg_attn_fp8_out* fp8, void* stream);

/* Document-masked attention (opt-in): no attention across a separator token of a packed corpus -- ref: get_batch (src/model.py) cuts
 * its windows out of ONE concatenated text, and Head2.forward src/model_component.py:392-405 (the tril mask of :401) lets a token
 * attend to the document before it; there is no ATen call site for the mask itself, it is one more compare in the score loops of
 * K5..K11's kernels.  A document ends WITH its separator:
 *   starts[b, t] = 1 + max{ j < t : ids[b, j] == sep }, or 0 without such a j     (0 <= starts[t] <= t, non-decreasing in t)
 * and query i attends to keys starts[i] <= j <= i.  Everything else is dg_attn_fwd's: scale, softmax, dropout without
 * renormalisation, the dropout element index on absolute positions.  A masked probability and its gradient are exact zeros.
 * dg_doc_starts: ids int64 [B, ld_ids >= T], starts int32 [B*T]; a max-scan along each row, no atomics. */
int dg_doc_starts(const int64_t* ids, int64_t ld_ids, int B, int T, int64_t sep, int32_t* starts, void* stream);
/* dg_attn_fwd_fp8 / dg_attn_bwd_fp8 (fp8 nullable) with the document starts.  starts == NULL: exactly their launches.  On a shape
 * that takes the MFMA kernels the backward entry needs the tile scratch (workspace of dg_attn_bwd_workspace_bytes): DG_ERR_ARG
 * without.  The kernels assume the invariants above; other values are clamped to [0, t] (results unspecified, accesses in bounds). */
int dg_attn_fwd_doc(const void* qkv, void* out, float* lse, int B, int T, int NH, int H,
                    float scale, float dropout_p, const uint32_t* rng_state, uint32_t site,
                    int dtype, void* keep_bits, int64_t keep_bits_bytes, const dg_attn_fp8_out* fp8,
                    const int32_t* starts, void* stream);
int dg_attn_bwd_doc(const void* qkv, const void* out, const void* dout, const float* lse,
                    void* dqkv, void* workspace, int64_t workspace_bytes, int B, int T, int NH, int H,
                    float scale, float dropout_p, const uint32_t* rng_state, uint32_t site,
                    int dtype, const void* keep_bits, int64_t keep_bits_bytes, const dg_attn_fp8_out* fp8,
                    const int32_t* starts, void* stream);

/* Single-query attention against a K/V cache for generate() -- ref: src/model.py:625-635 re-runs the
 * whole forward per new token; with the cache only the new position is computed.  qkv_cache:
 * [B, Tcap, 3*NH*H] in the training layout (row = position; the QKV GEMM of the new token writes row t);
 * out [B, NH*H] = attention output of query row t over keys 0..t.  Same arithmetic and order as the
 * generic forward kernel, so fp32 decoding is bit-identical to the uncached forward. */
int dg_attn_decode(const void* qkv_cache, void* out, int B, int Tcap, int t, int NH, int H,
                   float scale, int dtype, void* stream);

/* dg_attn_decode with t = L - 1 read from the decode state (4 device uint32 in the rng_state format, {seed_lo, seed_hi, L, 0},
 * L = current length of the sequence; dg_state_advance does L += 1), so that a captured decode step replays for every token --
 * ref: src/model.py:625-635.  The new token's q/k/v row arrives in the fixed staging buffer qkv_row [B, 3*NH*H]; the kernel
 * writes it into qkv_cache[b, t] and attends over keys 0..t with dg_attn_decode's arithmetic and order (fp32 decoding stays
 * bit-identical to the uncached forward).  L == 0 or L - 1 >= Tcap: nothing is read or written. */
int dg_attn_decode_append(const void* qkv_row, void* qkv_cache, void* out, const uint32_t* state, int B, int Tcap,
                          int NH, int H, float scale, int dtype, void* stream);

/* The embedding of a decode step, position read from the decode state -- ref: src/model.py:625 (crop to the context window)
 * + :595-597.  ids: int64 [B, ld_ids], the sequence so far in columns 0..L-1; pos has Tw rows (the context length).
 *   mode 0: x[b, :]    = tok[ids[b, L-1]] + pos[L-1]             (one position; 1 <= L <= Tw)
 *   mode 1: x[b, i, :] = tok[ids[b, L-Tw+i]] + pos[i], i < Tw    (the full sliding window; L >= Tw)
 * ids are clamped to [0, V) as in dg_embed_fwd.  An L outside the mode's range or beyond ld_ids writes nothing. */
int dg_embed_window(const int64_t* ids, int64_t ld_ids, const uint32_t* state, const float* tok, const float* pos,
                    float* x, int B, int Tw, int C, int V, int mode, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sampling on the device -- ref: src/model.py:625-635: F.softmax at :631 and torch.multinomial at :633, with the temperature
 * and top-k filter every GPT sampler has.  One token per row of fp32 logits [M, V] (leading dimension ldl; columns V..ldl-1
 * are never read).  params (device): {float inv_temp, int32 top_k}, read by the kernel so that a captured graph picks up new
 * settings.  state: the decode state {seed_lo, seed_hi, L, 0}.
 *   inv_temp > 0:  z_j = logits_j * inv_temp (fp32).   inv_temp == 0: greedy -- the lowest index among the maxima, no random
 *                  number consumed, probs one-hot.
 *   top_k == 0 (or >= V): off; else tau = the k-th largest z and every j with z_j >= tau is kept (ties at the threshold are all
 *                  kept).  -inf logits are never kept and never sampled.
 *   e_j = exp(z_j - max z) for kept j (the subtraction in fp32, exp and everything after it in fp64), else 0;  S = sum e_j;  p_j = e_j / S.
 *   u = (h >> 8) * 2^-24,  h = dg_hash_w(dg_site_key(seed_lo, seed_hi, L, DG_SITE_SAMPLE = 0x53414D50), row * DG_WEYL)
 *   token = the smallest n with sum_{j <= n} e_j > u * S; if rounding leaves none, the last kept index.
 * Outputs (each nullable, not both): ids int64 -- ld_ids > 0: row m's token goes to ids[m * ld_ids + L] (not written when
 * L >= ld_ids); ld_ids == 0: to ids[m] -- and probs [M, ldp] fp32, the filtered distribution p.  state may be NULL without ids.
 * One workgroup per row, no floating-point atomics: the result is a pure function of (logits, state, params, row).  V <= 2^20. */
int dg_sample_rows(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                   int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, void* stream);

/* dg_sample_rows with a top-p (nucleus) and a min-p filter after top-k.  params (device, four words):
 * {float inv_temp, int32 top_k, float top_p, float min_p}; everything else as dg_sample_rows.  0 < top_p <= 1, 1 = off;
 * 0 <= min_p <= 1, 0 = off (the kernel takes a top_p outside (0, 1) as off and a min_p above 1 as 1).  Greedy ignores both.
 *   K0 = the set top-k keeps (z_j >= tau_k, never -inf), e_j = exp((double)(z_j - max z)) as above.
 *   min-p:  K1 = { j in K0 : e_j >= (double)min_p }.  The maximum has e = 1: K1 is never empty.
 *   top-p:  integer masses, so that no result depends on a summation order:
 *             w_j = rint(e_j * 2^40) as uint64 for j in K1, else 0;   S1 = sum w_j  (exact: V <= 2^20 gives S1 <= 2^60);
 *             G(t) = sum { w_i : i in K1, z_i > t };   T = (double)top_p * (double)S1;
 *             K = { j in K1 : (double)G(z_j) < T }.
 *           G depends on j only through z_j and is monotone, so K is a threshold set z_j >= tau_p and ties at the threshold are
 *           all kept: in a descending sort, the shortest prefix whose mass reaches top_p of the mass left by top-k and min-p,
 *           plus its ties.
 *   Then as dg_sample_rows on K: S = sum_{j in K} e_j in fp64 in index order, p_j = e_j / S on K, else 0, the same u and the
 *   same token rule.  Rows without a finite logit behave as in dg_sample_rows.
 * With top_p == 1 and min_p == 0 tokens and probs are bit-identical to dg_sample_rows; a filter that is off costs no pass. */
int dg_sample_rows_nucleus(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                           int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, void* stream);

/* dg_sample_rows_nucleus with repetition / presence / frequency penalties, a logit bias and stop tokens.  control (device, 16
 * 32-bit words, read by the kernel so that one captured graph serves every setting):
 *   {float inv_rep, float rep, float presence, float frequency, int32 use_bias, int32 n_stop, int32 pad_id, int32 reserved,
 *    int32 stop[DG_SAMPLE_MAX_STOP]}
 * bias: fp32 [V], read only when use_bias != 0.  counts: int32 [M, ldc], ldc >= V, nullable: counts[m, j] = how often token j
 * occurs in row m's sequence so far, prompt included.  lengths: int32 [M], nullable: 0 = the row is running, else its final
 * length, stop token included.
 *   Every place where dg_sample_rows reads logits_i reads y_i instead; with c = counts[m, i] (0 without counts) each line is one
 *   fp32 rounding, in this order:
 *     y = c > 0 ? (x > 0 ? x * inv_rep : x * rep) : x      repetition penalty (CTRL, HF's repetition_penalty); inv_rep is
 *                                                          fp32(1 / rep) made on the host: a correctly rounded product that
 *                                                          numpy restates bit for bit, within one rounding of HF's x / rep
 *     y = y - (c > 0 ? presence : 0)
 *     y = y - frequency * (float)c
 *     y = use_bias ? y + bias[i] : y                       a bias of -inf bans the token
 *   Greedy, top-k, min-p, top-p, the fp64 sums, u, the token rule and the rows without a finite entry: as in
 *   dg_sample_rows_nucleus on y.  With rep = inv_rep = 1, presence = frequency = 0 and use_bias = 0, y == x bit for bit.
 * Only where the token t of row m is written (ids given, L < ld_ids or ld_ids == 0), the thread that writes it also does
 *   counts[m, t] += 1 (one workgroup per row: a plain load, add and store), and with lengths and ld_ids > 0:
 *   lengths[m] = L + 1 if t is one of stop[0 .. min(n_stop, DG_SAMPLE_MAX_STOP)).
 * A row that arrives with lengths[m] != 0 is finished: pad_id goes to ids[m, L] (L < ld_ids), no logit is read, counts and
 * lengths stay as they are (and its row of probs, if asked for, is not written).  With probs and no ids, counts is only read.
 * Refused: a NULL control, counts with ldc < V, lengths without ids or with ld_ids == 0, and what dg_sample_rows_nucleus
 * refuses.  No floating-point atomics: a pure function of (logits, state, params, control, bias, counts, lengths, row). */
#define DG_SAMPLE_MAX_STOP 8
int dg_sample_rows_control(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                           int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, const void* control,
                           const float* bias, int32_t* counts, int64_t ldc, int32_t* lengths, void* stream);

/* dg_sample_rows_control for a batch whose rows start at different lengths (right-padded prompts) and share one position L.
 * spans (device): int32 [M, 2], {first, end} per row with 1 <= first < end: first = the row's prompt length, the position of its
 * first sampled token; end = first + its budget of new tokens.  ids, lengths and ld_ids > 0 are required.  With L = state[2], per
 * row, decided before anything else:
 *   lengths[m] != 0:  finished, as in dg_sample_rows_control: pad_id goes to ids[m, L] (L < ld_ids), nothing else happens.
 *   L < first:        forced -- ids[m, L] already holds a prompt token.  No logit is read (the row may hold anything, NaN
 *                     included), nothing is drawn, and ids, counts, lengths and the row of probs stay as they are.
 *   otherwise:        dg_sample_rows_control on the same operands, bit for bit: y, the filters, the fp64 sums, the same u (keyed
 *                     by (seed, L, row): a row's draws do not depend on what the other rows do), the token rule,
 *                     counts[m, t] += 1 and the stop rule.  Then, if lengths[m] is still 0 and L + 1 >= end, the thread that
 *                     wrote the token also writes lengths[m] = L + 1: the budget is used up, and from the next position on the
 *                     row is padded like a stopped one.
 * Refused: NULL spans, NULL lengths, NULL ids, ld_ids == 0, and what dg_sample_rows_control refuses. */
int dg_sample_rows_ragged(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                          int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, const void* control,
                          const float* bias, int32_t* counts, int64_t ldc, int32_t* lengths, const int32_t* spans, void* stream);

/* Token counts for dg_sample_rows_control: counts[m, clamp(ids[m * ld_ids + j])] += 1 for j < n (n <= ld_ids), ids clamped to
 * [0, V) as in dg_embed_fwd.  accumulate == 0: row m's V counts are zeroed first.  One workgroup per row (its own barrier
 * orders the zeroes before the increments), integer atomics: the result does not depend on an order.  counts: int32 [M, ldc],
 * ldc >= V; columns V..ldc-1 are never touched.  n == 0 with accumulate == 0 just zeroes. */
int dg_token_counts(const int64_t* ids, int64_t ld_ids, int M, int n, int V, int32_t* counts, int64_t ldc,
                    int accumulate, void* stream);

/* dg_token_counts with a prefix length per row: row m counts ids[m, 0 .. n_m), n_m = clamp(n_rows[m * n_stride], 0, ld_ids)
 * (n_rows: device int32; the `first` column of dg_sample_rows_ragged's spans is passed with n_stride = 2).  Zeroing, the
 * clamping of ids, the integer atomics and the untouched columns V..ldc-1: as in dg_token_counts. */
int dg_token_counts_rows(const int64_t* ids, int64_t ld_ids, int M, const int32_t* n_rows, int64_t n_stride, int V,
                         int32_t* counts, int64_t ldc, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * Token log-probabilities: how likely the model found a token, for generate(return_logprobs=) and score().  What OpenAI's
 * `logprobs`, HF's compute_transition_scores and vLLM report: log_softmax of the RAW logits at the token -- no temperature,
 * penalty, bias or filter.  One workgroup per row of logits [M, V] (leading dimension ldl; columns V..ldl-1 are never read),
 * logits_dtype DG_F32 or DG_BF16 (widened exactly).  V <= 2^20.  Per row m, with x the row as fp32:
 *   m* = max_i x_i (fp32);  d_j = x_j - m*, ONE fp32 rounding (never contracted);  e_j = exp((double)d_j);
 *   Z  = sum_i e_i in fp64, in the order of dg_sample_rows' S: NT = 256 threads for V <= 8192, else 1024; chunk = ceil(V / NT);
 *        thread t adds e_j, j in [t * chunk, min((t + 1) * chunk, V)), in index order starting from 0.0; in every wave of 64
 *        consecutive threads the chunk sums go through an inclusive scan, for o = 1, 2, 4, .., 32: c[l] += c[l - o] for every
 *        l >= o at once; the wave's total is c[63]; Z = ((0.0 + total_0) + total_1) + ... in wave order.
 *   lp_j = (float)((double)d_j - log(Z)).  Never log(p_j): a dominated token gets a large finite negative value, not -inf from
 *        an underflowing p.  x_j = -inf gives -inf; a row without a finite entry gives NaN, as torch.log_softmax does.
 * The token t of row m, clamped to [0, V) as in dg_embed_fwd, and the output element e:
 *   ld_tok > 0:  L = state[2] (the decode state {seed_lo, seed_hi, L, 0}); t = tokens[m * ld_tok + L], e = m * ld_tok + L --
 *                column L of outputs laid out like tokens.  L >= ld_tok: nothing is read or written.
 *   ld_tok == 0: t = tokens[m], e = m.
 * Outputs, each nullable:
 *   tok_lp   fp32  [e]:  lp_t
 *   tok_rank int32 [e]:  #{i : x_i > x_t} + #{i < t : x_i == x_t} -- 0 exactly when t is what greedy picks
 *   top_ids  int32 [e * DG_LOGPROBS_MAX_TOP + s], top_lp fp32 likewise (both or neither): slot s < n holds the s-th largest x_i
 *            > -inf and its lp, descending, ties by lowest index first (the order of the fp32 bit patterns: -0 sorts below
 *            +0), n = min(top_n, DG_LOGPROBS_MAX_TOP, the number of entries > -inf).  Every other slot of the
 *            DG_LOGPROBS_MAX_TOP holds id = -1, lp = -inf.
 * top_n (device int32, nullable = 0) is read by the kernel, so that one captured graph serves every setting; a value above
 * DG_LOGPROBS_MAX_TOP is clamped, 0 (or no top_ids) runs no selection pass.
 * Skipped rows -- no logit is read, no byte is written -- need ld_tok > 0; lengths int32 [M] and spans int32 [M, 2] (those of
 * dg_sample_rows_control / _ragged) are each nullable:
 *   lengths[m] != 0 && L >= lengths[m]:  the row finished before this position.  Its stop token, at L = lengths[m] - 1, IS scored.
 *   spans given && L < spans[2 * m]:     the row is forced, still inside its prompt.
 * Refused, nothing launched: NULL logits or tokens; ld_tok > 0 without state; lengths or spans with ld_tok == 0; top_ids without
 * top_lp or the reverse; a dtype other than the two; V > 2^20; ldl < V.
 * No floating-point atomics: a pure function of (logits, tokens, state, lengths, spans, top_n). */
#define DG_LOGPROBS_MAX_TOP 20
int dg_token_logprobs(const void* logits, int logits_dtype, int64_t ldl, int M, int V, const int64_t* tokens,
                      int64_t ld_tok, const uint32_t* state, const int32_t* lengths, const int32_t* spans,
                      const int32_t* top_n, float* tok_lp, int32_t* tok_rank, int32_t* top_ids, float* top_lp,
                      void* stream);

/* ---------------------------------------------------------------------------------------
 * Cross entropy, mean over rows -- ref: F.cross_entropy at src/model.py:604-607 (K16).
 * loss_rows[m] = logsumexp(logits[m,:]) - logits[m,target[m]].  If dlogits != NULL also writes
 * dlogits[m,n] = (softmax(logits[m,:])[n] - [n == target]) * grad_scale (* *grad_scale_dev) in
 * `dtype`, with columns
 * V..ldd-1 zero-filled.  dg_reduce_mean then gives the scalar loss.
 * logits_dtype DG_F32, or DG_BF16 (rows up to 53248 wide, bf16 gradient): the engine's lm_head at the GPT-2 vocabulary writes
 * bf16 logits (0.82 GB instead of 1.65 GB at M = 8192) and lets this kernel overwrite them IN PLACE with their gradient
 * (dlogits == logits, ldd == ldl). */
int dg_cross_entropy(const void* logits, int logits_dtype, int64_t ldl, const int64_t* targets, float* loss_rows,
                     void* dlogits, int64_t ldd, int dtype, float grad_scale,
                     const float* grad_scale_dev /* nullable: multiplies grad_scale */,
                     int M, int V, void* stream);
/* dg_cross_entropy on bf16 logits (large vocabularies, gradient written in place or elsewhere in bf16) that ALSO leaves the
 * gradient as OCP e5m2 for precision "fp8": dlogits_fp8 [M, ld8] = e5m2(dlogits * 57344 / grad_scale) -- |softmax - onehot| <= 1
 * bounds |dlogits| by grad_scale, so the scale is known a priori (no amax pass, no history) and the consumer's dequantisation
 * factor is the constant grad_scale / 57344.  ld8 % 16 == 0, V <= ld8 <= ldd; columns V .. ld8 - 1 are written as zeros (the dX
 * contraction of lm_head runs over the padded width).  ref: F.cross_entropy at src/model.py:604-607. */
int dg_cross_entropy_fp8(const void* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                         float grad_scale, int M, int V, void* dlogits_fp8, int64_t ld8, void* stream);
/* The loss head of a captured step at a small vocabulary (ldd <= 128, fp32 logits): dg_cross_entropy + the column sums of
 * the gradient (lm_head bias gradient: partial row b of colsum_part = rows [b * ceil(M / n_partials), ...), fp32, nullable) +
 * the scalar loss (loss_out[0] = loss_scale * sum of loss_rows, added in a fixed order by the workgroup that finishes last;
 * loss_part: n_partials floats of scratch, loss_counter: one device word, zero before the first launch and again after
 * every launch; all three nullable together) in ONE launch of n_partials (<= 2048) workgroups. */
int dg_cross_entropy_fused(const float* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                           int dtype, float grad_scale, int M, int V, float* colsum_part, int64_t part_stride, int n_partials,
                           float* loss_part, uint32_t* loss_counter, float* loss_out, float loss_scale, void* stream);
/* The three entry points above with the two knobs of a training objective: label smoothing eps = label_smoothing in [0, 1)
 * (F.cross_entropy(label_smoothing=)) and the z-loss zeta = z_loss >= 0.  Per row, lse = logsumexp(logits[m,:]), p = softmax, t the target:
 *   loss_rows[m] = lse - (1 - eps) x_t - (eps / V) sum_{i < V} x_i + zeta lse^2
 *   dlogits[m,n] = grad_scale (p_n (1 + 2 zeta lse) - (1 - eps) [n == t] - eps / V),   columns V .. ldd - 1 zero
 * The sum runs over the V logits only, whatever columns V .. ldl - 1 hold.  With zeta > 0 a gradient row sums to 2 zeta lse grad_scale;
 * the fused head's column-sum partials are the sums of what was written and loss_out = loss_scale * sum of loss_rows.  The e5m2
 * copy's a-priori scale needs |dlogits| <= grad_scale, which label smoothing keeps and a z-loss does not: the fp8 entry takes
 * label_smoothing only.  Values outside the ranges (or not finite): DG_ERR_ARG.  Both at 0: the old entry point, bit for bit. */
int dg_cross_entropy_smooth(const void* logits, int logits_dtype, int64_t ldl, const int64_t* targets, float* loss_rows,
                            void* dlogits, int64_t ldd, int dtype, float grad_scale, const float* grad_scale_dev, int M, int V,
                            float label_smoothing, float z_loss, void* stream);
int dg_cross_entropy_fp8_smooth(const void* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                float grad_scale, int M, int V, void* dlogits_fp8, int64_t ld8, float label_smoothing, void* stream);
int dg_cross_entropy_fused_smooth(const float* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                  int dtype, float grad_scale, int M, int V, float* colsum_part, int64_t part_stride, int n_partials,
                                  float* loss_part, uint32_t* loss_counter, float* loss_out, float loss_scale,
                                  float label_smoothing, float z_loss, void* stream);
/* ignore_index (F.cross_entropy(ignore_index=)): rows whose target equals ignore_index -- any int64, inside [0, V) or not -- are
 * left out, and the mean is taken over the N rows that remain.
 *   dg_ce_count_valid: out[0] = (float)N, out[1] = 1.0f / (float)N (one correctly rounded fp32 division; +inf at N = 0), N = #{m <
 *   M : targets[m] != ignore_index}.  One launch of one workgroup, an integer sum, no host involvement: safe under graph capture.
 *   dg_cross_entropy_ignore / dg_cross_entropy_fused_ignore: dg_cross_entropy_smooth / dg_cross_entropy_fused_smooth with
 *     loss_rows[m] = keep_m l_m                            (an ignored row: exactly 0)
 *     dlogits[m,n] = keep_m g_mn grad_scale inv_count[0]   (an ignored row: STORED as zeros, columns V .. ldd - 1 included, in place too)
 *   l, g the row objective and gradient above, inv_count a device pointer to 1 / N (out + 1 of dg_ce_count_valid; NULL: DG_ERR_ARG).
 *   An ignored row is recognised from its target before any of its logits is read.  The fused head's column-sum partials hold the
 *   rows that count and loss_out = loss_scale * inv_count[0] * sum of loss_rows; elsewhere dg_reduce_sum_scaled gives the mean.
 *   Targets that are neither ignore_index nor in [0, V) are clamped as in every entry above.  N = 0: the mean is NaN (0 * inf, as
 *   torch's) and every gradient row is zeros (torch's are NaN).  There is no fp8 form: the e5m2 scale rests on |dlogits| <= 1 / M. */
int dg_ce_count_valid(const int64_t* targets, int M, int64_t ignore_index, float* out, void* stream);
int dg_cross_entropy_ignore(const void* logits, int logits_dtype, int64_t ldl, const int64_t* targets, float* loss_rows,
                            void* dlogits, int64_t ldd, int dtype, float grad_scale, const float* grad_scale_dev, int M, int V,
                            float label_smoothing, float z_loss, int64_t ignore_index, const float* inv_count, void* stream);
int dg_cross_entropy_fused_ignore(const float* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                  int dtype, float grad_scale, int M, int V, float* colsum_part, int64_t part_stride, int n_partials,
                                  float* loss_part, uint32_t* loss_counter, float* loss_out, float loss_scale,
                                  float label_smoothing, float z_loss, int64_t ignore_index, const float* inv_count, void* stream);
/* out[0] = scale * sum_i x[i] (single workgroup, fixed order). */
int dg_reduce_sum(const float* x, int64_t n, float scale, float* out, void* stream);
/* out[0] = scale * scale_dev[0] * sum_i x[i]: dg_reduce_sum's order, one more factor read on the device. */
int dg_reduce_sum_scaled(const float* x, int64_t n, float scale, const float* scale_dev, float* out, void* stream);

/* probs = softmax(logits) row-wise, fp32 -- ref: F.softmax at src/model.py:631 (generate). */
int dg_softmax_rows(const float* logits, int64_t ldl, float* probs, int64_t ldp, int M, int V,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * AdamW over one flat fp32 buffer -- ref: torch.optim.AdamW(model.parameters(), lr, betas)
 * at src/train.py:121,151 (eps 1e-8, weight_decay 1e-2 unless overridden):
 *   p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 *   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps),   t = rng_state.step + 1
 * hyper (device): {lr, beta1, beta2, eps, weight_decay}.  grad_scale multiplies g first
 * (1/world_size after a sum all-reduce).  Optionally refreshes a bf16 shadow copy of p.
 * advance_step != 0: the launch also does dg_state_advance -- the workgroup that finishes last writes step + 1 (word 3 of
 * rng_state is its arrival counter: zero before and after every launch).
 * dg_adamw_step and the four dg_adamw_step_* entries below are one kernel template, one argument check and one dispatch: each
 * entry names what it requires and which optional operands it takes, and every one decides DG_ERR_ARG before DG_ERR_ALIGN. */
int dg_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                  uint32_t* rng_state, float grad_scale, void* shadow_bf16, int advance_step, void* stream);

/* ---------------------------------------------------------------------------------------
 * Global-norm gradient clipping -- ref: torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) (norm_type 2,
 * error_if_nonfinite False) ahead of optimizer.step(), on the gradient the optimizer applies, without clipping it in place:
 *   dg_sumsq_partials: sum of squares of g[0, n) (fp32, 16-byte aligned), one fp64 partial per workgroup written to
 *     part[0, dg_sumsq_parts(n)).  The partition depends on n alone, so the partials are bitwise reproducible.  Several
 *     buffers (parameter groups) share one norm: each writes its own range of one partial array.
 *   dg_grad_norm_finalize: ONE workgroup sums part[0, n_parts) in index order (fp64) and writes, in fp32,
 *     out[0] = total_norm = grad_scale * sqrt(sum)          (what clip_grad_norm_ returns, before clipping)
 *     out[1] = coef = min(1, max_norm[0] / (total_norm + 1e-6))   (torch's formula; a NaN norm gives a NaN coef)
 *     max_norm is read from device memory (a captured graph picks up a new value without recapture).
 *   dg_adamw_step_clip: dg_adamw_step with grad_scale multiplied by clip_coef[0] (a device float, e.g. out + 1) inside the
 *     launch: the AdamW step on g * grad_scale * coef.  The stored gradient g is left unclipped.  A coefficient of exactly 1
 *     gives the same bits as dg_adamw_step. */
int64_t dg_sumsq_parts(int64_t n);
int dg_sumsq_partials(const float* g, int64_t n, double* part, void* stream);
int dg_grad_norm_finalize(const double* part, int n_parts, float grad_scale, const float* max_norm, float* out, void* stream);
int dg_adamw_step_clip(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, uint32_t* rng_state,
                       float grad_scale, const float* clip_coef, void* shadow_bf16, int advance_step, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-step learning rate and weight-decay groups inside the AdamW launch -- ref: torch.optim.lr_scheduler stepped after every
 * optimizer.step(), and torch.optim.AdamW over two parameter groups of which one has weight_decay = 0.
 *   s = rng_state.step (read once per workgroup, before any arrival),  t = s + 1
 *   lr_table (device fp32 [lr_table_len], lr_table_len >= 1; may be NULL with lr_table_len == 0):
 *     lr = lr_table[min(s, lr_table_len - 1)]  instead of hyper[0]: past the end of the table its last entry holds.
 *   no_decay_bits (device uint32 [ceil(ceil(n / 64) / 32)]; may be NULL): bit (G & 31) of word (G >> 5) covers the granule of
 *     elements [64 G, 64 G + 64).  A set bit: p *= 1.0f for those elements instead of p *= 1 - lr*wd, which is exact, so they
 *     get the bits dg_adamw_step gives with weight_decay = 0; every other element gets the bits it gets without a bitmap.
 *   clip_coef (device fp32 [1]; may be NULL): as in dg_adamw_step_clip.
 * With all three NULL the result is dg_adamw_step's, bit for bit; the lr that was used is written nowhere (the host knows the
 * table and the step).  One extra cached word per wave iteration (256 floats); no LDS, no further atomics.
 * DG_ERR_ARG: what dg_adamw_step refuses, a NULL lr_table with lr_table_len != 0, an lr_table with lr_table_len < 1. */
int dg_adamw_step_sched(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, uint32_t* rng_state,
                        float grad_scale, const float* clip_coef, const float* lr_table, int64_t lr_table_len,
                        const uint32_t* no_decay_bits, void* shadow_bf16, int advance_step, void* stream);

/* ---------------------------------------------------------------------------------------
 * Exponential moving average of the weights inside the AdamW launch.
 * dg_adamw_step_ema: dg_adamw_step_sched (same arguments, same p, m, v, shadow and state words, bit for bit, for every
 * combination of clip_coef / lr_table / no_decay_bits) which also updates ema (n floats, 16-byte aligned) from the weight the
 * same thread has just stored.  ema_hyper = device fp32 {decay, warmup}, read from device memory (a captured graph picks up a
 * new decay without recapture).  With s the step word the launch reads (before any advance):
 *     d_s = decay, or, if warmup != 0, min(decay, ((float)s + 1) / ((float)s + 10))          w = 1.0f - d_s
 *     s == 0:  ema[i] = p_new[i]                         (ema is not read: it may hold anything)
 *     s >  0:  ema[i] = ema[i] + (p_new[i] - ema[i]) * w (three separately rounded fp32 operations, never an FMA)
 * One more 16 B/lane stream (8 B/param); d_s and w once per workgroup; no LDS, no further atomics.
 * DG_ERR_ARG: what dg_adamw_step_sched refuses, a NULL ema, a NULL ema_hyper.  DG_ERR_ALIGN: also a misaligned ema.
 * dg_swap_f32: exchanges a[0, n) and b[0, n) (two distinct buffers, both 16-byte aligned) in one streaming launch. */
int dg_adamw_step_ema(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, uint32_t* rng_state,
                      float grad_scale, const float* clip_coef, const float* lr_table, int64_t lr_table_len,
                      const uint32_t* no_decay_bits, void* shadow_bf16, int advance_step, float* ema, const float* ema_hyper,
                      void* stream);
int dg_swap_f32(float* a, float* b, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------
 * Update guard -- ref: torch.amp.GradScaler's found_inf skip of optimizer.step(), and "skip the batch on a gradient spike":
 * the decision whether a step's update is applied is taken on the device, and a skipped update costs a launch.
 *   guard (4 device uint32) = {apply, total skipped, consecutive skipped, spare}
 * dg_grad_norm_finalize_guard: dg_grad_norm_finalize (the same workgroup, the same fixed-order fp64 sum, the same out[0] bits, and
 *   with max_norm != NULL the same out[1] bits; max_norm == NULL: out[1] is not written), which also writes
 *     guard[0] = apply = total_norm <= limit[0] && (loss == NULL || isfinite(loss[0]))
 *     guard[1] += !apply;   guard[2] = apply ? 0 : guard[2] + 1
 *   limit is a device fp32 scalar: FLT_MAX guards non-finite gradients alone (a NaN or Inf norm fails the comparison; +inf would
 *   let an Inf norm through).  dg_sumsq_partials squares in fp32, so a finite element beyond 1.8e19 in magnitude reads as
 *   non-finite as well.  DG_ERR_ARG: NULL part / out / limit / guard, n_parts <= 0.
 * dg_adamw_step_guard: dg_adamw_step_ema's arguments with ema (and ema_hyper, together), lr_table, no_decay_bits and clip_coef
 *   each NULL or not, plus guard and data_state (4 device uint32, may be NULL; not rng_state itself).
 *     guard[0] != 0: p, m, v, shadow, ema and rng_state[2] get the bits the unguarded entry with the same operands gives.
 *     guard[0] == 0: none of p / g / m / v / ema / shadow is read or written, and rng_state[2] stays: bias correction, the
 *       lr_table index and the EMA warm-up stand still.
 *   With advance_step != 0 and data_state != NULL the launch writes data_state[2] + 1 in either case: the word that keys
 *   dropout, the staged offset row and the fp8 amax slot moves on over a skipped update.  Every workgroup reads guard[0] once and
 *   registers at rng_state[3] (zero before and after every launch); the last one to arrive writes the words; nobody waits.
 *   DG_ERR_ARG: what dg_adamw_step_sched refuses, a NULL guard, one of ema / ema_hyper alone, data_state == rng_state. */
int dg_grad_norm_finalize_guard(const double* part, int n_parts, float grad_scale, const float* max_norm, float* out,
                                const float* limit, const float* loss, uint32_t* guard, void* stream);
int dg_adamw_step_guard(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, uint32_t* rng_state,
                        float grad_scale, const float* clip_coef, const float* lr_table, int64_t lr_table_len,
                        const uint32_t* no_decay_bits, void* shadow_bf16, int advance_step, float* ema, const float* ema_hyper,
                        const uint32_t* guard, uint32_t* data_state, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gradient accumulation -- ref: k x `(loss / k).backward()` summing into p.grad between two optimizer.step() calls.  One
 * streaming pass per micro-step over the flat fp32 gradient g[0, n) of that micro-batch:
 *   ctl (4 device uint32) = {j, k, arrival counter, 0}: j = micro-step inside the current optimizer step, k = accum_steps >= 1
 *   j == 0: acc[i] = g[i]  (acc is not read: it never needs a zero fill; 8 B/param)      j > 0: acc[i] = acc[i] + g[i]  (12 B/param)
 * exactly one fp32 add per element (no scale, no FMA), so acc holds the SUM of the micro-batch gradients: pass
 * grad_scale = 1 / k (times 1 / world_size) to dg_sumsq / dg_adamw_step for the mean.
 * loss / loss_out (both given or both NULL; device fp32 [1] / [2]): loss_out[0] = (j == 0 ? loss[0] : loss_out[0] + loss[0]), and on
 * the last micro-step (j == k - 1) loss_out[1] = loss_out[0] / k, the mean loss of the optimizer step.
 * The launch moves the counters on itself, like dg_adamw_step's advance: the workgroup that finishes last clears ctl[2], writes
 * ctl[0] = (j + 1 == k ? 0 : j + 1) and, with rng_state != NULL, rng_state[2] = step + 1 -- the micro-step word that keys dropout,
 * the staged offset row and the fp8 amax slot (rng_state[3] is not touched).  ctl[2] is zero before and after every launch.
 * DG_ERR_ARG: NULL acc / g / ctl, n <= 0, one of loss / loss_out alone.  DG_ERR_ALIGN: acc or g not 16-byte aligned. */
int dg_grad_accumulate(float* acc, const float* g, int64_t n, uint32_t* ctl, const float* loss, float* loss_out,
                       uint32_t* rng_state, void* stream);

/* ---------------------------------------------------------------------------------------
 * The row-local chain of one residual block in ONE launch (bf16 operands, C = 384, M % 64 == 0) -- ref:
 * src/model_component.py:454 (proj) + :505 (x + ...), :506 + :488-489 (LayerNorm 2), :320-325 (FeedForward3), the second
 * residual add, and the NEXT block's :505 LayerNorm 1 + :392-393,404 (its 3 * NH per-head Linears as one packed operand):
 *     x1 = x + dropout(o wproj^T + bproj; site_proj)      h2 = LN(x1; ln2w, ln2b)      f = relu(h2 w1^T + b1)
 *     x2 = x1 + dropout(f w2^T + b2; site_ffn)            h1 = LN(x2; ln1w, ln1b)      qkv = h1 wqkv^T
 * It replaces four dg_gemm_nt launches and two dg_layernorm_fwd launches per block and writes exactly what they wrote (the
 * tensors the backward pass reads): x1, mean2 / rstd2, h2, f, the ReLU sign bits in dg_gemm_nt's opaque layout for an
 * [M, 4C] output (dg_gemm_nt_sign_bits_bytes(M, 4 * C) bytes), x2, mean1 / rstd1, h1, qkv.  Dropout masks are those of
 * dg_gemm_nt's epilogue (same site keys and element indices).  A workgroup owns 64 rows and walks the whole chain for them.
 * The four weight operands (wproj [C, C], w1 [4C, C], w2 [C, 4C], wqkv [3C, C]; bf16, [out, in]) are passed PACKED: in the
 * order the kernel streams them, as written by dg_pack_chain_weights (same byte count as the matrix; refresh after every
 * optimizer step, like the W^T operands of the dX GEMMs).
 * mode 0: everything above.  mode 1 (last block): stops behind the second residual add and writes x2 as bf16 (x2_bf16, the
 * operand of lm_head; x2 / ln1* / h1 / wqkv / qkv unused).  mode 2 (head: the first block's LayerNorm 1 on the embedding
 * output): h1 = LN(x), qkv = h1 wqkv^T only. */
typedef struct dg_block_chain_args {
    int32_t mode, M, C;
    float eps;
    const void* o; const float* x;
    const void* wproj; const float* bproj; float* x1;
    const float* ln2w; const float* ln2b; float* mean2; float* rstd2; void* h2;
    const void* w1; const float* b1; void* f; uint8_t* sign_bits; int64_t sign_bits_bytes;
    const void* w2; const float* b2; float* x2; void* x2_bf16;
    const float* ln1w; const float* ln1b; float* mean1; float* rstd1; void* h1;
    const void* wqkv; void* qkv;
    float dropout_p; const uint32_t* rng_state; uint32_t site_proj, site_ffn;
} dg_block_chain_args;
int dg_block_chain_supported(int M, int C);
int dg_block_chain_fwd(const dg_block_chain_args* args, void* stream);
/* w [N, K] bf16 row-major with leading dimension ld (N % 384 == 0, K % 32 == 0) -> packed (N * K elements).  Batched form: a
 * device table of n_desc rows {src, dst, N, K, first stage of the matrix (prefix sum of N / 384 * K / 32), ld} (int64 each):
 * every weight matrix of a model in one launch of total_stages workgroups. */
/* touch every 128-byte line of [p, p + bytes) once from every XCD (p 128-byte aligned): an L2 warm-up for a weight stream that the
 * next launch reads from all workgroups in lockstep */
int dg_l2_warm(const void* p, int64_t bytes, void* stream);
int dg_pack_chain_weights(const void* w, int64_t ld, void* packed, int N, int K, void* stream);
int dg_pack_chain_weights_batched(const int64_t* desc, int n_desc, int total_stages, void* stream);

/* ---------------------------------------------------------------------------------------
 * The row-local chain of the BACKWARD pass between two attention-backward calls in ONE launch (bf16 operands and gradient
 * stream, C = 384, M % 64 == 0, M / 64 <= #CUs) -- ref: autograd through src/model_component.py:392-393,404 (dX of the packed
 * q / k / v Linears), :505 (LayerNorm 1 + residual branch), :324 (the Dropout of the block below), :322-323 (dX of the
 * second FFN Linear through the ReLU), :321 (dX of the first), :506 (LayerNorm 2 + residual branch), :454 (proj's Dropout, dX):
 *   [block l]     dh  = dqkv wqkvT        dx1 = LN'(dh; x, mean1, rstd1, ln1w) + dresid1       g1 = dropout_bwd(dx1; site_ffn_below)
 *   [block l - 1] df  = (g1 w2T) masked by sign_bits      dh2 = df w1T
 *                 dx2 = LN'(dh2; x1, mean2, rstd2, ln2w) + dx1      g2 = dropout_bwd(dx2; site_proj)      dout = g2 wprojT
 * It replaces four dg_gemm_nt launches and two dg_layernorm_bwd_fused launches and leaves what they left: df, g1, g2 (the dY
 * operands of the weight gradients), dx1 / dx2 (the bf16 gradient stream), dout (the attention backward's input) and the
 * partial rows of b1 (column sums of df), b2 / bproj (column sums of g1 / g2) and both LayerNorms' dgamma / dbeta: TWO rows
 * per 64-row block, row 2 * block + {0, 1} at `part_stride` floats (2 * M / 64 rows for dg_reduce_partials).  The LayerNorm
 * backward takes the dX GEMM's accumulators rounded to bf16 in registers (what the separate dX launch hands over).  The four weight
 * operands are the W^T shadows ([in, out] bf16) PACKED by dg_pack_chain_weights (wqkvT: N = C, K = 3C; w2T: N = 4C, K = C;
 * w1T: N = C, K = 4C; wprojT: N = C, K = C).  sign_bits: dg_gemm_nt's layout for an [M, 4C] output.
 * mode 0: everything above (dresid2 is dx1: pass the same pointer).  mode 1 (top of the stack): the second half only, g1
 * arrives as g_in.  mode 2 (block 0): the first half only; gbias1_part NULL = no dropout and no bias behind LayerNorm 1. */
typedef struct dg_block_chain_bwd_args {
    int32_t mode, M, C, reserved;
    const void* dqkv; const void* wqkvT; const float* x; const float* mean1; const float* rstd1; const float* ln1w;
    const void* dresid1; void* dx1; void* g1;
    float* dln1w_part; float* dln1b_part; float* gbias1_part;
    const void* g_in;
    const void* w2T; const uint8_t* sign_bits; int64_t sign_bits_bytes; void* df; float* db1_part;
    const void* w1T; const float* x1; const float* mean2; const float* rstd2; const float* ln2w;
    const void* dresid2; void* dx2; void* g2;
    float* dln2w_part; float* dln2b_part; float* gbias2_part;
    const void* wprojT; void* dout;
    int64_t part_stride;
    float dropout_p; const uint32_t* rng_state; uint32_t site_ffn_below, site_proj;
} dg_block_chain_bwd_args;
int dg_block_chain_bwd_supported(int M, int C);
int dg_block_chain_bwd(const dg_block_chain_bwd_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRAKEGPT_HIP_H */
