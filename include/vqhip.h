/*
 * vqhip.h — C ABI of the MI355X (gfx950) VQ codebook-lookup library (libvqhip.so).
 *
 * Drop-in boundary for ONE path of magic-research/vector_quantization: the `vq.algorithms` quantizer
 * forward (distance over the whole codebook → row argmin → gather/STE/loss → codebook update).  The
 * reference has no FFI of its own (it is pure Python on ATen ops); each entry point below replaces the
 * ATen call(s) named next to it (paths relative to the reference root), and is what the reference-side
 * binding in INTEGRATION.md (a ctypes stub inside the quantizer modules) calls.
 *
 * Conventions: every pointer is a DEVICE pointer unless noted; tensors are dense row-major; `stream`
 * is a hipStream_t passed as void*; functions never allocate, never synchronise, never touch another
 * stream; they return 0 or a negative VQHIP_E* code.  Two documented exceptions to "never synchronise", both host-side waits the
 * CALLER arms: the vqhip_rccl_* set-up calls (they block inside RCCL), and vqhip_cvq_forward with cap < 0, which waits on the
 * caller's own event (hipEventSynchronize(count_event)) for a count the previous call queued a whole step earlier and then reads
 * the caller's pinned host word — that word must be host-coherent memory (hipHostMalloc's default; not under HIP_HOST_COHERENT=0:
 * pass cap >= 0 there).  x_dtype selects the latent storage type
 * (fp32, or bf16 as produced under autocast); codebooks are fp32 like nn.Embedding.weight.
 * Every caller-owned scratch buffer travels with its size (`ws_bytes`, `cb_bytes`): a buffer smaller than the matching
 * *_bytes function asks for is refused with VQHIP_EINVAL before anything is launched (vqhip_last_error names both numbers).
 *
 * LIMITS (checked; VQHIP_EINVAL beyond them)
 *   N, K                 < 2^31 (row lists and candidate codes are 32-bit)
 *   D                    >= 1; the fp16-MFMA proposal pass exists for D <= 1024 with D % 8 == 0 (every shipped config: 8, 32,
 *                        256, 768) — other D take the all-fp32 route transparently (vqhip_argmin, vqhip_col_argmin) or are
 *                        refused where only the proposal form exists (vqhip_col_argmin_rows, VQHIP_METRIC_COS_BF16 encode)
 *   ordered sums         K <= 32768, D % 4 == 0, ceil(N/1024) * K < 2^31 (vqhip_token_order and the two sums built on it)
 *   packed exchange      <= 256 ranks (count pieces stay exact in fp32), per-rank counts < 2^31, token count < 2^48
 *   vqhip_transpose      B <= 65535 per launch
 *   alignment            every buffer pointer 16-byte aligned (hipMalloc / torch allocations are); rows dense, no padding.
 *                        The entry points that state "element alignment only" below (sampler, token cross-entropy, cosine
 *                        embedding, LPIPS, bias-activation / FIR, GroupNorm, the ViT row ops, image metrics) mean it for every
 *                        pointer they take except `ws`: the small vectors are read and written element by element (u, targets,
 *                        weight, lse, g, weight_sum, stats, seed, g_out, bias, gamma, beta; tokens, cut, loss, hit, out, value,
 *                        the fp32 column sums), and an output tensor needs the alignment of its element type as an input does:
 *                        no result bit depends on an address.  Workspaces keep the 16 bytes.
 *   device               all pointers belong to the device `stream` was created on, which is the current HIP device
 */
#ifndef VQHIP_H_
#define VQHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VERSION 600   /* round 6: + NearestAnchor(sync=True) across ranks by a key exchange (vqhip_cvq_col_keys, vqhip_cvq_pack_sync,
                              * vqhip_allreduce_min_i64, vqhip_cvq_forward_t.anchor_sync / rank / keys); vqhip_cvq_apply takes the capacity */

#define VQHIP_METRIC_L2 0   /* L2Distance      vq/algorithms/vq/distances.py:28-32 */
#define VQHIP_METRIC_COS 1  /* CosineDistance  vq/algorithms/vq/distances.py:35-46 */
/* CosineDistance as the reference's GPU runs evaluate it under bf16 autocast (vq/runners/base.py:30-48: normalize is on
 * autocast's fp32 list, the einsum on its bf16 list): operands rounded to bf16 after the fp32 normalisation, products
 * summed in fp32 (here: the k-ordered fma chain of the fp32 definition), the sum rounded to bf16, 1 - s rounded to bf16,
 * lowest index among equal bf16 distances.  This is what the reference returns inside its autocast region: a caller of
 * this ABI that replaces distances.py:39-46 there must pass THIS metric (check torch.is_autocast_enabled('cuda') and
 * torch.get_autocast_dtype('cuda') == torch.bfloat16, as the Python CosineDistance of this package does by itself;
 * INTEGRATION.md, binding B) — VQHIP_METRIC_COS is the fp32 definition, the reference's result OUTSIDE autocast.  Exists
 * where the proposal image does (D <= 1024, D % 8 == 0). */
#define VQHIP_METRIC_COS_BF16 5

#define VQHIP_DTYPE_F32 0
#define VQHIP_DTYPE_BF16 1
/* (2 and 3 are the token dtypes VQHIP_DTYPE_I32 / VQHIP_DTYPE_I64, defined with the FSQ entry points below) */
#define VQHIP_DTYPE_F16 4   /* the sampler, token cross-entropy and the activation ops (cosine embedding, LPIPS, StyleGAN2,
                             * GroupNorm, image metrics) read it; the quantizer core and FSQ take F32 or BF16 rows only */

#define VQHIP_OK 0
#define VQHIP_EINVAL (-22)      /* bad argument (null pointer, unsupported D, ...) */
#define VQHIP_ELAUNCH (-5)      /* hip launch error */
#define VQHIP_ERCCL (-71)       /* librccl.so not loadable, or an RCCL call failed (vqhip_last_error carries RCCL's text) */

int vqhip_version(void);
const char *vqhip_last_error(void); /* host string describing the last non-zero return on this thread */

/* ---- sizes of caller-owned buffers -------------------------------------------------------------- */
/* bytes of the prepared-codebook image produced by vqhip_codebook_prepare for a [K,D] codebook */
int64_t vqhip_codebook_bytes(int64_t K, int D);
/* vqhip_codebook_prepare + (cosine: vqhip_normalize_rows of x) + vqhip_argmin in one call with two launches less on the
 * critical path: the codebook statistics and the whole token side (normalisation included) are independent and run as ONE
 * launch (cosine: the whole codebook preparation — statistics AND image — rides in that launch).  This is the training-time shape of vq/algorithms/vq/quantizers.py:92-100, where the codebook changes every
 * step; with a frozen codebook prepare once and call vqhip_argmin.
 *   x [N,D] fp32|bf16: the latents as the quantizer receives them (NOT normalised, also for cosine);
 *   cb: vqhip_codebook_bytes(K,D), written; idx [N] int64; hist [K] int32 or NULL (counts are ADDED);
 *   xq [N,D] fp32: cosine only — receives F.normalize(x, dim=1) (bit-identical to vqhip_normalize_rows; under
 *   VQHIP_METRIC_COS_BF16 each element additionally rounded to the nearest bf16: the operand of THAT metric), which is also the
 *   operand of the exact re-rank: keep it alive until the call has completed on the stream; NULL for L2;
 *   ws: vqhip_workspace_bytes(N,K,D).  Results are those of the separate calls, bit for bit. */
int vqhip_encode(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, void *cb, int64_t cb_bytes,
                 int64_t *idx, int32_t *hist, float *xq, void *ws, int64_t ws_bytes, void *stream);
/* The same with flags: VQHIP_ENCODE_ZERO_HIST — `hist` is zeroed by the call's first launch (no separate fill), so the
 * histogram on return is exactly this call's code counts. */
#define VQHIP_ENCODE_ZERO_HIST 1
int vqhip_encode_ex(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, void *cb, int64_t cb_bytes,
                    int64_t *idx, int32_t *hist, float *xq, void *ws, int64_t ws_bytes, int flags, void *stream);

/* vqhip_encode_ex for latents that arrive as the FEATURE MAP [B, D, HW] the encoder / post_encode connector produced: the
 * 'b c h w -> (b h w) c' rearrangement of vq/tasks/image_tokenization/models/base.py:124,140 is folded into the call's first
 * launch (64-dim x 32-token tiles are read with the tokens along the lanes and turned through LDS), so no transpose kernel
 * runs and the map is read once.  N = B*HW tokens, token n = (b, p) with n = b*HW + p.
 *   xrows [N, D] in x_dtype: receives the token-major copy of the latents the rest of the step works on (the exact re-rank of
 *   this call for L2, vqhip_gather_ste_*, vqhip_vq_backward); xq [N, D] fp32: cosine only — F.normalize(x), as in vqhip_encode
 *   (NULL for L2).  Keep both alive until the call has completed.  D <= 1024, D % 8 == 0.  Same results as transposing and
 *   calling vqhip_encode_ex, bit for bit. */
int vqhip_encode_map(const void *x_map, int x_dtype, const float *e, int64_t B, int64_t HW, int64_t K, int D, int metric, void *cb,
                     int64_t cb_bytes, int64_t *idx, int32_t *hist, void *xrows, float *xq, void *ws, int64_t ws_bytes, int flags,
                     void *stream);

/* Byte offset, inside an image prepared with VQHIP_METRIC_COS, of the fp32 [K, D] rows F.normalize(e, dim=1) the exact
 * definition consumes (bit-identical to vqhip_normalize_rows(e)); 256-byte aligned.  Lets a caller that needs the
 * normalised codebook again in the same step (NearestAnchor's column argmin, vq/algorithms/cvqvae/anchors.py:83-84)
 * read it instead of normalising twice.  Not written for the L2 metric. */
int64_t vqhip_codebook_exact_offset(int64_t K, int D);
/* bytes of per-call scratch for vqhip_argmin / vqhip_argmin_exact / vqhip_distance over N rows.
 * (vqhip_col_argmin needs the LARGER vqhip_col_workspace_bytes, declared next to it below.)
 * (Alignment, density and device preconditions: the LIMITS block at the top of this header.) */
int64_t vqhip_workspace_bytes(int64_t N, int64_t K, int D);

/* ---- codebook preparation --------------------------------------------------------------------------
 * Reads e[K,D] fp32 and writes into `cb` (vqhip_codebook_bytes): the oracle-order row norms |e_k|^2,
 * for COS the normalised codebook F.normalize(e) (distances.py:41), a power-of-two-scaled fp16 copy in
 * MFMA-fragment order, and the error bounds the exact re-rank needs.  Must be re-run whenever e changes
 * (callbacks rebind weight.data every forward: vq/algorithms/vq/callbacks/update.py:56). */
int vqhip_codebook_prepare(const float *e, int64_t K, int D, int metric, void *cb, int64_t cb_bytes, void *stream);

/* ---- fused distance + argmin  (replaces quantizers.py:97-99: distance(x, W) → torch.argmin(d, -1)) ---
 * idx[n] = argmin_k d(x_n, e_k), lowest k on ties, bit-identical to the fp32 definition
 *   L2 : sqrt(clamp_min((sum_d(-2 x_d e_kd) + |x|^2) + |e_k|^2, 0))   (torch.cdist mm path)
 *   COS: 1 - sum_d xh_d eh_kd, xh/eh = F.normalize(.)                  (x must already be normalised:
 *        pass the output of vqhip_normalize_rows; the codebook is normalised by codebook_prepare)
 * evaluated with k-ordered fp32 fma chains (see DESIGN.md "Arithmetic contract").  A fp16 MFMA pass
 * proposes candidates under a rigorous error bound and an exact fp32 re-rank decides; rows the bound
 * cannot settle are re-evaluated over the whole codebook in fp32.  The proposal pass exists for D <= 1024 with
 * D % 8 == 0 (every shipped config: 8, 32, 256, 768); any other D takes the all-fp32 route of vqhip_argmin_exact.
 * Optional outputs (nullable):
 *   hist[K] int32 += code-hit histogram (quant.bincount, vq/algorithms/vq/utils.py:42);
 * `ws` = vqhip_workspace_bytes(N,K,D) of scratch. */
int vqhip_argmin(const void *x, int x_dtype, const float *e, const void *cb, int64_t cb_bytes, int64_t N, int64_t K, int D,
                 int metric, int64_t *idx, int32_t *hist, void *ws, int64_t ws_bytes, void *stream);

/* Same result computed entirely in fp32 (v_mfma_f32_32x32x2_f32) without the fp16 proposal pass.
 * dmin (nullable) receives the winning distance.  For COS `e` must be the normalised codebook. */
int vqhip_argmin_exact(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric,
                       int64_t *idx, float *dmin, int32_t *hist, void *ws, int64_t ws_bytes, void *stream);

/* Materialise d[N,K] fp32 (memo['distance'], quantizers.py:98) — or a row block of it, for a row slice of x: the bits do not
 * depend on the slice.  No shipped consumer needs the whole matrix any more: EntropyLoss (losses.py:143) and MultinomialAnchor
 * (anchors.py:100) walk bounded row blocks (vqhip_entropy_*, vqhip_col_multinomial_*); third-party code that touches
 * memo['distance'] still gets it from here.  COS: x and e already normalised. */
int vqhip_distance(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric,
                   float *d, void *ws, int64_t ws_bytes, void *stream);

/* NearestAnchor: col_idx[k] = argmin_n d[n,k], lowest n on ties (vq/algorithms/cvqvae/anchors.py:83), same arithmetic
 * contract as vqhip_argmin (bit-identical to the fp32 definition, operand order of the reference kept); never
 * materialises d.  Runs the proposal + re-rank pipeline with the roles of latents and codes swapped.
 * COS: x and e already normalised.  `ws` = vqhip_col_workspace_bytes(N, K, D). */
int64_t vqhip_col_workspace_bytes(int64_t N, int64_t K, int D);
int vqhip_col_argmin(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric,
                     int64_t *col_idx, void *ws, int64_t ws_bytes, void *stream);

/* ---- fused MultinomialAnchor (vq/algorithms/cvqvae/anchors.py:88-104) on row blocks of the distance matrix -----------------
 * One latent per code, drawn from the softmax down the code's column of d: what `d.t().softmax(1).multinomial(1)` draws, without
 * the [N, K] matrix, its transposed softmax, or a sort.  Caller-supplied uniforms, exact fixed-point masses, an inverse-CDF walk
 * in row order: the draw of vqhip_sample_tokens applied down the columns of a matrix that is never stored.
 * THE SIGN IS THE REFERENCE'S: it softmaxes +d, so FARTHER latents are likelier.  That is reproduced here, not corrected.
 * DEFINITION  x [N, D], e [K, D], metric L2 or COS; d[n, k] = the fp32 definition of DESIGN.md §2, the bits vqhip_distance
 *   writes (COS: both operands already normalised by the caller).  All arithmetic below is fp32 IEEE without contraction unless
 *   it says otherwise.  For each code k:
 *       m_k      = max_n d[n, k]
 *       M[n, k]  = (int64) trunc(expf(fl(d[n, k] - m_k)) * 2^40)      expf at <= 1 ulp; the product is exact (formed in double)
 *       Z_k      = sum_n M[n, k]                                      an exact integer sum; Z_k >= 2^40 (the maximal row has
 *                                                                     mass exactly 2^40) and Z_k < 2^61 for N <= 2^20
 *       T_k      = min(floor((double)u_k * (double)Z_k), Z_k - 1)     u fp32 [K] in [0, 1)  (a NaN or negative u counts as 0)
 *       col_idx[k] = the first n, in increasing n, whose running sum C_n = sum_{n' <= n} M[n', k] exceeds T_k
 *   - the inverse-CDF draw multinomial(1) makes on row k of d.t().softmax(1).  C_{N-1} = Z_k > T_k: the crossing always exists.
 * BAD COLUMNS  a column that holds a NaN or a +inf gets col_idx[k] = -1; nothing is dereferenced out of range and no other
 *   column is affected.  (A NaN latent row makes every column bad; a NaN codebook row exactly its own.  A distance is never -inf.)
 * ERROR BOUND  the kernel's cumulative share C_n / Z_k differs from the exact share (float64 exp of the fp32 distances' exact
 *   differences) by at most
 *       VQHIP_SAMPLE_DELTA(N) = 2^-18 + N * 2^-39          (4.1e-6 at N = 2^17, 5.7e-6 at N = 2^20)
 *   Derivation (the sampler's, with V replaced by N): expf(x) 2^40 < 1 for x < -40 ln 2 = -27.7, so a mass that is not truncated
 *   to 0 has |d - m| < 28.  Its relative error is at most 28 * 2^-24 (the rounded difference, half an ulp of a value below 32,
 *   carried into the exponent) + 2^-23 (expf) < 1.8e-6 = e; truncation loses less than 2^-40 per row.  A share S / Z of two such
 *   sums, Z >= 1 in units of 2^40, is then off by at most 2 (e Z + N 2^-40) / (Z (1 - e) - N 2^-40) <= 2^-18 + N 2^-39; the fp64
 *   product u Z and the conversion of Z add less than 2^-50.  So the picked row j satisfies
 *       sum_{n < j} s_n / S <= u_k + delta   and   sum_{n <= j} s_n / S >= u_k - delta,   s_n = exp(d[n, k] - m_k) exactly,
 *   and d[j, k] - m_k >= -28 (a row of zero mass is never picked).  A measurement beyond it means the kernels or this derivation
 *   are wrong.
 * INVARIANCE  every sum is an integer sum: the result is a pure function of (x, e, metric, u) - not of block_rows, the grid or
 *   the run.  No float atomics (no atomics at all), no memset the caller must issue, no allocation, no synchronisation.
 * THE WALK  the caller owns one dense fp32 [block_rows, K] tile and `ws`, and walks the row blocks b = 0 .. B - 1
 *   (B = ceil(N / block_rows); block b is rows [r0, r0 + r), r0 = b * block_rows, r = min(block_rows, N - r0)) three times:
 *       for each block in order:  vqhip_distance(x + r0 rows, .., r, .., tile);  vqhip_col_multinomial_max(tile, r0, ..)
 *       for each block:           vqhip_distance(..);                            vqhip_col_multinomial_mass(tile, r0, ..)
 *       vqhip_col_multinomial_pick(u, .., col_idx)
 *       for each block:           vqhip_distance(..);                            vqhip_col_multinomial_resolve(tile, r0, .., col_idx)
 *   Each d[n, k] is evaluated at most three times (B = 1: once - the tile stays).  _max takes the blocks in increasing r0 (r0 = 0
 *   overwrites the running maximum); _mass and _resolve take them in any order.  Everything is sequential on `stream`.
 * WORKSPACE  vqhip_col_multinomial_workspace_bytes(N, K, block_rows) = 16 K + 8 B K bytes + padding: the running maximum, the
 *   picked block and residual target per column, and the int64 column masses of every block.  Every byte is written before it
 *   is read.  Nothing grows with N * K but the caller's tile, whose size is the caller's choice (ops.py: 64 MiB).
 * LIMITS (VQHIP_EINVAL before any HIP call): no null pointer; 1 <= N <= 2^20 (VQHIP_COL_MULTINOMIAL_MAX_N: keeps Z < 2^61);
 *   1 <= K < 2^31; 1 <= block_rows <= N; r0 a multiple of block_rows below N; ws_bytes as asked for.  D and the metric are
 *   vqhip_distance's (any D >= 1; L2 or COS - VQHIP_METRIC_COS_BF16 is the reference's bf16 matrix, not this definition). */
#define VQHIP_COL_MULTINOMIAL_MAX_N (1ll << 20)
int64_t vqhip_col_multinomial_workspace_bytes(int64_t N, int64_t K, int64_t block_rows);
int vqhip_col_multinomial_max(const float *tile, int64_t r0, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes,
                              void *stream);
int vqhip_col_multinomial_mass(const float *tile, int64_t r0, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes,
                               void *stream);
int vqhip_col_multinomial_pick(const float *u /* [K] */, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes,
                               int64_t *col_idx /* [K], written: -1 */, void *stream);
int vqhip_col_multinomial_resolve(const float *tile, int64_t r0, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes,
                                  int64_t *col_idx /* [K] */, void *stream);

/* ---- row kernels ------------------------------------------------------------------------------------ */
/* out[r] = |v_r|^2 in the oracle's order (64 interleaved fma partials + halving tree) */
int vqhip_row_sqnorm(const void *v, int dtype, int64_t R, int D, float *out, void *stream);
/* out = F.normalize(v, dim=1, eps) (callbacks/normalize.py:24,27; distances.py:40-41) */
int vqhip_normalize_rows(const void *v, int dtype, int64_t R, int D, float eps, float *out, void *stream);

/* ---- decode + straight-through + loss partial sums --------------------------------------------------
 * z[n] = e[idx[n]]                       (nn.Embedding gather, quantizers.py:107)
 * z_ste[n] = x[n] + (z[n] - x[n])        (utils/ste.py:10)        — either output may be NULL
 * sse[0] += sum (z - x)^2 in double      (both MSE terms of losses.py:50,62 share this sum; the host
 *                                         divides by N*D).  sse may be NULL. */
int vqhip_gather_ste_loss(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D,
                          float *z, float *z_ste, double *sse, void *stream);
/* The same pass with the mean finished on the device: mse[0] = mse[1] = mean((z - x)^2) as fp32 (double sum, one division,
 * one cast: what `mse_loss` of losses.py:50,62 returns for both terms), mse[2] = mse[0] + beta*mse[1] (VQGANLoss.forward,
 * losses.py:119-127: a product and a sum, each rounded, like the reference's two ops), mse[3] = 0 — mse is fp32[4].
 * `scratch16`: 16 bytes of device memory that are ZERO on entry and are left zero on return (one scratch per stream in
 * flight); N > 0. */
int vqhip_gather_ste_mse(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D,
                         float *z, float *z_ste, float *mse, float beta, void *scratch16, void *stream);

/* The same with the OUTPUT written as the feature map [B, D, HW] ('(b h w) c -> b c h w' + .contiguous(), models/base.py:126-127,
 * folded into the gather: 64 x 64 tiles turned through LDS, 256 contiguous bytes per channel and wave-instruction):
 *   x_rows != NULL: out_map = x + (e[idx] - x) (straight-through output), mse[4] as vqhip_gather_ste_mse, scratch16 as there;
 *   x_rows == NULL: out_map = e[idx] (decode_from_quant, image_reconstruction/models.py:97-106); mse, scratch16 unused. */
int vqhip_gather_ste_map(const void *x_rows, int x_dtype, const float *e, const int64_t *idx, int64_t B, int64_t HW, int D,
                         float *out_map, float *mse, float beta, void *scratch16, void *stream);

/* hist[K] int32 += bincount(idx) (utils.py:42; runners/metrics.py:40-44) */
int vqhip_hist(const int64_t *idx, int64_t N, int64_t K, int32_t *hist, void *stream);

/* vqhip_hist for int32 tokens (FiniteScalarQuantizer's, vq/algorithms/fsq/quantizers.py:61-64): the same rule, only
 * 0 <= idx < K is counted. */
int vqhip_hist_i32(const int32_t *idx, int64_t N, int64_t K, int32_t *hist, void *stream);

/* ---- FiniteScalarQuantizer (vq/algorithms/fsq/quantizers.py:74-150) ------------------------------------------------------
 * Element-wise, one launch per call.  The per-channel constants are computed by the caller with the reference's own torch
 * expressions (M = (L - 1) * (1 - eps), shift = atanh(((L - 1) % 2) / M), both fp32) and never recomputed on the device; the
 * library derives the integers odd = (L - 1) % 2, h = L // 2 and cumprod from `levels`.
 *   encode   t = (tanh(x + shift) * M - odd) / 2;  r = round-half-even(t);  z = (t + (r - t)) / h                (fp32)
 *            quant = int32(sum_i (r_i + h_i) * cumprod_i)  (fp32 sum of exact integers; a NaN latent gives INT32_MIN)
 *   backward grad_x = (((g / h) / 2) * M) * (1 - y * y),  y = tanh(x + shift), cast to x's dtype (round to nearest even)
 *   decode   z = ((quant // cumprod) % L) / h - 1  for any int32 / int64 token (floor division, non-negative remainder)
 * Layouts: VQHIP_LAYOUT_ROWS = token-major [N, C]; VQHIP_LAYOUT_MAP = the NCHW-contiguous map [B, C, HW] with N = B * HW.
 * LIMITS (VQHIP_EINVAL, checked before any HIP call): 1 <= C <= 16, every level >= 3 (2 makes atanh's argument > 1, the
 * reference's NaN), prod(levels) <= 2^24 (the fp32 digit sum stays exact), 0 <= N < 2^31, for the map HW >= 1 and N % HW == 0. */
#define VQHIP_FSQ_MAX_C 16
#define VQHIP_LAYOUT_ROWS 0
#define VQHIP_LAYOUT_MAP 1
#define VQHIP_DTYPE_I32 2     /* token dtypes of vqhip_fsq_decode */
#define VQHIP_DTYPE_I64 3

typedef struct {
    int64_t struct_bytes;                 /* sizeof(vqhip_fsq_t) */
    int32_t C;                            /* channels = number of levels */
    int32_t levels[VQHIP_FSQ_MAX_C];      /* L_i (num_scalars_per_channel) */
    float shift[VQHIP_FSQ_MAX_C];         /* atanh(odd_i / M_i) */
    float scale[VQHIP_FSQ_MAX_C];         /* M_i */
} vqhip_fsq_t;

/* quant int32 [N] (required); z fp32 (nullable) in x's layout — or token-major [N, C] when z_rows != 0; x_rows (nullable, MAP
 * only) = the token-major copy of x in x's dtype; hist int32 [prod(levels)] (nullable) += the tokens (not zeroed here). */
int vqhip_fsq_encode(const vqhip_fsq_t *q, const void *x, int x_dtype, int layout, int64_t N, int64_t HW, int32_t *quant,
                     float *z, int z_rows, void *x_rows, int32_t *hist, void *stream);
/* grad_x (x's dtype and layout) of the encode's z from g = dL/dz (fp32, x's layout) */
int vqhip_fsq_backward(const vqhip_fsq_t *q, const void *x, int x_dtype, int layout, int64_t N, int64_t HW, const float *g,
                       void *grad_x, void *stream);
/* z fp32 [N, C] (ROWS) or [B, C, HW] (MAP) of tokens quant (quant_dtype VQHIP_DTYPE_I32 or VQHIP_DTYPE_I64) */
int vqhip_fsq_decode(const vqhip_fsq_t *q, const void *quant, int quant_dtype, int layout, int64_t N, int64_t HW, float *z,
                     void *stream);

/* ---- pooled code features (the linear probe, vq/tasks/image_classification/models.py:101-109) ---------------------------
 * tokens quant [B, HW] (quant_dtype VQHIP_DTYPE_I32 or VQHIP_DTYPE_I64) -> the mean over the positions of the decoded rows,
 * out fp32 [B, D]: `quantizer.decode` followed by einops.reduce(z, 'b h w c -> b c', 'mean'), one launch, and the decoded
 * [B * HW, D] rows never exist in memory.  Everything is fp32 IEEE arithmetic without contraction, in ONE order.  With
 * v_p = e[quant[b, p], c] (vqhip_fsq_decode_pool: the fp32 value vqhip_fsq_decode gives for that token and channel, bit for bit):
 *   s_j = +0.0f;  for p = j, j + 8, j + 16, .. < HW (increasing):  s_j = s_j + v_p              (j = 0 .. 7)
 *   out[b, c] = (((s_0 + s_1) + (s_2 + s_3)) + ((s_4 + s_5) + (s_6 + s_7))) / (float)HW         (a true division)
 * The order depends on HW alone — not on B, D, the launch geometry or the token dtype — and the forward uses no float atomics:
 * the result is bit-reproducible from run to run and from shape to shape.
 * Tokens outside [0, K) (vqhip_decode_pool): never dereferenced; every channel of that image's row of `out` is NaN; the
 * backward skips them.  vqhip_fsq_decode_pool decodes any token, as vqhip_fsq_decode does.
 * vqhip_decode_pool_bwd: grad_e[quant[b, p], c] += g[b, c] / (float)HW with float atomics (not ordered); grad_e is accumulated
 * into, the caller zeroes it.
 * LIMITS (VQHIP_EINVAL, checked before any HIP call): no null pointer, B >= 1, HW >= 1, B * HW < 2^31, K >= 1, D >= 1 (any D:
 * 16-byte loads where D % 4 == 0 and e, out are 16-byte aligned, channel by channel otherwise), the token dtype one of the
 * two; vqhip_fsq_decode_pool also the limits of the FSQ constants above.  No allocation, no synchronisation, no workspace. */
int vqhip_decode_pool(const float *e, int64_t K, int D, const void *quant, int quant_dtype, int64_t B, int64_t HW,
                      float *out /* [B, D] */, void *stream);
int vqhip_decode_pool_bwd(const float *g /* [B, D] */, const void *quant, int quant_dtype, int64_t B, int64_t HW, int64_t K, int D,
                          float *grad_e /* [K, D], += */, void *stream);
int vqhip_fsq_decode_pool(const vqhip_fsq_t *q, const void *quant, int quant_dtype, int64_t B, int64_t HW,
                          float *out /* [B, C] */, void *stream);

/* ---- fused token sampler of stage-2 generation (vq/tasks/sequence_modeling/models/samplers.py:20-120) --------------------
 * BaseSampler / TopKTopPSampler / CFGSampler as BaseTransformer.sample calls them once per generated position
 * (vq/tasks/sequence_modeling/models/transformers.py:58-70): slice, CFG mix, temperature, top-k, top-p, one draw per row, + start and
 * the CFG duplication, ONE launch, one workgroup per output row.  No sort, no [R, V] temporary, no workspace.
 * INPUT   logits [R, >= end] in `dtype` (VQHIP_DTYPE_F32, _BF16 or _F16), element stride 1, row stride `row_stride` >= end elements;
 *   only columns [start, end) are read, V = end - start.  The pointer and the slice start need only element alignment (16-byte
 *   loads are used where a row's slice allows them, element loads otherwise: bf16 with start = 1001 is a shipped case).  Every
 *   element is converted to fp32 exactly; all arithmetic below is fp32 IEEE without contraction.  (The reference computes in the
 *   input dtype: for 16-bit logits this is a stated difference, not a parity claim.)
 * CFG     cfg != 0: R even, Ro = R / 2 output rows; row r < Ro is unconditional, row r + Ro conditional (logits.chunk(2));
 *   a = fl(fl((float)(1.0 - (double)cfg_alpha) * uncond) + fl(cfg_alpha * cond)).  cfg == 0: Ro = R, a = the logit.
 * TEMPERATURE  a = a / temperature, a true fp32 division, skipped when temperature == 1.  (-0 counts as +0 from here on.)
 * ORDER   tokens of a row are ordered by (a, -index): among equal values the lower index ranks higher.
 * TOP-K   top_k <= 0: off.  Else k = min(top_k, V); a token survives iff a >= the k-th largest value of the row; all ties at that
 *   value survive (transformers' TopKLogitsWarper).  Pure comparison: exact.
 * TOP-P   applied iff 0 <= top_p <= 1.  m_i = exp(a_i - max) over the top-k survivors; c_i = the share of the survivors' mass held
 *   by the tokens ranked at or below i (ascending cumulative); token i is removed iff c_i <= 1 - top_p (1.0 - (double)top_p); the
 *   top-ranked token is never removed.  The kept set is an upper set of the order.  This restates transformers 4.35.2's
 *   ascending-sort TopPLogitsWarper with min_tokens_to_keep = 1 from memory; that library version was not at hand when this was
 *   written, and THE DEFINITION WRITTEN HERE GOVERNS.
 * DRAW    u [Ro] fp32 in [0, 1).  Walk the kept tokens in index order with running mass C; the token is the first j with
 *   C_j > u * Z (Z = the kept mass); if rounding leaves none, the last kept one (the inverse-CDF draw multinomial makes on a row).
 * OUTPUT  tokens int64: tokens[r] = j + start for r < Ro; under CFG also tokens[r + Ro] (einops.repeat 'b ... -> (two b) ...').
 * BAD ROWS  a row whose inputs or mixed values contain a NaN or a +inf, or no finite value, gets -1 (both halves) and a zeroed cut
 *   with cut_index = -1; nothing is dereferenced out of range and no other row is affected.  -inf is an ordinary token of mass 0.
 * CUT (nullable, [Ro]): kept / topk_kept = tokens that survive both filters / top-k alone; cut_value, cut_index = the lowest-ranked
 *   kept token (the kept set is {a > cut_value} + {a == cut_value, index <= cut_index}); max = the row maximum of a; z = Z.
 * MASSES AND THE ERROR BOUND  a mass is computed as expf(fl(a_i - max)) (expf: at most 1 ulp), multiplied by 2^40 exactly and
 *   truncated to a 64-bit integer; every sum of masses is an integer sum - exact, below 2^61 for V <= 2^20, and independent of the
 *   order of the additions, so the result is bit-reproducible from run to run; no float atomic exists in the kernel.  The
 *   comparisons c_i <= 1 - p and C_j > u Z are made on those integers against floor((1 - p) Z) and floor(u Z) formed in fp64.
 *   Distance between the kernel's share and the exact share (float64 exp of the exact difference):
 *       delta(V) = 2^-18 + V * 2^-39          (VQHIP_SAMPLE_DELTA; 5.7e-6 at V = 2^20, 3.8e-6 at V = 16 384)
 *   Derivation: a mass that is not truncated to 0 has |a_i - max| < 28, so its relative error is at most 28 * 2^-24 (the rounded
 *   difference in the exponent) + 2^-23 (expf) < 1.8e-6 = e; truncation loses less than 2^-40 per token.  A share S / Z of two
 *   such sums with Z >= 1 is then off by at most 2 (e Z + V 2^-40) / (Z (1 - e) - V 2^-40) <= 2^-18 + V 2^-39; the fp64 products
 *   add less than 2^-50.  A token whose exact share lies further than delta from the threshold is decided as the definition says.
 * LIMITS (VQHIP_EINVAL before any HIP call): logits, u, tokens not null; 1 <= R < 2^31, R even under CFG; 0 <= start < end <=
 *   row_stride; V <= 2^20; temperature finite and > 0; cfg_alpha finite (under CFG).  Rows up to V = 32 768 keep their keys in LDS
 *   after one read; longer rows re-read the logits in every pass; both forms give the same bits. */
#define VQHIP_SAMPLE_DELTA(V) (3.814697265625e-06 + (double)(V) * 1.8189894035458565e-12)
typedef struct vqhip_sample_cut_t {
    int32_t kept, topk_kept;
    float cut_value;
    int32_t cut_index;
    float max, z;
} vqhip_sample_cut_t;
int vqhip_sample_tokens(const void *logits, int dtype, int64_t R, int64_t row_stride, int64_t start, int64_t end,
                        float cfg_alpha, int cfg, float temperature, int top_k, float top_p,
                        const float *u, int64_t *tokens, vqhip_sample_cut_t *cut /* or NULL */, void *stream);

/* ---- fused token cross-entropy of stage-2 training --------------------------------------------------------------------------
 * The loss a stage-2 transformer trains on: AR, the shifted mean cross-entropy HF computes for `labels=tokens`
 * (vq/algorithms/ar/transformers/hf.py:61-69); NAR, MAGE's LabelSmoothingCrossEntropy(0.1) averaged with the mask as weights
 * (vq/algorithms/nar/transformers/mage.py:107-123, 479-489).  Forward: the logits are read ONCE (one workgroup per row) and a
 * second, single-workgroup launch forms the scalars.  Backward: one read of the logits, one write of the gradient.  No
 * [R, V] temporary, no workspace, no atomics, no allocation and no synchronisation.
 * INPUT   logits [R, >= end] in `dtype` (VQHIP_DTYPE_F32, _BF16 or _F16), element stride 1, row stride `row_stride` >= end
 *   elements, element alignment only; columns [start, end) are read, V = end - start.  Every element a_j (j the index inside the
 *   slice) is converted to fp32 exactly; all arithmetic below is fp32 IEEE without contraction, expf / logf at <= 1 ulp.
 * TARGETS [R] int32 or int64 (`target_dtype` VQHIP_DTYPE_I32 / _I64), values in the vocabulary: class t means a_{t - start}.
 *   shift_len = 0: the target of row r is targets[r].  shift_len = L > 0 (R % L == 0): the rows are R / L sequences of L
 *   positions, the target of row r is targets[r + 1], and the last row of every sequence is IGNORED (HF's logits[..., :-1, :]
 *   against labels[..., 1:] with neither tensor sliced).  A target equal to `ignore_index` makes its row IGNORED: loss 0, hit 0, a
 *   zero gradient row, not counted in W.  Any other target outside [start, end) is never dereferenced: that row's loss and its
 *   gradient slice are NaN (and so are the scalars).
 * DEFINITION  with e = label_smoothing, t the row's target, w_r = weight[r] (1 without weights):
 *       lse_r  = max + log(sum_j exp(a_j - max))
 *       loss_r = lse_r - a_t                                               (e == 0: the smoothing term is not formed)
 *       loss_r = (1 - e)(lse_r - a_t) + e (lse_r - (sum_j a_j) / V)        (e > 0;  1 - e is (float)(1.0 - (double)e))
 *       hit_r  = 1 iff lse_r is not NaN and the arg-max of the slice, the LOWEST index among equal values, is t; else 0
 *       out[0] = sum_r w_r loss_r, out[1] = W = sum_r w_r, both over the rows that are not ignored; out[2] = (float)(sum_r hit_r)
 *       (an exact integer sum, converted once); out[3] = out[0] / out[1], a true division on the device: W = 0 gives NaN.
 *       grad[r, j] = c_r ((p_j - (1 - e)[j = t]) - e / V),  p_j = exp(a_j - lse_r) from the SAVED lse (no second reduction),
 *       c_r = g w_r / W with `wsum` (the mean: pass out + 1), c_r = g w_r without; g = g[r] if g_per_row else g[0].
 *   The gradient is rounded to nearest even into the logits' dtype and written to grad [R, row_stride_out]: columns [0, cols)
 *   of every row are written, zeros outside [start, end) and in every column of an ignored row (the caller does not memset);
 *   columns [cols, row_stride_out) are not touched.
 * ORDER OF EVERY SUM  T = 256 threads, W = 4 (fp32) or 8 (16-bit) elements per 16 bytes.  The slice is cut by the index j, not by
 *   the address: piece q is elements [W q, W q + W) for q < V / W, then V % W pieces of one element; piece q belongs to thread
 *   q % T, which takes its pieces in increasing q.  A thread keeps (m, s, sa) = (-inf, 0, 0) and for a piece with maximum pm:
 *   if pm > m: s = s * expf(m - pm), m = pm;  then for its elements in order  s = s + expf(a - m),  sa = sa + a.  Two partials
 *   merge as M = max(m_A, m_B), s = s_A f_A + s_B f_B with f_X = 1 if m_X == M else expf(m_X - M), sa = sa_A + sa_B; the 256
 *   threads merge as a balanced binary tree in thread order.  lse = M + logf(s).  The scalars: partial j = r mod 256 adds its
 *   rows in increasing r (s_j = s_j + w_r * loss_r; W alike), the 256 partials add as the same balanced tree.  The order is a
 *   function of V and the dtype's W for a row and of R alone for the scalars: not of the address or alignment of a row (a
 *   strided view and its copy give the same bits), not of the target dtype, not of the other rows, and run to run the same bits.
 * NON-FINITE INPUTS  (the pattern float64 log_softmax arithmetic gives; a row never affects another row's per-row outputs)
 *       the slice holds                          lse     loss, e == 0        loss, e > 0     gradient slice
 *       a NaN                                    NaN     NaN                 NaN             NaN
 *       a +inf                                   NaN     NaN                 NaN             NaN
 *       -inf entries, finite maximum             finite  finite              +inf            finite (p = 0 at the -inf entries)
 *       the same with a_t = -inf                 finite  +inf                +inf            finite
 *       nothing but -inf                         NaN     NaN                 NaN             NaN
 *   hit is 0 wherever lse is NaN.  A non-finite loss_r reaches out[0] and out[3] as IEEE addition carries it.
 * ERROR BOUND  against the exact value of the definition on the converted inputs, amax = the row's largest |a_j|, all a_j
 *   finite; N = VQHIP_TOKEN_CE_CHAIN(V) = V / 256 + 20 (integer division) bounds the longest chain of fp32 additions of a row (a thread
 *   adds at most ceil(V / (256 W)) W + 1 <= V / 256 + 10 elements, the tree adds 8 levels).  In units of u = 2^-24, first order:
 *     s: a term expf(fl(a - m)) carries 2 amax (the rounded difference, |a - m| <= 2 amax) + 2 (expf); the rescalings of a
 *        partial telescope, since m only grows: sum |m_old - m_new| <= 2 amax, so all of them together carry 2 amax, plus 2
 *        (expf) + 1 (the product) for each of at most N rescalings; the additions of positive terms carry N.  Relative error of
 *        s: (4 amax + 2 + 4 N) u.   (Terms flushed below 2^-126 change s >= 1 by less than V 2^-126.)
 *     lse = fl(M + logf(s)): the above, + 2 ln(V) <= 28 (logf at 1 ulp of ln s <= ln V < 14), + amax + 14 (the last addition):
 *        VQHIP_TOKEN_CE_LSE_BOUND = (5 amax + 44 + 4 N) u (1 + 2^-9); the last factor covers every second-order product
 *        (the sum is below 2^-9 for V <= 2^20, amax <= 2^10).
 *     loss: d1 = fl(lse - a_t) and d2 = fl(lse - fl(sa / V)) are each <= 2 amax + 14 in size; sa / V carries N amax (the chain,
 *        |a| <= amax) + amax (the division); the two products, the rounded 1 - e and the final addition carry 5 (2 amax + 14):
 *        VQHIP_TOKEN_CE_BOUND = VQHIP_TOKEN_CE_LSE_BOUND + ((N + 11) amax + 70) u   (holds for lse and for loss_r, any e).
 *     gradient element in fp32, before the rounding to the output dtype, per unit of |c_r|: the exponent fl(a - lse) carries
 *        the lse error + (2 amax + 14), expf 2, on p <= 1 (1 + small); the two subtractions, the rounded 1 - e and e / V and the
 *        product carry 6 on values <= 1:  VQHIP_TOKEN_CE_GRAD_BOUND = VQHIP_TOKEN_CE_LSE_BOUND + (2 amax + 22) u.
 *        c_r itself is fl(fl(g w_r) / W): 2 u relative, plus W's own sum, (R / 256 + 20) u relative (exact for unit weights
 *        below 2^24 rows).  The scalars add (R / 256 + 20) u sum_r |w_r loss_r| to sum_r w_r (error of loss_r).
 *   A measurement beyond these bounds means the kernel or this derivation is wrong.
 * LIMITS (VQHIP_EINVAL before any HIP call): logits, targets, loss, lse, out (fwd) / logits, targets, lse, g, grad (bwd) not
 *   null (hit, weight, wsum may be); 1 <= R < 2^31; 0 <= start < end <= row_stride; V <= 2^20; 0 <= label_smoothing < 1;
 *   shift_len >= 0 and R % shift_len == 0; dtype one of F32 / BF16 / F16; target_dtype one of I32 / I64; bwd: end <= cols <=
 *   row_stride_out, cols < 2^31. */
#define VQHIP_TOKEN_CE_CHAIN(V) ((double)((V) / 256 + 20))
#define VQHIP_TOKEN_CE_LSE_BOUND(V, amax) \
    ((5.0 * (double)(amax) + 44.0 + 4.0 * VQHIP_TOKEN_CE_CHAIN(V)) * 5.9604644775390625e-08 * 1.001953125)
#define VQHIP_TOKEN_CE_BOUND(V, amax) \
    (VQHIP_TOKEN_CE_LSE_BOUND(V, amax) + ((VQHIP_TOKEN_CE_CHAIN(V) + 11.0) * (double)(amax) + 70.0) * 5.9604644775390625e-08)
#define VQHIP_TOKEN_CE_GRAD_BOUND(V, amax) \
    (VQHIP_TOKEN_CE_LSE_BOUND(V, amax) + (2.0 * (double)(amax) + 22.0) * 5.9604644775390625e-08)
int vqhip_token_ce_fwd(const void *logits, int dtype, int64_t R, int64_t row_stride, int64_t start, int64_t end,
                       const void *targets, int target_dtype, int64_t shift_len, int64_t ignore_index, float label_smoothing,
                       const float *weight /* [R] or NULL */, float *loss /* [R] */, float *lse /* [R] */,
                       int32_t *hit /* [R] or NULL */, float *out /* [4] */, void *stream);
int vqhip_token_ce_bwd(const void *logits, int dtype, int64_t R, int64_t row_stride, int64_t start, int64_t end,
                       const void *targets, int target_dtype, int64_t shift_len, int64_t ignore_index, float label_smoothing,
                       const float *weight /* [R] or NULL */, const float *lse /* [R] */, const float *g /* [R] or [1] */,
                       int g_per_row, const float *wsum /* [1] (the mean) or NULL */, void *grad /* [R, row_stride_out] */,
                       int64_t cols, int64_t row_stride_out, void *stream);

/* ---- fused CosineEmbeddingLoss of VQ-KD distillation: loss and gradient ---------------------------------------------------
 * The reconstruction loss of VQ-KD (vq/algorithms/utils/losses.py:13-65, wired as r_loss in configs/vqkd/model.py:62-74 and added
 * to the quantizer's loss in vq/algorithms/vqkd/base.py:82-92): ATen's cosine_embedding_loss for target +1 - the only branch
 * the reference reaches - between the decoder's pred_features and the frozen teacher's target_features.  Forward: pred and
 * target are read ONCE, each in its own dtype, and a second, single-workgroup launch forms the scalars.  Backward: one launch,
 * one read of each, one write of the gradient.  No fp32 copy, no [R, C] temporary, no workspace, no atomics, no allocation
 * and no synchronisation.  No gradient is formed for the target.
 * INPUT   R = B * P rows of C channels.  target [R, C] in `target_dtype`, element stride 1, row stride `target_row_stride` >= C.
 *   pred in `pred_dtype`, either VQHIP_LAYOUT_ROWS: [R, C], element stride 1, row stride `pred_row_stride` >= C (B and P only
 *   enter through their product), or VQHIP_LAYOUT_MAP: the NCHW-contiguous map [B, C, P], row r = b P + p, read through the
 *   channel stride P with no transpose and no copy (`pred_row_stride` is ignored).  dtypes VQHIP_DTYPE_F32, _BF16 or _F16, the
 *   two may differ; element alignment only.  Every element is converted to fp32 exactly; all arithmetic below is fp32 IEEE
 *   without contraction, division and square root correctly rounded.
 * DEFINITION  per row, with e = (float)1e-12, the float constant ATen adds in every dtype (float64 included):
 *       dot = sum_j p_j t_j      pp = sum_j p_j^2 + e      tt = sum_j t_j^2 + e
 *       cos = dot / sqrt(pp tt)                   loss_r = 1 - cos
 *       stats[r] = (1 / sqrt(pp tt), cos, 1 / pp)             (what the backward needs: it does no second reduction)
 *       out[0] = sum_r loss_r,   out[1] = out[0] / (float)R, a true division on the device
 *       grad[r, j] = c_r ((cos (1 / pp)) p_j - t_j (1 / sqrt(pp tt)))  =  c_r dloss_r / dp_j,  from the SAVED stats;
 *       c_r = g (g / (float)R with `mean`, a true division); g = g[r] if g_per_row else g[0].
 *   The gradient is rounded to nearest even into pred's dtype and written in pred's layout (rows: row stride
 *   `grad_row_stride` >= C; map: [B, C, P] contiguous, `grad_row_stride` ignored): every element of every row is written (the
 *   caller does not memset); the columns [C, grad_row_stride) of a strided row are not touched.
 * ORDER OF EVERY SUM  W = 4 (fp32) or 8 (16-bit) elements per 16 bytes, PW = the larger W of the two operands.
 *   Rows: ONE WAVE OWNS A ROW.  The row is cut by the index j, not by the address: piece q is elements [PW q, PW q + PW) for
 *   q < C / PW (one or two 16-byte loads per operand), then C % PW pieces of one element; piece q belongs to lane q % 64, which
 *   takes its pieces in increasing q and adds element by element, in increasing j, to its three partial sums (from +0; each
 *   product rounded once); the 64 lanes add as a balanced binary tree in lane order; then + e.
 *   Map: a workgroup owns 32 consecutive rows times 8 channel groups.  Channels are cut into quads [4 k, 4 k + 4), k < C / 4; quad
 *   k belongs to group k % 8, which takes its quads in increasing k; a thread keeps four partial triples, triple i for channel
 *   4 k + i; the C % 4 last channels 4 (C / 4) + i go to group 0's triple i after its quads.  A thread's triples add as
 *   (a0 + a1) + (a2 + a3), the groups as ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)); then + e.
 *   The scalars: partial j = r mod 256 adds its rows in increasing r, the 256 partials add as a balanced tree in order.
 *   In each layout a row's outputs are a function of C and the two dtypes alone, the scalars of R and the rows: not of the
 *   address or alignment of a row (a strided view and its copy give the same bits), not of R or the other rows, and run to run
 *   the same bits.  The two layouts add in different orders and need not agree bit for bit.
 * DEGENERATE AND NON-FINITE ROWS  (the pattern the float64 evaluation of the definition gives; a row never affects another
 *   row's loss, stats or gradient)
 *       the row holds                            cos     loss    gradient row
 *       pred all zero, target not                0       1       finite: -c_r t_j / sqrt(e tt)
 *       target all zero (pred zero or not)       0       1       finite: 0 (both zero: exactly; pred not zero: t_j = 0 and cos = 0)
 *       a NaN in pred or in target               NaN     NaN     NaN in every element
 *       a +inf or -inf in pred or in target      NaN     NaN     NaN in every element   (inf / inf, or inf * 0 inside dot)
 *   A non-finite loss_r reaches out[0] and out[1] as IEEE addition carries it.
 * ERROR BOUND  against the exact value of the definition on the converted inputs, in units of u = 2^-24, first order, for
 *   2^-60 <= pp, tt <= 2^60 (no sum or product overflows, pp tt is normal, and the products p_j^2, t_j^2, p_j t_j that fall below
 *   2^-126 change a sum of at least 2^-60 by less than C 2^-149 / 2^-60 < 2^-73 of it).
 *   N = VQHIP_COSINE_EMBED_CHAIN(C) = C / 32 + 16 (integer division) bounds, in either layout, the additions one partial sum
 *   goes through plus one for the rounding of its product: rows C / 64 + 8 + 1 (a lane) + 6 (the tree) + 1; map C / 32 + 1 + 1 (a
 *   triple) + 5 (the merges) + 1.
 *     dot: its error is at most N u sum_j |p_j t_j| <= N u |p| |t| (Cauchy-Schwarz), and sqrt(pp tt) >= |p| |t|: N u in cos,
 *        absolute and free of the inputs' scale.
 *     pp, tt: positive terms, (N + 1) u relative each (the chain and the addition of e), so (N + 1) u / 2 each
 *        under the square root; the product pp tt adds 1 / 2, the square root 1, the division 1: on |cos| <= 1 (1 + small).
 *     loss = fl(1 - cos): one rounding of a value <= 2, absolute: 2 u.  (The cancellation for cos near 1 is absolute, not
 *        relative: the bound does not shrink with the loss.)
 *        VQHIP_COSINE_EMBED_BOUND(C) = (2 N + 6) u (1 + 2^-9)  for cos and for loss_r; the last factor covers every second-order
 *        product (their sum is below 2^-9 for C <= 2^16).
 *     gradient element in fp32, before the rounding to the output dtype, per unit of |g| (|g| / R for the mean), in units of
 *        h = 1 / sqrt(pp) <= 1 / |p| (the gradient scales as 1 / |p|; both terms below are at most h in size):
 *        t_j / sqrt(pp tt): (N + 1) + 1 / 2 + 1 + 1 for the stored reciprocal, + 1 for the product: (N + 5) u h;
 *        cos p_j / pp: the error of cos, 2 N + 4, on |p_j| / pp <= h; 1 / pp carries (N + 1) + 1, the two products 2: (3 N + 8) u h;
 *        the subtraction, of a value <= 2 h: 2; the product with c_r: 2; c_r itself for the mean (the conversion of R, the
 *        division), on 2 h: 4.
 *        VQHIP_COSINE_EMBED_GRAD_BOUND(C, h) = (4 N + 21) u (1 + 2^-9) h.
 *     The scalars add (R / 256 + 10) u sum_r |loss_r| to the sum of the rows' errors; out[1] adds 2 u of itself.
 *   Outside the range nothing is trapped: the fp32 arithmetic of the definition decides, as it does in ATen's fp32 evaluation
 *   (pp tt = inf gives cos = 0 and loss = 1; pp tt flushed towards 0 loses the relative accuracy of the denominator).
 *   A measurement beyond these bounds inside the range means the kernel or this derivation is wrong.
 * LIMITS (VQHIP_EINVAL before any HIP call): pred, target, loss, stats, out (fwd) / pred, target, stats, g, grad (bwd) not null;
 *   both dtypes one of F32 / BF16 / F16; pred_layout one of ROWS / MAP; B, P >= 1 and R = B P < 2^31; 1 <= C <= 2^16
 *   (VQHIP_COSINE_EMBED_MAX_C); target_row_stride >= C; rows layout: pred_row_stride >= C and (bwd) grad_row_stride >= C. */
#define VQHIP_COSINE_EMBED_MAX_C (1 << 16)
#define VQHIP_COSINE_EMBED_CHAIN(C) ((double)((C) / 32 + 16))
#define VQHIP_COSINE_EMBED_BOUND(C) ((2.0 * VQHIP_COSINE_EMBED_CHAIN(C) + 6.0) * 5.9604644775390625e-08 * 1.001953125)
#define VQHIP_COSINE_EMBED_GRAD_BOUND(C, h) \
    ((4.0 * VQHIP_COSINE_EMBED_CHAIN(C) + 21.0) * 5.9604644775390625e-08 * 1.001953125 * (double)(h))
int vqhip_cosine_embed_fwd(const void *pred, int pred_dtype, int pred_layout, int64_t pred_row_stride, const void *target,
                           int target_dtype, int64_t target_row_stride, int64_t B, int64_t P, int64_t C,
                           float *loss /* [R] */, float *stats /* [R, 3] */, float *out /* [2] */, void *stream);
int vqhip_cosine_embed_bwd(const void *pred, int pred_dtype, int pred_layout, int64_t pred_row_stride, const void *target,
                           int target_dtype, int64_t target_row_stride, int64_t B, int64_t P, int64_t C,
                           const float *stats /* [R, 3] */, const float *g /* [R] or [1] */, int g_per_row, int mean,
                           void *grad, int64_t grad_row_stride, void *stream);

/* ---- fused LPIPS tail: feature distance of one VGG16 layer, value and gradient ---------------------------------------------
 * The perceptual loss of the VQGAN generator step (vq/tasks/image_reconstruction/losses.py:99-178, wired as lpips_r_loss in
 * configs/vqgan/model.py:29 and reported as lpips_loss by configs/vqgan/runner.py:83-92).  The VGG16 convolutions stay with the
 * framework; everything behind them - F.normalize over the channels of both feature maps, mse_loss(reduction='none'), nn.Dropout,
 * the bias-free 1 x 1 convolution to one channel and the spatial mean - is ONE layer call here.  Forward: two launches (the
 * pixels; the mean of each image).  Backward: one launch.  No copy of the size of the features, no atomics, no memset, no
 * allocation and no synchronisation.  No gradient is formed for the target.
 * INPUT   pred f and target g, both [B, C, P] (P = H W) in ONE layout: VQHIP_LAYOUT_MAP, NCHW-contiguous (channel stride P), or
 *   VQHIP_LAYOUT_ROWS, channels-last dense (rows of C).  Each in its own dtype, VQHIP_DTYPE_F32, _BF16 or _F16; element alignment
 *   only.  w [C] fp32, any sign.  Every element is converted to fp32 exactly; all arithmetic below is fp32 IEEE without
 *   contraction, division and square root correctly rounded.
 * DEFINITION  per pixel (b, p), with e = (float)1e-10 and the keep factors m_c (DROPOUT; all 1 without a seed):
 *       nf = max(sqrt(sum_c f_c^2), e)    a_c = f_c / nf          (ATen's normalize: x / clamp_min(norm, e))
 *       ng = max(sqrt(sum_c g_c^2), e)    b_c = g_c / ng
 *       s(b, p) = sum_c m_c w_c (a_c - b_c)^2            value[b] = (1 / P) sum_p s(b, p)
 *       u_c = 2 m_c w_c (a_c - b_c);   ds/df_c = (u_c - a_c sum_j u_j a_j) / nf where nf is not clamped, u_c / e where it is
 *       grad[b, c, p] = (g_out[b] / (float)P) ds/df_c, rounded to nearest even into pred's dtype, in pred's layout.
 *   The kernels multiply by the once-rounded reciprocals inf = 1 / nf and ing = 1 / ng where the definition divides (one more
 *   rounding per element, counted in the bound), and form the sums over c in TWO passes over the pixel's channels inside one
 *   launch: the norms, then the differences (the second pass re-reads what the workgroup has just read).
 *       stats[b P + p] = (inf, ing, sum_j u_j a_j (+0 where nf is clamped), s): what the backward needs to read f and g once.
 *       value[b] = (float)(sum_p (double)s(b, p) / (double)P): a double sum rounded once, so its error does not grow with P;
 *       with `accumulate` the one thread that owns image b then stores value[b] + that, a plain fp32 add: the layers of one
 *       loss are added in the order of the calls.
 * ORDER OF EVERY SUM  Map: a workgroup owns 64 consecutive positions of one image times 4 channel groups; channel c belongs to
 *   group c mod 4, which adds its channels in increasing c to one partial per sum (from +0, each product rounded once); the
 *   groups add as (g0 + g1) + (g2 + g3).  Rows: 16 lanes own a pixel; its channels are cut into pieces [4 q, 4 q + 4), q < C / 4,
 *   piece q belongs to lane q mod 16, which takes its pieces in increasing q and their elements in increasing c, then the
 *   single channel 4 (C / 4) + lane (lane < C mod 4); the lanes add as a balanced binary tree in lane order.  The mean: partial
 *   j = p mod 256 adds its pixels in increasing p, the 256 partials add as a balanced tree in order.
 *   A pixel's stats and gradient are a function of C, the dtypes, w and the mask alone; value[b] of image b's pixels and P: not of
 *   B, the other images, the address, and run to run the same bits.  The two layouts add in different orders.
 * DROPOUT  `seed`: two uint32 on the DEVICE (null: no dropout, p is ignored); 0 <= p < 1.  Element (layer, b, c, p) is kept iff
 *       h >= p 2^32,  h = mix(mix(seed[0] ^ lo32(i)) ^ (seed[1] + hi32(i) * 0x9E3779B9 + layer * 0x85EBCA77))     (uint32 arithmetic)
 *       mix(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *   for the LOGICAL index i = (b C + c) P + p, whatever the layout.  m = fl(1 / fl(1 - p)) where kept, 0 where dropped; the
 *   product m w_c is rounded once.  The backward regenerates the mask from the same seed: none is stored.
 *   vqhip_lpips_keep_mask writes the mask [B, C, P] (1 kept, 0 dropped) with the same device function, for tests.
 * DEGENERATE AND NON-FINITE PIXELS  (what the fp32 evaluation of the definition gives; a pixel never affects another pixel's
 *   stats or gradient, an image never another image's value)
 *       the pixel holds                          a / b          s                       gradient column
 *       f all zero (g not)                       a = 0          sum m w b_c^2           -2 m_c w_c b_c / e   (nf clamped: huge, finite)
 *       g all zero (f not)                       b = 0          sum m w a_c^2           finite, the projected form
 *       both all zero                            a = b = 0      0                       0
 *       0 < |f| < e                              a = f / e      as defined              u_c / e  (no projection: the norm is the constant e)
 *       a NaN in f or in g                       NaN            NaN                     NaN in every element
 *       a +inf or -inf in f or in g              NaN there      NaN                     NaN in every element   (inf * (1 / inf))
 *   A NaN s makes value[b] of ITS image NaN; the other images' values and the other pixels' gradients keep their bits.
 * ERROR BOUND  against the exact value of the definition on the converted inputs, u = 2^-24, first order, for pixels whose
 *   non-zero elements have magnitudes in [2^-55, 2^55] (every square is normal, no sum overflows) and whose norms are not within
 *   N u of e (there the clamp may fall on the other side).
 *   N = VQHIP_LPIPS_CHAIN(C) = C / 4 + 12 (integer division) bounds, in either layout, the additions one partial sum goes through
 *   plus one for the rounding of its product: map ceil(C / 4) + 1 + 2; rows 4 ceil(C / 64) + 1 + 1 + 4.  wabs = max_c |w_c|.
 *     a_c: sum f^2 has positive terms, N u relative; N / 2 under the root, + 1 the root, + 1 the reciprocal, + 1 the product:
 *        E = N / 2 + 3, |a^_c - a_c| <= E u |a_c|; b_c likewise.
 *     d_c = a_c - b_c: |d^_c - d_c| <= E u (|a_c| + |b_c|) + u |d_c|.  With |a|, |b| <= 1 and Cauchy-Schwarz,
 *        sum_c |d_c| (|a_c| + |b_c|) <= 2 |d|, |d| = sqrt(sum d_c^2) <= 2.
 *     s: the error of d_c^2 is 2 |d_c| times that of d_c: wabs (4 E |d| + 2 |d|^2) u; the square, m w and their product: 3 u
 *        per term, the chain N u: wabs (N + 3) |d|^2 u.  Together wabs u (4 E |d| + (N + 5) |d|^2): PROPORTIONAL TO |d| - an identical
 *        pair of one dtype gives exactly 0 - and with |d| <= 2 at most wabs u (8 E + 4 N + 20) = wabs u (8 N + 44).
 *     value[b]: a mean does not exceed its largest term; the double sum adds nothing at this order, its one rounding to fp32 u of
 *        at most 4 wabs, the accumulating add u of the sum of two layers: 8 more.
 *        VQHIP_LPIPS_BOUND(C, wabs) = (8 N + 56) u (1 + 2^-9) wabs   for s(b, p) and for one layer's share of value[b]; the last
 *        factors cover the second-order products.  With dropout, times 1 / (1 - p).
 *     gradient element in fp32, before the rounding to the output dtype, per unit of |g_out[b]| / P and of 1 / (1 - p), in units
 *        of wabs h, h = 1 / nf (1 / e where clamped):
 *        u_c: 2 wabs times the error of d_c (<= (2 E + 2) u) plus two roundings on |d_c| <= 2: (4 E + 12) u;
 *        sum u a: sum |a_j| err(u_j) <= (4 E + 12) u, the relative error E + 1 of each term on sum |u_j a_j| <= 4: 4 E + 4, the
 *        chain 4 N: (8 E + 4 N + 16) u = (8 N + 40) u;  a_c sum u a: that, + (E + 1) 4: (10 N + 56) u;
 *        the difference: (4 E + 12) + (10 N + 56) + its rounding on <= 8: (12 N + 88) u;  times inf, (N / 2 + 2) u relative on
 *        <= 8 h, and the rounding: 4 N + 24;  times g_out[b] / P, two roundings and the product's: 24.
 *        VQHIP_LPIPS_GRAD_BOUND(C, wabs, h) = (16 N + 136) u (1 + 2^-9) wabs h.
 *   A measurement beyond these bounds inside the range means the kernel or this derivation is wrong.
 * LIMITS (VQHIP_EINVAL before any HIP call): pred, target, w, stats, value (fwd) / pred, target, w, stats, g_out, grad (bwd) /
 *   seed, out (keep_mask) not null; both dtypes one of F32 / BF16 / F16; layout one of ROWS / MAP; B, P >= 1, B P < 2^31 and
 *   B ceil(P / 64) < 2^31; 1 <= C <= 2^16 (VQHIP_LPIPS_MAX_C); 0 <= layer <= 2^16; with a seed 0 <= p < 1. */
#define VQHIP_LPIPS_MAX_C (1 << 16)
#define VQHIP_LPIPS_MAX_LAYER (1 << 16)
#define VQHIP_LPIPS_EPS 1e-10f
#define VQHIP_LPIPS_CHAIN(C) ((double)((C) / 4 + 12))
#define VQHIP_LPIPS_BOUND(C, wabs) \
    ((8.0 * VQHIP_LPIPS_CHAIN(C) + 56.0) * 5.9604644775390625e-08 * 1.001953125 * (double)(wabs))
#define VQHIP_LPIPS_GRAD_BOUND(C, wabs, h) \
    ((16.0 * VQHIP_LPIPS_CHAIN(C) + 136.0) * 5.9604644775390625e-08 * 1.001953125 * (double)(wabs) * (double)(h))
int vqhip_lpips_fwd(const void *pred, int pred_dtype, const void *target, int target_dtype, int layout, int64_t B, int64_t C,
                    int64_t P, const float *w /* [C] */, const uint32_t *seed /* [2] on the device, or NULL */, float p, int64_t layer,
                    float *stats /* [B P, 4] */, float *value /* [B] */, int accumulate, void *stream);
int vqhip_lpips_bwd(const void *pred, int pred_dtype, const void *target, int target_dtype, int layout, int64_t B, int64_t C,
                    int64_t P, const float *w /* [C] */, const uint32_t *seed, float p, int64_t layer, const float *stats /* [B P, 4] */,
                    const float *g_out /* [B] */, void *grad, void *stream);
int vqhip_lpips_keep_mask(const uint32_t *seed, float p, int64_t layer, int64_t B, int64_t C, int64_t P, uint8_t *out /* [B, C, P] */,
                          void *stream);

/* ---- StyleGAN2 discriminator ops: bias-activation and the 4-tap FIR blur, forward, backward and fused ---------------------------
 * What StyleGAN2Discriminator (vq/algorithms/vqgan/discriminators/stylegan2.py, selected by configs/vqgan/8192_stylegan2_imagenet_ddp.py
 * and configs/llamagen/vqgan_stylegan2_imagenet_ddp.py) takes from mmcv.ops.FusedBiasLeakyReLU and mmcv.ops.upfirdn2d, restated
 * here because mmcv is no dependency.  The convolutions stay with the framework.  No copy, no atomics, no memset, no allocation and
 * no synchronisation; one launch per call, two where gbias is formed.
 * INPUT   a logical [B, C, P] tensor (P = H W; a [B, C] matrix is P = 1) in VQHIP_LAYOUT_MAP (NCHW-contiguous) or VQHIP_LAYOUT_ROWS
 *   (channels-last dense), VQHIP_DTYPE_F32, _BF16 or _F16, element alignment only; outputs in the same dtype and layout.  bias [C]
 *   and gbias [C] are fp32.  Every element is converted to fp32 exactly; all arithmetic is fp32 IEEE without contraction; a result
 *   is rounded to nearest even into the output dtype.
 * DEFINITION, BIAS-ACTIVATION  (FusedBiasLeakyReLU(C): slope = 0.2, scale = 2^0.5; the kernels hold both as fp32 constants)
 *       fwd    t = x + bias[c];   y = (t > 0 ? t : t * slope) * scale
 *       bwd    gx = g * (y > 0 ? scale : scale * slope)   from the SAVED OUTPUT y, as mmcv's, so x is not kept;
 *              gbias[c] = sum_{b, p} gx, over the fp32 gx before their rounding to the output dtype
 *   A NaN in x gives NaN in y; t == 0 gives y = 0 (of t's sign), and the backward takes the slope branch there and for a NaN y
 *   (y > 0 is false).  +-inf pass through with their sign.  The backward is linear in g: its own derivative with respect to g is
 *   the same call on the incoming second-order gradient; the second derivative with respect to x is zero, as in mmcv.
 * DEFINITION, FIR BLUR  (upfirdn2d(x, k, padding) with k = outer([1, 3, 3, 1]) / 64, per channel, zero padding, down factor d)
 *       out[b, c, y, x] = sum_{i, j < 4} k[i] k[j] xpad[b, c, y d + i, x d + j],   k = (1/8, 3/8, 3/8, 1/8)  (exact in every dtype)
 *       OH = (H + py0 + py1 - 4) / d + 1 (integer division), OW likewise; xpad has py0 zero rows in front, py1 behind, px0 / px1 columns.
 *       bwd: the exact adjoint, gx[b, c, h, w] = sum over (y, i) with y d + i - py0 == h and (x, j) likewise of k[i] k[j] g[b, c, y, x]
 *       (zero insertion by d, correlation with the flipped kernel, the complementary padding).  (H, W) is the blur's input plane in
 *       both calls.  The blur is linear: the derivative of bwd is fwd.
 *   FUSED: fwd with bias != NULL is blur(act(x + bias)), the activation applied on the way into the tile, the padding staying 0;
 *       bwd with x and bias != NULL is gx = adjoint(g) * (x + bias[c] > 0 ? scale : scale * slope) over the SAVED INPUT x of the fused
 *       forward, and gbias[c] = sum gx as above.
 * ORDER OF EVERY SUM  a blur output: h(r) = ((k0 s0 + k1 s1) + k2 s2) + k3 s3 along a source row, then the same form down the four
 *   h.  gbias: a first launch leaves one partial per SLAB and channel in ws [slabs, C] (see vqhip_stylegan2_kernels.h for who adds
 *   what), a second adds slabs j, j + 16, .. in increasing order into 16 partials and those as a balanced tree.  Nothing depends
 *   on the address or on timing: the same inputs give the same bits, run to run.
 * SHAPES AND LIMITS (VQHIP_EINVAL before any HIP call)
 *       pointer          required                      shape                 dtype
 *       x, y, g, gx      always                        [B, C, P] / planes     the call's dtype
 *       bias             bias_act_fwd; fused fir4      [C]                   fp32
 *       gbias, ws        optional in bias_act_bwd      [C], [slabs, C]       fp32      (both or neither; fused fir4_bwd: required)
 *   dtype one of F32 / BF16 / F16; layout one of ROWS / MAP; B, P >= 1; 1 <= C <= 2^16 (VQHIP_SG2_MAX_C); B C P < 2^31;
 *   d in {1, 2}; every padding in 0 .. 3; H + py0 + py1 >= 4 and W + px0 + px1 >= 4; the tiles of one launch below 2^31;
 *   ws_bytes >= 4 C vqhip_bias_act_slabs(..) / 4 C vqhip_fir4_slabs(..) where gbias is formed.
 * ERROR BOUND  against the exact value of the definition on the converted inputs, u = 2^-24, first order, no overflow or underflow
 *   in fp32; the factor 1 + 2^-9 covers the second order.
 *     bias-activation, y and gx in fp32: the add, the slope product and the scale product round once each (3 u), the two fp32
 *       constants are within u / 2 of 0.2 and 2^0.5 (1 u):                         VQHIP_BIAS_ACT_BOUND(y) = 4 u |y|
 *       (gx: scale * slope rounds once, the constants, the product with g: 3 u, under the same macro).
 *     blur, an output in fp32, a = the same blur (or adjoint) of |source|: the 16 weights sum to 1 and are formed separably, so a
 *       term passes one rounded product and three additions per axis, 4 u along the row and 4 u down the column:
 *                                                                                  VQHIP_FIR4_BOUND(a) = 8 u a
 *       fused: + 4 u for the activated source (fwd, a = blur of |act|), or + 3 u for the factor (bwd, a = adjoint(|g|) factor):
 *                                                                                  VQHIP_FIR4_ACT_BOUND(a) = 12 u a
 *     gbias: N = VQHIP_SG2_GBIAS_CHAIN(slabs) = slabs / 16 + 80 bounds the additions a term passes: at most 64 in its thread and 8
 *       in its workgroup's tree in the first launch, ceil(slabs / 16) + 4 in the second.  With e = 4 (bias-activation) or 12 (fused)
 *       for the terms' own errors and sumabs = the sum of the terms' magnitudes a:   VQHIP_SG2_GBIAS_BOUND(slabs, e, sumabs) = (N + e) u sumabs
 *     the store: half an ulp of the output dtype on top, VQHIP_SG2_STORE_U(dtype) = 0 (fp32: nothing is rounded again), 2^-8
 *       (bf16) or 2^-11 (fp16) times |value|, plus 2^-25 absolute for fp16 (its subnormals).
 *   A measurement beyond these bounds inside the range means the kernel or this derivation is wrong. */
#define VQHIP_SG2_MAX_C (1 << 16)
#define VQHIP_SG2_SLOPE 0.2
#define VQHIP_SG2_SCALE 1.4142135623730951
#define VQHIP_SG2_U (5.9604644775390625e-08 * 1.001953125)
#define VQHIP_BIAS_ACT_BOUND(y) (4.0 * VQHIP_SG2_U * (double)(y))
#define VQHIP_FIR4_BOUND(a) (8.0 * VQHIP_SG2_U * (double)(a))
#define VQHIP_FIR4_ACT_BOUND(a) (12.0 * VQHIP_SG2_U * (double)(a))
#define VQHIP_SG2_GBIAS_CHAIN(slabs) ((double)((slabs) / 16 + 80))
#define VQHIP_SG2_GBIAS_BOUND(slabs, e, sumabs) ((VQHIP_SG2_GBIAS_CHAIN(slabs) + (double)(e)) * VQHIP_SG2_U * (double)(sumabs))
#define VQHIP_SG2_STORE_U(dtype) ((dtype) == VQHIP_DTYPE_BF16 ? 0.00390625 : (dtype) == VQHIP_DTYPE_F16 ? 0.00048828125 : 0.0)
int64_t vqhip_bias_act_slabs(int layout, int64_t B, int64_t C, int64_t P);      /* -1 for sizes the calls refuse */
int vqhip_bias_act_fwd(const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t P, const float *bias /* [C] */, void *y,
                       void *stream);
int vqhip_bias_act_bwd(const void *g, const void *y, int dtype, int layout, int64_t B, int64_t C, int64_t P, void *gx,
                       float *gbias /* [C] or NULL */, float *ws, int64_t ws_bytes, void *stream);
int64_t vqhip_fir4_slabs(int layout, int64_t B, int64_t C, int64_t H, int64_t W);  /* of the fused backward; -1 for sizes it refuses */
int vqhip_fir4_fwd(const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W, int down, int py0, int py1, int px0,
                   int px1, const float *bias /* [C], or NULL: the plain blur */, void *out /* [B, C, OH, OW] */, void *stream);
int vqhip_fir4_bwd(const void *g /* [B, C, OH, OW] */, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W, int down, int py0,
                   int py1, int px0, int px1, const void *x /* [B, C, H, W], or NULL */, const float *bias /* with x */,
                   void *gx /* [B, C, H, W] */, float *gbias /* [C], with x */, float *ws, int64_t ws_bytes, void *stream);

/* ---- GroupNorm / BatchNorm with an optional fused SiLU / LeakyReLU, forward and backward ----------------------------------------------------------------
 * The step in front of every convolution of VQGANEncoder / VQGANDecoder (vq/algorithms/vqgan/autoencoder.py: GroupNorm(32, C, 1e-6)
 * followed by SiLU; GroupNorm alone in Attention).  No copy, no atomics, no memset, no allocation and no synchronisation.  One launch
 * where a group fits one workgroup (n <= 8192), two otherwise; the backward adds the two launches of the dgamma / dbeta second stage.
 * INPUT   a logical [B, C, P] tensor (P = H W) in VQHIP_LAYOUT_MAP (NCHW-contiguous: a group is one contiguous run) or
 *   VQHIP_LAYOUT_ROWS (channels-last dense: a group is C / G adjacent channels at every position), VQHIP_DTYPE_F32, _BF16 or _F16,
 *   element alignment only; y and gx in the same dtype and layout.  gamma, beta, dgamma, dbeta [C] and stats [B G 2] are fp32.
 *   Every element is converted to fp32 exactly; all arithmetic is fp32 IEEE without contraction; a result is rounded to nearest
 *   even into the output dtype.
 * DEFINITION  for image b and group g, over the n = (C / G) P values of the group:
 *       mean = sum x / n;   var = sum (x - mean)^2 / n  (biased);   rstd = 1 / sqrt(var + eps)
 *       xh = (x - mean) rstd;   u = xh gamma[c] + beta[c];   y = u  (act 0)   or   y = u sigmoid(u)  (act 1, SiLU)
 *       stats[2 (b G + g)] = mean, stats[2 (b G + g) + 1] = rstd
 *   The variance is a second pass over the values a workgroup holds in registers, about that chunk's own mean; chunks recombine
 *   as M2 = sum_c (M2_c + n_c (mean_c - mean)^2), every term non-negative.  E[x^2] - mean^2 is never formed.
 *       bwd    d = 1 (act 0) or s (1 + u (1 - s)), s = sigmoid(u), recomputed from x and stats;   gu = g d;   t = gu gamma[c]
 *              gx = rstd (t - mean_grp(t) - xh mean_grp(t xh));   dgamma[c] = sum_{b, p} gu xh;   dbeta[c] = sum_{b, p} gu
 *   Nothing of the activation's size is kept besides x.  A NaN or an infinity in a group makes that group's y NaN and touches no
 *   other group.  A constant group has var = 0 and y = act(beta) within the bound below.
 * ORDER OF EVERY SUM  fixed by the shape alone (vqhip_group_norm_kernels.h says who adds what): the same inputs give the same
 *   bits of y, stats, gx, dgamma and dbeta, run to run.
 * LAUNCH SHAPE  n <= 2048: one wave per group, four groups per workgroup.  2048 < n <= 8192: one workgroup per group.  Beyond:
 *   S = ceil(n / 8192) workgroups per group leave partials in ws; a second launch combines them and writes the result (the
 *   configs' first layer at B = 8 has 256 groups of 262144 values: 8192 workgroups instead of 256).
 * SHAPES AND LIMITS (VQHIP_EINVAL before any HIP call, and no launch)  dtype one of F32 / BF16 / F16; layout one of ROWS / MAP;
 *   B, C, P, G >= 1 (or G == VQHIP_GN_BATCH: BATCH STATISTICS below); C a multiple of G; B, C, P < 2^31; B C P no overflow of
 *   int64; n < 2^31; B G S < 2^31; act 0 or 1 (with VQHIP_GN_BATCH also 2: LEAKY RELU below); eps >= 0 and finite; every pointer required; ws_bytes >= vqhip_group_norm_ws_bytes(..) (-1 for sizes the calls refuse), in both calls.
 * ERROR BOUND  against the exact value of the definition on the converted inputs; u0 = VQHIP_GN_U = 2^-24 (1 + 2^-9); first order
 *   in u0 except where a square is written; no overflow in fp32 and no underflow of exp(-u).  All quantities are magnitudes.
 *     N = VQHIP_GN_CHAIN(n) = n / 2^21 + 56 bounds the roundings a value passes into a group's sum: 32 in its thread, 6 in the
 *       wave, 2 across waves, one product and ceil(S / 256) + 8 additions across chunks, two divisions.
 *     mean: within N u0 mabs, mabs = the group's mean of |x|.  q = VQHIP_GN_Q(n, mabs, rstd) = N u0 mabs rstd is that error in
 *       units of the deviation: the part no fp32 algorithm escapes when |mean| >> sigma.
 *     rstd: M2 adds non-negative terms, each from one subtraction and one product: relative (N + 4) u0.  Inside a chunk
 *       sum (x - m)^2 = sum (x - mean_c)^2 + n_c (m - mean_c)^2 exactly, so the chunk mean's error enters squared; between chunks
 *       the means' errors dm enter as 4 sigma dm + 4 dm^2.  With sigma rstd <= 1, and 3 u0 for the addition of eps, the root and
 *       the division, and 3 u0 reserved for the subtraction and products of xh and u:
 *                                       rho = VQHIP_GN_RHO(n, q) = (N / 2 + 8) u0 + 2 q + 2 q^2
 *     xh:  E_xh = xh rho + q.      u:  E_u = gamma E_xh + 2 u0 u.
 *     y:   act 0: E_u.   act 1: 1.1 E_u + 8 u0 y   (|SiLU'| <= 1.1; exp, the addition, the division and the product: 8 u0).
 *     d:   E_d = 0 (act 0) or 0.5 E_u + 10 u0  (|SiLU''| <= 0.5).      t:  E_t = g gamma E_d + 2 u0 t.
 *     m1 = mean_grp(t): E_1 = N u0 mean_grp(t) + mean_grp(E_t).   m2 = mean_grp(t xh): E_2 = (N + 1) u0 mean_grp(t xh) + mean_grp(E_t xh + t E_xh).
 *     gx:  E_gx = rstd (E_t + E_1 + xh E_2 + m2 E_xh + 4 u0 (t + m1 + xh m2)) + rho gx.
 *     dgamma[c]: (M + 2) u0 sum(gu xh) + sum(E_gu xh + gu E_xh), dbeta[c]: M u0 sum(gu) + sum(E_gu), with E_gu = g E_d + u0 gu and
 *       M = VQHIP_SG2_GBIAS_CHAIN(slabs), slabs = B S (at most 32 + 8 additions in the first launch, the second stage above).
 *     the store: VQHIP_SG2_STORE_U(dtype) on top, as for the StyleGAN2 ops.
 *   A measurement beyond these bounds inside the range means the kernel or this derivation is wrong.
 *
 * LEAKY RELU  act == VQHIP_GN_ACT_LEAKY (2), valid with G == VQHIP_GN_BATCH only (with G >= 1 it stays VQHIP_EINVAL, as every
 *   earlier version of this header answers it): y = u for u > 0, otherwise VQHIP_GN_LEAKY_SLOPE u (0.2, held as its
 *   fp32 rounding); the backward's factor is d = 1 for u > 0, otherwise the slope, so u == 0 takes the slope as F.leaky_relu does.
 *   The backward recomputes u from x and stats with the very instruction sequence of the forward (no contraction): both directions
 *   agree on the branch.  Bound: E_y = E_u + 2 u0 y (the product and the rounding of the slope).  E_d = 0 wherever |u| > E_u;
 *   within E_u of zero the branch of the exact u is undetermined, d may be either of the two values, and no bound on t, gx,
 *   dgamma or dbeta is stated for such an element.
 *
 * BATCH STATISTICS  G == VQHIP_GN_BATCH (-2; G == 0 and G == -1 stay VQHIP_EINVAL, as every earlier version of this header answers
 *   them): BatchNorm2d in training mode, the step between the convolutions of
 *   PatchGANDiscriminator (vq/algorithms/vqgan/discriminators/: Conv2d -> BatchNorm2d -> LeakyReLU(0.2)).
 *   DEFINITION  one group per channel, spanning all B images: n = B P.  mean, the biased var, rstd, xh, u and y as above with the
 *     sums over (b, p) of channel c; stats is [C, 2]: stats[2 c] = mean, stats[2 c + 1] = rstd.  vqhip_group_norm_fwd also leaves
 *     ws[c] = mean and ws[C + c] = M2 / (n - 1), the UNBIASED variance, for c < C: an output of the call, what the host's
 *     running statistics take (no cancellation of 1 / rstd^2 - eps).  The rest of ws is scratch.
 *       bwd    gu = g d;   dbeta[c] = sum gu;   dgamma[c] = sum gu xh;   gx = gamma[c] rstd (gu - dbeta / n - xh dgamma / n),
 *              evaluated as rstd ((t - m1) - xh m2) with t = gu gamma[c], m1 = dbeta gamma[c] / n, m2 = dgamma gamma[c] / n.
 *     The channel sums are the parameter gradients: there is no dgamma / dbeta second stage.  A NaN or an infinity in a channel
 *     makes that channel's y NaN and touches no other channel.  A constant channel has var = 0 and y = act(beta) within the bound.
 *   ORDER OF EVERY SUM  fixed by the shape and the dtype alone: the same inputs give the same bits of y, stats, the block, gx,
 *     dgamma and dbeta, run to run.  No atomics, no memset, no allocation, no synchronisation.
 *   LAUNCH SHAPE  MAP: a channel's B runs of P values are cut into chunks of 8192; S = ceil(n / 8192) workgroups per channel.
 *     ROWS: a workgroup takes 8 PW adjacent channels (PW = the widest of 16 bytes, 8 bytes or one element that divides C) and a slab
 *     of 1024 / PW positions; S = ceil(n PW / 1024).  S == 1 (MAP: n <= 8192; ROWS: n <= 1024 / PW): one launch.  S > 1: three -
 *     the chunks' partials (n_c, mean_c, M2_c; backward: sum gu, sum gu xh; n_c is a function of the shape and is not stored) go to
 *     ws; one workgroup per channel combines them in a fixed order, M2 = sum_c (M2_c + n_c (mean_c - mean)^2), and writes stats and
 *     the block (backward: dgamma and dbeta, once); the last writes y (gx).  The configs' sites at B = 8, [8, 128, 64, 64],
 *     [8, 256, 32, 32] and [8, 512, 31, 31], are 512, 256 and 512 workgroups in NCHW.
 *   SHAPES AND LIMITS  as above with B G S read as C S (S of the 16-bit dtypes, the larger), and n >= 2: one value per channel is
 *     VQHIP_EINVAL (torch raises in training).  vqhip_group_norm_ws_bytes(layout, B, C, P, VQHIP_GN_BATCH) >= 8 C covers every dtype.
 *   ERROR BOUND  the one above with n = B P: every value's path into a sum stays within VQHIP_GN_CHAIN(n) roundings
 *     (vqhip_group_norm_kernels.h counts them).  mean, rstd, xh, u, y, d, t, m1, m2 and gx as above (mean_grp = the channel's mean);
 *     the block's mean within N u0 mabs, its variance within 2 VQHIP_GN_RHO(n, q) (var + eps) n / (n - 1) (rho halves the error
 *     of M2 under the root; here it is whole);  dgamma[c]: (N + 2) u0 sum(gu xh) + sum(E_gu xh + gu E_xh), dbeta[c]: N u0 sum(gu) + sum(E_gu),
 *     N = VQHIP_GN_CHAIN(n) in place of the second stage's M. */
#define VQHIP_GN_BATCH (-2)               /* G: batch statistics, one group per channel over all images */
#define VQHIP_GN_ACT_LEAKY 2              /* act: LeakyReLU(VQHIP_GN_LEAKY_SLOPE) */
#define VQHIP_GN_LEAKY_SLOPE 0.2f
#define VQHIP_GN_U (5.9604644775390625e-08 * 1.001953125)
#define VQHIP_GN_CHAIN(n) ((double)((n) / 2097152 + 56))
#define VQHIP_GN_Q(n, mabs, rstd) (VQHIP_GN_CHAIN(n) * VQHIP_GN_U * (double)(mabs) * (double)(rstd))
#define VQHIP_GN_RHO(n, q) ((VQHIP_GN_CHAIN(n) / 2.0 + 8.0) * VQHIP_GN_U + 2.0 * (double)(q) + 2.0 * (double)(q) * (double)(q))
int64_t vqhip_group_norm_ws_bytes(int layout, int64_t B, int64_t C, int64_t P, int64_t G);   /* -1 for sizes the calls refuse */
int vqhip_group_norm_fwd(const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t P, int64_t G, const float *gamma /* [C] */,
                         const float *beta /* [C] */, float eps, int act, void *y, float *stats /* [B G 2] */, float *ws, int64_t ws_bytes,
                         void *stream);
int vqhip_group_norm_bwd(const void *g, const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t P, int64_t G,
                         const float *gamma, const float *beta, const float *stats, int act, void *gx, float *dgamma /* [C] */,
                         float *dbeta /* [C] */, float *ws, int64_t ws_bytes, void *stream);

/* ---- the row ops of VQKDEncoder / VQKDDecoder: residual add + LayerNorm, bias + GELU / tanh, forward and backward --------------------
 * Everything between the GEMMs and the attention core of the pre-norm ViT of vq/algorithms/vqkd/autoencoder.py.  No copy, no atomics,
 * no memset, no allocation and no synchronisation.  Rows [R, D], dense (row stride D), element alignment only.  Every element is
 * converted to fp32 exactly; all arithmetic is fp32 IEEE without contraction; a result is rounded to nearest even into its dtype.
 * ADD + LAYER NORM
 *       fwd    s = round_to_x_dtype(x + res)  (res == NULL: s = x, sum_out is not written);   sum_out = s
 *              mean = sum s / D;   var = sum (s - mean)^2 / D  (biased, second pass from registers);   rstd = 1 / sqrt(var + eps)
 *              y = ((s - mean) rstd) gamma[c] + beta[c]  in y_dtype;   stats[2 r] = mean, stats[2 r + 1] = rstd
 *       bwd    xh = (s - mean) rstd from the saved s and stats;   t = g gamma[c]
 *              gx = rstd (t - mean_row(t) - xh mean_row(t xh)) + g_skip  (g_skip == NULL: nothing is added)
 *              dgamma[c] = sum_r g xh;   dbeta[c] = sum_r g
 *   s is what torch's `x + branch` leaves behind, bit for bit; the norm reads the ROUNDED s, as torch's LayerNorm would.
 *   Dtypes (x, res, y):  (F32, F32, F32)  (F32, BF16, BF16)  (F32, F16, F16)  (BF16, BF16, BF16)  (F16, F16, F16).  sum_out has x's dtype.  The
 *   two mixed rows are autocast: the residual stream stays fp32, the branch arrives in the autocast dtype and y leaves in it - an fp32
 *   layer norm rounded once, as by the linear that follows torch's.  res_dtype is read only where res != NULL.  Backward:
 *   s, g_skip and gx have the forward's x dtype (s_dtype), g the forward's y dtype (g_dtype); dgamma, dbeta, stats, gamma, beta fp32.
 *   A NaN or an infinity in a row makes that row's y (and gx) NaN and touches no other row.  A constant row has var = 0 and y = beta
 *   within the bound below.
 * ROW BIAS-ACTIVATION   t = x + bias[c];   y = act(t)
 *       act VQHIP_ROW_ACT_GELU   y = (t / 2) (1 + erf(t / 2^0.5))             d = (1 + erf(t / 2^0.5)) / 2 + t exp(-t^2 / 2) / (2 pi)^0.5
 *       act VQHIP_ROW_ACT_TANH   y = tanh(t)                                  d = 1 - tanh(t)^2
 *       bwd    gx = g d, recomputed from x and bias (y is not kept);   dbias[c] = sum_r of the fp32 gx  (dbias == NULL: not formed)
 *   x, y, g and gx in the call's one dtype; bias and dbias fp32.  An element's result depends on that element alone: a NaN stays
 *   where it is.
 * ADD + RMS NORM  the mode of the two add + layer norm calls with beta == NULL (fwd) / dbeta == NULL (bwd): the norms of
 *   LlamaTransformer (transformers' LlamaRMSNorm), each with the residual add in front of it folded in.
 *       fwd    s = round_to_x_dtype(x + res)  (res == NULL: s = x, sum_out is not written);   sum_out = s
 *              ms = sum s^2 / D;   rstd = 1 / sqrt(ms + eps);   y = (s rstd) gamma[c]  in fp32, rounded once into y_dtype
 *              stats[2 r] = 0, stats[2 r + 1] = rstd
 *       bwd    xh = s rstd from the saved s and stats;   t = g gamma[c]
 *              gx = rstd (t - xh mean_row(t xh)) + g_skip  (g_skip == NULL: nothing is added);   dgamma[c] = sum_r g xh
 *   dbeta is not written, and the second half of ws is not touched (ws_bytes is held to the same size).  The two calls are
 *   independent: no call sees both beta and dbeta, so a forward in one mode followed by a backward in the other is not refused - it
 *   is the caller's to pair them (vector_quantization_amd/ops.py does).  The dtype table, the sum_out rule, the g_skip rule, the slab
 *   workspace, the order of the sums, the limits on R and D and the launch shapes are the layer norm's.  A NaN in a row makes that
 *   row's y (and gx) NaN; an infinity makes ms infinite and rstd = 0, so y is 0 at the row's finite elements and NaN at the infinite
 *   one (gx: NaN); neither touches another row.  An all-zero row has ms = 0 and y = 0 (eps > 0).
 *   transformers' LlamaRMSNorm rounds s rstd to the input dtype BEFORE the product with gamma where the stream is 16-bit; this mode
 *   does not: it rounds once, at the end.  Under bf16 autocast the stream is fp32 and the two definitions coincide.
 * SWIGLU  act == VQHIP_ROW_ACT_SWIGLU (3; 2 stays VQHIP_EINVAL, as every earlier version of this header answers it) of the two row
 *   bias-activation calls: the gated MLP of LlamaTransformer behind ONE GEMM against cat(gate_proj.weight, up_proj.weight).
 *   D is the OUTPUT width F.  x is [R, 2 F] dense, gate = x[:, :F], up = x[:, F:];  y and g are [R, F];  gx is [R, 2 F].
 *       fwd    y = silu(gate) up,   silu(a) = a / (1 + exp(-a)) for a >= 0,  a exp(a) / (1 + exp(a)) for a < 0
 *       bwd    sg = sigmoid(a), recomputed from x (y is not kept):   gx[:, :F] = g up sg (1 + a (1 - sg));   gx[:, F:] = g silu(a)
 *   fp32 from the exactly converted inputs, each result rounded once.  Both directions evaluate ONE exponential per element,
 *   e = expf(max(-|a|, -88)): expf sees [-88, 0] only, the range VQHIP_VIT_EXP_ULPS was measured over; sigmoid and 1 - sigmoid are
 *   1 / (1 + e) and e / (1 + e) (a >= 0; exchanged for a < 0), so no subtraction cancels.  bias, dbias and ws must be NULL
 *   (a model with mlp_bias=True takes the torch route).  An element's result depends on its own (gate, up) pair (and g) alone: a NaN
 *   or an infinity stays in its element (backward: in the two elements of its pair).  Alignment is by element only.
 * ORDER OF EVERY SUM  fixed by the shape alone (vqhip_vit_kernels.h says who adds what): the same inputs give the same bits of
 *   every output, run to run.
 * LAUNCH SHAPE  add + layer norm, a piece = 8 elements where all tensors are 16-bit and D % 8 == 0, else 4 where D % 4 == 0, else 1:
 *   D <= 2048: one wave per row, four rows per workgroup;  2048 < D <= 8192: one workgroup per row.  The backward gives a
 *   workgroup a slab of 16 rows and leaves its column sums in ws [2, slabs, D]; two launches of the second stage follow.
 *   Row bias-activation: forward one launch over 16-byte pieces of the flat tensor, a thread per piece up to 8192 workgroups of
 *   256 threads = 2 097 152 pieces (8.4 M fp32 or 16.8 M 16-bit elements); beyond that the grid stays at 8192 workgroups and
 *   every thread strides through pieces q, q + 2 097 152, ..  Backward a workgroup per 256 rows x 64 pieces, column sums in ws
 *   [slabs, D], one launch of the second stage.  SwiGLU, both directions: one launch over the 16-byte pieces of the flat [R, F]
 *   side on the forward's grid; a piece that crosses a row end (F % 4 != 0, or F % 8 != 0 in a 16-bit dtype) goes element by element.
 * SHAPES AND LIMITS (VQHIP_EINVAL before any HIP call, and no launch)  1 <= R <= VQHIP_VIT_MAX_R = 2^24 (no launch of more than 2^32
 *   threads: the widest is 256 threads per row); 1 <= D <= VQHIP_VIT_MAX_D = 8192; R D < 2^31; a dtype
 *   combination outside the table; res != NULL with res_dtype != y_dtype; res without sum_out; eps negative or not finite; act not 0
 *   or 1; a NULL among x, gamma, beta, y, stats (fwd), g, s, gamma, stats, gx, dgamma, dbeta, ws (bwd), x, bias, y (act fwd), g, x, bias,
 *   gx (act bwd); dbias without ws; ws_bytes < 8 D vqhip_add_layer_norm_slabs(..) / 4 D vqhip_row_bias_act_slabs(..) (-1 for sizes
 *   the calls refuse).  RMS mode: beta (fwd) and dbeta (bwd) are NULL and every other pointer stays required.  SwiGLU:
 *   R 2 D >= 2^31; a bias, a dbias or a ws that is not NULL; a NULL among x, y (fwd), g, x, gx (bwd).  act 2 is refused.
 * ERROR BOUND  against the exact value of the definition on the converted inputs (for the norm: on the rounded s); u0 = VQHIP_GN_U.
 *   add + layer norm: a row is a group of n = D of the group norm, act 0, summed by the same code, so its bounds hold as they stand:
 *     mean within VQHIP_GN_CHAIN(D) u0 mabs, rstd within VQHIP_GN_RHO(D, q) rstd, y within E_u, gx within E_gx; the addition of g_skip
 *     rounds once more:  E_gx' = E_gx + u0 |gx + g_skip|.  dgamma / dbeta: the group norm's, with M = VQHIP_SG2_GBIAS_CHAIN(slabs),
 *     slabs = ceil(R / 16) (a term passes at most 16 additions in its thread and 2 across teams in the first launch).  s itself is
 *     exact: one correctly rounded addition.
 *   row bias-activation: the one thing that cannot be derived is the accuracy of the device library's erff, tanhf and expf.  No
 *     document shipped with the toolchain states it, so each was measured once on an MI355X against the float64 function over
 *     every fp32 value of erff [-6, 6], tanhf [-12, 12], expf [-88, 0] (tools/measure_libm_ulp.hip; profiles/vqkd_autoencoder.txt):
 *     1.5098, 1.4052 and 0.8907 ulp.  The constants are twice that, rounded up: L_erf = VQHIP_VIT_ERF_ULPS = 3.02, L_tanh =
 *     VQHIP_VIT_TANH_ULPS = 2.82, L_exp = VQHIP_VIT_EXP_ULPS = 1.79.  An ulp of a result of magnitude at most 1 is at most 2 u0 absolute
 *     and at most 2 u0 relative.
 *     GELU, y: t carries u0 |t|; z = t c with c within u0 / 2 of 2^-0.5: relative 2.5 u0; |z erf'(z)| <= 0.49, so erf(z) is within
 *       (1.3 + 2 L_erf) u0 absolute; h = 1 + erf rounds once (2 u0); y = (t / 2) h rounds once:
 *                               VQHIP_ROW_GELU_BOUND(t, y) = ((3 + L_erf) |t| + 2 |y|) u0         (absolute in |t|: 1 + erf cancels for t < 0)
 *     GELU, d: h / 2 within (1.7 + L_erf) u0; w = -t^2 / 2 is within 3 u0 |w|, exp(w) relative 3 u0 |w| + 2 L_exp u0, the constant and two
 *       products 3.5 u0; |t| phi(t) <= 0.242 and |w t| phi(t) <= 0.231 give (1.8 + 0.5 L_exp) u0; the sum rounds once (|d| <= 1.13):
 *                               VQHIP_ROW_GELU_GRAD_BOUND = (5 + L_erf + L_exp / 2) u0                                      (absolute)
 *     tanh, y: |t tanh'(t)| <= |tanh(t)|, so t's rounding costs u0 |y|:   VQHIP_ROW_TANH_BOUND(y) = (1 + 2 L_tanh) u0 |y|
 *     tanh, d: y^2 within (3 + 4 L_tanh) u0 y^2, the subtraction rounds once:
 *                               VQHIP_ROW_TANH_GRAD_BOUND(y, d) = ((3 + 4 L_tanh) y^2 + |d|) u0
 *     gx = g d: |g| E_d + u0 |gx|.   dbias[c]: M u0 sum |gx| + sum E_gx, M = VQHIP_SG2_GBIAS_CHAIN(slabs), slabs = ceil(R / 256).
 *     Both y bounds carry VQHIP_VIT_TINY = 2^-148 absolute: a subnormal t loses up to half a subnormal ulp in t / 2 and in t c.
 *   add + RMS norm: the layer norm's derivation with no mean, so q = 0 and every m1 term is absent; N = VQHIP_GN_CHAIN(D).
 *     ms adds D non-negative terms of one product each: relative (N + 1) u0; half of that under the root, 3 u0 for the addition of
 *     eps, the root and the division, and 3 u0 reserved for the products of xh and y:   rho = VQHIP_GN_RHO(D, 0) = (N / 2 + 8) u0.
 *     rstd: within rho rstd.      xh: E_xh = rho |xh|.      y: E_y = |gamma| E_xh + 2 u0 |y|.
 *     t = g gamma: E_t = 2 u0 |t|.   m2 = mean_row(t xh): E_2 = (N + 1) u0 mean_row(|t xh|) + mean_row(E_t |xh| + |t| E_xh).
 *     gx: E_gx = rstd (E_t + |xh| E_2 + |m2| E_xh + 4 u0 (|t| + |xh m2|)) + rho |gx|;   with g_skip: E_gx' = E_gx + u0 |gx + g_skip|.
 *     dgamma[c]: (M + 2) u0 sum |g xh| + sum (u0 |g xh| + |g| E_xh), M = VQHIP_SG2_GBIAS_CHAIN(slabs), slabs = ceil(R / 16).
 *     (These are the group norm's E_u, E_gx and dgamma formulas evaluated at q = 0, beta = 0, m1 = 0, act 0.)
 *   SwiGLU: L = VQHIP_VIT_EXP_ULPS, so e = expf(..) is within 2 L u0 e; den = 1 + e rounds once and e / (1 + e) <= 1 / 2:
 *     relative (L + 1) u0.  a >= 0: s = a / den, (L + 2) u0 |s|.  a < 0: a e carries (2 L + 1) u0, the division one more: (3 L + 3) u0 |s|.
 *       silu:  E_s = (3 L + 3) u0 |s|.        y = s up rounds once:        E_y = (3 L + 4) u0 |y|
 *     sg and qc = 1 - sg are 1 / den or e / den: relative (3 L + 2) u0.  a qc: (3 L + 3) u0 |a| qc;  w = 1 + a qc rounds once; d = sg w
 *     rounds once; sg |a| qc = |a sigmoid'(a)| <= 0.224:
 *       d:     E_d = ((3 L + 3) |a| sg (1 - sg) + (3 L + 4) |d|) u0                                                   (absolute)
 *       gx gate = (g up) d:  |g up| E_d + 2 u0 |gx|.        gx up = g s:  |g| E_s + u0 |gx|.
 *     Underflow: where e, a e or a result is subnormal an absolute term takes the place of a relative one, VQHIP_VIT_TINY (1 + (1 + |a|) |f|)
 *     with f = up (y), g up (gx gate), g (gx up): L + 1 subnormal ulps of s per unit of |a|, and half of one for the result itself.
 *     |a| > 88: the held argument leaves e within exp(-88) < 2^-126 of exp(-|a|):  2^-126 (1 + |a|) |f| more, the same f.
 *   the store: VQHIP_SG2_STORE_U(dtype) on top, as for the StyleGAN2 ops.
 *   A measurement beyond these bounds inside the range means the kernel or this derivation is wrong. */
#define VQHIP_VIT_MAX_D 8192
#define VQHIP_VIT_MAX_R (1 << 24)
#define VQHIP_ROW_ACT_GELU 0
#define VQHIP_ROW_ACT_TANH 1
#define VQHIP_ROW_ACT_SWIGLU 3            /* x = (gate | up) [R, 2 D]; 2 is not an activation */
#define VQHIP_VIT_ERF_ULPS 3.02
#define VQHIP_VIT_TANH_ULPS 2.82
#define VQHIP_VIT_EXP_ULPS 1.79
#define VQHIP_VIT_TINY 2.8025969286496341e-45
#define VQHIP_ROW_GELU_BOUND(t, y) (((3.0 + VQHIP_VIT_ERF_ULPS) * (double)(t) + 2.0 * (double)(y)) * VQHIP_GN_U + VQHIP_VIT_TINY)
#define VQHIP_ROW_GELU_GRAD_BOUND ((5.0 + VQHIP_VIT_ERF_ULPS + VQHIP_VIT_EXP_ULPS / 2.0) * VQHIP_GN_U)
#define VQHIP_ROW_TANH_BOUND(y) ((1.0 + 2.0 * VQHIP_VIT_TANH_ULPS) * VQHIP_GN_U * (double)(y) + VQHIP_VIT_TINY)
#define VQHIP_ROW_TANH_GRAD_BOUND(y, d) (((3.0 + 4.0 * VQHIP_VIT_TANH_ULPS) * (double)(y) * (double)(y) + (double)(d)) * VQHIP_GN_U)
int64_t vqhip_add_layer_norm_slabs(int64_t R, int64_t D);                       /* -1 for sizes the calls refuse */
int vqhip_add_layer_norm_fwd(const void *x, int x_dtype, const void *res /* or NULL */, int res_dtype, int64_t R, int64_t D,
                             const float *gamma /* [D] */, const float *beta /* [D], or NULL: RMS */, float eps, void *sum_out /* with res */, void *y,
                             int y_dtype, float *stats /* [R, 2] */, void *stream);
int vqhip_add_layer_norm_bwd(const void *g, int g_dtype, const void *s, int s_dtype, const void *g_skip /* or NULL */, int64_t R, int64_t D,
                             const float *gamma, const float *stats, void *gx, float *dgamma /* [D] */, float *dbeta /* [D], or NULL: RMS */, float *ws,
                             int64_t ws_bytes, void *stream);
int64_t vqhip_row_bias_act_slabs(int64_t R, int64_t D);                         /* -1 for sizes the calls refuse */
int vqhip_row_bias_act_fwd(const void *x, int dtype, int64_t R, int64_t D, const float *bias /* [D]; SwiGLU: NULL */, int act, void *y,
                           void *stream);
int vqhip_row_bias_act_bwd(const void *g, const void *x, int dtype, int64_t R, int64_t D, const float *bias, int act, void *gx,
                           float *dbias /* [D] or NULL */, float *ws, int64_t ws_bytes, void *stream);

/* ---- static KV cache: the attention step of cached generation (LlamaTransformer with static_cache=True) --------------------
 * What transformers' LlamaAttention does between its projections and o_proj when one token follows a cache - apply_rotary_pos_emb,
 * two torch.cat of DynamicCache.update, sdpa, a transpose - as ONE launch on caches allocated once; and the same storage rule for
 * the L >= 1 tokens of a prompt, whose (MFMA) attention stays with the framework.
 * INPUT   q, k, v: the new tokens' projections, rows [R, H Dh] with the heads contiguous inside a row (H = Hq for q, Hkv for k
 *   and v), each with its own row stride in elements (>= H Dh), so the three may be views into one packed [R, (Hq + 2 Hkv) Dh]
 *   GEMM output; R = B (decode) or B L (append, row r = b L + t).  dtype VQHIP_DTYPE_F32, _BF16 or _F16.  cos, sin: fp32 [L, Dh]
 *   for the new positions, as LlamaRotaryEmbedding holds them before its cast.  k_cache, v_cache: [B, Hkv, cap, Dh], contiguous,
 *   in dtype.  seen: the positions already stored, a host integer by value (a captured vqhip_decode_attention or
 *   vqhip_rope_append launch replays the same position; vqhip_decode_attention_at below reads it from device memory instead).
 * ROTARY  transformers' rotate_half convention, half = Dh / 2:  x'[i] = x[i] cos[i] - x[i + half] sin[i],
 *   x'[i + half] = x[i + half] cos[i + half] + x[i] sin[i + half].  fp32 arithmetic on the loaded values, the two products kept
 *   with their remainders (fma) and summed by a two-sum, so x' is the fp32 nearest to the exact value of the fp32 inputs or its
 *   neighbour whatever cancels between the products.
 * STORE   k' is rounded once (nearest even) to dtype and stored at position seen + t; v is copied there bit for bit.  Nothing past
 *   position seen + L - 1 and nothing of another batch row's cache is written.
 * vqhip_rope_append  writes q' rounded once to dtype as q_out [B, Hq, L, Dh] (what a causal sdpa reads) beside the store.
 * vqhip_decode_attention (L = 1)  q' stays fp32.  With n = seen + 1, the step's own key read back as stored (after its rounding, so
 *   that a later step sees the same value), group G = Hq / Hkv, and query head h reading kv head h / G:
 *       s_j = scale * dot(q'_h, K[b, h / G, j]),  j = 0 .. n - 1;   p_j = exp(s_j - max_j s_j);
 *       out[b, h Dh + i] = (sum_j p_j V[b, h / G, j, i]) / (sum_j p_j), rounded once to dtype: rows [B, Hq Dh], dense, the layout
 *   o_proj reads.  All of it fp32 on the loaded values, as an online softmax (running maximum subtracted) per group of positions,
 *   the groups merged in a fixed order: no atomics, a row's bits depend on (its own inputs, seen, Dh, G, dtype) alone - not on B,
 *   on other rows, on cap or on the run.  Positions >= n are never read: whatever they hold (NaN included) cannot reach out.
 *   One workgroup per (b, kv head) serves the G query heads from one pass over K and V in 16-byte loads; the length is not split
 *   across workgroups.
 * LIMITS  each refused with VQHIP_EINVAL before any HIP call, vqhip_last_error naming the clause: Dh a multiple of 8 with
 *   16 <= Dh <= VQHIP_ATTN_MAX_HEAD_DIM; Hq % Hkv == 0 and Hq / Hkv <= VQHIP_ATTN_MAX_GROUP; 1 <= cap <= VQHIP_ATTN_MAX_LEN;
 *   0 <= seen and seen + L <= cap; row strides >= H Dh; B, L >= 1, B L and B Hkv < 2^31; scale finite; k_cache and v_cache
 *   16-byte aligned (they are read 16 bytes at a time: a cache one element off a boundary is refused by name); q, k, v, cos,
 *   sin and the output are read and written element by element and need the alignment of their element type only.
 * ERROR   of out against the definition in exact arithmetic on the same stored cache, u = VQHIP_GN_U, A = max_j sum_i |q'_i K_j,i|,
 *   vmax = max_j |V_j,i|:   S = 17 u scale A  bounds a score (q' 1, product 1, at most 7 + 5 additions, the scale 1 rounding, (1 + u)^17);
 *   a weight p_j then carries exp(+-S), one expf and at most two roundings per rescale or merge it passes through - at most
 *   n / 8 + 10 of them (a slot holds every 8th position at least; 5 butterfly levels, 4 waves) at 6 u each with expf within
 *   VQHIP_VIT_EXP_ULPS ulps - and the roundings of the exponents' arguments, which telescope to u (max - s_j) and weigh at most
 *   u ln n in the mean:   eta = expm1(S) + (6 (n / 8 + 10) + 10) u;   |out - exact| <= 2 eta / (1 - eta) vmax + u |out|
 *   + n 2^-126 vmax (weights that underflow) in fp32 before the store, VQHIP_SG2_STORE_U(dtype) on top.  The Python form of this
 *   bound lives beside the float64 restatement of the tests (tests/decode_attention_ref.py); DESIGN.md §8 has the derivation.
 * vqhip_decode_attention_at  the same step with the position in DEVICE memory, so that one captured launch serves every generated
 *   token: every workgroup loads s = *pos (int32, 4-byte aligned) once, uses seen = s and row s of cos_table and sin_table, fp32
 *   [cap, Dh] (row j: the cos, sin of position j).  The kernel body is vqhip_decode_attention's: with *pos == s and the tables' row s
 *   equal to the cos, sin of the by-value call, every byte written - out, row s of k_cache, row s of v_cache - is the byte that
 *   vqhip_decode_attention(..., seen = s, ...) writes, and the error bound above holds unchanged.  With s < 0 or s >= cap the launch
 *   writes nothing at all: out and the caches are left as they are.  LIMITS as above without the seen clause; pos must not be null
 *   and must be 4-byte aligned.
 * vqhip_decode_advance  the end of a replayed step, one workgroup: with s = *pos, if 0 <= s and s + 1 < length then
 *   sequence[r, s + 1] = token[r] as it is (the sampler's -1 for a bad row stays visible), next[r] = token[r] < 0 ? 0 : token[r] (no
 *   embedding gather of a later replay leaves its table) for r = 0 .. R - 1, and afterwards *pos = s + 1; otherwise nothing is
 *   written and pos stays where it is.  token [R], next [R], sequence [R, length] are int64 on the device.  Every thread reads pos
 *   in front of a barrier, thread 0 stores the new count behind the writes with an ordinary store: no atomics.  LIMITS (VQHIP_EINVAL
 *   before any HIP call): all pointers non-null, token, next and sequence 8-byte and pos 4-byte aligned, 1 <= R < 2^31,
 *   2 <= length <= VQHIP_ATTN_MAX_LEN.
 * The last parameter of each is the hipStream_t the launch goes to. */
#define VQHIP_ATTN_MAX_HEAD_DIM 128
#define VQHIP_ATTN_MAX_GROUP 8
#define VQHIP_ATTN_MAX_LEN 4096
int vqhip_decode_attention(const void *q, int64_t q_stride, const void *k, int64_t k_stride, const void *v, int64_t v_stride, int dtype,
                           const float *cos, const float *sin, void *k_cache, void *v_cache, int64_t seen, int64_t cap, float scale,
                           int64_t B, int Hq, int Hkv, int Dh, void *out, void *hip_stream);
int vqhip_decode_attention_at(const void *q, int64_t q_stride, const void *k, int64_t k_stride, const void *v, int64_t v_stride, int dtype,
                              const float *cos_table, const float *sin_table /* fp32 [cap, Dh] */, void *k_cache, void *v_cache,
                              const int32_t *pos /* device, 4-byte aligned */, int64_t cap, float scale,
                              int64_t B, int Hq, int Hkv, int Dh, void *out, void *hip_stream);
int vqhip_decode_advance(const int64_t *token /* [R] */, int64_t *next /* [R] */, int64_t *sequence /* [R, length] */,
                         int64_t R, int64_t length, int32_t *pos, void *hip_stream);
int vqhip_rope_append(const void *q, int64_t q_stride, const void *k, int64_t k_stride, const void *v, int64_t v_stride, int dtype,
                      const float *cos, const float *sin, void *k_cache, void *v_cache, int64_t seen, int64_t cap, int64_t B, int64_t L,
                      int Hq, int Hkv, int Dh, void *q_out, void *hip_stream);

/* ---- fused reconstruction metrics: L1, MSE, PSNR and SSIM of a validation pass ---------------------------------------------
 * The four numbers of the reference's table per tokenizer (docs/pretrained_models.md:47-51) that come from ImageLossMetric
 * (vq/runners/metrics/loss.py) over L1Loss, MSELoss, PSNRLoss and SSIMLoss (vq/tasks/image_reconstruction/losses.py), each of
 * which decodes both images again, and SSIM on the host through scikit-image.  Here: two launches, both images read once, no
 * image-sized intermediate, no atomics, no memset, no allocation and no synchronisation.
 * INPUT   pred and image, both [B, C, H, W], each with its own dtype (VQHIP_DTYPE_F32, _BF16, _F16: values in the model's range
 *   [-1, 1]; VQHIP_DTYPE_U8: bytes already decoded) and its own layout (VQHIP_IMAGE_NCHW contiguous, VQHIP_IMAGE_NHWC
 *   channels-last dense); element alignment only.
 * DECODE  vq/datasets/base.py:70-73, `((v + 1) * 127.5).clamp(0, 255).to(uint8)`, literally in the tensor's dtype:
 *       fp32           t = (v + 1.0f) * 127.5f                                   (two fp32 operations, no contraction)
 *       bf16 / fp16    t1 = rnd(float(v) + 1.0f);  t = rnd(float(t1) * 127.5f)   (rnd: nearest even into the dtype, as torch)
 *       byte = (uint8)min(max(t, 0), 255), truncated.  The bytes equal the reference's decode of the same tensor bit for bit.
 *   A NaN has no defined byte in torch (the cast is undefined there): here it counts as byte 0 in the integer sums, and makes
 *   all four values of ITS image NaN; other images are untouched.  +-inf decode to 255 / 0 like any value beyond the range.
 * SUMS    with the bytes p (pred), q (image) and n = C H W, per image:  abs_sum = sum |p - q|,  sq_sum = sum (p - q)^2, int64, exact.
 * VALUES  l1 = abs_sum / (255 n);  mse = sq_sum / (255^2 n): one IEEE double division each (255 n and 65025 n are exact);
 *   psnr = -10 log10(mse) in double, +inf where sq_sum == 0.
 *   ssim: scikit-image's structural_similarity(pred / 255, image / 255, channel_axis=0, data_range=1) with its defaults -
 *   uniform 7 x 7 window, sample covariance (N / (N - 1), N = 49), K1 = 0.01, K2 = 0.03, a 3-pixel border cropped (every window
 *   lies inside the image: the filter's boundary mode never matters), mean over the windows of a channel, then over channels -
 *   evaluated from EXACT integer moments.  Per window, with the sums sx, sy, sxx, syy, sxy of p, q, p^2, q^2, p q (int32):
 *       ux = sx / (49 * 255)                       uy = sy / (49 * 255)
 *       vx  = (49 sxx - sx^2)  / (49 * 48 * 255^2)  vy = (49 syy - sy^2) / (49 * 48 * 255^2)
 *       vxy = (49 sxy - sx sy) / (49 * 48 * 255^2)                        (the numerators are exact integers below 2^28)
 *       S   = ((2 ux uy + c1) (2 vxy + c2)) / ((ux^2 + uy^2 + c1) (vx + vy + c2))                  in double, no contraction
 *   c1, c2 are passed by value: the doubles Python gives for (0.01 * 1) ** 2 and (0.03 * 1) ** 2.  Each window adds
 *   llrint(S 2^40) to an int64; ssim = (double)sum / 2^40 / (C (H - 6) (W - 6)).  The differences that cancel in scikit-image's
 *   float32 filter are exact here.  An identical pair gives S == 1 in every window (numerator and denominator are the same
 *   doubles) and ssim == 1.0 exactly.  want_ssim == 0: the ssim column is NaN, nothing of SSIM is computed, any H, W >= 1.
 * ORDER   every sum over pixels or windows is an integer sum, so no result depends on the order of the additions: not on the
 *   tile size, the grid, the layout, the other images of the batch, and run to run the same bits.
 * ERROR BOUND of ssim against the float64 evaluation of the same definition, VQHIP_IMAGE_SSIM_BOUND = 2^-40.  With u = 2^-53:
 *   ux, uy, vx, vy, vxy carry one rounding each.  The factors of positive terms (2 ux uy + c1, ux^2 + uy^2 + c1, vx + vy + c2)
 *   carry at most 4 u relative.  2 vxy + c2 may cancel: its absolute error is at most 3 u (|2 vxy| + c2) <= 3 u (vx + vy + c2),
 *   because |2 vxy| <= vx + vy, which is 3 u relative to the denominator's factor, so it moves S by at most 3 u.  The two
 *   products and the division add 3 u on |S| <= 1.  |S_kernel - S_exact| <= 14 u (1 + small) < 2^-49; another float64
 *   evaluation of the definition is as far from S_exact, so two evaluations differ by less than 2^-48.  The rounding to fixed
 *   point adds 2^-41 per window, and a mean does not exceed its largest term; the conversion of the int64 sum and the two last
 *   divisions add 3 u.  In all 2^-41 + 2^-48 + 3 u < 2^-40.  A measurement beyond it means the kernel or this derivation is wrong.
 * WORKSPACE  vqhip_image_metrics_workspace_bytes(B, C, H, W): 32 bytes per workgroup (one per image, channel and T x T tile of
 *   pixels, T = VQHIP_IMAGE_METRICS_TILE), every byte written before it is read.
 * OUTPUT  values64 [B, 4] double = l1, mse, psnr, ssim;  values32 [B, 4] float = the same, rounded once;  sums [B, 2] int64 =
 *   abs_sum, sq_sum.
 * LIMITS (VQHIP_EINVAL before any HIP call): no null pointer; dtypes and layouts as above; B, C >= 1; 1 <= H, W <= 2^30;
 *   B * C * ceil(H / T) * ceil(W / T) < 2^31 and C H W < 2^37; with want_ssim: H >= 7 and W >= 7 (scikit-image raises there
 *   too) and C (H - 6) (W - 6) <= 2^22 (beyond it the fixed-point sum could leave int64); ws_bytes as asked for. */
#define VQHIP_DTYPE_U8 5      /* images of vqhip_image_metrics only */
#define VQHIP_IMAGE_NCHW 0
#define VQHIP_IMAGE_NHWC 1
#define VQHIP_IMAGE_METRICS_TILE 32
#define VQHIP_IMAGE_SSIM_MAX_WINDOWS (1ll << 22)
#define VQHIP_IMAGE_SSIM_BOUND 9.094947017729282e-13   /* 2^-40 */
int64_t vqhip_image_metrics_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int vqhip_image_metrics(const void *pred, int pred_dtype, int pred_layout, const void *image, int image_dtype, int image_layout,
                        int64_t B, int64_t C, int64_t H, int64_t W, int want_ssim, double c1, double c2,
                        void *ws, int64_t ws_bytes, double *values64 /* [B, 4] */, float *values32 /* [B, 4] */,
                        int64_t *sums /* [B, 2] */, void *stream);

/* ---- EntropyLoss (vq/algorithms/vq/losses.py:130-153) on row blocks of the distance matrix ------------------------------
 * With a = d / T, p = softmax(a, -1), q_k = (1/N) sum_n p_nk:
 *   L = (1/N) sum_n (lse_n - sum_k p_nk a_nk) + sum_k q_k log(q_k + 1e-5)
 *   dL/da_nj = (p_nj / N) (c_j - a_nj - S_n),  c_k = log(q_k + 1e-5) + q_k / (q_k + 1e-5),  S_n = sum_k p_nk (c_k - a_nk).
 * The caller walks the rows in blocks: `tile` is the dense fp32 [R, K] block of distances (vqhip_distance of a row slice),
 * 16-byte aligned.  No [N, K] object is needed: forward = vqhip_entropy_rows per block, then vqhip_entropy_finish once;
 * backward = vqhip_entropy_grad per block on the recomputed tile.  All sums run in a fixed order (no atomics).
 * `ws`: vqhip_entropy_workspace_bytes(R, K) bytes of scratch (column partials), reusable from block to block.
 * LIMITS (VQHIP_EINVAL before any launch): 1 <= R < 2^31, 1 <= K <= 2^31 - 2048 (a row is indexed with int), T finite and
 * non-zero (negative allowed), metric L2 or COS.  The tile's R * K elements are addressed in int64; bounding its bytes is the
 * caller's business (ops.py: 64 MiB). */
int64_t vqhip_entropy_workspace_bytes(int64_t R, int64_t K);
/* lse[R], spa[R] = sum_k p a of the block's rows; qacc double[K] (+)= sum over the block's rows of p_nk (init != 0: the
 * first block, qacc is overwritten). */
int vqhip_entropy_rows(const float *tile, int64_t R, int64_t K, float temperature, float *lse, float *spa, double *qacc,
                       int init, void *ws, int64_t ws_bytes, void *stream);
/* after the last block: q[K] = qacc / N, c[K], loss[1] from lse[N], spa[N] of all rows */
int vqhip_entropy_finish(const float *lse, const float *spa, const double *qacc, int64_t N, int64_t K, float *q, float *c,
                         float *loss, void *stream);
/* tile <- upstream * dL/dd = upstream * dL/da / T (COS), divided once more by d with 0 where d == 0 (L2: the G of
 * torch.cdist's backward); rowsum[R] = its row sums; L2 only: colacc double[K] (+)= its column sums (init as above; COS
 * ignores colacc and ws).  lse, spa: this block's rows; inv_nt = 1 / (N T); upstream: DEVICE scalar (null = 1). */
int vqhip_entropy_grad(float *tile, int64_t R, int64_t K, float temperature, const float *lse, const float *spa,
                       const float *c, float inv_nt, const float *upstream, int metric, float *rowsum, double *colacc,
                       int init, void *ws, int64_t ws_bytes, void *stream);

/* dst[idx[n], :] += src[n, :]  (centroids.scatter_add_, vqkd/quantizers/callbacks.py:60-62; also the
 * dense embedding backward).  fp32 atomics. */
int vqhip_scatter_add_rows(const float *src, const int64_t *idx, int64_t N, int64_t K, int D, float *dst,
                           void *stream);

/* ---- codebook updates ------------------------------------------------------------------------------- */
/* VQKDCallback._kmeans tail + after_encode (callbacks.py:66-70,126-128,73-75):
 *   c = where(hist>0, sums/max(hist,1), w); c = normalize(c); c = w*decay + c*(1-decay); w = normalize(c)
 * hist int64[K] / sums[K,D] are the (all-reduced) statistics.  In place on w.  centroid_only != 0 stops after the
 * first line (VQKDCallback._kmeans as used by the k-means lazy init, callbacks.py:104-107). */
int vqhip_vqkd_update(float *w, const int64_t *hist, const float *sums, int64_t K, int D, float decay,
                      int centroid_only, void *stream);
/* CVQVAECallback.after_encode (quantizer_callback.py:94-102):
 *   p = p*ema_decay + (hist/numel)*(1-ema_decay);  decay_k = 1 - exp(-p_k*K*10/(1-ema_decay) - eps)
 *   w_k = w_k*decay_k + anchors_k*(1-decay_k)      — in place on p[K] and w[K,D].
 * numel_dev (nullable DEVICE int64) overrides numel: the all-reduced token count can stay on the device.
 * stage: 1 = update p only (the anchor sampler runs between the two halves, quantizer_callback.py:94-96),
 *        2 = update w only from the current p, 3 = both. */
int vqhip_cvq_update(float *w, float *p, const int64_t *hist, int64_t numel, const int64_t *numel_dev,
                     const float *anchors, int64_t K, int D, float ema_decay, float eps, int stage, void *stream);
/* The whole single-rank update with NearestAnchor in ONE launch (quantizer_callback.py:89-103 + anchors.py:83-84):
 *   p_out[k] = p_in[k]*g + (hist[k]/numel)*(1-g);  decay_k = 1 - exp(-p_out[k]*K*10/(1-g) - eps)
 *   w_out[k] = w_in[k]*decay_k + x[col_idx[k]]*(1-decay_k)
 * hist is the int32 histogram of the argmin epilogue, col_idx the output of vqhip_col_argmin, x the latents [N,D]
 * (fp32 or bf16).  Same expressions in the same order as stage 1 + vqhip_gather_rows + stage 2 (bit-identical);
 * w_out may alias w_in, p_out may alias p_in.  With more than one rank the histogram and the anchors are all-reduced
 * between the stages, so the staged form above is the one to use. */
int vqhip_cvq_step(const float *w_in, float *w_out, const float *p_in, float *p_out, const int32_t *hist, int64_t numel,
                   const void *x, int x_dtype, const int64_t *col_idx, int64_t K, int D, float ema_decay, float eps,
                   void *stream);
/* The same update for a subset of the codes.  decay_k == 1.0f (every code with p_k above ~1e-6 at K = 16384) multiplies
 * the code's anchor by exactly 0, so only the codes with decay_k < 1 need an anchor at all: vqhip_cvq_decay writes
 * decay[K] with the update's own expression (bit for bit), the caller selects rows = {k : decay_k < 1}, computes /
 * all-reduces anchors for those M codes only, and vqhip_cvq_update_rows applies
 *   w[rows[i]] = w[rows[i]]*decay + anchors_sub[i]*(1-decay).
 * Identical to stage 2 of vqhip_cvq_update on every finite input (a skipped code keeps w_k instead of w_k*1 + a*0: only a
 * negative-zero weight or a non-finite anchor could tell the difference). */
int vqhip_cvq_decay(const float *p, int64_t K, float ema_decay, float eps, float *decay, void *stream);
int vqhip_cvq_update_rows(float *w, const float *p, const int64_t *rows, const float *anchors_sub, int64_t M, int64_t K, int D,
                          float ema_decay, float eps, void *stream);
/* ---- the ONE exchange step of a training forward --------------------------------------------------
 * Packed fp32 buffer = [counts: low 16 bits, K floats][counts: bits above, K floats][token count in 16-bit pieces, 3 floats]
 * [0][payload rows M x D], vqhip_pack_floats(K, M, D) floats in all.  Each count piece is an integer < 2^16, so a SUM
 * all-reduce over up to 256 ranks adds them EXACTLY in fp32 whatever the order: the code-hit histogram and the token
 * count (QuantStatistics' two int64 all-reduces, vq/algorithms/vq/utils.py:34-35) travel in the same collective as the fp32
 * payload (VQ-KD centroid sums, vqkd/quantizers/callbacks.py:63-64; CVQ-VAE anchors, cvqvae/anchors.py:65-67).
 * vqhip_pack_counts writes the header from an int32 (hist_is_int64 = 0) or int64 histogram; vqhip_unpack_counts turns an
 * all-reduced header back into int64 out[K+1] = counts ‖ token count. */
int64_t vqhip_pack_floats(int64_t K, int64_t M, int D);
int vqhip_pack_counts(const void *hist, int hist_is_int64, int64_t numel, int64_t K, float *packed, void *stream);
int vqhip_unpack_counts(const float *packed, int64_t K, int64_t *out, void *stream);

/* ---- the collective of that exchange step, on the CALLER'S stream (vqhip_allreduce_packed) ------------
 * Replaces the reference's per-quantity torch.distributed.all_reduce calls (vq/algorithms/vq/utils.py:34-35,
 * vqkd/quantizers/callbacks.py:63-64, cvqvae/anchors.py:65-67) by ONE in-place fp32 SUM over the packed buffer, enqueued
 * by RCCL on the very stream the pack / apply kernels run on: no side stream, no event hop either side, capturable into a
 * HIP graph with the rest of the step.  libvqhip does not link RCCL: the symbols are resolved at run time from the
 * librccl.so the process already has (PyTorch-ROCm ships one; two RCCL copies in one process must be avoided) or from
 * `path`.  These four are HOST-side set-up calls and the only entry points that block or allocate (inside RCCL):
 *   vqhip_rccl_load(path)            path NULL or "": the librccl.so already mapped into the process (never a fresh copy from the
 *                                    loader's search path: VQHIP_ERCCL if none is mapped under that name); idempotent.
 *   vqhip_rccl_unique_id(id)         HOST buffer of VQHIP_RCCL_ID_BYTES; called on ONE rank, the bytes are handed to the
 *                                    others by whatever the application has (torch.distributed's store here).
 *   vqhip_rccl_comm_init(&comm, nranks, id, rank)   collective over the ranks; binds the CURRENT HIP device.
 *   vqhip_rccl_comm_destroy(comm)
 * vqhip_allreduce_packed: buf[0..floats) += the same range of every other rank, result on every rank; the first
 *   vqhip_pack_floats(K, M, D) floats of a packed buffer.  Never synchronises. */
#define VQHIP_RCCL_ID_BYTES 128
int vqhip_rccl_load(const char *path);
int vqhip_rccl_unique_id(void *id_host);
int vqhip_rccl_comm_init(void **comm, int nranks, const void *id_host, int rank);
int vqhip_rccl_comm_destroy(void *comm);
int vqhip_allreduce_packed(float *buf, int64_t floats, void *comm, void *stream);

/* CVQ-VAE with anchors for the codes that can need one (quantizer_callback.py:85-103, NearestAnchor anchors.py:83-84).
 * decay_k == 1.0f — every code in regular use — multiplies the code's anchor by exactly 0.  vqhip_cvq_rows lists, from the
 * probabilities BEFORE this step's update, the codes whose decay can still come out below 1 (the coming p is >= p*ema_decay
 * and decay is monotone in p; a safety factor of 14 on the rounding boundary: vqhip_exchange_kernels.h): rows[0..count)
 * ascending, slot[k] = position of code k in rows or -1, count[0] — all DEVICE int32 (rows, slot: K entries).  The set
 * depends only on the synchronised p, so every rank derives the same one before anything is exchanged.
 * vqhip_col_argmin_rows: col_idx[i] = nearest latent of code rows[i] for i < count — vqhip_col_argmin's pipeline and
 *   arithmetic on the listed codes; the launches are sized for `cap` (>= the count; the host need not know it: a HIP graph
 *   captures cap = K), rows past the count cost an early exit; ws = vqhip_col_rows_workspace_bytes(N, cap, D).  A SHORT list
 *   (ceil(cap / 32) * ceil(N / 128) * D <= 2^18; fp32 latents) skips the proposal pipeline: the whole-batch fp32 pass of the
 *   definition itself over the listed codes, one launch behind a tiny one (two more for the L2 norms) instead of five — the
 *   same indices (tuning key 15 = 0 sends short lists through the pipeline as well: A/B, tests).
 * vqhip_cvq_pack: this rank's packed buffer — header from the int32 epilogue histogram, payload row i = x[col_idx[i]]
 *   for i < count, zeros up to cap.  All-reduce the first vqhip_pack_floats(K, cap, D) floats.
 * vqhip_cvq_apply: p_out = p_in*g + (hist/numel)*(1-g); decay as above; w_out[k] = w_in[k]*decay + a*(1-decay) for listed
 *   codes, w_in[k]*decay (= w_in[k]) for the others.  packed != NULL: counts and anchor sums from the all-reduced buffer,
 *   a = sum/world; packed == NULL (one rank): counts from hist/numel, a = x[col_idx[slot[k]]].  Outputs may alias inputs.
 *   cap: the capacity the column pass / pack were sized for; a code whose slot lies at or beyond it has no anchor in
 *   col_idx / packed (a list longer than the capacity the caller chose is the caller's error): it keeps w_k * decay_k and
 *   nothing outside the buffers is read.
 *   Bit-identical to vqhip_cvq_update / vqhip_cvq_step on finite data (a non-listed code keeps w_k instead of w_k*1 + a*0:
 *   only a negative-zero weight or a non-finite anchor could tell the difference). */
int vqhip_cvq_rows(const float *p, int64_t K, float ema_decay, float eps, int32_t *rows, int32_t *slot, int32_t *count,
                   void *stream);
int64_t vqhip_col_rows_workspace_bytes(int64_t N, int64_t cap, int D);
int vqhip_col_argmin_rows(const void *x, int x_dtype, const float *e, const int32_t *rows, const int32_t *count, int64_t cap,
                          int64_t N, int64_t K, int D, int metric, int64_t *col_idx, void *ws, int64_t ws_bytes, void *stream);
int vqhip_cvq_pack(const int32_t *hist, int64_t numel, const void *x, int x_dtype, const int64_t *col_idx, const int32_t *count,
                   int64_t cap, int64_t K, int D, float *packed, void *stream);
int vqhip_cvq_apply(const float *w_in, float *w_out, const float *p_in, float *p_out, const int32_t *hist, int64_t numel,
                    const void *x, int x_dtype, const int64_t *col_idx, const float *packed, int world, const int32_t *slot,
                    int64_t cap, int64_t K, int D, float ema_decay, float eps, void *stream);
/* NearestAnchor(sync=True) over more than one rank (vq/algorithms/cvqvae/anchors.py:50-57,83-84; configs/cluster/model.py:28).
 * The reference all-gathers the latents and the whole [N, K] matrix and takes the column argmin of the concatenation — the
 * nearest latent of a code over ALL ranks' tokens, the lowest (rank, row) among equal distances; the anchor is NOT averaged.
 * Here every rank runs vqhip_col_argmin_rows over its own tokens, then:
 * vqhip_cvq_col_keys: keys[i] = (distance of listed code rows[i] to its local winner col_idx[i] — the fp32 definition's own
 *   value, ordered as torch.argmin orders it: NaN first, -0 == +0 — : rank, 8 bits : row, 24 bits) for i < count, INT64_MAX up
 *   to cap; stored as int64 with the top bit flipped, so that a SIGNED MIN all-reduce over keys[0 .. cap) (8 cap bytes; gloo
 *   and RCCL both have it) leaves on every rank the key of the global winner.  x / e are the operands the column pass was
 *   given (cosine: both normalised).  N <= VQHIP_SYNC_MAX_ROWS tokens per rank, rank < 256.
 * vqhip_cvq_pack_sync: vqhip_cvq_pack with payload row i = x[row] on the rank the reduced key names and -0.0f elsewhere
 *   (x + (-0) == x for every x), so the SUM all-reduce of the packed buffer delivers the winner's row bit for bit whatever
 *   the order of the sum; vqhip_cvq_apply is then called with world = 1 (no averaging: anchors.py:59-63).
 * Exchange per step: 8 cap + 4 (2K + 4 + cap D) bytes, against the reference's all-gather of world * N * (K + D) floats.
 * vqhip_allreduce_min_i64: the MIN on a vqhip_rccl_comm_init communicator, on the caller's stream (as vqhip_allreduce_packed). */
#define VQHIP_SYNC_MAX_ROWS (1 << 24)
int vqhip_cvq_col_keys(const void *x, int x_dtype, const float *e, const int32_t *rows, const int32_t *count, int64_t cap,
                       const int64_t *col_idx, int64_t N, int64_t K, int D, int metric, int rank, int64_t *keys, void *stream);
int vqhip_cvq_pack_sync(const int32_t *hist, int64_t numel, const void *x, int x_dtype, const int64_t *keys, const int32_t *count,
                        int64_t cap, int rank, int64_t K, int D, float *packed, void *stream);
int vqhip_allreduce_min_i64(int64_t *buf, int64_t n, void *comm, void *stream);
/* ---- ONE host call per training forward (round 5) -------------------------------------------------------------------------
 * The reference's training step runs the quantizer's forward as ~20 ATen calls; the entry points above
 * replace them one for one, which leaves an eager nn.Module step with ~10 host calls — at the reference's per-rank batches
 * (3 072-12 544 tokens) the HOST is then the bound.  The two entry points below enqueue a whole training forward from one
 * call: encode -> the codebook update of the callback, exchange included -> decode / straight-through / loss.  Every launch
 * is one the separate entry points would have made, in the same order on the same stream: the results are those of the
 * chain, bit for bit.  The argument block is a plain struct of pointers and sizes (struct_bytes = sizeof, checked).
 *
 * `phases`: VQHIP_STEP_ALL — everything, with the all-reduce issued by the library on `comm` (a vqhip_rccl_comm_init
 *   communicator) when `exchange` != 0; comm may be NULL only for world == 1 (a one-rank SUM is the identity).
 *   VQHIP_STEP_BEFORE_EXCHANGE / VQHIP_STEP_AFTER_EXCHANGE — the two halves around a collective the CALLER issues on
 *   packed[0 .. exchange_floats) (torch.distributed.all_reduce: the default route of the Python callbacks); the same struct,
 *   untouched, goes into both calls.
 * `exchange` == 0: one rank, no packed buffer (counts from the epilogue histogram).
 *
 * vqhip_cvq_forward — VQGANQuantizer + CVQVAECallback(NearestAnchor) in train mode (vq/algorithms/vq/quantizers.py:92-117,
 *   vq/algorithms/cvqvae/quantizer_callback.py:75-105, anchors.py:41-85; sparse anchors as vqhip_cvq_rows describes):
 *   vqhip_encode_ex(x, w_in; ZERO_HIST) -> [vqhip_cvq_rows(p_in) unless list_ready] -> vqhip_col_argmin_rows(cap) ->
 *   [vqhip_cvq_pack -> all-reduce] -> vqhip_cvq_apply(w_in, p_in -> w_out, p_out) -> [prefetch: vqhip_cvq_rows(p_out) into
 *   rows/slot/count for the NEXT step, count copied to the pinned HOST word count_host, count_event recorded] ->
 *   vqhip_gather_ste_mse(x, w_out, idx).
 *   cap >= 0: the capacity the listed-code launches are sized for (>= the count; K under HIP-graph capture).
 *   cap <  0: the call reads it from *count_host after hipEventSynchronize(count_event) — the copy the PREVIOUS call's
 *   prefetch queued a whole step earlier; the wait sits behind the enqueue of the encode, so the GPU has work while the host
 *   looks.  This is the ONE place a compute entry point of this library may block the host, and only on the caller's event.
 *   rows / slot / count: K, K, 1 int32, caller-owned and persistent across steps.  cap_used / exchange_floats: written by the
 *   BEFORE phase (host fields).  ws: vqhip_cvq_forward_ws_bytes(N, K, D, cap_max) with cap_max >= cap; packed: at least
 *   vqhip_pack_floats(K, cap, D) floats (exchange != 0).  xq: cosine only (as vqhip_encode).  z_ste / mse nullable together
 *   (no decode tail).  w_out / p_out may alias w_in / p_in.  early_word_host / early_seq_dev: see the struct.
 *   anchor_sync != 0 (with exchange != 0): NearestAnchor(sync=True) — BEFORE ends with vqhip_cvq_col_keys into `keys` instead
 *   of the pack; the caller MIN-all-reduces keys[0 .. cap_used) as int64, calls the VQHIP_STEP_PACK_SYNC phase
 *   (vqhip_cvq_pack_sync), SUM-all-reduces packed[0 .. exchange_floats) and calls AFTER (anchors not averaged).
 *   VQHIP_STEP_ALL does all of it on `comm` (vqhip_allreduce_min_i64 + vqhip_allreduce_packed).
 *
 * vqhip_vqkd_forward — VQKDQuantizer + VQKDCallback in train mode (vq/algorithms/vq/callbacks/normalize.py:22-29,
 *   vq/algorithms/vqkd/quantizers/callbacks.py:44-75,114-129, vq/algorithms/vq/losses.py:53-62 with mse norm=True):
 *   w_mid = normalize(normalize(w_in)), xn = normalize(x), payload zeroed (ONE launch) -> vqhip_encode_ex(xn, w_mid, cosine)
 *   -> histogram header + centroid sums of normalize(xn) scattered straight into the packed buffer (ONE launch; `ordered`
 *   != 0: vqhip_token_order + vqhip_segsum_rows instead, bit-reproducible) -> [all-reduce] -> the EMA update read straight
 *   from the packed buffer (w_mid -> w_out) -> tail (tail != 0): z_ste = xn + (w_out[idx] - xn), mse[0] = mse[1] =
 *   mean((normalize(w_out[idx]) - normalize(xn))^2), mse[2] = mse[3] = 0 — a double-precision sum of per-workgroup partials
 *   added in a fixed order (they are parked in the record area of `ws`, free by then): the same step gives the same bits.
 *   xq: the encode's by-product (as vqhip_encode).  packed: vqhip_pack_floats(K, K, D) floats, always used.
 *   At D <= 32 the front, the tail and the backward give a row 8 / 16 / 32 lanes instead of a wave (same values).
 *   metric: VQHIP_METRIC_COS or VQHIP_METRIC_COS_BF16.  ws: vqhip_vqkd_forward_ws_bytes(N, K, D).
 * vqhip_vqkd_backward — gradient of that tail with respect to x: grad_x = normalize_bwd(x; g_zste + normalize_bwd(xn;
 *   g_loss * 2/(N D) * (normalize(xn) - normalize(w[idx])))); g_zste [N, D] / g_loss (DEVICE scalar) nullable. */
#define VQHIP_STEP_BEFORE_EXCHANGE 1
#define VQHIP_STEP_AFTER_EXCHANGE 2
#define VQHIP_STEP_ALL 3
#define VQHIP_STEP_PACK_SYNC 4     /* anchor_sync only: between the caller's MIN all-reduce of the keys and its SUM all-reduce of packed */
typedef struct vqhip_cvq_forward_t {
    int64_t struct_bytes;
    int64_t N, K;
    int32_t D, x_dtype, metric, world;
    float ema_decay, eps, beta;
    int32_t phases, exchange, list_ready, prefetch;
    int32_t anchor_sync, rank;      /* NearestAnchor(sync=True) with exchange != 0: the key exchange of vqhip_cvq_col_keys; this rank's number */
    int64_t cap;
    const void *x;
    const float *w_in, *p_in;
    float *w_out, *p_out;
    int32_t *rows, *slot, *count;
    int32_t *count_host;            /* pinned HOST word (nullable) */
    void *count_event;              /* hipEvent_t of the caller (nullable) */
    void *comm;
    void *cb; int64_t cb_bytes;
    int64_t *idx; int32_t *hist; float *xq;
    float *packed; int64_t packed_floats;
    float *z_ste, *mse; void *scratch16;
    void *ws; int64_t ws_bytes;
    int64_t cap_used, exchange_floats;      /* OUT (host), written by the BEFORE phase */
    /* early count (nullable pair): as soon as this step's histogram is final (behind the encode at one rank, behind the exchange
     * otherwise) one small launch writes {sequence number << 32 | length of the NEXT step's list} to the pinned HOST word
     * early_word_host and advances the DEVICE counter early_seq_dev by one — for a caller that replays this call from a HIP graph
     * and must choose the next replay's capacity without an event in the middle of the graph (it polls the word) */
    unsigned long long *early_word_host;
    int32_t *early_seq_dev;
    int64_t *keys;                  /* anchor_sync: cap int64 (DEVICE), MIN-all-reduced between BEFORE and PACK_SYNC */
} vqhip_cvq_forward_t;
int64_t vqhip_cvq_forward_ws_bytes(int64_t N, int64_t K, int D, int64_t cap_max);
int vqhip_cvq_forward(vqhip_cvq_forward_t *args, void *stream);

typedef struct vqhip_vqkd_forward_t {
    int64_t struct_bytes;
    int64_t N, K;
    int32_t D, x_dtype, metric, world;
    float ema_decay;
    int32_t phases, exchange, ordered, tail, reserved0;
    const void *x;
    const float *w_in;
    float *w_mid, *w_out;           /* w_out may alias w_mid */
    float *xn, *xq;                 /* [N, D] fp32 each */
    void *comm;
    void *cb; int64_t cb_bytes;
    int64_t *idx; int32_t *hist;
    float *packed; int64_t packed_floats;
    float *z_ste, *mse; void *scratch16;
    void *ws; int64_t ws_bytes;
    int64_t exchange_floats;        /* OUT (host), written by the BEFORE phase */
} vqhip_vqkd_forward_t;
int64_t vqhip_vqkd_forward_ws_bytes(int64_t N, int64_t K, int D);
int vqhip_vqkd_forward(vqhip_vqkd_forward_t *args, void *stream);
int vqhip_vqkd_backward(const void *x, int x_dtype, const float *xn, const float *w, const int64_t *idx, int64_t N, int D,
                        const float *g_zste, const float *g_loss, float *grad_x, void *stream);

/* vqhip_vq_forward — the forward of a quantizer WITHOUT an update callback, or with NormalizeCallback alone (the LlamaGen
 * tokenizer, configs/llamagen/vqgan.py:18-20), as one host call (vq/algorithms/vq/quantizers.py:92-117, callbacks/normalize.py:22-29,
 * losses.py:41-127): [w_out = normalize(w_in) and xn = normalize(x): ONE launch] -> vqhip_encode_ex(xn | x, w_out | w_in) ->
 * vqhip_gather_ste_mse on the same operands.  normalize != 0: both normalisations (w_out [K, D] and xn [N, D] fp32 are written; w_out
 * may alias w_in); normalize == 0: w_out / xn unused.  hist nullable; xq: cosine only; z_ste / mse nullable together.
 * ws: vqhip_workspace_bytes(N, K, D). */
typedef struct vqhip_vq_forward_t {
    int64_t struct_bytes;
    int64_t N, K;
    int32_t D, x_dtype, metric, normalize;
    float beta;
    int32_t reserved0;
    const void *x;
    const float *w_in;
    float *w_out, *xn;
    void *cb; int64_t cb_bytes;
    int64_t *idx; int32_t *hist; float *xq;
    float *z_ste, *mse; void *scratch16;
    void *ws; int64_t ws_bytes;
} vqhip_vq_forward_t;
int vqhip_vq_forward(vqhip_vq_forward_t *args, void *stream);

/* anchors[k] = x[col_idx[k]] (anchors.py:84) as fp32 */
int vqhip_gather_rows(const void *x, int x_dtype, const int64_t *row_idx, int64_t K, int D, float *out,
                      void *stream);

/* ---- elementwise pieces of the backward / unfused path ------------------------------------------------
 * vqhip_diff: sse[0] += sum (a-b)^2 in double (MSELoss forward, losses.py:50,62) and/or out = (a-b)*scale
 *             (its backward); a, b may each be fp32 or bf16; out / sse nullable (not both).
 * vqhip_ste:  out = x + (z - x)                                      (utils/ste.py:10)
 * vqhip_normalize_rows_bwd: gradient of F.normalize(v, dim=1, eps) given the output gradient g. */
int vqhip_diff(const void *a, int a_dtype, const void *b, int b_dtype, int64_t n, float scale,
               const float *scale_dev /* nullable DEVICE scalar multiplied into scale */, float *out, double *sse,
               void *stream);
/* Fused backward of the quantizer forward (embedding_dense_backward + both MSE gradients + STE):
 *   z = W[idx], z_ste = x + sg(z - x), m_cb = mse(z, sg x) (losses.py:50), m_cm = mse(sg z, x) (losses.py:62)
 *   grad_x = g_zste + g_cm*(2/ND)*(x - z);   grad_w[idx] += g_cb*(2/ND)*(z - x)  (fp32 atomics)
 * g_cb, g_cm: DEVICE scalars (upstream gradients of the two MSE values, nullable = 0); g_zste, grad_x, grad_w
 * nullable (grad_w must be zero-initialised by the caller). */
int vqhip_vq_backward(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D,
                      const float *g_zste, const float *g_cb, const float *g_cm, float *grad_x, float *grad_w,
                      void *stream);
/* ... with the upstream gradient g_comb (nullable DEVICE scalar) of the combined value mse[2] = m_cb + beta*m_cm of
 * vqhip_gather_ste_mse: the effective gradients are g_cb + g_comb and g_cm + beta*g_comb (no scalar kernels in between). */
int vqhip_vq_backward_ex(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D,
                         const float *g_zste, const float *g_cb, const float *g_cm, const float *g_comb, float beta,
                         float *grad_x, float *grad_w, void *stream);
/* grad_x of vqhip_vq_backward_ex for a quantizer call on the NCHW feature map (vq/tasks/image_tokenization/models/base.py:116-128),
 * with both rearrangements folded in: g_map [B, D, HW] fp32 is the upstream gradient of the straight-through output AS the map it
 * arrives in (nullable = 0), grad_map [B, D, HW] receives the gradient of the latents as the map the encoder's backward consumes,
 * in grad_dtype (VQHIP_DTYPE_F32 / _BF16: the map's own dtype; bf16 rounds to nearest even):
 *   grad_map[b, d, p] = g_map[b, d, p] + (g_cm + beta*g_comb) * 2/(N D) * (x_rows[n][d] - e[idx[n]][d]),  n = b*HW + p.
 * No transpose launch and no cast around it.  HW % 256 == 0 and D % 32 == 0 (16 x 16 and larger power-of-two maps; other shapes:
 * vqhip_transpose + vqhip_vq_backward_ex).  The codebook gradient is formed by vqhip_vq_backward_ex with grad_x = NULL (or the
 * ordered route). */
int vqhip_vq_backward_map(const void *x_rows, int x_dtype, const float *e, const int64_t *idx, int64_t B, int64_t HW, int D,
                          const float *g_map, const float *g_cm, const float *g_comb, float beta, void *grad_map, int grad_dtype,
                          void *stream);
int vqhip_ste(const void *x, int x_dtype, const float *z, int64_t n, float *out, void *stream);
int vqhip_normalize_rows_bwd(const void *v, int dtype, const float *g, int64_t R, int D, float eps, float *gv,
                             void *stream);

/* ---- deterministic (ordered) codebook-side sums  (SURVEY.md §7 hard part 9) ---------------------------------------
 * vqhip_scatter_add_rows and the grad_w leg of vqhip_vq_backward add with floating-point atomics, i.e. in arrival
 * order.  The ordered route fixes the order instead: vqhip_token_order sorts the token ids by code (stable counting
 * sort, integer arithmetic only): counts[K] = bincount, offsets[K+1] = its exclusive scan, order[N] = token ids, code
 * by code, ascending within a code.  K <= 32768.  `ws` = vqhip_order_workspace_bytes(N, K).
 * Sums: the sorted order is cut into ranges of 64 positions; rows are added in order inside a range; a code whose
 * tokens span several ranges is the sum of its range pieces in range order — an association fixed by the counts alone.
 * vqhip_segsum_rows: dst[k] = that sum of src[order[p]], p in [offsets[k], offsets[k+1]) (all K rows are written, zero
 * for unused codes) — the centroid sums of callbacks.py:60-64.  vqhip_vq_backward_w_ordered: grad_w[k] = the same sum
 * of g_cb * 2/(N*D) * (e_k - x_n) — the codebook gradient of vqhip_vq_backward (call that one with grad_w = NULL).
 * `ws` of the two sums = vqhip_segsum_workspace_bytes(N, D). */
int64_t vqhip_order_workspace_bytes(int64_t N, int64_t K);
int64_t vqhip_segsum_workspace_bytes(int64_t N, int D);
int vqhip_token_order(const int64_t *idx, int64_t N, int64_t K, int32_t *counts, int32_t *offsets, int32_t *order, void *ws,
                      int64_t ws_bytes, void *stream);
int vqhip_segsum_rows(const float *src, const int64_t *idx, const int32_t *order, const int32_t *offsets, int64_t N, int64_t K,
                      int D, float *dst, void *ws, int64_t ws_bytes, void *stream);
int vqhip_vq_backward_w_ordered(const void *x, int x_dtype, const float *e, const int64_t *idx, const int32_t *order,
                                const int32_t *offsets, int64_t N, int64_t K, int D, const float *g_cb, float *grad_w, void *ws,
                                int64_t ws_bytes, void *stream);

/* ---- callers either side of the path ------------------------------------------------------
 * vqhip_transpose: in[B][R][C] -> out[B][C][R] for 2- or 4-byte elements.  With R = channels, C = h*w it is
 *   'b c h w -> (b h w) c' (vq/tasks/image_tokenization/models/base.py:124,140); with R = h*w, C = channels the
 *   inverse '(b h w) c -> b c h w' (base.py:126).
 * vqhip_codebook_metrics: out[0] = nonzero(counts)/K (CodebookUsageMetric, runners/metrics.py:58-62),
 *   out[1] = entropy of counts/sum(counts) in nats (CodebookPPLMetric, :65-73); counts int64[K], out double[2]. */
int vqhip_transpose(const void *in, void *out, int elem_bytes, int64_t B, int R, int C, void *stream);
int vqhip_codebook_metrics(const int64_t *counts, int64_t K, double *out, void *stream);

/* ---- diagnostics ------------------------------------------------------------------------------------
 * Copies the counters of the last vqhip_argmin on `ws` to out[4] (DEVICE int32): rows given a second proposal
 * pass, rows with more than one identified candidate (re-ranked exactly), rows sent to the whole-codebook fp32
 * pass, reserved. */
int vqhip_argmin_stats(const void *ws, int32_t *out, void *stream);

/* Verification aid: scores[N*K] = the fp16-MFMA proposal score of every (row, code) pair (same operands and
 * instruction sequence as the production kernels), margin[N] = the per-row margin the decision step uses (scaled
 * score units, negative = no usable bound), scale[1] = the power-of-two codebook scale.  A test checks the error
 * bound |score - exact score| <= margin/2 against float64. */
int vqhip_debug_proposal_scores(const void *x, int x_dtype, const void *cb, int64_t N, int64_t K, int D, int metric,
                                float *scores, float *margin, float *scale, void *ws, int64_t ws_bytes, void *stream);

/* Per-launch timing of the proposal (distance+argmin) kernel with HIP events recorded on the caller's stream
 * around that launch (bench.py's roofline leg).  enable(1) starts collecting, collect() synchronises on the
 * recorded events, returns the summed kernel milliseconds and launch count (HOST pointers) and resets. */
int vqhip_profile_enable(int on);
/* Verification aids (results never change; process-wide host state): key 2 = number of codebook slices of the proposal
 * pass (1,2,4,8,16; 0 = automatic); key 18 = the streamed form of the whole-batch fp32 pass (vqhip_argmin_exact,
 * vqhip_distance, the column fallback: exact_stream_kernel) where D % 4 == 0 (bf16 rows: D % 8 == 0) (1, default; 0 = the
 * register form, which D % 4 != 0 takes anyway).  Key 12: value V > 0 sends rows 0 .. min(V, N, 1024) - 1 of every
 * vqhip_argmin batch through the last-resort whole-codebook fp32 pass as well (its indices replace the ones the earlier stages
 * wrote — the same ones; a histogram requested from the call counts those rows twice); 0 = off (default).
 * Any other key: VQHIP_EINVAL. */
int vqhip_set_tuning(int key, int value);
int vqhip_profile_collect(double *ms_sum, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* VQHIP_H_ */
