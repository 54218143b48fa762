// libvqhip — what the translation units of the quantizer core share on the host side (vqhip.hip, vqhip_exact.hip,
// vqhip_decode.hip, vqhip_fsq.hip, vqhip_update.hip, vqhip_step.hip).  A helper that is used on both sides of a cut is defined
// once, in the unit that owns the kernels it launches, and declared here; like fail and ensure_dyn_lds (vqhip_host.h) these
// cross translation units inside the library only (hidden visibility).  A unit that needs a kernel of another unit's header
// calls the owner's function below: a header with a non-template kernel is included by one unit alone
// (tests/test_build_units_cpu.py).
#pragma once
#include "vqhip_host.h"
#include "vqhip_kernels.h"

// rows of at most 32 elements take L = 8, 16 or 32 lanes each: 64 / L rows per wave
static inline int vq_small_lanes(int D) { return D <= 8 ? 8 : (D <= 16 ? 16 : 32); }

// The column pass, roles swapped: the codebook rows are the "rows", the N latents are the "codes"; the same proposal + exact
// re-rank pipeline then returns for every code its nearest latent.  Its metric word: the exact finishing keeps the reference's
// operand order, (chain + |x_n|^2) + |e_k|^2 = (chain + code norm) + row norm (VQ_METRIC_SWAP); cosine uses the operands as
// given (both normalised by the caller): VQ_METRIC_DOT.
static inline int vq_swapped_metric(int metric) {
    return (metric == VQHIP_METRIC_L2) ? (VQHIP_METRIC_L2 | VQ_METRIC_SWAP) : (VQ_METRIC_DOT | (metric & VQ_METRIC_BF16));
}

// ---- vqhip.hip -------------------------------------------------------------------------------------------------------
// vqhip_set_tuning key 18, for the one reader outside its unit: 0 = the whole-batch fp32 pass keeps its register form
VQ_HIDDEN int vq_tune_stream();
// The launch of exact_stream_kernel<bf, MODE> (vqhip_stream_kernels.h), on behalf of run_exact_tiled<MODE> in vqhip_exact.hip.
// It is compiled here because its dynamic LDS array carries the name `lds`, as the proposal kernels' does: the block-scope
// declarations of one translation unit name ONE array, whose alignment is that of the first kernel emitted — 16 bytes next to
// the proposal kernels, the kernel's own 128 in a unit of its own, where the compiler then allocates its registers differently.
template <int MODE>
VQ_HIDDEN int run_exact_stream(const void *x, int bf, const float *e, const float *en, const float *xn, int64_t N, int64_t K, int D,
                               int metric, u64 *keys, float *dout, int64_t items, hipStream_t s);

// ---- vqhip_exact.hip (vqhip_exact_kernels.h, vqhip_stream_kernels.h) ------------------------------------------------------
// last resort of the proposal pipeline: the listed rows against the whole codebook
VQ_HIDDEN int run_exact_rows(const void *x, int x_dtype, const float *e, const float *en, const float *xn, int64_t N, int64_t K, int D,
                             int metric, const int *row_list, const int *nrows_dev, u64 *keys, int *ticket, int64_t *idx,
                             int32_t *hist, hipStream_t s);
// vqhip_set_tuning key 12: the first `nforce` rows of a batch join that list (force_exact_rows_kernel)
VQ_HIDDEN int force_exact_rows(int nforce, int *exact_list, int *counters, u64 *keys, hipStream_t s);
// vqhip_col_argmin where D has no proposal image: the whole-batch fp32 pass with one key per code
VQ_HIDDEN int exact_whole_cols(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, const VqWsView &V,
                               int64_t *col_idx, hipStream_t s);
// the column pass over a short list, directly in fp32 (vqhip_col_argmin_rows, where col_direct_ok)
VQ_HIDDEN int col_rows_direct(const void *x, const float *e, const int32_t *rows, const int32_t *count, int64_t cap, int64_t N,
                              int64_t K, int D, int metric, int64_t *col_idx, char *ws, const float *tok_norm, const float *row_norm,
                              hipStream_t s);

// ---- vqhip_update.hip (vqhip_update_kernels.h, vqhip_exchange_kernels.h, vqhip_sort_kernels.h) -----------------------------
// what vqhip_cvq_forward launches of the exchange kernels itself: the next step's list with its length also stored to the
// caller's pinned host word (cvq_rows_kernel), and the early count of that list (cvq_count_next_kernel<PACKED>)
VQ_HIDDEN int cvq_rows_prefetch(const float *p, int64_t K, float ema_decay, float eps, int32_t *rows, int32_t *slot, int32_t *count,
                                int32_t *count_host, hipStream_t s);
VQ_HIDDEN int cvq_count_next(bool packed_form, const float *p_in, const int32_t *hist, int64_t numel, const float *packed, int64_t K,
                             float ema_decay, float eps, int32_t *seq_dev, unsigned long long *word_host, hipStream_t s);
