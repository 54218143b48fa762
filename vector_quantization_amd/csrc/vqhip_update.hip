// libvqhip — codebook updates: scatter / gather of rows, the VQ-KD and CVQ-VAE EMA updates, the packed exchange buffer and the
// sync-anchor keys, and the deterministic (ordered) codebook-side sums.  gfx950 only.
// Kernels: vqhip_update_kernels.h, vqhip_exchange_kernels.h, vqhip_sort_kernels.h.
#include "vqhip.h"

#include <hip/hip_runtime.h>

#include "vqhip_core.h"
#include "vqhip_update_kernels.h"
#include "vqhip_sort_kernels.h"
#include "vqhip_exchange_kernels.h"

template <int MODE>
static int run_segsum(const void *src, int x_dtype, const float *e, const int64_t *idx, const int32_t *order,
                      const int32_t *offsets, int64_t N, int64_t K, int D, const float *g_cb, float *dst, void *ws,
                      hipStream_t s) {
    float *partial = (float *)ws;
    const int64_t nranges = (N + VQ_SEG_RANGE - 1) / VQ_SEG_RANGE;
    int grid = (int)((nranges + 3) / 4); grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);
    if (x_dtype == VQHIP_DTYPE_F32) segsum_rows_kernel<MODE, 0><<<grid, 256, 0, s>>>(src, e, idx, order, offsets, N, (int)K, D, g_cb, dst, partial);
    else segsum_rows_kernel<MODE, 1><<<grid, 256, 0, s>>>(src, e, idx, order, offsets, N, (int)K, D, g_cb, dst, partial);
    VQ_CHECK_LAUNCH("segsum_rows_kernel");
    int fgrid = (int)((K + 3) / 4); fgrid = fgrid > 2048 ? 2048 : fgrid;
    segsum_fixup_kernel<<<fgrid, 256, 0, s>>>(offsets, (int)K, D, partial, dst);
    VQ_CHECK_LAUNCH("segsum_fixup_kernel");
    return VQHIP_OK;
}

int cvq_rows_prefetch(const float *p, int64_t K, float ema_decay, float eps, int32_t *rows, int32_t *slot, int32_t *count,
                      int32_t *count_host, hipStream_t s) {
    cvq_rows_kernel<<<1, 1024, 0, s>>>(p, K, ema_decay, eps, rows, slot, count, count_host);
    VQ_CHECK_LAUNCH("cvq_rows_kernel");
    return VQHIP_OK;
}

int cvq_count_next(bool packed_form, const float *p_in, const int32_t *hist, int64_t numel, const float *packed, int64_t K,
                   float ema_decay, float eps, int32_t *seq_dev, unsigned long long *word_host, hipStream_t s) {
    if (packed_form) cvq_count_next_kernel<true><<<1, 1024, 0, s>>>(p_in, hist, numel, packed, K, ema_decay, eps, seq_dev, word_host);
    else cvq_count_next_kernel<false><<<1, 1024, 0, s>>>(p_in, hist, numel, packed, K, ema_decay, eps, seq_dev, word_host);
    VQ_CHECK_LAUNCH("cvq_count_next_kernel");
    return VQHIP_OK;
}

extern "C" {

int vqhip_scatter_add_rows(const float *src, const int64_t *idx, int64_t N, int64_t K, int D, float *dst, void *stream) {
    if (!src || !idx || !dst || N < 0 || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_scatter_add_rows: bad argument");
    if (N == 0) return VQHIP_OK;
    scatter_add_rows_kernel<<<waves_grid(N, 4), 256, 0, (hipStream_t)stream>>>(src, idx, N, K, D, dst);
    VQ_CHECK_LAUNCH("scatter_add_rows_kernel");
    return VQHIP_OK;
}

int vqhip_gather_rows(const void *x, int x_dtype, const int64_t *row_idx, int64_t K, int D, float *out, void *stream) {
    if (!x || !row_idx || !out || K < 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_gather_rows: bad argument");
    if (K == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (x_dtype == VQHIP_DTYPE_F32) gather_rows_kernel<0><<<waves_grid(K, 4), 256, 0, s>>>(x, row_idx, K, D, out);
    else if (x_dtype == VQHIP_DTYPE_BF16) gather_rows_kernel<1><<<waves_grid(K, 4), 256, 0, s>>>(x, row_idx, K, D, out);
    else return fail(VQHIP_EINVAL, "vqhip_gather_rows: x_dtype");
    VQ_CHECK_LAUNCH("gather_rows_kernel");
    return VQHIP_OK;
}

int vqhip_vqkd_update(float *w, const int64_t *hist, const float *sums, int64_t K, int D, float decay, int centroid_only,
                      void *stream) {
    if (!w || !hist || !sums || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_vqkd_update: bad argument");
    vqkd_update_kernel<<<waves_grid(K, 4), 256, 0, (hipStream_t)stream>>>(w, hist, sums, K, D, decay, centroid_only);
    VQ_CHECK_LAUNCH("vqkd_update_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_update(float *w, float *p, const int64_t *hist, int64_t numel, const int64_t *numel_dev, const float *anchors,
                     int64_t K, int D, float ema_decay, float eps, int stage, void *stream) {
    if (!w || !p || K <= 0 || D <= 0 || stage < 1 || stage > 3 || ((stage & 1) && (!hist || (numel <= 0 && !numel_dev))) ||
        ((stage & 2) && !anchors)) return fail(VQHIP_EINVAL, "vqhip_cvq_update: bad argument");
    cvq_update_kernel<<<waves_grid(K, 4), 256, 0, (hipStream_t)stream>>>(w, p, hist, numel, numel_dev, anchors, K, D, ema_decay, eps, stage);
    VQ_CHECK_LAUNCH("cvq_update_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_step(const float *w_in, float *w_out, const float *p_in, float *p_out, const int32_t *hist, int64_t numel,
                   const void *x, int x_dtype, const int64_t *col_idx, int64_t K, int D, float ema_decay, float eps,
                   void *stream) {
    if (!w_in || !w_out || !p_in || !p_out || !hist || !x || !col_idx || K <= 0 || D <= 0 || numel <= 0)
        return fail(VQHIP_EINVAL, "vqhip_cvq_step: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (x_dtype == VQHIP_DTYPE_F32) cvq_step_kernel<0><<<waves_grid(K, 4), 256, 0, s>>>(w_in, w_out, p_in, p_out, hist, numel, x, col_idx, K, D, ema_decay, eps);
    else if (x_dtype == VQHIP_DTYPE_BF16) cvq_step_kernel<1><<<waves_grid(K, 4), 256, 0, s>>>(w_in, w_out, p_in, p_out, hist, numel, x, col_idx, K, D, ema_decay, eps);
    else return fail(VQHIP_EINVAL, "vqhip_cvq_step: x_dtype");
    VQ_CHECK_LAUNCH("cvq_step_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_decay(const float *p, int64_t K, float ema_decay, float eps, float *decay, void *stream) {
    if (!p || !decay || K <= 0) return fail(VQHIP_EINVAL, "vqhip_cvq_decay: bad argument");
    cvq_decay_kernel<<<(int)((K + 255) / 256), 256, 0, (hipStream_t)stream>>>(p, K, ema_decay, eps, decay);
    VQ_CHECK_LAUNCH("cvq_decay_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_update_rows(float *w, const float *p, const int64_t *rows, const float *anchors_sub, int64_t M, int64_t K, int D,
                          float ema_decay, float eps, void *stream) {
    if (!w || !p || K <= 0 || D <= 0 || M < 0 || (M > 0 && (!rows || !anchors_sub)))
        return fail(VQHIP_EINVAL, "vqhip_cvq_update_rows: bad argument");
    if (M == 0) return VQHIP_OK;
    cvq_update_rows_kernel<<<waves_grid(M, 4), 256, 0, (hipStream_t)stream>>>(w, p, rows, anchors_sub, M, K, D, ema_decay, eps);
    VQ_CHECK_LAUNCH("cvq_update_rows_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_rows(const float *p, int64_t K, float ema_decay, float eps, int32_t *rows, int32_t *slot, int32_t *count,
                   void *stream) {
    if (!p || !rows || !slot || !count || K <= 0 || K >= (1ll << 31)) return fail(VQHIP_EINVAL, "vqhip_cvq_rows: bad argument");
    cvq_rows_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(p, K, ema_decay, eps, rows, slot, count);
    VQ_CHECK_LAUNCH("cvq_rows_kernel");
    return VQHIP_OK;
}

int64_t vqhip_pack_floats(int64_t K, int64_t M, int D) {
    if (K <= 0 || M < 0 || D <= 0) return 0;
    return VQ_PACK_HEADER(K) + M * (int64_t)D;
}

int vqhip_pack_counts(const void *hist, int hist_is_int64, int64_t numel, int64_t K, float *packed, void *stream) {
    if (!hist || !packed || K <= 0 || numel < 0) return fail(VQHIP_EINVAL, "vqhip_pack_counts: bad argument");
    const int grid = (int)((K + 255) / 256);
    if (hist_is_int64) pack_counts_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(hist, numel, K, packed);
    else pack_counts_kernel<0><<<grid, 256, 0, (hipStream_t)stream>>>(hist, numel, K, packed);
    VQ_CHECK_LAUNCH("pack_counts_kernel");
    return VQHIP_OK;
}

int vqhip_unpack_counts(const float *packed, int64_t K, int64_t *out, void *stream) {
    if (!packed || !out || K <= 0) return fail(VQHIP_EINVAL, "vqhip_unpack_counts: bad argument");
    unpack_counts_kernel<<<(int)((K + 255) / 256), 256, 0, (hipStream_t)stream>>>(packed, K, out);
    VQ_CHECK_LAUNCH("unpack_counts_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_pack(const int32_t *hist, int64_t numel, const void *x, int x_dtype, const int64_t *col_idx, const int32_t *count,
                   int64_t cap, int64_t K, int D, float *packed, void *stream) {
    if (!hist || !packed || K <= 0 || D <= 0 || numel <= 0 || cap < 0 || cap > K || (cap > 0 && (!x || !col_idx || !count)))
        return fail(VQHIP_EINVAL, "vqhip_cvq_pack: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int hb = (int)((K + 255) / 256);
    const int grid = hb + waves_grid(cap, 4);
    if (x_dtype == VQHIP_DTYPE_BF16) cvq_pack_kernel<1><<<grid, 256, 0, s>>>(hist, numel, x, col_idx, count, cap, K, D, packed, hb);
    else if (x_dtype == VQHIP_DTYPE_F32) cvq_pack_kernel<0><<<grid, 256, 0, s>>>(hist, numel, x, col_idx, count, cap, K, D, packed, hb);
    else return fail(VQHIP_EINVAL, "vqhip_cvq_pack: x_dtype");
    VQ_CHECK_LAUNCH("cvq_pack_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_apply(const float *w_in, float *w_out, const float *p_in, float *p_out, const int32_t *hist, int64_t numel,
                    const void *x, int x_dtype, const int64_t *col_idx, const float *packed, int world, const int32_t *slot,
                    int64_t cap, int64_t K, int D, float ema_decay, float eps, void *stream) {
    if (!w_in || !w_out || !p_in || !p_out || !slot || K <= 0 || D <= 0 || cap < 0 || cap > K) return fail(VQHIP_EINVAL, "vqhip_cvq_apply: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (packed != nullptr) {
        if (world < 1 || world > VQ_PACK_MAX_WORLD) return fail(VQHIP_EINVAL, "vqhip_cvq_apply: world must be in [1, 256] (exact fp32 count sums)");
        cvq_apply_kernel<0, true><<<waves_grid(K, 4), 256, 0, s>>>(w_in, w_out, p_in, p_out, nullptr, 0, nullptr, nullptr, packed, world, slot, (int)cap, K, D, ema_decay, eps);
    } else {
        if (!hist || numel <= 0) return fail(VQHIP_EINVAL, "vqhip_cvq_apply: the one-rank form needs hist and numel");   // (x, col_idx: read for listed codes only)
        if (x_dtype == VQHIP_DTYPE_F32) cvq_apply_kernel<0, false><<<waves_grid(K, 4), 256, 0, s>>>(w_in, w_out, p_in, p_out, hist, numel, x, col_idx, nullptr, 1, slot, (int)cap, K, D, ema_decay, eps);
        else if (x_dtype == VQHIP_DTYPE_BF16) cvq_apply_kernel<1, false><<<waves_grid(K, 4), 256, 0, s>>>(w_in, w_out, p_in, p_out, hist, numel, x, col_idx, nullptr, 1, slot, (int)cap, K, D, ema_decay, eps);
        else return fail(VQHIP_EINVAL, "vqhip_cvq_apply: x_dtype");
    }
    VQ_CHECK_LAUNCH("cvq_apply_kernel");
    return VQHIP_OK;
}

// ---- NearestAnchor(sync=True) across ranks: keys of the local winners, the masked pack (include/vqhip.h) ---------------
int vqhip_cvq_col_keys(const void *x, int x_dtype, const float *e, const int32_t *rows, const int32_t *count, int64_t cap,
                       const int64_t *col_idx, int64_t N, int64_t K, int D, int metric, int rank, int64_t *keys, void *stream) {
    if (!x || !e || !rows || !count || !col_idx || !keys || N <= 0 || K <= 0 || D <= 0 || cap < 0 || cap > K)
        return fail(VQHIP_EINVAL, "vqhip_cvq_col_keys: bad argument");
    if (N > VQHIP_SYNC_MAX_ROWS || rank < 0 || rank >= VQ_PACK_MAX_WORLD)
        return fail(VQHIP_EINVAL, "vqhip_cvq_col_keys: a key holds 24 bits of row and 8 bits of rank (N <= 2^24, rank < 256)");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_cvq_col_keys: metric");
    if (cap == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)((cap + 63) / 64);
    if (x_dtype == VQHIP_DTYPE_F32) cvq_col_keys_kernel<0><<<grid, 64, 0, s>>>(x, e, rows, count, cap, col_idx, D, metric, rank, keys);
    else if (x_dtype == VQHIP_DTYPE_BF16) cvq_col_keys_kernel<1><<<grid, 64, 0, s>>>(x, e, rows, count, cap, col_idx, D, metric, rank, keys);
    else return fail(VQHIP_EINVAL, "vqhip_cvq_col_keys: x_dtype");
    VQ_CHECK_LAUNCH("cvq_col_keys_kernel");
    return VQHIP_OK;
}

int vqhip_cvq_pack_sync(const int32_t *hist, int64_t numel, const void *x, int x_dtype, const int64_t *keys, const int32_t *count,
                        int64_t cap, int rank, int64_t K, int D, float *packed, void *stream) {
    if (!hist || !packed || K <= 0 || D <= 0 || numel <= 0 || cap < 0 || cap > K || rank < 0 || rank >= VQ_PACK_MAX_WORLD ||
        (cap > 0 && (!x || !keys || !count)))
        return fail(VQHIP_EINVAL, "vqhip_cvq_pack_sync: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int hb = (int)((K + 255) / 256);
    const int grid = hb + waves_grid(cap, 4);
    if (x_dtype == VQHIP_DTYPE_BF16) cvq_pack_sync_kernel<1><<<grid, 256, 0, s>>>(hist, numel, x, keys, count, cap, rank, K, D, packed, hb);
    else if (x_dtype == VQHIP_DTYPE_F32) cvq_pack_sync_kernel<0><<<grid, 256, 0, s>>>(hist, numel, x, keys, count, cap, rank, K, D, packed, hb);
    else return fail(VQHIP_EINVAL, "vqhip_cvq_pack_sync: x_dtype");
    VQ_CHECK_LAUNCH("cvq_pack_sync_kernel");
    return VQHIP_OK;
}

// ---- deterministic (ordered) codebook-side sums -----------------------------------------------------------------
int64_t vqhip_order_workspace_bytes(int64_t N, int64_t K) {
    if (N < 0 || K <= 0) return 0;
    const int64_t nchunks = (N + VQ_SORT_CHUNK - 1) / VQ_SORT_CHUNK;
    return (nchunks > 0 ? nchunks : 1) * K * 4;
}

int vqhip_token_order(const int64_t *idx, int64_t N, int64_t K, int32_t *counts, int32_t *offsets, int32_t *order, void *ws,
                      int64_t ws_bytes, void *stream) {
    if (!idx || !counts || !offsets || !order || !ws || N < 0 || K <= 0) return fail(VQHIP_EINVAL, "vqhip_token_order: bad argument");
    VQ_NEED("vqhip_token_order: ws too small", ws_bytes, vqhip_order_workspace_bytes(N, K));
    if (K > 32768) return fail(VQHIP_EINVAL, "vqhip_token_order: K > 32768 (per-chunk histogram must fit in LDS)");
    if (N >= (1ll << 31)) return fail(VQHIP_EINVAL, "vqhip_token_order: N too large");
    const int64_t nchunks = (N + VQ_SORT_CHUNK - 1) / VQ_SORT_CHUNK;
    if (nchunks * K >= (1ll << 31)) return fail(VQHIP_EINVAL, "vqhip_token_order: N*K too large for the ordered route");
    hipStream_t s = (hipStream_t)stream;
    int *blockhist = (int *)ws;
    const size_t lds = (size_t)K * 4;
    static LdsCache lds_set;
    if (int rc = ensure_dyn_lds((const void *)sort_hist_kernel, lds, lds_set)) return rc;
    if (nchunks > 0) {
        sort_hist_kernel<<<(int)nchunks, VQ_SORT_CHUNK, lds, s>>>(idx, N, (int)K, blockhist);
        VQ_CHECK_LAUNCH("sort_hist_kernel");
    }
    sort_colscan_kernel<<<(int)((K + 255) / 256), 256, 0, s>>>(blockhist, (int)nchunks, (int)K, counts);
    VQ_CHECK_LAUNCH("sort_colscan_kernel");
    sort_offsets_kernel<<<1, 1024, 0, s>>>(counts, (int)K, offsets);
    VQ_CHECK_LAUNCH("sort_offsets_kernel");
    if (nchunks > 0) {
        sort_place_kernel<<<(int)nchunks, VQ_SORT_CHUNK, 0, s>>>(idx, N, (int)K, blockhist, offsets, order);
        VQ_CHECK_LAUNCH("sort_place_kernel");
    }
    return VQHIP_OK;
}

int64_t vqhip_segsum_workspace_bytes(int64_t N, int D) {
    if (N < 0 || D <= 0) return 0;
    return ((N + VQ_SEG_RANGE - 1) / VQ_SEG_RANGE + 1) * 2 * (int64_t)D * 4;
}

int vqhip_segsum_rows(const float *src, const int64_t *idx, const int32_t *order, const int32_t *offsets, int64_t N, int64_t K,
                      int D, float *dst, void *ws, int64_t ws_bytes, void *stream) {
    if (!src || !idx || !order || !offsets || !dst || !ws || N < 0 || K <= 0 || D <= 0 || (D % 4) != 0)
        return fail(VQHIP_EINVAL, "vqhip_segsum_rows: bad argument (D must be a multiple of 4)");
    VQ_NEED("vqhip_segsum_rows: ws too small", ws_bytes, vqhip_segsum_workspace_bytes(N, D));
    return run_segsum<0>(src, VQHIP_DTYPE_F32, nullptr, idx, order, offsets, N, K, D, nullptr, dst, ws, (hipStream_t)stream);
}

int vqhip_vq_backward_w_ordered(const void *x, int x_dtype, const float *e, const int64_t *idx, const int32_t *order,
                                const int32_t *offsets, int64_t N, int64_t K, int D, const float *g_cb, float *grad_w, void *ws,
                                int64_t ws_bytes, void *stream) {
    if (!x || !e || !idx || !order || !offsets || !grad_w || !ws || N < 0 || K <= 0 || D <= 0 || (D % 4) != 0)
        return fail(VQHIP_EINVAL, "vqhip_vq_backward_w_ordered: bad argument (D must be a multiple of 4)");
    VQ_NEED("vqhip_vq_backward_w_ordered: ws too small", ws_bytes, vqhip_segsum_workspace_bytes(N, D));
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_vq_backward_w_ordered: x_dtype");
    return run_segsum<1>(x, x_dtype, e, idx, order, offsets, N, K, D, g_cb, grad_w, ws, (hipStream_t)stream);
}

}  // extern "C"
