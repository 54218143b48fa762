// libvqhip — one host call per training forward (vqhip_cvq_forward, vqhip_vqkd_forward, vqhip_vq_forward) and the backwards of
// the VQ-KD tail and of the NCHW map, whose kernels live with the forwards'.  gfx950 only.  The forwards reach the rest of the
// core through its public entry points (vqhip_encode_ex, vqhip_col_argmin_rows, vqhip_cvq_apply, vqhip_gather_ste_mse, ...)
// and the two launches vqhip_core.h declares.  Kernels: vqhip_step_kernels.h.
#include "vqhip.h"

#include <hip/hip_runtime.h>

#include "vqhip_core.h"
#include "vqhip_step_kernels.h"

// front of the VQ-KD / NormalizeCallback forwards (vqhip_step_kernels.h): the L-lanes-per-row form at D <= 32
static int launch_vqkd_front(const float *w_in, float *w_mid, int64_t K, const void *x, int x_dtype, float *xn, int64_t N, int D, float eps,
                             float *zero, int64_t nzero, int w_passes, hipStream_t s) {
    if (D <= 32) {
        const int L = vq_small_lanes(D), rpb = 4 * (64 / L);
        const int kblocks = (int)((K + rpb - 1) / rpb), xblocks = (int)((N + rpb - 1) / rpb);
#define VQ_FRONT_SMALL(DT, LL) vqkd_front_small_kernel<DT, LL><<<kblocks + xblocks, 256, 0, s>>>(w_in, w_mid, K, x, xn, N, D, eps, kblocks, zero, nzero, w_passes)
        if (x_dtype == VQHIP_DTYPE_F32) { if (L == 8) VQ_FRONT_SMALL(0, 8); else if (L == 16) VQ_FRONT_SMALL(0, 16); else VQ_FRONT_SMALL(0, 32); }
        else { if (L == 8) VQ_FRONT_SMALL(1, 8); else if (L == 16) VQ_FRONT_SMALL(1, 16); else VQ_FRONT_SMALL(1, 32); }
#undef VQ_FRONT_SMALL
    } else {
        const int kblocks = (int)((K + 3) / 4), xblocks = (int)((N + 3) / 4);
        if (x_dtype == VQHIP_DTYPE_F32) vqkd_front_kernel<0><<<kblocks + xblocks, 256, 0, s>>>(w_in, w_mid, K, x, xn, N, D, eps, kblocks, zero, nzero, w_passes);
        else vqkd_front_kernel<1><<<kblocks + xblocks, 256, 0, s>>>(w_in, w_mid, K, x, xn, N, D, eps, kblocks, zero, nzero, w_passes);
    }
    VQ_CHECK_LAUNCH("vqkd_front_kernel");
    return VQHIP_OK;
}

extern "C" {

// ---- one host call per training forward (include/vqhip.h) ------------------------------------------------------------
int64_t vqhip_cvq_forward_ws_bytes(int64_t N, int64_t K, int D, int64_t cap_max) {
    if (N <= 0 || K <= 0 || D <= 0 || cap_max < 0 || cap_max > K) return 0;
    return vq_cvq_ws_layout(N, K, D, cap_max).total;
}

int vqhip_cvq_forward(vqhip_cvq_forward_t *a, void *stream) {
    if (!a || a->struct_bytes != (int64_t)sizeof(vqhip_cvq_forward_t)) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: struct_bytes != sizeof(vqhip_cvq_forward_t)");
    const int64_t N = a->N, K = a->K;
    const int D = a->D, metric = a->metric;
    VQ_REQUIRE(N > 0 && K > 0 && D > 0 && vq_fits_i31(N, K) && vq_coarse_supported(D), "vqhip_cvq_forward: needs N, K > 0 and D <= 1024, D % 8 == 0");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_cvq_forward: metric");
    VQ_REQUIRE(vq_row_dtype(a->x_dtype), "vqhip_cvq_forward: x_dtype");
    const bool sync = a->exchange && a->anchor_sync;
    if (a->phases < 1 || (a->phases > VQHIP_STEP_ALL && !(sync && a->phases == VQHIP_STEP_PACK_SYNC))) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: phases");
    if (!a->x || !a->w_in || !a->p_in || !a->w_out || !a->p_out || !a->rows || !a->slot || !a->count || !a->cb || !a->idx || !a->hist || !a->ws)
        return fail(VQHIP_EINVAL, "vqhip_cvq_forward: null pointer");
    const bool cos = VQ_IS_COS(metric);
    if (cos && !a->xq) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: the cosine metric needs the xq buffer");
    if ((a->z_ste || a->mse) && (!a->mse || !a->scratch16)) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: the decode tail needs mse and scratch16");
    if (a->exchange) {
        if (!a->packed) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: exchange without a packed buffer");
        if (a->world < 1 || a->world > VQ_PACK_MAX_WORLD) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: world must be in [1, 256]");
        if (a->phases == VQHIP_STEP_ALL && !a->comm && a->world > 1)
            return fail(VQHIP_EINVAL, "vqhip_cvq_forward: VQHIP_STEP_ALL over more than one rank needs a communicator (or issue the collective between the two phases)");
    }
    if (sync) {
        if (!a->keys) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: anchor_sync needs the keys buffer");
        if (a->rank < 0 || a->rank >= a->world) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: anchor_sync needs this rank's number in [0, world)");
        if (N > VQHIP_SYNC_MAX_ROWS) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: anchor_sync holds a row in 24 bits (N <= 2^24 per rank)");
    }
    hipStream_t s = (hipStream_t)stream;
    const VqCvqWsLayout C = vq_cvq_ws_layout(N, K, D, 0);       // the column pass is sized once this step's capacity is known
    VQ_NEED("vqhip_cvq_forward: ws too small", a->ws_bytes, C.total);
    char *w = (char *)a->ws;
    int64_t *col_idx = (int64_t *)(w + C.off_col_idx);
    char *col_ws = w + C.off_col_ws;
    const int64_t col_ws_have = a->ws_bytes - C.off_col_ws;
    if (a->phases != VQHIP_STEP_PACK_SYNC && (a->phases & VQHIP_STEP_BEFORE_EXCHANGE)) {
        if (int rc = vqhip_encode_ex(a->x, a->x_dtype, a->w_in, N, K, D, metric, a->cb, a->cb_bytes, a->idx, a->hist, a->xq, a->ws,
                                     C.enc_bytes, VQHIP_ENCODE_ZERO_HIST, stream)) return rc;
        if (!a->list_ready)
            if (int rc = vqhip_cvq_rows(a->p_in, K, a->ema_decay, a->eps, a->rows, a->slot, a->count, stream)) return rc;
        if (!a->exchange && a->early_word_host && a->early_seq_dev) {     // one rank: the histogram is final behind the encode
            if (int rc = cvq_count_next(false, a->p_in, a->hist, N, nullptr, K, a->ema_decay, a->eps, a->early_seq_dev, a->early_word_host, s)) return rc;
        }
        int64_t cap = a->cap;
        if (cap < 0) {                   // the count the previous call's prefetch copied out: queued a whole step ago
            if (!a->count_host) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: cap < 0 needs count_host");
            if (a->count_event) VQ_HIP(hipEventSynchronize((hipEvent_t)a->count_event));
            cap = (int64_t)*(volatile const int32_t *)a->count_host;
        }
        if (cap < 0 || cap > K) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: capacity outside [0, K]");
        a->cap_used = cap;
        a->exchange_floats = a->exchange ? vqhip_pack_floats(K, cap, D) : 0;
        if (a->exchange) VQ_NEED("vqhip_cvq_forward: packed buffer too small (floats)", a->packed_floats, a->exchange_floats);
        if (cap > 0) {
            VQ_NEED("vqhip_cvq_forward: ws too small for the column pass", col_ws_have, vqhip_col_rows_workspace_bytes(N, cap, D));
            const VqCbLayout L = vq_cb_layout(K, D);
            const void *rows_x = cos ? (const void *)a->xq : a->x;
            const float *codes = cos ? (const float *)((const char *)a->cb + L.off_eexact) : a->w_in;
            if (int rc = vqhip_col_argmin_rows(rows_x, cos ? VQHIP_DTYPE_F32 : a->x_dtype, codes, a->rows, a->count, cap, N, K, D, metric,
                                               col_idx, col_ws, col_ws_have, stream)) return rc;
            if (sync)                    // the local winners' keys: the ranks agree on the global winner by a MIN all-reduce
                if (int rc = vqhip_cvq_col_keys(rows_x, cos ? VQHIP_DTYPE_F32 : a->x_dtype, codes, a->rows, a->count, cap, col_idx, N, K, D, metric,
                                                a->rank, a->keys, stream)) return rc;
        }
        if (a->exchange && !sync)
            if (int rc = vqhip_cvq_pack(a->hist, N, a->x, a->x_dtype, col_idx, a->count, cap, K, D, a->packed, stream)) return rc;
    }
    if (sync && (a->phases == VQHIP_STEP_ALL || a->phases == VQHIP_STEP_PACK_SYNC)) {
        if (a->cap_used < 0 || a->cap_used > K) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: cap_used (the BEFORE phase writes it)");
        if (a->phases == VQHIP_STEP_ALL && a->comm && a->cap_used > 0)
            if (int rc = vqhip_allreduce_min_i64(a->keys, a->cap_used, a->comm, stream)) return rc;
        if (int rc = vqhip_cvq_pack_sync(a->hist, N, a->x, a->x_dtype, a->keys, a->count, a->cap_used, a->rank, K, D, a->packed, stream)) return rc;
    }
    if (a->phases == VQHIP_STEP_ALL && a->exchange && a->comm)
        if (int rc = vqhip_allreduce_packed(a->packed, a->exchange_floats, a->comm, stream)) return rc;
    if (a->phases != VQHIP_STEP_PACK_SYNC && (a->phases & VQHIP_STEP_AFTER_EXCHANGE)) {
        if (a->cap_used < 0 || a->cap_used > K) return fail(VQHIP_EINVAL, "vqhip_cvq_forward: cap_used (the BEFORE phase writes it)");
        if (a->exchange && a->early_word_host && a->early_seq_dev) {      // the next list's length, right behind the reduced histogram
            if (int rc = cvq_count_next(true, a->p_in, nullptr, 0, a->packed, K, a->ema_decay, a->eps, a->early_seq_dev, a->early_word_host, s)) return rc;
        }
        // sync: the packed rows ARE the global winners' latents (every other rank added -0): no averaging (anchors.py:59-63)
        if (int rc = vqhip_cvq_apply(a->w_in, a->w_out, a->p_in, a->p_out, a->hist, N, a->x, a->x_dtype, col_idx, a->exchange ? a->packed : nullptr,
                                     sync ? 1 : a->world, a->slot, a->cap_used, K, D, a->ema_decay, a->eps, stream)) return rc;
        if (a->prefetch) {
            // the list of the NEXT step; its length also goes straight to the caller's pinned host word (a store of the kernel
            // itself — pinned host memory is device-visible at its own address — instead of a 4-byte copy launch behind it)
            if (int rc = cvq_rows_prefetch(a->p_out, K, a->ema_decay, a->eps, a->rows, a->slot, a->count, a->count_host, s)) return rc;
            if (a->count_host && a->count_event) VQ_HIP(hipEventRecord((hipEvent_t)a->count_event, s));
        }
        if (a->mse)
            if (int rc = vqhip_gather_ste_mse(a->x, a->x_dtype, a->w_out, a->idx, N, D, nullptr, a->z_ste, a->mse, a->beta, a->scratch16, stream)) return rc;
    }
    return VQHIP_OK;
}

static inline VqKdWsLayout vqkd_ws_layout(int64_t N, int64_t K, int D) {
    return vq_kd_ws_layout(N, K, D, vqhip_order_workspace_bytes(N, K), vqhip_segsum_workspace_bytes(N, D));
}

int64_t vqhip_vqkd_forward_ws_bytes(int64_t N, int64_t K, int D) {
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    return vqkd_ws_layout(N, K, D).total;
}

int vqhip_vqkd_forward(vqhip_vqkd_forward_t *a, void *stream) {
    if (!a || a->struct_bytes != (int64_t)sizeof(vqhip_vqkd_forward_t)) return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: struct_bytes != sizeof(vqhip_vqkd_forward_t)");
    const int64_t N = a->N, K = a->K;
    const int D = a->D;
    VQ_REQUIRE(N > 0 && K > 0 && D > 0 && vq_fits_i31(N, K) && vq_coarse_supported(D), "vqhip_vqkd_forward: needs N, K > 0 and D <= 1024, D % 8 == 0");
    if (a->metric != VQHIP_METRIC_COS && a->metric != VQHIP_METRIC_COS_BF16) return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: metric (cosine only)");
    VQ_REQUIRE(vq_row_dtype(a->x_dtype), "vqhip_vqkd_forward: x_dtype");
    if (a->phases < 1 || a->phases > VQHIP_STEP_ALL) return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: phases");
    if (!a->x || !a->w_in || !a->w_mid || !a->w_out || !a->xn || !a->xq || !a->cb || !a->idx || !a->hist || !a->packed || !a->ws)
        return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: null pointer");
    if (a->tail && (!a->mse || !a->scratch16)) return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: the tail needs mse and scratch16");
    if (a->world < 1 || a->world > VQ_PACK_MAX_WORLD) return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: world must be in [1, 256]");
    if (a->phases == VQHIP_STEP_ALL && a->exchange && !a->comm && a->world > 1)
        return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: VQHIP_STEP_ALL over more than one rank needs a communicator (or issue the collective between the two phases)");
    if (a->ordered && (K > 32768 || (D % 4) != 0)) return fail(VQHIP_EINVAL, "vqhip_vqkd_forward: ordered sums need K <= 32768 and D % 4 == 0");
    const int64_t floats = vqhip_pack_floats(K, K, D);
    VQ_NEED("vqhip_vqkd_forward: packed buffer too small (floats)", a->packed_floats, floats);
    const VqKdWsLayout C = vqkd_ws_layout(N, K, D);
    VQ_NEED("vqhip_vqkd_forward: ws too small", a->ws_bytes, C.total);
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)a->ws;
    float *payload = a->packed + VQ_PACK_HEADER(K);
    if (a->phases & VQHIP_STEP_BEFORE_EXCHANGE) {
        a->exchange_floats = floats;
        // front: codebook normalised twice, latents normalised, payload zeroed (the atomic sums need it; the ordered sums write every row)
        int64_t nzero = a->ordered ? 0 : K * (int64_t)D;
        if (nzero && ((K & 1) || (nzero % 4))) {            // a payload that is not 16-byte aligned / sized: plain memset
            VQ_HIP(hipMemsetAsync(payload, 0, (size_t)nzero * 4, s));
            nzero = 0;
        }
        if (int rc = launch_vqkd_front(a->w_in, a->w_mid, K, a->x, a->x_dtype, a->xn, N, D, 1e-12f, payload, nzero, 2, s)) return rc;
        const int xblocks = (int)((N + 3) / 4);             // wave per token: the scatter below
        if (int rc = vqhip_encode_ex(a->xn, VQHIP_DTYPE_F32, a->w_mid, N, K, D, a->metric, a->cb, a->cb_bytes, a->idx, a->hist, a->xq, a->ws,
                                     C.enc_bytes, VQHIP_ENCODE_ZERO_HIST, stream)) return rc;
        const int hb = (int)((K + 255) / 256);
        if (a->ordered) {
            int32_t *counts = (int32_t *)(w + C.off_counts), *offsets = (int32_t *)(w + C.off_offsets), *order = (int32_t *)(w + C.off_order);
            if (int rc = vqhip_token_order(a->idx, N, K, counts, offsets, order, w + C.off_order_ws, vqhip_order_workspace_bytes(N, K), stream)) return rc;
            const float *x2 = a->xq;                      // F.normalize(xn): the encode's by-product — except under the bf16-autocast
            if (VQ_IS_BF16(a->metric)) {                  // metric, where xq holds the ROUNDED rows (the operand of that metric)
                if (int rc = vqhip_normalize_rows(a->xn, VQHIP_DTYPE_F32, N, D, 1e-12f, (float *)(w + C.off_x2), stream)) return rc;
                x2 = (const float *)(w + C.off_x2);
            }
            if (int rc = vqhip_segsum_rows(x2, a->idx, order, offsets, N, K, D, payload, w + C.off_segsum_ws, vqhip_segsum_workspace_bytes(N, D), stream)) return rc;
            vqkd_scatter_pack_kernel<<<hb, 256, 0, s>>>(a->hist, N, a->xn, a->idx, N, K, D, 1e-12f, a->packed, hb, 0);
        } else {
            vqkd_scatter_pack_kernel<<<hb + xblocks, 256, 0, s>>>(a->hist, N, a->xn, a->idx, N, K, D, 1e-12f, a->packed, hb, 1);
        }
        VQ_CHECK_LAUNCH("vqkd_scatter_pack_kernel");
    }
    if (a->phases == VQHIP_STEP_ALL && a->exchange && a->comm)
        if (int rc = vqhip_allreduce_packed(a->packed, floats, a->comm, stream)) return rc;
    if (a->phases & VQHIP_STEP_AFTER_EXCHANGE) {
        vqkd_update_packed_kernel<<<waves_grid(K, 4), 256, 0, s>>>(a->w_mid, a->w_out, a->packed, K, D, a->ema_decay);
        VQ_CHECK_LAUNCH("vqkd_update_packed_kernel");
        if (a->tail) {
            // per-workgroup partial sums of the loss (<= 256 doubles): the record area of the encode's workspace, free by now
            double *tail_partials = (double *)vq_ws_view(a->ws, vq_ws_layout(N, K, D)).rec;
            if (D <= 32) {                                  // L lanes per token (vqhip_step_kernels.h)
                const int L = vq_small_lanes(D), rpb = 16 * (64 / L);
                int grid = (int)((N + rpb - 1) / rpb); grid = grid > 256 ? 256 : grid;
                if (L == 8) vqkd_tail_small_kernel<8><<<grid, 1024, 0, s>>>(a->xn, a->w_out, a->idx, N, D, 1e-12f, a->z_ste, (double *)a->scratch16, a->mse, tail_partials);
                else if (L == 16) vqkd_tail_small_kernel<16><<<grid, 1024, 0, s>>>(a->xn, a->w_out, a->idx, N, D, 1e-12f, a->z_ste, (double *)a->scratch16, a->mse, tail_partials);
                else vqkd_tail_small_kernel<32><<<grid, 1024, 0, s>>>(a->xn, a->w_out, a->idx, N, D, 1e-12f, a->z_ste, (double *)a->scratch16, a->mse, tail_partials);
            } else {
                int grid = (int)((N + 15) / 16); grid = grid > 256 ? 256 : grid;
                vqkd_tail_kernel<<<grid, 1024, 0, s>>>(a->xn, a->w_out, a->idx, N, D, 1e-12f, a->z_ste, (double *)a->scratch16, a->mse, tail_partials);
            }
            VQ_CHECK_LAUNCH("vqkd_tail_kernel");
        }
    }
    return VQHIP_OK;
}

int vqhip_vq_forward(vqhip_vq_forward_t *a, void *stream) {
    if (!a || a->struct_bytes != (int64_t)sizeof(vqhip_vq_forward_t)) return fail(VQHIP_EINVAL, "vqhip_vq_forward: struct_bytes != sizeof(vqhip_vq_forward_t)");
    const int64_t N = a->N, K = a->K;
    const int D = a->D;
    VQ_REQUIRE(N > 0 && K > 0 && D > 0 && vq_fits_i31(N, K), "vqhip_vq_forward: N, K, D");
    VQ_REQUIRE(vq_public_metric(a->metric), "vqhip_vq_forward: metric");
    VQ_REQUIRE(vq_row_dtype(a->x_dtype), "vqhip_vq_forward: x_dtype");
    if (!a->x || !a->w_in || !a->cb || !a->idx || !a->ws || (a->normalize && (!a->w_out || !a->xn))) return fail(VQHIP_EINVAL, "vqhip_vq_forward: null pointer");
    if (VQ_IS_COS(a->metric) && !a->xq) return fail(VQHIP_EINVAL, "vqhip_vq_forward: the cosine metric needs the xq buffer");
    if ((a->z_ste || a->mse) && (!a->mse || !a->scratch16)) return fail(VQHIP_EINVAL, "vqhip_vq_forward: the decode tail needs mse and scratch16");
    VQ_NEED("vqhip_vq_forward: ws too small", a->ws_bytes, vqhip_workspace_bytes(N, K, D));
    hipStream_t s = (hipStream_t)stream;
    const void *rows = a->x;
    int rows_dtype = a->x_dtype;
    const float *codes = a->w_in;
    if (a->normalize) {
        if (int rc = launch_vqkd_front(a->w_in, a->w_out, K, a->x, a->x_dtype, a->xn, N, D, 1e-12f, nullptr, 0, 1, s)) return rc;
        rows = a->xn; rows_dtype = VQHIP_DTYPE_F32; codes = a->w_out;
    }
    if (int rc = vqhip_encode_ex(rows, rows_dtype, codes, N, K, D, a->metric, a->cb, a->cb_bytes, a->idx, a->hist, a->xq, a->ws, a->ws_bytes,
                                 a->hist ? VQHIP_ENCODE_ZERO_HIST : 0, stream)) return rc;
    if (a->mse)
        if (int rc = vqhip_gather_ste_mse(rows, rows_dtype, codes, a->idx, N, D, nullptr, a->z_ste, a->mse, a->beta, a->scratch16, stream)) return rc;
    return VQHIP_OK;
}

int vqhip_vqkd_backward(const void *x, int x_dtype, const float *xn, const float *w, const int64_t *idx, int64_t N, int D,
                        const float *g_zste, const float *g_loss, float *grad_x, void *stream) {
    if (!x || !xn || !w || !idx || !grad_x || N < 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_vqkd_backward: bad argument");
    if (N == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_vqkd_backward: x_dtype");
    if (D <= 32) {                                          // L lanes per token (vqhip_step_kernels.h)
        const int L = vq_small_lanes(D), rpb = 4 * (64 / L);
        int grid = (int)((N + rpb - 1) / rpb); grid = grid > 2048 ? 2048 : grid;
#define VQ_BWD_SMALL(DT, LL) vqkd_backward_small_kernel<DT, LL><<<grid, 256, 0, s>>>(x, xn, w, idx, N, D, 1e-12f, g_zste, g_loss, grad_x)
        if (x_dtype == VQHIP_DTYPE_F32) { if (L == 8) VQ_BWD_SMALL(0, 8); else if (L == 16) VQ_BWD_SMALL(0, 16); else VQ_BWD_SMALL(0, 32); }
        else { if (L == 8) VQ_BWD_SMALL(1, 8); else if (L == 16) VQ_BWD_SMALL(1, 16); else VQ_BWD_SMALL(1, 32); }
#undef VQ_BWD_SMALL
        VQ_CHECK_LAUNCH("vqkd_backward_kernel");
        return VQHIP_OK;
    }
    int grid = (int)((N + 3) / 4); grid = grid > 2048 ? 2048 : grid;
    if (x_dtype == VQHIP_DTYPE_F32) vqkd_backward_kernel<0><<<grid, 256, 0, s>>>(x, xn, w, idx, N, D, 1e-12f, g_zste, g_loss, grad_x);
    else vqkd_backward_kernel<1><<<grid, 256, 0, s>>>(x, xn, w, idx, N, D, 1e-12f, g_zste, g_loss, grad_x);
    VQ_CHECK_LAUNCH("vqkd_backward_kernel");
    return VQHIP_OK;
}

int vqhip_vq_backward_map(const void *x_rows, int x_dtype, const float *e, const int64_t *idx, int64_t B, int64_t HW, int D,
                          const float *g_map, const float *g_cm, const float *g_comb, float beta, void *grad_map, int grad_dtype,
                          void *stream) {
    if (!x_rows || !e || !idx || !grad_map || B <= 0 || HW <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_vq_backward_map: bad argument");
    if ((HW % 256) != 0 || (D % 32) != 0) return fail(VQHIP_EINVAL, "vqhip_vq_backward_map: needs HW % 256 == 0 and D % 32 == 0 (transpose and use vqhip_vq_backward_ex)");
    VQ_REQUIRE(vq_row_dtype(x_dtype) && vq_row_dtype(grad_dtype), "vqhip_vq_backward_map: dtype");
    const int64_t N = B * HW, nt = N / 256;
    int csplit = 1;
    while (nt * csplit < 512 && (D / 32) % (csplit * 2) == 0) csplit *= 2;
    const int64_t items = nt * csplit;
    const int grid = (int)(items < 1024 ? items : 1024);
    constexpr int LDS = 2 * 32 * 256 * 4;
    static LdsCache sets[4];
    const int v = (x_dtype == VQHIP_DTYPE_BF16 ? 1 : 0) + (grad_dtype == VQHIP_DTYPE_BF16 ? 2 : 0);
    const void *kerns[4] = {(const void *)vq_backward_map256_kernel<0, 0>, (const void *)vq_backward_map256_kernel<1, 0>,
                            (const void *)vq_backward_map256_kernel<0, 1>, (const void *)vq_backward_map256_kernel<1, 1>};
    if (int rc = ensure_dyn_lds(kerns[v], LDS, sets[v])) return rc;
    hipStream_t s = (hipStream_t)stream;
#define VQ_BMAP(DT, ODT) vq_backward_map256_kernel<DT, ODT><<<grid, 512, LDS, s>>>(x_rows, e, idx, N, D, HW, csplit, g_map, g_cm, g_comb, beta, grad_map)
    if (v == 0) VQ_BMAP(0, 0); else if (v == 1) VQ_BMAP(1, 0); else if (v == 2) VQ_BMAP(0, 1); else VQ_BMAP(1, 1);
#undef VQ_BMAP
    VQ_CHECK_LAUNCH("vq_backward_map256_kernel");
    return VQHIP_OK;
}

}  // extern "C"
