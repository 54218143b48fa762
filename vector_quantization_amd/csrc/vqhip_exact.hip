// libvqhip — the all-fp32 MFMA pass, the definition itself: over a whole batch (vqhip_argmin_exact, vqhip_distance, the column
// pass where D has no proposal image) and over listed rows (the last resort of the proposal pipeline in vqhip.hip, the column
// pass over a short list).  gfx950 only.  The pipeline reaches it through the functions vqhip_core.h declares.  The streamed
// form of the whole-batch pass (vqhip_stream_kernels.h) is launched from vqhip.hip: run_exact_stream in vqhip_core.h says why.
#include "vqhip.h"

#include <hip/hip_runtime.h>

#include <atomic>

#include "vqhip_core.h"
#include "vqhip_exact_kernels.h"

// The all-fp32 MFMA pass over a whole batch.  Streamed form (exact_stream_kernel, both operands from LDS, two workgroups per CU,
// contiguous spans of work items) wherever rows and codes move as whole 16-byte pieces; the register form
// (exact_tiled_kernel) for the other D and on request (vqhip_set_tuning key 18 = 0, A/B: the results are identical).
template <int MODE>
static int run_exact_tiled(const void *x, int x_dtype, const float *e, const float *en, const float *xn, int64_t N, int64_t K,
                           int D, int metric, u64 *keys, float *dout, hipStream_t s) {
    const int bf = x_dtype == VQHIP_DTYPE_F32 ? 0 : 1;
    const int64_t items = ((N + 127) / 128) * ((K + 255) / 256);
    if (vq_tune_stream() && D % (bf ? 8 : 4) == 0 && items < (int64_t)1 << 31) {
        return run_exact_stream<MODE>(x, bf, e, en, xn, N, K, D, metric, keys, dout, items, s);      // (launched by vqhip.hip)
    }
    constexpr int LDS = 2 * 32 * 128 * 4 + 8 * 32 * 4;      // two staged tiles + the |e|^2 of an item's 256 codes
    static LdsCache sets[4];
    const void *kerns[4] = {(const void *)exact_tiled_kernel<0, MODE, false>, (const void *)exact_tiled_kernel<1, MODE, false>,
                            (const void *)exact_tiled_kernel<0, MODE, true>, (const void *)exact_tiled_kernel<1, MODE, true>};
    const int v4 = (D % 4 == 0) ? 2 : 0;
    if (int rc = ensure_dyn_lds(kerns[v4 + bf], LDS, sets[v4 + bf])) return rc;
    int grid = (int)(items < 1024 ? items : 1024);
#define VQ_TILED(DT, V4) exact_tiled_kernel<DT, MODE, V4><<<grid, 256, LDS, s>>>(x, e, en, xn, N, K, D, metric, keys, dout)
    if (v4) { if (bf) VQ_TILED(1, true); else VQ_TILED(0, true); }
    else { if (bf) VQ_TILED(1, false); else VQ_TILED(0, false); }
#undef VQ_TILED
    VQ_CHECK_LAUNCH("exact_tiled_kernel");
    return VQHIP_OK;
}

// The fp32-only route over a whole batch, in an encode workspace: the oracle-order norms of both sides under L2, then
// run_exact_tiled<MODE>.  MODE 0: the keys are armed in front and turned into idx / dmin / hist behind; MODE 2 (`dout`) has none.
template <int MODE>
static int exact_whole(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, const VqWsView &V,
                       int64_t *idx, float *dmin, int32_t *hist, float *dout, hipStream_t s) {
    constexpr bool keyed = MODE != 2;
    const bool l2 = metric == VQHIP_METRIC_L2;
    if (l2) if (int rc = vqhip_row_sqnorm(e, VQHIP_DTYPE_F32, K, D, V.en, s)) return rc;
    if constexpr (keyed) { fill_u64_kernel<<<256, 256, 0, s>>>(V.keys, N, ~0ull); VQ_CHECK_LAUNCH("fill_u64_kernel"); }
    if (l2) if (int rc = vqhip_row_sqnorm(x, x_dtype, N, D, V.xn_whole, s)) return rc;
    if (int rc = run_exact_tiled<MODE>(x, x_dtype, e, V.en, V.xn_whole, N, K, D, metric, keyed ? V.keys : nullptr, dout, s)) return rc;
    if constexpr (keyed) { finalize_kernel<<<256, 256, 0, s>>>(V.keys, nullptr, nullptr, N, idx, dmin, hist); VQ_CHECK_LAUNCH("finalize_kernel"); }
    return VQHIP_OK;
}

// The few-rows (VALU) form of exact_kernel stages its operands in dynamic LDS: a 64 KiB ring + 64 D bytes.  The request applies to
// the LAUNCH, i.e. also when the device-side count picks the MFMA form: at D > 512 (96 KiB) that would leave the MFMA form one
// workgroup per CU, and a part with less LDS per workgroup than asked for would refuse the launch — so the form is offered only
// where the request stays within 96 KiB and within what the device grants a workgroup.
static int exact_few_max(int D) {
    if (D > 512 || D > VQ_FEW_MAX_D) return 0;
    static std::atomic<int> lds_limit{-1};
    int lim = lds_limit.load(std::memory_order_relaxed);
    if (lim < 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) v = 65536;
        lim = v;
        lds_limit.store(lim);
    }
    return vq_few_lds_bytes(D) <= lim ? VQ_EXACT_FEW_MAX : 0;
}

int run_exact_rows(const void *x, int x_dtype, const float *e, const float *en, const float *xn, int64_t N, int64_t K, int D,
                          int metric, const int *row_list, const int *nrows_dev, u64 *keys, int *ticket, int64_t *idx,
                          int32_t *hist, hipStream_t s) {
    // last-resort path of vqhip_argmin: a few listed rows against the whole codebook (small work items); the workgroup
    // that finishes last turns the keys into indices (ticket: zeroed by x_prep_kernel with the other counters)
    const int64_t ncb = (K + 63) / 64;           // work items of the few-rows form per 16 listed rows
    const int grid = (int)(ncb < 256 ? 256 : (ncb > 1024 ? 1024 : ncb));
    if (D % 4) return fail(VQHIP_EINVAL, "exact_kernel: D % 4 != 0 (the proposal route has D % 8 == 0)");
    const int few_max = exact_few_max(D);
    const int lds = few_max ? vq_few_lds_bytes(D) : 0;
    static LdsCache sets[2];
    const int bf = x_dtype == VQHIP_DTYPE_F32 ? 0 : 1;
    if (int rc = ensure_dyn_lds(bf ? (const void *)exact_kernel<1> : (const void *)exact_kernel<0>, lds, sets[bf])) return rc;
    if (!bf)
        exact_kernel<0><<<grid, 256, lds, s>>>(x, e, en, xn, N, K, D, metric, row_list, nrows_dev, keys, ticket, idx, hist, few_max);
    else
        exact_kernel<1><<<grid, 256, lds, s>>>(x, e, en, xn, N, K, D, metric, row_list, nrows_dev, keys, ticket, idx, hist, few_max);
    VQ_CHECK_LAUNCH("exact_kernel");
    return VQHIP_OK;
}

int force_exact_rows(int nforce, int *exact_list, int *counters, u64 *keys, hipStream_t s) {
    force_exact_rows_kernel<<<1, 1024, 0, s>>>(nforce, exact_list, counters, keys);
    VQ_CHECK_LAUNCH("force_exact_rows_kernel");
    return VQHIP_OK;
}

int exact_whole_cols(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, const VqWsView &V,
                     int64_t *col_idx, hipStream_t s) {
    if (metric == VQHIP_METRIC_L2) {
        if (int rc = vqhip_row_sqnorm(e, VQHIP_DTYPE_F32, K, D, V.en, s)) return rc;
        if (int rc = vqhip_row_sqnorm(x, x_dtype, N, D, V.xn_whole, s)) return rc;
    }
    fill_u64_kernel<<<256, 256, 0, s>>>(V.keys, K, ~0ull);
    VQ_CHECK_LAUNCH("fill_u64_kernel");
    if (int rc = run_exact_tiled<1>(x, x_dtype, e, V.en, V.xn_whole, N, K, D, metric, V.keys, nullptr, s)) return rc;
    finalize_kernel<<<256, 256, 0, s>>>(V.keys, nullptr, nullptr, K, col_idx, nullptr, nullptr);
    VQ_CHECK_LAUNCH("finalize_kernel");
    return VQHIP_OK;
}

// x: the tokens [N, D] as the exact definition consumes them (fp32), e: the codebook rows [K, D] likewise; tok_norm / row_norm:
// oracle-order |x_n|^2 [N] / |e_k|^2 [K] where a caller has them already (L2 only; nullable: computed here)
int col_rows_direct(const void *x, const float *e, const int32_t *rows, const int32_t *count, int64_t cap, int64_t N,
                           int64_t K, int D, int metric, int64_t *col_idx, char *ws, const float *tok_norm, const float *row_norm,
                           hipStream_t s) {
    const VqColDirectLayout C = vq_col_direct_layout(N, K);
    u64 *keys = (u64 *)ws;
    int *ticket = (int *)(ws + C.off_ticket);
    float *tok_ws = (float *)(ws + C.off_tok_norm), *row_ws = (float *)(ws + C.off_row_norm);
    col_direct_init_kernel<<<(int)((cap + 255) / 256), 256, 0, s>>>(rows, count, cap, keys, ticket);
    VQ_CHECK_LAUNCH("col_direct_init_kernel");
    const int m = vq_swapped_metric(metric);
    if (metric == VQHIP_METRIC_L2) {
        if (!tok_norm) { if (int rc = vqhip_row_sqnorm(x, VQHIP_DTYPE_F32, N, D, tok_ws, s)) return rc; tok_norm = tok_ws; }
        if (!row_norm) { if (int rc = vqhip_row_sqnorm(e, VQHIP_DTYPE_F32, K, D, row_ws, s)) return rc; row_norm = row_ws; }
    }
    const int64_t ncb = (N + 63) / 64;
    const int grid = (int)(ncb < 256 ? 256 : (ncb > 1024 ? 1024 : ncb));
    const int few_max = exact_few_max(D);
    const int lds = few_max ? vq_few_lds_bytes(D) : 0;
    static LdsCache lds_set;
    if (int rc = ensure_dyn_lds((const void *)exact_kernel<0>, lds, lds_set)) return rc;
    // roles swapped: the listed codebook rows are the "rows", the tokens the "codes"
    exact_kernel<0><<<grid, 256, lds, s>>>(e, (const float *)x, tok_norm, row_norm, K, N, D, m, (const int *)rows, (const int *)count, keys, ticket,
                                           col_idx, nullptr, few_max, 1);
    VQ_CHECK_LAUNCH("exact_kernel (direct column pass)");
    return VQHIP_OK;
}

extern "C" {

int vqhip_argmin_exact(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, int64_t *idx,
                       float *dmin, int32_t *hist, void *ws, int64_t ws_bytes, void *stream) {
    if (N == 0) return VQHIP_OK;
    if (!x || !e || !idx || !ws || N < 0 || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_argmin_exact: bad argument");
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_argmin_exact: x_dtype");
    VQ_REQUIRE(vq_fits_i31(N, K), "vqhip_argmin_exact: N or K too large");
    VQ_NEED("vqhip_argmin_exact: ws too small", ws_bytes, vqhip_workspace_bytes(N, K, D));
    return exact_whole<0>(x, x_dtype, e, N, K, D, metric, vq_ws_view(ws, vq_ws_layout(N, K, D)), idx, dmin, hist, nullptr, (hipStream_t)stream);
}

int vqhip_distance(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, float *d, void *ws,
                   int64_t ws_bytes, void *stream) {
    if (!x || !e || !d || !ws || N <= 0 || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_distance: bad argument");
    VQ_NEED("vqhip_distance: ws too small", ws_bytes, vqhip_workspace_bytes(N, K, D));
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_distance: x_dtype");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_distance: metric");
    return exact_whole<2>(x, x_dtype, e, N, K, D, metric, vq_ws_view(ws, vq_ws_layout(N, K, D)), nullptr, nullptr, nullptr, d, (hipStream_t)stream);
}

}  // extern "C"
