// libvqhip — the losses on row blocks of the distance matrix: EntropyLoss and the column multinomial of MultinomialAnchor.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "vqhip_host.h"
#include "vqhip_entropy_kernels.h"
#include "vqhip_col_multinomial_kernels.h"

extern "C" {

// ---- EntropyLoss on row blocks of the distance matrix (vqhip_entropy_kernels.h) ----------------------------------------
static int entropy_check(const char *what, int64_t R, int64_t K, float T) {
    // the kernels index a row with int and step by up to VQ_ENT_COLS past K before they stop; R * K elements are addressed in int64
    if (R <= 0 || K <= 0 || R >= (1ll << 31) || K > (1ll << 31) - 2 * VQ_ENT_COLS) return fail(VQHIP_EINVAL, what, "R must be in 1 .. 2^31 - 1, K in 1 .. 2^31 - 2048");
    if (!(T == T) || T == 0.0f || T - T != 0.0f) return fail(VQHIP_EINVAL, what, "the temperature must be finite and non-zero");
    return VQHIP_OK;
}

int64_t vqhip_entropy_workspace_bytes(int64_t R, int64_t K) {
    if (R <= 0 || K <= 0) return 0;
    return ((R + VQ_ENT_CHUNK - 1) / VQ_ENT_CHUNK) * K * (int64_t)sizeof(double);
}

// column sums of the tile (MODE 0: of p, MODE 1: of its values) added into acc[K], chunk by chunk
static int entropy_colsums(int mode, const float *tile, int64_t R, int64_t K, float T, const float *lse, double *acc, int init,
                           void *ws, hipStream_t s) {
    const int nchunks = (int)((R + VQ_ENT_CHUNK - 1) / VQ_ENT_CHUNK);
    const dim3 grid((unsigned)((K + VQ_ENT_COLS - 1) / VQ_ENT_COLS), (unsigned)(nchunks < 65535 ? nchunks : 65535));
#define VQ_ENT_COL(MODE, VEC) entropy_colsum_kernel<MODE, VEC><<<grid, 256, 0, s>>>(tile, (int)R, (int)K, T, lse, (double *)ws)
    if (K % 4 == 0) { if (mode == 0) VQ_ENT_COL(0, true); else VQ_ENT_COL(1, true); }
    else { if (mode == 0) VQ_ENT_COL(0, false); else VQ_ENT_COL(1, false); }
#undef VQ_ENT_COL
    VQ_CHECK_LAUNCH("entropy_colsum_kernel");
    int rgrid = (int)((K + 255) / 256); rgrid = rgrid > 4096 ? 4096 : rgrid;
    entropy_colreduce_kernel<<<rgrid, 256, 0, s>>>((const double *)ws, nchunks, (int)K, acc, init);
    VQ_CHECK_LAUNCH("entropy_colreduce_kernel");
    return VQHIP_OK;
}

int vqhip_entropy_rows(const float *tile, int64_t R, int64_t K, float temperature, float *lse, float *spa, double *qacc,
                       int init, void *ws, int64_t ws_bytes, void *stream) {
    const char *what = "vqhip_entropy_rows";
    if (int rc = entropy_check(what, R, K, temperature)) return rc;
    if (!tile || !lse || !spa || !qacc || !ws) return fail(VQHIP_EINVAL, what, "null pointer");
    if ((uintptr_t)tile % 16) return fail(VQHIP_EINVAL, what, "the tile must be 16-byte aligned");
    VQ_NEED("vqhip_entropy_rows: ws too small", ws_bytes, vqhip_entropy_workspace_bytes(R, K));
    hipStream_t s = (hipStream_t)stream;
    int grid = waves_grid(R, 4); grid = grid > 8192 ? 8192 : grid;
    if (K % 4 == 0) entropy_rows_kernel<true><<<grid, 256, 0, s>>>(tile, (int)R, (int)K, temperature, lse, spa);
    else entropy_rows_kernel<false><<<grid, 256, 0, s>>>(tile, (int)R, (int)K, temperature, lse, spa);
    VQ_CHECK_LAUNCH("entropy_rows_kernel");
    return entropy_colsums(0, tile, R, K, temperature, lse, qacc, init, ws, s);
}

int vqhip_entropy_finish(const float *lse, const float *spa, const double *qacc, int64_t N, int64_t K, float *q, float *c,
                         float *loss, void *stream) {
    const char *what = "vqhip_entropy_finish";
    if (int rc = entropy_check(what, N, K, 1.0f)) return rc;
    if (!lse || !spa || !qacc || !q || !c || !loss) return fail(VQHIP_EINVAL, what, "null pointer");
    entropy_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(lse, spa, qacc, (int)N, (int)K, q, c, loss);
    VQ_CHECK_LAUNCH("entropy_finish_kernel");
    return VQHIP_OK;
}

int vqhip_entropy_grad(float *tile, int64_t R, int64_t K, float temperature, const float *lse, const float *spa,
                       const float *c, float inv_nt, const float *upstream, int metric, float *rowsum, double *colacc,
                       int init, void *ws, int64_t ws_bytes, void *stream) {
    const char *what = "vqhip_entropy_grad";
    if (int rc = entropy_check(what, R, K, temperature)) return rc;
    if (metric != VQHIP_METRIC_L2 && metric != VQHIP_METRIC_COS) return fail(VQHIP_EINVAL, what, "metric (L2 or COS)");
    if (!tile || !lse || !spa || !c || !rowsum) return fail(VQHIP_EINVAL, what, "null pointer");
    if ((uintptr_t)tile % 16) return fail(VQHIP_EINVAL, what, "the tile must be 16-byte aligned");
    if (!(inv_nt == inv_nt) || inv_nt - inv_nt != 0.0f) return fail(VQHIP_EINVAL, what, "inv_nt must be finite");
    const bool l2 = metric == VQHIP_METRIC_L2;
    if (l2) {
        if (!colacc || !ws) return fail(VQHIP_EINVAL, what, "L2 needs colacc and ws");
        VQ_NEED("vqhip_entropy_grad: ws too small", ws_bytes, vqhip_entropy_workspace_bytes(R, K));
    }
    hipStream_t s = (hipStream_t)stream;
    int grid = waves_grid(R, 4); grid = grid > 8192 ? 8192 : grid;
    const int r = (int)R, k = (int)K;
#define VQ_ENT_GRAD(VEC, L2) entropy_grad_kernel<VEC, L2><<<grid, 256, 0, s>>>(tile, r, k, temperature, lse, spa, c, inv_nt, upstream, rowsum)
    if (K % 4 == 0) { if (l2) VQ_ENT_GRAD(true, true); else VQ_ENT_GRAD(true, false); }
    else { if (l2) VQ_ENT_GRAD(false, true); else VQ_ENT_GRAD(false, false); }
#undef VQ_ENT_GRAD
    VQ_CHECK_LAUNCH("entropy_grad_kernel");
    if (!l2) return VQHIP_OK;
    return entropy_colsums(1, tile, R, K, temperature, lse, colacc, init, ws, s);
}

// ---- fused MultinomialAnchor on row blocks of the distance matrix (vqhip_col_multinomial_kernels.h) -----------------------
struct VqColMultiWs {
    float *colmax;       // [K] running column maximum; NaN = bad column
    int32_t *sel;        // [K] the block that holds the column's crossing, -1 = none
    cm_u64 *resid;       // [K] the target inside that block
    cm_u64 *mass;        // [blocks, K] column masses per block
    int64_t blocks, total;
};

// what every entry point refuses, and the carve of `ws` (ws may be null: sizes only)
static int col_multinomial_setup(const char *what, int64_t N, int64_t K, int64_t R, void *ws, VqColMultiWs *w) {
    if (N < 1 || N > VQHIP_COL_MULTINOMIAL_MAX_N) return fail(VQHIP_EINVAL, what, "N must be in 1 .. 2^20");
    if (K < 1 || K >= (1ll << 31)) return fail(VQHIP_EINVAL, what, "K must be in 1 .. 2^31 - 1");
    if (R < 1 || R > N) return fail(VQHIP_EINVAL, what, "block_rows must be in 1 .. N");
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    char *c = (char *)ws;
    w->blocks = (N + R - 1) / R;                                                 // <= 2^20: blocks * K * 8 < 2^54
    int64_t off = 0;
    w->colmax = (float *)(c + off); off += up(K * 4);
    w->sel = (int32_t *)(c + off); off += up(K * 4);
    w->resid = (cm_u64 *)(c + off); off += up(K * 8);
    w->mass = (cm_u64 *)(c + off); off += up(w->blocks * K * 8);
    w->total = off;
    return VQHIP_OK;
}

int64_t vqhip_col_multinomial_workspace_bytes(int64_t N, int64_t K, int64_t block_rows) {
    VqColMultiWs w;
    if (col_multinomial_setup("vqhip_col_multinomial_workspace_bytes", N, K, block_rows, nullptr, &w)) return 0;
    return w.total;
}

// the checks of a call that takes a block: rows [r0, r0 + *r) with *r = min(block_rows, N - r0)
static int col_multinomial_block(const char *what, const float *tile, int64_t r0, int64_t N, int64_t K, int64_t R, void *ws,
                                 int64_t ws_bytes, VqColMultiWs *w, int64_t *r) {
    if (int rc = col_multinomial_setup(what, N, K, R, ws, w)) return rc;
    if (!tile || !ws) return fail(VQHIP_EINVAL, what, "null pointer");
    if (r0 < 0 || r0 >= N || r0 % R != 0) return fail(VQHIP_EINVAL, what, "r0 must be a multiple of block_rows below N");
    if (ws_bytes < w->total) {
        char msg[160];
        snprintf(msg, sizeof(msg), "ws too small: %lld bytes given, %lld needed", (long long)ws_bytes, (long long)w->total);
        return fail(VQHIP_EINVAL, what, msg);
    }
    *r = N - r0 < R ? N - r0 : R;
    return VQHIP_OK;
}

int vqhip_col_multinomial_max(const float *tile, int64_t r0, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes,
                              void *stream) {
    VqColMultiWs w;
    int64_t r;
    if (int rc = col_multinomial_block("vqhip_col_multinomial_max", tile, r0, N, K, block_rows, ws, ws_bytes, &w, &r)) return rc;
    const unsigned grid = (unsigned)((K + VQ_CM_COLS - 1) / VQ_CM_COLS);
    col_multinomial_max_kernel<<<grid, VQ_CM_COLS * VQ_CM_WAVES, 0, (hipStream_t)stream>>>(tile, (int)r, K, w.colmax, r0 == 0 ? 1 : 0);
    VQ_CHECK_LAUNCH("col_multinomial_max_kernel");
    return VQHIP_OK;
}

int vqhip_col_multinomial_mass(const float *tile, int64_t r0, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes,
                               void *stream) {
    VqColMultiWs w;
    int64_t r;
    if (int rc = col_multinomial_block("vqhip_col_multinomial_mass", tile, r0, N, K, block_rows, ws, ws_bytes, &w, &r)) return rc;
    const unsigned grid = (unsigned)((K + VQ_CM_COLS - 1) / VQ_CM_COLS);
    col_multinomial_mass_kernel<<<grid, VQ_CM_COLS * VQ_CM_WAVES, 0, (hipStream_t)stream>>>(tile, (int)r, K, w.colmax,
                                                                                           w.mass + (r0 / block_rows) * K);
    VQ_CHECK_LAUNCH("col_multinomial_mass_kernel");
    return VQHIP_OK;
}

int vqhip_col_multinomial_pick(const float *u, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes, int64_t *col_idx,
                               void *stream) {
    const char *what = "vqhip_col_multinomial_pick";
    VqColMultiWs w;
    if (int rc = col_multinomial_setup(what, N, K, block_rows, ws, &w)) return rc;
    if (!u || !ws || !col_idx) return fail(VQHIP_EINVAL, what, "null pointer");
    VQ_NEED("vqhip_col_multinomial_pick: ws too small", ws_bytes, w.total);
    col_multinomial_pick_kernel<<<(unsigned)((K + 255) / 256), 256, 0, (hipStream_t)stream>>>(w.mass, (int)w.blocks, K, w.colmax, u, w.sel,
                                                                                              w.resid, col_idx);
    VQ_CHECK_LAUNCH("col_multinomial_pick_kernel");
    return VQHIP_OK;
}

int vqhip_col_multinomial_resolve(const float *tile, int64_t r0, int64_t N, int64_t K, int64_t block_rows, void *ws, int64_t ws_bytes,
                                  int64_t *col_idx, void *stream) {
    const char *what = "vqhip_col_multinomial_resolve";
    VqColMultiWs w;
    int64_t r;
    if (int rc = col_multinomial_block(what, tile, r0, N, K, block_rows, ws, ws_bytes, &w, &r)) return rc;
    if (!col_idx) return fail(VQHIP_EINVAL, what, "null pointer");
    col_multinomial_resolve_kernel<<<(unsigned)((K + 63) / 64), 64, 0, (hipStream_t)stream>>>(tile, (int)r, K, (int)(r0 / block_rows), r0,
                                                                                              w.colmax, w.sel, w.resid, col_idx);
    VQ_CHECK_LAUNCH("col_multinomial_resolve_kernel");
    return VQHIP_OK;
}

}  // extern "C"
