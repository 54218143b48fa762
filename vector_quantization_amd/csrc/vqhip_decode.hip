// libvqhip — what surrounds the argmin of a quantizer step: gather / straight-through / MSE decode, histograms, row norms and
// F.normalize with its backward, the element-wise autograd pieces, the fused VQ backward, transposes and the codebook metrics.
// gfx950 only.  Kernels: vqhip_decode_kernels.h.
#include "vqhip.h"

#include <hip/hip_runtime.h>

#include "vqhip_core.h"
#include "vqhip_decode_kernels.h"

// |v|^2 / F.normalize for rows of at most 32 elements (row_small_kernel)
template <bool NORMALIZE>
static int launch_row_small(const void *v, int dtype, int64_t R, int D, float eps, float *out, hipStream_t s) {
    const int L = vq_small_lanes(D);
    const int grid = waves_grid((R + 64 / L - 1) / (64 / L), 4);
#define VQ_ROW_SMALL(DT, LL) row_small_kernel<DT, LL, NORMALIZE><<<grid, 256, 0, s>>>(v, R, D, eps, out)
    if (dtype == VQHIP_DTYPE_F32) { if (L == 8) VQ_ROW_SMALL(0, 8); else if (L == 16) VQ_ROW_SMALL(0, 16); else VQ_ROW_SMALL(0, 32); }
    else { if (L == 8) VQ_ROW_SMALL(1, 8); else if (L == 16) VQ_ROW_SMALL(1, 16); else VQ_ROW_SMALL(1, 32); }
#undef VQ_ROW_SMALL
    VQ_CHECK_LAUNCH("row_small_kernel");
    return VQHIP_OK;
}

// hist[K] += bincount(idx) for int64 (hist_kernel, hist_lds_kernel) or int32 tokens (their _i32 twins)
template <typename IdxT>
static int launch_hist(const IdxT *idx, int64_t N, int64_t K, int32_t *hist, void *stream) {
    constexpr bool i64 = sizeof(IdxT) == 8;
    VQ_REQUIRE(idx && hist && N >= 0 && K > 0, i64 ? "vqhip_hist: bad argument" : "vqhip_hist_i32: bad argument");
    if (N == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (K <= 32768 && N >= 16384) {            // enough tokens per block that the K-bin flush pays: at most 256 blocks, >= 2048 tokens each
        static LdsCache lds_set;
        if (int rc = ensure_dyn_lds(i64 ? (const void *)hist_lds_kernel : (const void *)hist_i32_lds_kernel, (size_t)K * 4, lds_set)) return rc;
        int grid = (int)((N + 2047) / 2048); grid = grid > 256 ? 256 : grid;
        if constexpr (i64) hist_lds_kernel<<<grid, 1024, (size_t)K * 4, s>>>(idx, N, (int)K, hist);
        else hist_i32_lds_kernel<<<grid, 1024, (size_t)K * 4, s>>>(idx, N, (int)K, hist);
    } else {
        int grid = (int)((N + 255) / 256); grid = grid > 2048 ? 2048 : grid;
        if constexpr (i64) hist_kernel<<<grid, 256, 0, s>>>(idx, N, K, hist);
        else hist_i32_kernel<<<grid, 256, 0, s>>>(idx, N, K, hist);
    }
    VQ_CHECK_LAUNCH(i64 ? "hist_kernel" : "hist_i32_kernel");
    return VQHIP_OK;
}

extern "C" {

int vqhip_row_sqnorm(const void *v, int dtype, int64_t R, int D, float *out, void *stream) {
    if (!v || !out || D <= 0 || R < 0) return fail(VQHIP_EINVAL, "vqhip_row_sqnorm: bad argument");
    if (R == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (D <= 32 && (dtype == VQHIP_DTYPE_F32 || dtype == VQHIP_DTYPE_BF16)) return launch_row_small<false>(v, dtype, R, D, 0.0f, out, s);
    if (dtype == VQHIP_DTYPE_F32) row_sqnorm_kernel<0><<<waves_grid(R, 4), 256, 0, s>>>(v, R, D, out);
    else if (dtype == VQHIP_DTYPE_BF16) row_sqnorm_kernel<1><<<waves_grid(R, 4), 256, 0, s>>>(v, R, D, out);
    else return fail(VQHIP_EINVAL, "vqhip_row_sqnorm: dtype");
    VQ_CHECK_LAUNCH("row_sqnorm_kernel");
    return VQHIP_OK;
}

int vqhip_normalize_rows(const void *v, int dtype, int64_t R, int D, float eps, float *out, void *stream) {
    if (!v || !out || D <= 0 || R < 0) return fail(VQHIP_EINVAL, "vqhip_normalize_rows: bad argument");
    if (R == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (D <= 32 && (dtype == VQHIP_DTYPE_F32 || dtype == VQHIP_DTYPE_BF16)) return launch_row_small<true>(v, dtype, R, D, eps, out, s);
    if (dtype == VQHIP_DTYPE_F32) normalize_rows_kernel<0><<<waves_grid(R, 4), 256, 0, s>>>(v, R, D, eps, out);
    else if (dtype == VQHIP_DTYPE_BF16) normalize_rows_kernel<1><<<waves_grid(R, 4), 256, 0, s>>>(v, R, D, eps, out);
    else return fail(VQHIP_EINVAL, "vqhip_normalize_rows: dtype");
    VQ_CHECK_LAUNCH("normalize_rows_kernel");
    return VQHIP_OK;
}

static int gather_ste_impl(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D, float *z,
                           float *z_ste, double *sse, float *mse, void *stream, float beta = 0.0f);

int vqhip_gather_ste_loss(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D, float *z,
                          float *z_ste, double *sse, void *stream) {
    if (!x || !e || !idx || N < 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_gather_ste_loss: bad argument");
    return gather_ste_impl(x, x_dtype, e, idx, N, D, z, z_ste, sse, nullptr, stream);
}

int vqhip_gather_ste_mse(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D, float *z,
                         float *z_ste, float *mse, float beta, void *scratch16, void *stream) {
    if (!x || !e || !idx || !mse || !scratch16 || N <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_gather_ste_mse: bad argument");
    return gather_ste_impl(x, x_dtype, e, idx, N, D, z, z_ste, (double *)scratch16, mse, stream, beta);
}

int vqhip_gather_ste_map(const void *x_rows, int x_dtype, const float *e, const int64_t *idx, int64_t B, int64_t HW, int D,
                         float *out_map, float *mse, float beta, void *scratch16, void *stream) {
    const int64_t N = B * HW;
    if (!e || !idx || !out_map || B <= 0 || HW <= 0 || D <= 0 || (x_rows && (!mse || !scratch16)))
        return fail(VQHIP_EINVAL, "vqhip_gather_ste_map: bad argument");
    hipStream_t s = (hipStream_t)stream;
    double *sse = x_rows ? (double *)scratch16 : nullptr;
    VQ_REQUIRE(!x_rows || vq_row_dtype(x_dtype), "vqhip_gather_ste_map: x_dtype");
    if (HW % 256 == 0 && D % 32 == 0) {
        // images of a multiple of 256 positions: whole 1 KiB channel rows per wave-store (gather_ste_map256_kernel)
        const int64_t nt = N / 256;
        int csplit = 1;                                     // share the channels while that still leaves whole chunks and the grid is short
        while (nt * csplit < 512 && (D / 32) % (csplit * 2) == 0) csplit *= 2;
        const int64_t items = nt * csplit;
        const int grid256 = (int)(items < 1024 ? items : 1024);
        constexpr int LDS = 2 * 32 * 256 * 4;
        static LdsCache sets[2];
        const int bf = (x_rows && x_dtype == VQHIP_DTYPE_BF16) ? 1 : 0;
        if (int rc = ensure_dyn_lds(bf ? (const void *)gather_ste_map256_kernel<1> : (const void *)gather_ste_map256_kernel<0>, LDS, sets[bf])) return rc;
        if (!bf) gather_ste_map256_kernel<0><<<grid256, 512, LDS, s>>>(x_rows, e, idx, N, D, HW, csplit, out_map, sse, mse, beta);
        else gather_ste_map256_kernel<1><<<grid256, 512, LDS, s>>>(x_rows, e, idx, N, D, HW, csplit, out_map, sse, mse, beta);
        VQ_CHECK_LAUNCH("gather_ste_map256_kernel");
        return VQHIP_OK;
    }
    int64_t ntiles = (N + 63) / 64;
    const int grid = (int)(ntiles < 2048 ? ntiles : 2048);
    if (!x_rows || x_dtype == VQHIP_DTYPE_F32) gather_ste_map_kernel<0><<<grid, 256, 0, s>>>(x_rows, e, idx, N, D, HW, out_map, sse, mse, beta);
    else if (x_dtype == VQHIP_DTYPE_BF16) gather_ste_map_kernel<1><<<grid, 256, 0, s>>>(x_rows, e, idx, N, D, HW, out_map, sse, mse, beta);
    else return fail(VQHIP_EINVAL, "vqhip_gather_ste_map: x_dtype");
    VQ_CHECK_LAUNCH("gather_ste_map_kernel");
    return VQHIP_OK;
}

static int gather_ste_impl(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D, float *z,
                           float *z_ste, double *sse, float *mse, void *stream, float beta) {
    if (N == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    // outputs beyond the Infinity Cache (256 MiB) are streamed: non-temporal accesses and twice the waves in flight
    const int64_t out_bytes = (int64_t)N * D * 4 * ((z ? 1 : 0) + (z_ste ? 1 : 0));
    const bool streamed = out_bytes > (192ll << 20);
    int cap = streamed ? 512 : 256;                                    // blocks of 16 waves
    int grid = (int)((N + 15) / 16);
    grid = grid > cap ? cap : grid;
#define VQ_GATHER(DT, NT) gather_ste_loss_kernel<DT, NT><<<grid, 1024, 0, s>>>(x, e, idx, N, D, z, z_ste, sse, mse, beta)
    if (x_dtype == VQHIP_DTYPE_F32) { if (streamed) VQ_GATHER(0, 1); else VQ_GATHER(0, 0); }
    else if (x_dtype == VQHIP_DTYPE_BF16) { if (streamed) VQ_GATHER(1, 1); else VQ_GATHER(1, 0); }
    else return fail(VQHIP_EINVAL, "vqhip_gather_ste_loss: x_dtype");
#undef VQ_GATHER
    VQ_CHECK_LAUNCH("gather_ste_loss_kernel");
    return VQHIP_OK;
}

int vqhip_hist(const int64_t *idx, int64_t N, int64_t K, int32_t *hist, void *stream) { return launch_hist(idx, N, K, hist, stream); }
int vqhip_hist_i32(const int32_t *idx, int64_t N, int64_t K, int32_t *hist, void *stream) { return launch_hist(idx, N, K, hist, stream); }

int vqhip_diff(const void *a, int a_dtype, const void *b, int b_dtype, int64_t n, float scale, const float *scale_dev,
               float *out, double *sse, void *stream) {
    if (!a || !b || n < 0 || (!out && !sse)) return fail(VQHIP_EINVAL, "vqhip_diff: bad argument");
    if (n == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    int grid = (int)((n + 255) / 256); grid = grid > 2048 ? 2048 : grid;
    if (a_dtype == 0 && b_dtype == 0) diff_kernel<0, 0><<<grid, 256, 0, s>>>(a, b, n, scale, scale_dev, out, sse);
    else if (a_dtype == 0 && b_dtype == 1) diff_kernel<0, 1><<<grid, 256, 0, s>>>(a, b, n, scale, scale_dev, out, sse);
    else if (a_dtype == 1 && b_dtype == 0) diff_kernel<1, 0><<<grid, 256, 0, s>>>(a, b, n, scale, scale_dev, out, sse);
    else if (a_dtype == 1 && b_dtype == 1) diff_kernel<1, 1><<<grid, 256, 0, s>>>(a, b, n, scale, scale_dev, out, sse);
    else return fail(VQHIP_EINVAL, "vqhip_diff: dtype");
    VQ_CHECK_LAUNCH("diff_kernel");
    return VQHIP_OK;
}

int vqhip_vq_backward(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D, const float *g_zste,
                      const float *g_cb, const float *g_cm, float *grad_x, float *grad_w, void *stream) {
    return vqhip_vq_backward_ex(x, x_dtype, e, idx, N, D, g_zste, g_cb, g_cm, nullptr, 0.0f, grad_x, grad_w, stream);
}

int vqhip_vq_backward_ex(const void *x, int x_dtype, const float *e, const int64_t *idx, int64_t N, int D, const float *g_zste,
                         const float *g_cb, const float *g_cm, const float *g_comb, float beta, float *grad_x, float *grad_w,
                         void *stream) {
    if (!x || !e || !idx || N < 0 || D <= 0 || (!grad_x && !grad_w)) return fail(VQHIP_EINVAL, "vqhip_vq_backward: bad argument");
    if (N == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    int grid = (int)((N + 3) / 4); grid = grid > 2048 ? 2048 : grid;
    if (x_dtype == VQHIP_DTYPE_F32)
        vq_backward_kernel<0><<<grid, 256, 0, s>>>(x, e, idx, N, D, g_zste, g_cb, g_cm, grad_x, grad_w, g_comb, beta);
    else if (x_dtype == VQHIP_DTYPE_BF16)
        vq_backward_kernel<1><<<grid, 256, 0, s>>>(x, e, idx, N, D, g_zste, g_cb, g_cm, grad_x, grad_w, g_comb, beta);
    else return fail(VQHIP_EINVAL, "vqhip_vq_backward: x_dtype");
    VQ_CHECK_LAUNCH("vq_backward_kernel");
    return VQHIP_OK;
}

int vqhip_ste(const void *x, int x_dtype, const float *z, int64_t n, float *out, void *stream) {
    if (!x || !z || !out || n < 0) return fail(VQHIP_EINVAL, "vqhip_ste: bad argument");
    if (n == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    int grid = (int)((n + 255) / 256); grid = grid > 4096 ? 4096 : grid;
    if (x_dtype == VQHIP_DTYPE_F32) ste_kernel<0><<<grid, 256, 0, s>>>(x, z, n, out);
    else if (x_dtype == VQHIP_DTYPE_BF16) ste_kernel<1><<<grid, 256, 0, s>>>(x, z, n, out);
    else return fail(VQHIP_EINVAL, "vqhip_ste: dtype");
    VQ_CHECK_LAUNCH("ste_kernel");
    return VQHIP_OK;
}

int vqhip_normalize_rows_bwd(const void *v, int dtype, const float *g, int64_t R, int D, float eps, float *gv, void *stream) {
    if (!v || !g || !gv || R < 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_normalize_rows_bwd: bad argument");
    if (R == 0) return VQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VQHIP_DTYPE_F32) normalize_bwd_kernel<0><<<waves_grid(R, 4), 256, 0, s>>>(v, g, R, D, eps, gv);
    else if (dtype == VQHIP_DTYPE_BF16) normalize_bwd_kernel<1><<<waves_grid(R, 4), 256, 0, s>>>(v, g, R, D, eps, gv);
    else return fail(VQHIP_EINVAL, "vqhip_normalize_rows_bwd: dtype");
    VQ_CHECK_LAUNCH("normalize_bwd_kernel");
    return VQHIP_OK;
}

int vqhip_transpose(const void *in, void *out, int elem_bytes, int64_t B, int R, int C, void *stream) {
    if (!in || !out || B < 0 || R <= 0 || C <= 0 || (elem_bytes != 2 && elem_bytes != 4))
        return fail(VQHIP_EINVAL, "vqhip_transpose: bad argument");
    if (B == 0) return VQHIP_OK;
    if (B > 65535) return fail(VQHIP_EINVAL, "vqhip_transpose: batch too large for one launch");
    dim3 grid((C + 63) / 64, (R + 63) / 64, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (elem_bytes == 4) transpose_kernel<uint32_t><<<grid, 256, 0, s>>>((const uint32_t *)in, (uint32_t *)out, B, R, C);
    else transpose_kernel<uint16_t><<<grid, 256, 0, s>>>((const uint16_t *)in, (uint16_t *)out, B, R, C);
    VQ_CHECK_LAUNCH("transpose_kernel");
    return VQHIP_OK;
}

int vqhip_codebook_metrics(const int64_t *counts, int64_t K, double *out, void *stream) {
    if (!counts || !out || K <= 0) return fail(VQHIP_EINVAL, "vqhip_codebook_metrics: bad argument");
    codebook_metrics_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(counts, K, out);
    VQ_CHECK_LAUNCH("codebook_metrics_kernel");
    return VQHIP_OK;
}

}  // extern "C"
