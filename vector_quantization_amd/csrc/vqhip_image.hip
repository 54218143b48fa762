// libvqhip — the image and distillation losses: CosineEmbeddingLoss, the LPIPS tail, the reconstruction metrics.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "vqhip_host.h"
#include "vqhip_cosine_embed_kernels.h"
#include "vqhip_lpips_kernels.h"
#include "vqhip_image_metrics_kernels.h"

// ---- fused CosineEmbeddingLoss: the launches (vqhip_cosine_embed_kernels.h) -----------------------------------------------
template <int DP, int DT>
static int launch_cosine_embed_fwd(const VqCoseArgs &a, int layout, float *loss, float *stats, float *out, hipStream_t s) {
    if (layout == VQHIP_LAYOUT_ROWS) {
        cosine_embed_rows_fwd_kernel<DP, DT><<<(unsigned)((a.R + VQ_COSE_WAVES - 1) / VQ_COSE_WAVES), VQ_COSE_THREADS, 0, s>>>(a, loss, stats);
        VQ_CHECK_LAUNCH("cosine_embed_rows_fwd_kernel");
    } else {
        cosine_embed_map_fwd_kernel<DP, DT><<<(unsigned)((a.R + VQ_COSE_MAP_POS - 1) / VQ_COSE_MAP_POS), VQ_COSE_THREADS, 0, s>>>(a, loss, stats);
        VQ_CHECK_LAUNCH("cosine_embed_map_fwd_kernel");
    }
    cosine_embed_reduce_kernel<<<1, VQ_COSE_THREADS, 0, s>>>(loss, a.R, out);
    VQ_CHECK_LAUNCH("cosine_embed_reduce_kernel");
    return VQHIP_OK;
}

template <int DP, int DT>
static int launch_cosine_embed_bwd(const VqCoseArgs &a, int layout, const float *stats, const float *g, int g_per_row, int mean,
                                   void *grad, int64_t grad_stride, hipStream_t s) {
    if (layout == VQHIP_LAYOUT_ROWS) {
        cosine_embed_rows_bwd_kernel<DP, DT><<<(unsigned)((a.R + VQ_COSE_WAVES - 1) / VQ_COSE_WAVES), VQ_COSE_THREADS, 0, s>>>(
            a, stats, g, g_per_row, mean, grad, grad_stride);
        VQ_CHECK_LAUNCH("cosine_embed_rows_bwd_kernel");
    } else {
        cosine_embed_map_bwd_kernel<DP, DT><<<(unsigned)((a.R + VQ_COSE_MAP_POS - 1) / VQ_COSE_MAP_POS), VQ_COSE_THREADS, 0, s>>>(
            a, stats, g, g_per_row, mean, grad);
        VQ_CHECK_LAUNCH("cosine_embed_map_bwd_kernel");
    }
    return VQHIP_OK;
}

// ---- fused LPIPS tail: the launches (vqhip_lpips_kernels.h) ----------------------------------------------------------------
static unsigned lpips_grid(const VqLpipsArgs &a, int layout) {
    return layout == VQHIP_LAYOUT_ROWS ? (unsigned)((a.B * a.P + VQ_LPIPS_ROWS - 1) / VQ_LPIPS_ROWS) : (unsigned)(a.B * a.tiles);
}

template <int DP, int DT>
static int launch_lpips_fwd(const VqLpipsArgs &a, int layout, float *stats, float *value, int accumulate, hipStream_t s) {
    if (layout == VQHIP_LAYOUT_ROWS) {
        lpips_rows_fwd_kernel<DP, DT><<<lpips_grid(a, layout), VQ_LPIPS_THREADS, 0, s>>>(a, stats);
        VQ_CHECK_LAUNCH("lpips_rows_fwd_kernel");
    } else {
        lpips_map_fwd_kernel<DP, DT><<<lpips_grid(a, layout), VQ_LPIPS_THREADS, 0, s>>>(a, stats);
        VQ_CHECK_LAUNCH("lpips_map_fwd_kernel");
    }
    lpips_reduce_kernel<<<(unsigned)a.B, VQ_LPIPS_THREADS, 0, s>>>(stats, a.P, accumulate, value);
    VQ_CHECK_LAUNCH("lpips_reduce_kernel");
    return VQHIP_OK;
}

template <int DP, int DT>
static int launch_lpips_bwd(const VqLpipsArgs &a, int layout, const float *stats, const float *g_out, void *grad, hipStream_t s) {
    if (layout == VQHIP_LAYOUT_ROWS) {
        lpips_rows_bwd_kernel<DP, DT><<<lpips_grid(a, layout), VQ_LPIPS_THREADS, 0, s>>>(a, stats, g_out, grad);
        VQ_CHECK_LAUNCH("lpips_rows_bwd_kernel");
    } else {
        lpips_map_bwd_kernel<DP, DT><<<lpips_grid(a, layout), VQ_LPIPS_THREADS, 0, s>>>(a, stats, g_out, grad);
        VQ_CHECK_LAUNCH("lpips_map_bwd_kernel");
    }
    return VQHIP_OK;
}

extern "C" {

// ---- fused CosineEmbeddingLoss (vqhip_cosine_embed_kernels.h) --------------------------------------------------------------
// what the two entry points refuse alike, and the arguments the kernels share
static int cosine_embed_setup(const char *what, const void *pred, int pred_dtype, int pred_layout, int64_t pred_row_stride,
                              const void *target, int target_dtype, int64_t target_row_stride, int64_t B, int64_t P, int64_t C,
                              VqCoseArgs *a) {
    if (!pred || !target) return fail(VQHIP_EINVAL, what, "pred and target are required");
    if (!vq_float_dtype(pred_dtype) || !vq_float_dtype(target_dtype)) return fail(VQHIP_EINVAL, what, "dtype");
    if (!vq_dense_layout(pred_layout)) return fail(VQHIP_EINVAL, what, "pred_layout");
    const int64_t cap = 1ll << 31;
    if (B < 1 || P < 1 || B >= cap || P >= cap || B * P >= cap) return fail(VQHIP_EINVAL, what, "R = B * P must be in 1 .. 2^31 - 1");
    if (C < 1 || C > VQHIP_COSINE_EMBED_MAX_C) return fail(VQHIP_EINVAL, what, "C must be in 1 .. 2^16");
    if (target_row_stride < C || (pred_layout == VQHIP_LAYOUT_ROWS && pred_row_stride < C))
        return fail(VQHIP_EINVAL, what, "a row stride is below C");
    a->pred = pred; a->target = target;
    a->pred_stride = pred_row_stride; a->target_stride = target_row_stride;
    a->R = B * P; a->P = P; a->C = (int)C;
    return VQHIP_OK;
}

int vqhip_cosine_embed_fwd(const void *pred, int pred_dtype, int pred_layout, int64_t pred_row_stride, const void *target,
                           int target_dtype, int64_t target_row_stride, int64_t B, int64_t P, int64_t C, float *loss, float *stats,
                           float *out, void *stream) {
    VqCoseArgs a;
    if (int rc = cosine_embed_setup("vqhip_cosine_embed_fwd", pred, pred_dtype, pred_layout, pred_row_stride, target, target_dtype,
                                    target_row_stride, B, P, C, &a)) return rc;
    VQ_REQUIRE(loss && stats && out, "vqhip_cosine_embed_fwd: loss, stats and out are required");
    return vq_with_dtype(pred_dtype, [&](auto dp) { return vq_with_dtype(target_dtype, [&](auto dt) {
        return launch_cosine_embed_fwd<decltype(dp)::value, decltype(dt)::value>(a, pred_layout, loss, stats, out, (hipStream_t)stream);
    }); });
}

int vqhip_cosine_embed_bwd(const void *pred, int pred_dtype, int pred_layout, int64_t pred_row_stride, const void *target,
                           int target_dtype, int64_t target_row_stride, int64_t B, int64_t P, int64_t C, const float *stats,
                           const float *g, int g_per_row, int mean, void *grad, int64_t grad_row_stride, void *stream) {
    VqCoseArgs a;
    if (int rc = cosine_embed_setup("vqhip_cosine_embed_bwd", pred, pred_dtype, pred_layout, pred_row_stride, target, target_dtype,
                                    target_row_stride, B, P, C, &a)) return rc;
    VQ_REQUIRE(stats && g && grad, "vqhip_cosine_embed_bwd: stats, g and grad are required");
    VQ_REQUIRE(pred_layout != VQHIP_LAYOUT_ROWS || grad_row_stride >= C, "vqhip_cosine_embed_bwd: the row stride of grad is below C");
    return vq_with_dtype(pred_dtype, [&](auto dp) { return vq_with_dtype(target_dtype, [&](auto dt) {
        return launch_cosine_embed_bwd<decltype(dp)::value, decltype(dt)::value>(a, pred_layout, stats, g, g_per_row ? 1 : 0, mean ? 1 : 0, grad,
                                                                                 grad_row_stride, (hipStream_t)stream);
    }); });
}

// ---- fused LPIPS tail (vqhip_lpips_kernels.h) -------------------------------------------------------------------------------
// what the dropout of the three entry points refuses, and its threshold and scale
static int lpips_dropout(const char *what, const uint32_t *seed, float p, int64_t layer, VqLpipsArgs *a) {
    if (layer < 0 || layer > VQHIP_LPIPS_MAX_LAYER) return fail(VQHIP_EINVAL, what, "layer must be in 0 .. 2^16");
    a->seed = seed; a->layer = (uint32_t)layer; a->thr = 0u; a->scale = 1.0f;
    if (!seed) return VQHIP_OK;
    if (!(p >= 0.0f && p < 1.0f)) return fail(VQHIP_EINVAL, what, "p must be in [0, 1)");
    a->thr = (uint32_t)ceil((double)p * 4294967296.0);                          // p < 1 in fp32: at most 2^32 - 256
    a->scale = 1.0f / (1.0f - p);
    return VQHIP_OK;
}

static int lpips_sizes(const char *what, int64_t B, int64_t C, int64_t P, VqLpipsArgs *a) {
    const int64_t cap = 1ll << 31;
    if (B < 1 || P < 1 || B >= cap || P >= cap || B * P >= cap) return fail(VQHIP_EINVAL, what, "B * P must be in 1 .. 2^31 - 1");
    if (C < 1 || C > VQHIP_LPIPS_MAX_C) return fail(VQHIP_EINVAL, what, "C must be in 1 .. 2^16");
    a->B = B; a->P = P; a->C = (int)C;
    a->tiles = (P + VQ_LPIPS_MAP_POS - 1) / VQ_LPIPS_MAP_POS;
    if (B * a->tiles >= cap) return fail(VQHIP_EINVAL, what, "B * ceil(P / 64) must be below 2^31");
    return VQHIP_OK;
}

// what the forward and the backward refuse alike, and the arguments the kernels share
static int lpips_setup(const char *what, const void *pred, int pred_dtype, const void *target, int target_dtype, int layout, int64_t B,
                       int64_t C, int64_t P, const float *w, const uint32_t *seed, float p, int64_t layer, VqLpipsArgs *a) {
    if (!pred || !target || !w) return fail(VQHIP_EINVAL, what, "pred, target and w are required");
    if (!vq_float_dtype(pred_dtype) || !vq_float_dtype(target_dtype)) return fail(VQHIP_EINVAL, what, "dtype");
    if (!vq_dense_layout(layout)) return fail(VQHIP_EINVAL, what, "layout");
    if (int rc = lpips_sizes(what, B, C, P, a)) return rc;
    if (int rc = lpips_dropout(what, seed, p, layer, a)) return rc;
    a->pred = pred; a->target = target; a->w = w;
    return VQHIP_OK;
}

int vqhip_lpips_fwd(const void *pred, int pred_dtype, const void *target, int target_dtype, int layout, int64_t B, int64_t C,
                    int64_t P, const float *w, const uint32_t *seed, float p, int64_t layer, float *stats, float *value,
                    int accumulate, void *stream) {
    VqLpipsArgs a;
    if (int rc = lpips_setup("vqhip_lpips_fwd", pred, pred_dtype, target, target_dtype, layout, B, C, P, w, seed, p, layer, &a)) return rc;
    VQ_REQUIRE(stats && value, "vqhip_lpips_fwd: stats and value are required");
    return vq_with_dtype(pred_dtype, [&](auto dp) { return vq_with_dtype(target_dtype, [&](auto dt) {
        return launch_lpips_fwd<decltype(dp)::value, decltype(dt)::value>(a, layout, stats, value, accumulate ? 1 : 0, (hipStream_t)stream);
    }); });
}

int vqhip_lpips_bwd(const void *pred, int pred_dtype, const void *target, int target_dtype, int layout, int64_t B, int64_t C,
                    int64_t P, const float *w, const uint32_t *seed, float p, int64_t layer, const float *stats, const float *g_out,
                    void *grad, void *stream) {
    VqLpipsArgs a;
    if (int rc = lpips_setup("vqhip_lpips_bwd", pred, pred_dtype, target, target_dtype, layout, B, C, P, w, seed, p, layer, &a)) return rc;
    VQ_REQUIRE(stats && g_out && grad, "vqhip_lpips_bwd: stats, g_out and grad are required");
    return vq_with_dtype(pred_dtype, [&](auto dp) { return vq_with_dtype(target_dtype, [&](auto dt) {
        return launch_lpips_bwd<decltype(dp)::value, decltype(dt)::value>(a, layout, stats, g_out, grad, (hipStream_t)stream);
    }); });
}

int vqhip_lpips_keep_mask(const uint32_t *seed, float p, int64_t layer, int64_t B, int64_t C, int64_t P, uint8_t *out, void *stream) {
    const char *what = "vqhip_lpips_keep_mask";
    VqLpipsArgs a;
    if (!seed || !out) return fail(VQHIP_EINVAL, what, "seed and out are required");
    if (int rc = lpips_sizes(what, B, C, P, &a)) return rc;
    if (int rc = lpips_dropout(what, seed, p, layer, &a)) return rc;
    const int64_t n = B * C * P;                                                // below 2^47
    const int64_t blocks = (n + VQ_LPIPS_THREADS - 1) / VQ_LPIPS_THREADS;
    lpips_keep_mask_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), VQ_LPIPS_THREADS, 0, (hipStream_t)stream>>>(seed, a.layer, a.thr, n, out);
    VQ_CHECK_LAUNCH("lpips_keep_mask_kernel");
    return VQHIP_OK;
}

// ---- fused reconstruction metrics (vqhip_image_metrics_kernels.h) ---------------------------------------------------------
// what both entry points refuse; on success the number of workgroups of the first launch and the tiles along each axis
static int image_metrics_grid(const char *what, int64_t B, int64_t C, int64_t H, int64_t W, int64_t *groups, int64_t *tiles_x, int64_t *tiles_y) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || H > (1ll << 30) || W > (1ll << 30)) return fail(VQHIP_EINVAL, what, "need B, C >= 1 and 1 <= H, W <= 2^30");
    *tiles_x = (W + VQ_IM_T - 1) / VQ_IM_T;
    *tiles_y = (H + VQ_IM_T - 1) / VQ_IM_T;
    const int64_t tiles = *tiles_x * *tiles_y;                                 // below 2^50
    const int64_t cap = 1ll << 31;
    if (tiles >= cap || C >= cap || B >= cap || tiles * C >= cap || tiles * C * B >= cap) return fail(VQHIP_EINVAL, what, "B * C * tiles must be below 2^31");
    // C * H * W <= 1024 * tiles * C < 2^41: no overflow; below 2^37 the divisors 255 n and 65025 n are exact doubles
    if (C * H * W >= (1ll << 37)) return fail(VQHIP_EINVAL, what, "C * H * W must be below 2^37");
    *groups = tiles * C * B;
    return VQHIP_OK;
}

int64_t vqhip_image_metrics_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
    int64_t groups, tx, ty;
    if (image_metrics_grid("vqhip_image_metrics_workspace_bytes", B, C, H, W, &groups, &tx, &ty)) return 0;
    return groups * VQ_IM_SLOT * (int64_t)sizeof(long long);
}

static int image_metrics_side(const char *what, const void *p, int dtype, int layout, int64_t C, int64_t H, int64_t W, VqImSide *s) {
    if (!p) return fail(VQHIP_EINVAL, what, "pred and image are required");
    if (!vq_float_dtype(dtype) && dtype != VQHIP_DTYPE_U8) return fail(VQHIP_EINVAL, what, "dtype");
    if (layout != VQHIP_IMAGE_NCHW && layout != VQHIP_IMAGE_NHWC) return fail(VQHIP_EINVAL, what, "layout");
    s->p = p; s->dtype = dtype; s->sb = C * H * W;
    if (layout == VQHIP_IMAGE_NCHW) { s->sc = H * W; s->sy = W; s->sx = 1; }
    else { s->sc = 1; s->sy = W * C; s->sx = C; }
    return VQHIP_OK;
}

int vqhip_image_metrics(const void *pred, int pred_dtype, int pred_layout, const void *image, int image_dtype, int image_layout,
                        int64_t B, int64_t C, int64_t H, int64_t W, int want_ssim, double c1, double c2, void *ws, int64_t ws_bytes,
                        double *values64, float *values32, int64_t *sums, void *stream) {
    const char *what = "vqhip_image_metrics";
    int64_t groups, tiles_x, tiles_y;
    if (int rc = image_metrics_grid(what, B, C, H, W, &groups, &tiles_x, &tiles_y)) return rc;
    VqImArgs a;
    if (int rc = image_metrics_side(what, pred, pred_dtype, pred_layout, C, H, W, &a.a)) return rc;
    if (int rc = image_metrics_side(what, image, image_dtype, image_layout, C, H, W, &a.b)) return rc;
    VQ_REQUIRE(ws && values64 && values32 && sums, "vqhip_image_metrics: ws, values64, values32 and sums are required");
    int64_t windows = 0;
    if (want_ssim) {
        VQ_REQUIRE(H >= 7 && W >= 7, "vqhip_image_metrics: SSIM needs H >= 7 and W >= 7 (a 7 x 7 window)");
        windows = C * (H - 6) * (W - 6);                                       // C, H, W checked above: no overflow
        VQ_REQUIRE(windows <= VQHIP_IMAGE_SSIM_MAX_WINDOWS, "vqhip_image_metrics: C * (H - 6) * (W - 6) is beyond 2^22 windows");
        VQ_REQUIRE(c1 > 0.0 && c2 > 0.0, "vqhip_image_metrics: c1 and c2 must be positive");
    }
    VQ_NEED("vqhip_image_metrics: ws too small", ws_bytes, groups * VQ_IM_SLOT * (int64_t)sizeof(long long));
    a.C = (int)C; a.H = (int)H; a.W = (int)W; a.tiles_x = (int)tiles_x; a.tiles_y = (int)tiles_y;
    a.want_ssim = want_ssim ? 1 : 0; a.c1 = c1; a.c2 = c2;
    hipStream_t s = (hipStream_t)stream;
    image_metrics_tile_kernel<<<(unsigned)groups, VQ_IM_THREADS, 0, s>>>(a, (long long *)ws);
    VQ_CHECK_LAUNCH("image_metrics_tile_kernel");
    image_metrics_finish_kernel<<<1, VQ_IM_THREADS, 0, s>>>((const long long *)ws, B, groups / B, (double)(C * H * W), (double)windows,
                                                            a.want_ssim, values64, values32, (long long *)sums);
    VQ_CHECK_LAUNCH("image_metrics_finish_kernel");
    return VQHIP_OK;
}

}  // extern "C"
