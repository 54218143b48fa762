// libvqhip — FiniteScalarQuantizer and the pooled code features (which share FSQ's constants).  gfx950 only.
// Kernels: vqhip_fsq_kernels.h, vqhip_pool_kernels.h.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "vqhip_core.h"
#include "vqhip_pool_kernels.h"
#include "vqhip_fsq_kernels.h"

extern "C" {

// ---- FiniteScalarQuantizer ----------------------------------------------------------------------------------------------
// Validates the caller's constants and the shape, and turns them into the kernels' by-value argument.  Every refusal names
// the entry point (`what`).
static int fsq_setup(const char *what, const vqhip_fsq_t *q, int layout, int64_t N, int64_t HW, VqFsqConsts *k, int *grid) {
    char msg[160];
    if (!q) return fail(VQHIP_EINVAL, what, "null constants");
    if (q->struct_bytes != (int64_t)sizeof(vqhip_fsq_t)) return fail(VQHIP_EINVAL, what, "struct_bytes != sizeof(vqhip_fsq_t)");
    if (q->C < 1 || q->C > VQHIP_FSQ_MAX_C) {
        snprintf(msg, sizeof(msg), "C = %d outside 1..%d", q->C, VQHIP_FSQ_MAX_C);
        return fail(VQHIP_EINVAL, what, msg);
    }
    if (layout != VQHIP_LAYOUT_ROWS && layout != VQHIP_LAYOUT_MAP) return fail(VQHIP_EINVAL, what, "unknown layout");
    if (N < 0 || N >= (1ll << 31)) return fail(VQHIP_EINVAL, what, "N outside 0 .. 2^31 - 1");
    if (layout == VQHIP_LAYOUT_MAP && (HW < 1 || HW >= (1ll << 31) || N % HW != 0))
        return fail(VQHIP_EINVAL, what, "the map needs HW >= 1 and N % HW == 0");
    memset(k, 0, sizeof(*k));
    k->C = q->C;
    int64_t cum = 1;
    for (int i = 0; i < q->C; ++i) {
        const int L = q->levels[i];
        if (L < 3) {
            snprintf(msg, sizeof(msg), "level %d of channel %d < 3 (2 gives NaN, 1 divides by zero)", L, i);
            return fail(VQHIP_EINVAL, what, msg);
        }
        if (cum * L > (1ll << 24)) return fail(VQHIP_EINVAL, what, "prod(levels) > 2^24 (the fp32 digit sum would not be exact)");
        k->level[i] = L;
        k->cum[i] = (int)cum;
        k->cumf[i] = (float)cum;
        k->half[i] = (float)(L / 2);
        k->rhalf[i] = ((L / 2) & (L / 2 - 1)) == 0 ? 1.0f / (float)(L / 2) : 0.f;
        k->odd[i] = (float)((L - 1) % 2);
        k->shift[i] = q->shift[i];
        k->scale[i] = q->scale[i];
        cum *= L;
    }
    k->K = (int)cum;
    *grid = (int)((N + VQ_FSQ_TILE - 1) / VQ_FSQ_TILE);
    return VQHIP_OK;
}

static inline int fsq_aligned(const void *p, int flag) { return ((uintptr_t)p % 16 == 0) ? flag : 0; }

int vqhip_fsq_encode(const vqhip_fsq_t *q, const void *x, int x_dtype, int layout, int64_t N, int64_t HW, int32_t *quant,
                     float *z, int z_rows, void *x_rows, int32_t *hist, void *stream) {
    const char *what = "vqhip_fsq_encode";
    VqFsqConsts k;
    int grid = 0;
    if (int rc = fsq_setup(what, q, layout, N, HW, &k, &grid)) return rc;
    if (!x || !quant) return fail(VQHIP_EINVAL, what, "x and quant are required");
    if (!vq_row_dtype(x_dtype)) return fail(VQHIP_EINVAL, what, "x_dtype");
    if (x_rows && layout != VQHIP_LAYOUT_MAP) return fail(VQHIP_EINVAL, what, "x_rows is a by-product of the map layout");
    if (N == 0) return VQHIP_OK;
    const int vec = fsq_aligned(x, VQ_FSQ_VEC_X) | fsq_aligned(z, VQ_FSQ_VEC_Z) | fsq_aligned(x_rows, VQ_FSQ_VEC_ROWS);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)N, hw = (int)(layout == VQHIP_LAYOUT_MAP ? HW : 0);
#define VQ_FSQ_ENC(DT, MAP) fsq_encode_kernel<DT, MAP><<<grid, VQ_FSQ_TILE, 0, s>>>(k, x, n, hw, quant, z, z_rows, x_rows, hist, vec)
    if (layout == VQHIP_LAYOUT_ROWS) { if (x_dtype == VQHIP_DTYPE_F32) VQ_FSQ_ENC(0, false); else VQ_FSQ_ENC(1, false); }
    else { if (x_dtype == VQHIP_DTYPE_F32) VQ_FSQ_ENC(0, true); else VQ_FSQ_ENC(1, true); }
#undef VQ_FSQ_ENC
    VQ_CHECK_LAUNCH("fsq_encode_kernel");
    return VQHIP_OK;
}

int vqhip_fsq_backward(const vqhip_fsq_t *q, const void *x, int x_dtype, int layout, int64_t N, int64_t HW, const float *g,
                       void *grad_x, void *stream) {
    const char *what = "vqhip_fsq_backward";
    VqFsqConsts k;
    int grid = 0;
    if (int rc = fsq_setup(what, q, layout, N, HW, &k, &grid)) return rc;
    if (!x || !g || !grad_x) return fail(VQHIP_EINVAL, what, "x, g and grad_x are required");
    if (!vq_row_dtype(x_dtype)) return fail(VQHIP_EINVAL, what, "x_dtype");
    if (N == 0) return VQHIP_OK;
    const int vec = fsq_aligned(x, VQ_FSQ_VEC_X) | fsq_aligned(grad_x, VQ_FSQ_VEC_Z) | fsq_aligned(g, VQ_FSQ_VEC_G);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)N, hw = (int)(layout == VQHIP_LAYOUT_MAP ? HW : 0);
#define VQ_FSQ_BWD(DT, MAP) fsq_backward_kernel<DT, MAP><<<grid, VQ_FSQ_TILE, 0, s>>>(k, x, g, n, hw, grad_x, vec)
    if (layout == VQHIP_LAYOUT_ROWS) { if (x_dtype == VQHIP_DTYPE_F32) VQ_FSQ_BWD(0, false); else VQ_FSQ_BWD(1, false); }
    else { if (x_dtype == VQHIP_DTYPE_F32) VQ_FSQ_BWD(0, true); else VQ_FSQ_BWD(1, true); }
#undef VQ_FSQ_BWD
    VQ_CHECK_LAUNCH("fsq_backward_kernel");
    return VQHIP_OK;
}

int vqhip_fsq_decode(const vqhip_fsq_t *q, const void *quant, int quant_dtype, int layout, int64_t N, int64_t HW, float *z,
                     void *stream) {
    const char *what = "vqhip_fsq_decode";
    VqFsqConsts k;
    int grid = 0;
    if (int rc = fsq_setup(what, q, layout, N, HW, &k, &grid)) return rc;
    if (!quant || !z) return fail(VQHIP_EINVAL, what, "quant and z are required");
    if (quant_dtype != VQHIP_DTYPE_I32 && quant_dtype != VQHIP_DTYPE_I64) return fail(VQHIP_EINVAL, what, "quant_dtype");
    if (N == 0) return VQHIP_OK;
    const int vec = fsq_aligned(z, VQ_FSQ_VEC_Z);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)N, hw = (int)(layout == VQHIP_LAYOUT_MAP ? HW : 0);
#define VQ_FSQ_DEC(I64, MAP) fsq_decode_kernel<I64, MAP><<<grid, VQ_FSQ_TILE, 0, s>>>(k, quant, n, hw, z, vec)
    if (layout == VQHIP_LAYOUT_ROWS) { if (quant_dtype == VQHIP_DTYPE_I64) VQ_FSQ_DEC(true, false); else VQ_FSQ_DEC(false, false); }
    else { if (quant_dtype == VQHIP_DTYPE_I64) VQ_FSQ_DEC(true, true); else VQ_FSQ_DEC(false, true); }
#undef VQ_FSQ_DEC
    VQ_CHECK_LAUNCH("fsq_decode_kernel");
    return VQHIP_OK;
}

// ---- pooled code features (vqhip_pool_kernels.h) -----------------------------------------------------------------------
// what the three entry points refuse alike: B, HW >= 1 and B * HW < 2^31 (tokens are counted in 32 bits), a token dtype
static int pool_check(const char *what, int quant_dtype, int64_t B, int64_t HW) {
    if (B < 1 || HW < 1) return fail(VQHIP_EINVAL, what, "B and HW must be >= 1");
    if (B >= (1ll << 31) || HW >= (1ll << 31) || !vq_fits_i31(B * HW, 0)) return fail(VQHIP_EINVAL, what, "B * HW must be below 2^31");
    if (quant_dtype != VQHIP_DTYPE_I32 && quant_dtype != VQHIP_DTYPE_I64) return fail(VQHIP_EINVAL, what, "quant_dtype");
    return VQHIP_OK;
}

static inline int pool_log2_ceil(int64_t v, int cap_log2) {
    int l = 0;
    while (l < cap_log2 && (1ll << l) < v) ++l;
    return l;
}

int vqhip_decode_pool(const float *e, int64_t K, int D, const void *quant, int quant_dtype, int64_t B, int64_t HW, float *out,
                      void *stream) {
    const char *what = "vqhip_decode_pool";
    VQ_REQUIRE(e && quant && out, "vqhip_decode_pool: e, quant and out are required");
    VQ_REQUIRE(K >= 1 && D >= 1, "vqhip_decode_pool: K and D must be >= 1");
    if (int rc = pool_check(what, quant_dtype, B, HW)) return rc;
    // 16-byte columns where every row and the output row start aligned; else channel by channel
    const bool vec = D % 4 == 0 && (uintptr_t)e % 16 == 0 && (uintptr_t)out % 16 == 0;
    const int64_t cols = vec ? D / 4 : D;
    const int cw_log2 = pool_log2_ceil(cols, 6);
    const int64_t nchunks = (cols + (1ll << cw_log2) - 1) >> cw_log2;
    const int group_threads = VQ_POOL_PARTIALS << cw_log2;
    const int block = group_threads > 256 ? group_threads : 256;
    const int64_t per_block = block / group_threads;
    const int64_t grid = (B * nchunks + per_block - 1) / per_block;          // (B < 2^31, nchunks < 2^31: no overflow)
    VQ_REQUIRE(grid < (1ll << 31), "vqhip_decode_pool: B * ceil(D / 256) is beyond one launch");
    hipStream_t s = (hipStream_t)stream;
#define VQ_POOL(I64, VEC) decode_pool_kernel<I64, VEC><<<(unsigned)grid, block, 0, s>>>(e, K, D, quant, B, (int)HW, cw_log2, (int)nchunks, out)
    if (quant_dtype == VQHIP_DTYPE_I64) { if (vec) VQ_POOL(true, true); else VQ_POOL(true, false); }
    else { if (vec) VQ_POOL(false, true); else VQ_POOL(false, false); }
#undef VQ_POOL
    VQ_CHECK_LAUNCH("decode_pool_kernel");
    return VQHIP_OK;
}

int vqhip_decode_pool_bwd(const float *g, const void *quant, int quant_dtype, int64_t B, int64_t HW, int64_t K, int D,
                          float *grad_e, void *stream) {
    const char *what = "vqhip_decode_pool_bwd";
    VQ_REQUIRE(g && quant && grad_e, "vqhip_decode_pool_bwd: g, quant and grad_e are required");
    VQ_REQUIRE(K >= 1 && D >= 1, "vqhip_decode_pool_bwd: K and D must be >= 1");
    if (int rc = pool_check(what, quant_dtype, B, HW)) return rc;
    const int64_t N = B * HW;
    const int lp_log2 = pool_log2_ceil(D, 6);
    const int64_t grid = ((N << lp_log2) + 255) / 256;                       // N < 2^31, at most 64 lanes each
    VQ_REQUIRE(grid < (1ll << 31), "vqhip_decode_pool_bwd: B * HW is beyond one launch");
    hipStream_t s = (hipStream_t)stream;
    if (quant_dtype == VQHIP_DTYPE_I64) decode_pool_bwd_kernel<true><<<(unsigned)grid, 256, 0, s>>>(g, quant, N, (int)HW, K, D, lp_log2, grad_e);
    else decode_pool_bwd_kernel<false><<<(unsigned)grid, 256, 0, s>>>(g, quant, N, (int)HW, K, D, lp_log2, grad_e);
    VQ_CHECK_LAUNCH("decode_pool_bwd_kernel");
    return VQHIP_OK;
}

int vqhip_fsq_decode_pool(const vqhip_fsq_t *q, const void *quant, int quant_dtype, int64_t B, int64_t HW, float *out, void *stream) {
    const char *what = "vqhip_fsq_decode_pool";
    VQ_REQUIRE(q && quant && out, "vqhip_fsq_decode_pool: q, quant and out are required");
    if (int rc = pool_check(what, quant_dtype, B, HW)) return rc;
    VqFsqConsts k;
    int unused = 0;
    if (int rc = fsq_setup(what, q, VQHIP_LAYOUT_MAP, B * HW, HW, &k, &unused)) return rc;
    const int64_t grid = (B * k.C * VQ_POOL_PARTIALS + 255) / 256;           // B < 2^31, C <= 16
    VQ_REQUIRE(grid < (1ll << 31), "vqhip_fsq_decode_pool: B is beyond one launch");
    hipStream_t s = (hipStream_t)stream;
    if (quant_dtype == VQHIP_DTYPE_I64) fsq_decode_pool_kernel<true><<<(unsigned)grid, 256, 0, s>>>(k, quant, B, (int)HW, out);
    else fsq_decode_pool_kernel<false><<<(unsigned)grid, 256, 0, s>>>(k, quant, B, (int)HW, out);
    VQ_CHECK_LAUNCH("fsq_decode_pool_kernel");
    return VQHIP_OK;
}

}  // extern "C"
