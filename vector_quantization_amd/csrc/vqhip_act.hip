// libvqhip — the activation ops: StyleGAN2 bias-activation and FIR blur, GroupNorm / BatchNorm, the row ops of the ViT and Llama networks.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "vqhip_host.h"
#include "vqhip_slab_reduce.h"
#include "vqhip_stylegan2_kernels.h"
#include "vqhip_group_norm_kernels.h"
#include "vqhip_vit_kernels.h"

// ---- StyleGAN2 discriminator ops: the launches (vqhip_stylegan2_kernels.h) ---------------------------------------------------
template <int DT>
static int launch_bias_act_fwd(const VqBiasActArgs &a, bool rows, hipStream_t s) {
    const int64_t pieces = (a.n + SampleElem<DT>::W - 1) / SampleElem<DT>::W;
    const int64_t blocks = (pieces + VQ_SG2_THREADS - 1) / VQ_SG2_THREADS;
    const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
    if (rows) bias_act_fwd_kernel<DT, true><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
    else bias_act_fwd_kernel<DT, false><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
    VQ_CHECK_LAUNCH("bias_act_fwd_kernel");
    return VQHIP_OK;
}

template <int DT>
static int launch_bias_act_bwd(const VqBiasActArgs &a, bool rows, int64_t slabs, float *gbias, hipStream_t s) {
    if (rows) {
        const int per = 64 * SampleElem<DT>::W;
        bias_act_bwd_rows_kernel<DT><<<dim3((unsigned)slabs, (unsigned)((a.C + per - 1) / per)), VQ_SG2_THREADS, 0, s>>>(a);
        VQ_CHECK_LAUNCH("bias_act_bwd_rows_kernel");
    } else {
        bias_act_bwd_map_kernel<DT><<<(unsigned)((int64_t)a.B * a.C * a.chunks), VQ_SG2_THREADS, 0, s>>>(a);
        VQ_CHECK_LAUNCH("bias_act_bwd_map_kernel");
    }
    return gbias ? launch_sg2_reduce(a.ws, slabs, a.C, gbias, s) : VQHIP_OK;
}

template <int DT, bool ROWS, int DOWN, int FUSED>
static int launch_fir4_one(const VqFirArgs &a, hipStream_t s) {
    const int64_t grid = (int64_t)a.B * a.cblocks * a.tiles_y * a.tiles_x;
    fir4_kernel<DT, ROWS, DOWN, FUSED><<<(unsigned)grid, VQ_SG2_THREADS, 0, s>>>(a);
    VQ_CHECK_LAUNCH("fir4_kernel");
    return VQHIP_OK;
}

template <int DT>
static int launch_fir4(const VqFirArgs &a, bool rows, int down, int fused, hipStream_t s) {
#define VQ_FIR_CASE(R, D, F) if (rows == R && down == D && fused == F) return launch_fir4_one<DT, R, D, F>(a, s)
    VQ_FIR_CASE(false, 1, VQ_FIR_NONE); VQ_FIR_CASE(false, 1, VQ_FIR_ACT_IN); VQ_FIR_CASE(false, 1, VQ_FIR_MASK_OUT);
    VQ_FIR_CASE(false, 2, VQ_FIR_NONE); VQ_FIR_CASE(false, 2, VQ_FIR_ACT_IN);
    VQ_FIR_CASE(true, 1, VQ_FIR_NONE); VQ_FIR_CASE(true, 1, VQ_FIR_ACT_IN); VQ_FIR_CASE(true, 1, VQ_FIR_MASK_OUT);
    VQ_FIR_CASE(true, 2, VQ_FIR_NONE); VQ_FIR_CASE(true, 2, VQ_FIR_ACT_IN);
#undef VQ_FIR_CASE
    return fail(VQHIP_EINVAL, "fir4", "no kernel of this form");
}

// the adjoint blur; in the fused form (a.x) it masks on the way out and the bias gradient follows from its slabs
template <int DT>
static int fir4_bwd_run(const VqFirArgs &a, bool rows, float *gbias, hipStream_t s) {
    if (int rc = launch_fir4<DT>(a, rows, 1, a.x ? VQ_FIR_MASK_OUT : VQ_FIR_NONE, s)) return rc;
    return a.x ? launch_sg2_reduce(a.ws, (int64_t)a.B * a.tiles_y * a.tiles_x, a.C, gbias, s) : VQHIP_OK;
}

// ---- GroupNorm (+ SiLU): the launches (vqhip_group_norm_kernels.h) -------------------------------------------------------------
template <int DT, bool ROWS, int PW>
static int launch_gn_one(const VqGnArgs &a, int T, bool bwd, hipStream_t s) {
    const unsigned grid = (unsigned)(T == 64 ? (a.units + 3) / 4 : a.units);
    if (T == 64) {
        if (bwd) gn_bwd_kernel<DT, ROWS, PW, 64><<<grid, VQ_GN_THREADS, 0, s>>>(a);
        else gn_fwd_kernel<DT, ROWS, PW, 64><<<grid, VQ_GN_THREADS, 0, s>>>(a);
    } else {
        if (bwd) gn_bwd_kernel<DT, ROWS, PW, 256><<<grid, VQ_GN_THREADS, 0, s>>>(a);
        else gn_fwd_kernel<DT, ROWS, PW, 256><<<grid, VQ_GN_THREADS, 0, s>>>(a);
    }
    VQ_CHECK_LAUNCH(bwd ? "gn_bwd_kernel" : "gn_fwd_kernel");
    return VQHIP_OK;
}

// the piece of the rows layout: the widest of 16 bytes, 8 bytes or one element that divides the channels of a group
template <int DT>
static int launch_gn(const VqGnArgs &a, bool rows, int T, bool bwd, hipStream_t s) {
    constexpr int W = SampleElem<DT>::W;
    if (!rows) return launch_gn_one<DT, false, W>(a, T, bwd, s);
    if (a.cpg % W == 0) return launch_gn_one<DT, true, W>(a, T, bwd, s);
    if (W == 8 && a.cpg % 4 == 0) return launch_gn_one<DT, true, 4>(a, T, bwd, s);
    return launch_gn_one<DT, true, 1>(a, T, bwd, s);
}

// one launch where a group is one chunk; else the partials, and behind the launch boundary their combination and the result
template <int DT>
static int gn_run(VqGnArgs a, bool rows, int T, bool bwd, int64_t slabs, float *dgamma, float *dbeta, hipStream_t s) {
    if (a.S == 1) {
        a.phase = VQ_GN_ALL;
        if (int rc = launch_gn<DT>(a, rows, T, bwd, s)) return rc;
    } else {
        a.phase = VQ_GN_PART;
        if (int rc = launch_gn<DT>(a, rows, T, bwd, s)) return rc;
        a.phase = VQ_GN_APPLY;
        if (int rc = launch_gn<DT>(a, rows, T, bwd, s)) return rc;
    }
    if (!bwd) return VQHIP_OK;
    if (int rc = launch_sg2_reduce(a.ws_dg, slabs, a.C, dgamma, s)) return rc;
    return launch_sg2_reduce(a.ws_db, slabs, a.C, dbeta, s);
}

// batch statistics: one launch where a channel is one chunk; else the partials, their combination, the result
template <int DT, int PW>
static int launch_bn_one(const VqBnArgs &a, bool rows, bool bwd, unsigned grid, hipStream_t s) {
    if (rows) {
        if (bwd) bn_rows_bwd_kernel<DT, PW><<<grid, VQ_GN_THREADS, 0, s>>>(a);
        else bn_rows_fwd_kernel<DT, PW><<<grid, VQ_GN_THREADS, 0, s>>>(a);
    } else {
        if (bwd) bn_map_bwd_kernel<DT, PW><<<grid, VQ_GN_THREADS, 0, s>>>(a);
        else bn_map_fwd_kernel<DT, PW><<<grid, VQ_GN_THREADS, 0, s>>>(a);
    }
    VQ_CHECK_LAUNCH(bwd ? "bn_bwd_kernel" : "bn_fwd_kernel");
    return VQHIP_OK;
}

template <int DT>
static int launch_bn(const VqBnArgs &a, bool rows, int pw, bool bwd, unsigned grid, hipStream_t s) {
    constexpr int W = SampleElem<DT>::W;
    if (!rows || pw == W) return launch_bn_one<DT, W>(a, rows, bwd, grid, s);
    if (W == 8 && pw == 4) return launch_bn_one<DT, 4>(a, rows, bwd, grid, s);
    return launch_bn_one<DT, 1>(a, rows, bwd, grid, s);
}

template <int DT>
static int bn_run(VqBnArgs a, bool rows, int pw, bool bwd, unsigned grid, hipStream_t s) {
    if (a.S == 1) {
        a.phase = VQ_GN_ALL;
        return launch_bn<DT>(a, rows, pw, bwd, grid, s);
    }
    a.phase = VQ_GN_PART;
    if (int rc = launch_bn<DT>(a, rows, pw, bwd, grid, s)) return rc;
    bn_combine_kernel<<<(unsigned)a.C, VQ_GN_THREADS, 0, s>>>(a, bwd ? 1 : 0);
    VQ_CHECK_LAUNCH("bn_combine_kernel");
    a.phase = VQ_GN_APPLY;
    return launch_bn<DT>(a, rows, pw, bwd, grid, s);
}

// ---- the row ops of the VQ-KD networks: the launches (vqhip_vit_kernels.h) ---------------------------------------------------------
template <int XDT, int YDT, int PW, bool RMS>
static int launch_ln_one(const VqLnArgs &a, bool bwd, hipStream_t s) {
    if (a.D <= VQ_GN_SMALL) {
        if (bwd) ln_bwd_kernel<XDT, YDT, PW, 64, RMS><<<(unsigned)((a.R + VQ_LN_SLAB - 1) / VQ_LN_SLAB), VQ_LN_THREADS, 0, s>>>(a);
        else ln_fwd_kernel<XDT, YDT, PW, 64, RMS><<<(unsigned)((a.R + 3) / 4), VQ_LN_THREADS, 0, s>>>(a);
    } else {
        if (bwd) ln_bwd_kernel<XDT, YDT, PW, 256, RMS><<<(unsigned)((a.R + VQ_LN_SLAB - 1) / VQ_LN_SLAB), VQ_LN_THREADS, 0, s>>>(a);
        else ln_fwd_kernel<XDT, YDT, PW, 256, RMS><<<(unsigned)a.R, VQ_LN_THREADS, 0, s>>>(a);
    }
    VQ_CHECK_LAUNCH(bwd ? "ln_bwd_kernel" : "ln_fwd_kernel");
    return VQHIP_OK;
}

// the piece: 16 bytes of the narrowest dtype where they divide the row, else four elements, else one
template <int XDT, int YDT, bool RMS>
static int launch_ln(const VqLnArgs &a, bool bwd, hipStream_t s) {
    if constexpr (XDT == YDT || XDT == VQHIP_DTYPE_F32) {
        if constexpr (XDT != VQHIP_DTYPE_F32)
            if (a.D % 8 == 0) return launch_ln_one<XDT, YDT, 8, RMS>(a, bwd, s);
        if (a.D % 4 == 0) return launch_ln_one<XDT, YDT, 4, RMS>(a, bwd, s);
        return launch_ln_one<XDT, YDT, 1, RMS>(a, bwd, s);
    } else {
        return fail(VQHIP_EINVAL, "add_layer_norm", "no kernel of this dtype combination");
    }
}

template <int DT>
static int launch_row_act(const VqRowActArgs &a, int act, bool bwd, int64_t slabs, float *dbias, hipStream_t s) {
    if (act == VQHIP_ROW_ACT_SWIGLU) {                                          // both directions: the forward's grid over the [R, F] side
        const int64_t pieces = (a.R * a.D + SampleElem<DT>::W - 1) / SampleElem<DT>::W;
        const int64_t blocks = (pieces + VQ_SG2_THREADS - 1) / VQ_SG2_THREADS;
        const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
        if (bwd) swiglu_kernel<DT, true><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
        else swiglu_kernel<DT, false><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
        VQ_CHECK_LAUNCH("swiglu_kernel");
        return VQHIP_OK;
    }
    if (!bwd) {
        const int64_t pieces = (a.R * a.D + SampleElem<DT>::W - 1) / SampleElem<DT>::W;
        const int64_t blocks = (pieces + VQ_SG2_THREADS - 1) / VQ_SG2_THREADS;
        const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
        if (act == VQHIP_ROW_ACT_GELU) row_act_fwd_kernel<DT, VQHIP_ROW_ACT_GELU><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
        else row_act_fwd_kernel<DT, VQHIP_ROW_ACT_TANH><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
        VQ_CHECK_LAUNCH("row_act_fwd_kernel");
        return VQHIP_OK;
    }
    const int per = 64 * SampleElem<DT>::W;
    const dim3 grid((unsigned)slabs, (unsigned)((a.D + per - 1) / per));
    if (act == VQHIP_ROW_ACT_GELU) row_act_bwd_kernel<DT, VQHIP_ROW_ACT_GELU><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
    else row_act_bwd_kernel<DT, VQHIP_ROW_ACT_TANH><<<grid, VQ_SG2_THREADS, 0, s>>>(a);
    VQ_CHECK_LAUNCH("row_act_bwd_kernel");
    return dbias ? launch_sg2_reduce(a.ws, slabs, a.D, dbias, s) : VQHIP_OK;
}

extern "C" {

// ---- StyleGAN2 discriminator ops (vqhip_stylegan2_kernels.h) -----------------------------------------------------------------
// what every entry point of the block refuses alike
static int sg2_common(const char *what, int dtype, int layout, int64_t B, int64_t C, int64_t P) {
    if (!vq_float_dtype(dtype)) return fail(VQHIP_EINVAL, what, "dtype");
    if (!vq_dense_layout(layout)) return fail(VQHIP_EINVAL, what, "layout");
    const int64_t cap = 1ll << 31;
    if (B < 1 || C < 1 || P < 1 || B >= cap || P >= cap || C > VQHIP_SG2_MAX_C) return fail(VQHIP_EINVAL, what, "need B, P >= 1 and 1 <= C <= 2^16");
    if (B * P >= cap || B * P * C >= cap) return fail(VQHIP_EINVAL, what, "B * C * P must be below 2^31");
    return VQHIP_OK;
}

// a [B, C] matrix (P == 1) is the same memory in both layouts: it takes the rows kernels
static inline bool sg2_rows(int layout, int64_t P) { return layout == VQHIP_LAYOUT_ROWS || P == 1; }

int64_t vqhip_bias_act_slabs(int layout, int64_t B, int64_t C, int64_t P) {
    if (sg2_common("vqhip_bias_act_slabs", VQHIP_DTYPE_F32, layout, B, C, P)) return -1;
    if (sg2_rows(layout, P)) return (B * P + VQ_SG2_ROWS_SLAB - 1) / VQ_SG2_ROWS_SLAB;
    return B * ((P + VQ_SG2_MAP_CHUNK - 1) / VQ_SG2_MAP_CHUNK);
}

int vqhip_bias_act_fwd(const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t P, const float *bias, void *y, void *stream) {
    if (int rc = sg2_common("vqhip_bias_act_fwd", dtype, layout, B, C, P)) return rc;
    VQ_REQUIRE(x && bias && y, "vqhip_bias_act_fwd: x, bias and y are required");
    VqBiasActArgs a = {};
    a.x = x; a.bias = bias; a.out = y; a.n = B * C * P; a.B = (int)B; a.C = (int)C; a.P = (int)P;
    return vq_with_dtype(dtype, [&](auto dt) { return launch_bias_act_fwd<decltype(dt)::value>(a, sg2_rows(layout, P), (hipStream_t)stream); });
}

int vqhip_bias_act_bwd(const void *g, const void *y, int dtype, int layout, int64_t B, int64_t C, int64_t P, void *gx, float *gbias,
                       float *ws, int64_t ws_bytes, void *stream) {
    if (int rc = sg2_common("vqhip_bias_act_bwd", dtype, layout, B, C, P)) return rc;
    VQ_REQUIRE(g && y && gx, "vqhip_bias_act_bwd: g, y and gx are required");
    VQ_REQUIRE(!gbias || ws, "vqhip_bias_act_bwd: gbias needs the workspace");
    const int64_t slabs = vqhip_bias_act_slabs(layout, B, C, P);
    if (gbias) VQ_NEED("vqhip_bias_act_bwd: ws too small", ws_bytes, slabs * C * (int64_t)sizeof(float));
    VQ_REQUIRE(B * C * ((P + VQ_SG2_MAP_CHUNK - 1) / VQ_SG2_MAP_CHUNK) < (1ll << 31), "vqhip_bias_act_bwd: B * C * ceil(P / 4096) is beyond one launch");
    VqBiasActArgs a = {};
    a.x = g; a.y = y; a.out = gx; a.ws = gbias ? ws : nullptr; a.n = B * C * P; a.B = (int)B; a.C = (int)C; a.P = (int)P;
    a.chunks = (int)((P + VQ_SG2_MAP_CHUNK - 1) / VQ_SG2_MAP_CHUNK);
    return vq_with_dtype(dtype, [&](auto dt) {
        return launch_bias_act_bwd<decltype(dt)::value>(a, sg2_rows(layout, P), slabs, gbias, (hipStream_t)stream);
    });
}

// the sizes and tiles of a blur: (H, W) the blur's INPUT plane, (OH, OW) its output; `adjoint` walks tiles of the input plane
static int fir4_setup(const char *what, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W, int down, int py0, int py1,
                      int px0, int px1, bool adjoint, VqFirArgs *a) {
    const int64_t cap = 1ll << 31;
    if (H < 1 || W < 1 || H >= cap || W >= cap || H * W >= cap) return fail(VQHIP_EINVAL, what, "H * W must be in 1 .. 2^31 - 1");
    if (int rc = sg2_common(what, dtype, layout, B, C, H * W)) return rc;
    if (down != 1 && down != 2) return fail(VQHIP_EINVAL, what, "down must be 1 or 2");
    for (int p : {py0, py1, px0, px1})
        if (p < 0 || p > 3) return fail(VQHIP_EINVAL, what, "every padding must be in 0 .. 3");
    if (H + py0 + py1 < 4 || W + px0 + px1 < 4) return fail(VQHIP_EINVAL, what, "the padded plane is smaller than the 4 x 4 filter");
    const int64_t OH = (H + py0 + py1 - 4) / down + 1, OW = (W + px0 + px1 - 4) / down + 1;
    const bool rows = layout == VQHIP_LAYOUT_ROWS;
    const int CB = rows ? FirTile<true>::CB : FirTile<false>::CB;
    const int TOH = rows ? FirTile<true>::TOH : FirTile<false>::TOH, TOW = rows ? FirTile<true>::TOW : FirTile<false>::TOW;
    a->B = (int)B; a->C = (int)C;
    if (adjoint) {
        a->IH = (int)OH; a->IW = (int)OW; a->OH = (int)H; a->OW = (int)W;
        a->up = down; a->offy = 3 - py0; a->offx = 3 - px0;
    } else {
        a->IH = (int)H; a->IW = (int)W; a->OH = (int)OH; a->OW = (int)OW;
        a->up = 1; a->offy = py0; a->offx = px0;
    }
    a->cblocks = (int)((C + CB - 1) / CB);
    a->tiles_y = (a->OH + TOH - 1) / TOH; a->tiles_x = (a->OW + TOW - 1) / TOW;
    if (B * a->cblocks * a->tiles_y * a->tiles_x >= cap) return fail(VQHIP_EINVAL, what, "the number of tiles is beyond one launch");
    return VQHIP_OK;
}

int64_t vqhip_fir4_slabs(int layout, int64_t B, int64_t C, int64_t H, int64_t W) {
    VqFirArgs a = {};
    if (fir4_setup("vqhip_fir4_slabs", VQHIP_DTYPE_F32, layout, B, C, H, W, 1, 2, 2, 2, 2, true, &a)) return -1;
    return B * a.tiles_y * a.tiles_x;
}

int vqhip_fir4_fwd(const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W, int down, int py0, int py1, int px0,
                   int px1, const float *bias, void *out, void *stream) {
    VqFirArgs a = {};
    if (int rc = fir4_setup("vqhip_fir4_fwd", dtype, layout, B, C, H, W, down, py0, py1, px0, px1, false, &a)) return rc;
    VQ_REQUIRE(x && out, "vqhip_fir4_fwd: x and out are required");
    a.in = x; a.out = out; a.bias = bias;
    return vq_with_dtype(dtype, [&](auto dt) {
        return launch_fir4<decltype(dt)::value>(a, layout == VQHIP_LAYOUT_ROWS, down, bias ? VQ_FIR_ACT_IN : VQ_FIR_NONE, (hipStream_t)stream);
    });
}

int vqhip_fir4_bwd(const void *g, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W, int down, int py0, int py1, int px0,
                   int px1, const void *x, const float *bias, void *gx, float *gbias, float *ws, int64_t ws_bytes, void *stream) {
    VqFirArgs a = {};
    if (int rc = fir4_setup("vqhip_fir4_bwd", dtype, layout, B, C, H, W, down, py0, py1, px0, px1, true, &a)) return rc;
    VQ_REQUIRE(g && gx, "vqhip_fir4_bwd: g and gx are required");
    VQ_REQUIRE((x != nullptr) == (bias != nullptr), "vqhip_fir4_bwd: the fused form needs x and bias together");
    VQ_REQUIRE(!x || (gbias && ws), "vqhip_fir4_bwd: the fused form needs gbias and the workspace");
    if (x) VQ_NEED("vqhip_fir4_bwd: ws too small", ws_bytes, (int64_t)B * a.tiles_y * a.tiles_x * C * (int64_t)sizeof(float));
    a.in = g; a.out = gx; a.x = x; a.bias = bias; a.ws = ws;
    return vq_with_dtype(dtype, [&](auto dt) { return fir4_bwd_run<decltype(dt)::value>(a, layout == VQHIP_LAYOUT_ROWS, gbias, (hipStream_t)stream); });
}

// ---- GroupNorm (+ SiLU) (vqhip_group_norm_kernels.h) ---------------------------------------------------------------------------
struct VqGnPlan {
    int64_t n, S, units, slabs, ws_floats;
    int T;
    int pw;                                     // batch statistics: the piece (elements); units = workgroups of a launch
};

// the piece of the rows layout in batch mode: the widest of 16 bytes, 8 bytes or one element that divides C
static int bn_rows_pw(int dtype, int64_t C) {
    const int W = dtype == VQHIP_DTYPE_F32 ? 4 : 8;
    return C % W == 0 ? W : (W == 8 && C % 4 == 0 ? 4 : 1);
}

// G == VQHIP_GN_BATCH, behind the clauses every mode shares: a channel over all images
static int bn_plan(const char *what, int dtype, int layout, int64_t B, int64_t C, int64_t P, VqGnPlan *pl) {
    const int64_t cap = 1ll << 31;
    pl->n = B * P;
    if (pl->n >= cap) return fail(VQHIP_EINVAL, what, "a channel must hold fewer than 2^31 values over the batch");
    if (pl->n < 2) return fail(VQHIP_EINVAL, what, "batch statistics need more than one value per channel");
    const bool rows = layout == VQHIP_LAYOUT_ROWS;
    pl->pw = rows ? bn_rows_pw(dtype, C) : (dtype == VQHIP_DTYPE_F32 ? 4 : 8);
    const int64_t chunk = rows ? 1024 / pl->pw : VQ_GN_CHUNK;
    const int64_t chunk_ws = rows ? 1024 / bn_rows_pw(VQHIP_DTYPE_BF16, C) : VQ_GN_CHUNK;      // the workspace serves every dtype
    pl->S = (pl->n + chunk - 1) / chunk;
    const int64_t S_ws = (pl->n + chunk_ws - 1) / chunk_ws;
    if (C * S_ws >= cap) return fail(VQHIP_EINVAL, what, "C * S is beyond one launch");
    pl->units = (rows ? (C + VQ_BN_LX * pl->pw - 1) / (VQ_BN_LX * pl->pw) : C) * pl->S;
    pl->slabs = 0; pl->T = VQ_GN_THREADS;
    pl->ws_floats = 2 * C + 2 * C * S_ws;
    return VQHIP_OK;
}

// what the three entry points refuse alike; on success the launch shape
static int gn_plan(const char *what, int dtype, int layout, int64_t B, int64_t C, int64_t P, int64_t G, VqGnPlan *pl) {
    if (!vq_float_dtype(dtype)) return fail(VQHIP_EINVAL, what, "dtype");
    if (!vq_dense_layout(layout)) return fail(VQHIP_EINVAL, what, "layout");
    if (B < 1 || C < 1 || P < 1 || (G < 1 && G != VQHIP_GN_BATCH)) return fail(VQHIP_EINVAL, what, "B, C and P must be positive, G positive or VQHIP_GN_BATCH");
    if (G != VQHIP_GN_BATCH && C % G != 0) return fail(VQHIP_EINVAL, what, "C must be a multiple of G");
    const int64_t cap = 1ll << 31;
    if (B >= cap || C >= cap || P >= cap) return fail(VQHIP_EINVAL, what, "B, C and P must be below 2^31");
    if (B * C > INT64_MAX / P / 8) return fail(VQHIP_EINVAL, what, "B * C * P overflows");     // (8: bytes and the workspace's floats)
    pl->pw = 0;
    if (G == VQHIP_GN_BATCH) return bn_plan(what, dtype, layout, B, C, P, pl);
    pl->n = (C / G) * P;
    if (pl->n >= cap) return fail(VQHIP_EINVAL, what, "a group must hold fewer than 2^31 values");
    pl->T = pl->n <= VQ_GN_SMALL ? 64 : 256;
    pl->S = pl->T == 64 ? 1 : (pl->n + VQ_GN_CHUNK - 1) / VQ_GN_CHUNK;
    pl->units = B * G * pl->S;
    if (pl->units >= cap) return fail(VQHIP_EINVAL, what, "B * G * ceil(n / 8192) is beyond one launch");
    pl->slabs = B * pl->S;
    pl->ws_floats = 2 * pl->units + 2 * pl->slabs * C;
    return VQHIP_OK;
}

int64_t vqhip_group_norm_ws_bytes(int layout, int64_t B, int64_t C, int64_t P, int64_t G) {
    VqGnPlan pl;
    if (gn_plan("vqhip_group_norm_ws_bytes", VQHIP_DTYPE_BF16, layout, B, C, P, G, &pl)) return -1;   // (batch mode: the dtype of the most chunks)
    return pl.ws_floats * (int64_t)sizeof(float);
}

static void bn_fill(VqBnArgs *a, const VqGnPlan &pl, int layout, int64_t B, int64_t C, int64_t P, float *ws) {
    a->n = (uint32_t)pl.n; a->chunk = layout == VQHIP_LAYOUT_ROWS ? 1024u / (uint32_t)pl.pw : (uint32_t)VQ_GN_CHUNK;
    a->B = (int)B; a->C = (int)C; a->P = (int)P; a->S = (int)pl.S;
    a->mv = ws; a->part = ws + 2 * C;
}

static void gn_fill(VqGnArgs *a, const VqGnPlan &pl, int64_t B, int64_t C, int64_t P, int64_t G, float *ws) {
    a->units = pl.units; a->n = (uint32_t)pl.n;
    a->B = (int)B; a->C = (int)C; a->P = (int)P; a->G = (int)G; a->cpg = (int)(C / G); a->S = (int)pl.S;
    a->ws_grp = ws; a->ws_dg = ws + 2 * pl.units; a->ws_db = a->ws_dg + pl.slabs * C;
}

int vqhip_group_norm_fwd(const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t P, int64_t G, const float *gamma,
                         const float *beta, float eps, int act, void *y, float *stats, float *ws, int64_t ws_bytes, void *stream) {
    VqGnPlan pl;
    if (int rc = gn_plan("vqhip_group_norm_fwd", dtype, layout, B, C, P, G, &pl)) return rc;
    VQ_REQUIRE(act == 0 || act == 1 || (act == VQHIP_GN_ACT_LEAKY && G == VQHIP_GN_BATCH),
               "vqhip_group_norm_fwd: act must be 0 (none) or 1 (SiLU), with batch statistics also 2 (LeakyReLU)");
    VQ_REQUIRE(eps >= 0.0f && eps < INFINITY, "vqhip_group_norm_fwd: eps must be finite and not negative");
    VQ_REQUIRE(x && gamma && beta && y && stats && ws, "vqhip_group_norm_fwd: x, gamma, beta, y, stats and ws are required");
    VQ_NEED("vqhip_group_norm_fwd: ws too small", ws_bytes, pl.ws_floats * (int64_t)sizeof(float));
    if (G == VQHIP_GN_BATCH) {
        VqBnArgs a = {};
        bn_fill(&a, pl, layout, B, C, P, ws);
        a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.stats = stats; a.eps = eps; a.act = act;
        return vq_with_dtype(dtype, [&](auto dt) {
            return bn_run<decltype(dt)::value>(a, layout == VQHIP_LAYOUT_ROWS, pl.pw, false, (unsigned)pl.units, (hipStream_t)stream);
        });
    }
    VqGnArgs a = {};
    gn_fill(&a, pl, B, C, P, G, ws);
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.stats = stats; a.eps = eps; a.act = act;
    return vq_with_dtype(dtype, [&](auto dt) {
        return gn_run<decltype(dt)::value>(a, layout == VQHIP_LAYOUT_ROWS, pl.T, false, pl.slabs, nullptr, nullptr, (hipStream_t)stream);
    });
}

int vqhip_group_norm_bwd(const void *g, const void *x, int dtype, int layout, int64_t B, int64_t C, int64_t P, int64_t G,
                         const float *gamma, const float *beta, const float *stats, int act, void *gx, float *dgamma, float *dbeta,
                         float *ws, int64_t ws_bytes, void *stream) {
    VqGnPlan pl;
    if (int rc = gn_plan("vqhip_group_norm_bwd", dtype, layout, B, C, P, G, &pl)) return rc;
    VQ_REQUIRE(act == 0 || act == 1 || (act == VQHIP_GN_ACT_LEAKY && G == VQHIP_GN_BATCH),
               "vqhip_group_norm_bwd: act must be 0 (none) or 1 (SiLU), with batch statistics also 2 (LeakyReLU)");
    VQ_REQUIRE(g && x && gamma && beta && stats && gx && dgamma && dbeta && ws,
               "vqhip_group_norm_bwd: g, x, gamma, beta, stats, gx, dgamma, dbeta and ws are required");
    VQ_NEED("vqhip_group_norm_bwd: ws too small", ws_bytes, pl.ws_floats * (int64_t)sizeof(float));
    if (G == VQHIP_GN_BATCH) {
        VqBnArgs a = {};
        bn_fill(&a, pl, layout, B, C, P, ws);
        a.x = x; a.g = g; a.out = gx; a.gamma = gamma; a.beta = beta; a.stats = const_cast<float *>(stats); a.act = act;
        a.dgamma = dgamma; a.dbeta = dbeta;
        return vq_with_dtype(dtype, [&](auto dt) {
            return bn_run<decltype(dt)::value>(a, layout == VQHIP_LAYOUT_ROWS, pl.pw, true, (unsigned)pl.units, (hipStream_t)stream);
        });
    }
    VqGnArgs a = {};
    gn_fill(&a, pl, B, C, P, G, ws);
    a.x = x; a.g = g; a.out = gx; a.gamma = gamma; a.beta = beta; a.stats = const_cast<float *>(stats); a.act = act;
    return vq_with_dtype(dtype, [&](auto dt) {
        return gn_run<decltype(dt)::value>(a, layout == VQHIP_LAYOUT_ROWS, pl.T, true, pl.slabs, dgamma, dbeta, (hipStream_t)stream);
    });
}

// ---- the row ops of the VQ-KD networks (vqhip_vit_kernels.h) ---------------------------------------------------------------------
// what the six entry points refuse alike about the rows
static int vit_rows(const char *what, int64_t R, int64_t D) {
    if (R < 1 || R > VQHIP_VIT_MAX_R || D < 1 || D > VQHIP_VIT_MAX_D) return fail(VQHIP_EINVAL, what, "need 1 <= R <= 2^24 and 1 <= D <= 8192");
    if (R > ((1ll << 31) - 1) / D) return fail(VQHIP_EINVAL, what, "R * D must be below 2^31");
    return VQHIP_OK;
}

// (x, y): the same float dtype, or fp32 x with a 16-bit y (autocast); res, where given, in y's dtype
static inline bool vit_ln_pair(int x_dtype, int y_dtype) {
    return vq_float_dtype(x_dtype) && vq_float_dtype(y_dtype) && (x_dtype == y_dtype || x_dtype == VQHIP_DTYPE_F32);
}

int64_t vqhip_add_layer_norm_slabs(int64_t R, int64_t D) {
    if (vit_rows("vqhip_add_layer_norm_slabs", R, D)) return -1;
    return (R + VQ_LN_SLAB - 1) / VQ_LN_SLAB;
}

int vqhip_add_layer_norm_fwd(const void *x, int x_dtype, const void *res, int res_dtype, int64_t R, int64_t D, const float *gamma,
                             const float *beta, float eps, void *sum_out, void *y, int y_dtype, float *stats, void *stream) {
    if (int rc = vit_rows("vqhip_add_layer_norm_fwd", R, D)) return rc;
    VQ_REQUIRE(vit_ln_pair(x_dtype, y_dtype), "vqhip_add_layer_norm_fwd: (x, y) must be one float dtype, or fp32 x with a bf16 or fp16 y");
    VQ_REQUIRE(!res || res_dtype == y_dtype, "vqhip_add_layer_norm_fwd: res must have y's dtype");
    VQ_REQUIRE(eps >= 0.0f && eps < INFINITY, "vqhip_add_layer_norm_fwd: eps must be finite and not negative");
    VQ_REQUIRE(x && gamma && y && stats, "vqhip_add_layer_norm_fwd: x, gamma, y and stats are required (beta == NULL: RMS mode)");
    VQ_REQUIRE(!res || sum_out, "vqhip_add_layer_norm_fwd: res needs sum_out");
    VqLnArgs a = {};
    a.x = x; a.res = res; a.sum_out = sum_out; a.out = y; a.gamma = gamma; a.beta = beta; a.stats = stats; a.R = R; a.D = (int)D; a.eps = eps;
    return vq_with_dtype(x_dtype, [&](auto dx) { return vq_with_dtype(y_dtype, [&](auto dy) {
        if (!beta) return launch_ln<decltype(dx)::value, decltype(dy)::value, true>(a, false, (hipStream_t)stream);
        return launch_ln<decltype(dx)::value, decltype(dy)::value, false>(a, false, (hipStream_t)stream);
    }); });
}

int vqhip_add_layer_norm_bwd(const void *g, int g_dtype, const void *s, int s_dtype, const void *g_skip, int64_t R, int64_t D,
                             const float *gamma, const float *stats, void *gx, float *dgamma, float *dbeta, float *ws, int64_t ws_bytes,
                             void *stream) {
    if (int rc = vit_rows("vqhip_add_layer_norm_bwd", R, D)) return rc;
    VQ_REQUIRE(vit_ln_pair(s_dtype, g_dtype), "vqhip_add_layer_norm_bwd: (s, g) must be one float dtype, or fp32 s with a bf16 or fp16 g");
    VQ_REQUIRE(g && s && gamma && stats && gx && dgamma && ws,
               "vqhip_add_layer_norm_bwd: g, s, gamma, stats, gx, dgamma and ws are required (dbeta == NULL: RMS mode)");
    const int64_t slabs = (R + VQ_LN_SLAB - 1) / VQ_LN_SLAB;
    VQ_NEED("vqhip_add_layer_norm_bwd: ws too small", ws_bytes, 2 * slabs * D * (int64_t)sizeof(float));
    VqLnArgs a = {};
    a.x = s; a.res = g_skip; a.g = g; a.out = gx; a.gamma = gamma; a.stats = const_cast<float *>(stats); a.R = R; a.D = (int)D;
    a.ws_dg = ws; a.ws_db = ws + slabs * D;                                     // (RMS mode leaves the second half alone)
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = vq_with_dtype(s_dtype, [&](auto dx) { return vq_with_dtype(g_dtype, [&](auto dy) {
            if (!dbeta) return launch_ln<decltype(dx)::value, decltype(dy)::value, true>(a, true, st);
            return launch_ln<decltype(dx)::value, decltype(dy)::value, false>(a, true, st);
        }); })) return rc;
    if (int rc = launch_sg2_reduce(a.ws_dg, slabs, a.D, dgamma, st)) return rc;
    return dbeta ? launch_sg2_reduce(a.ws_db, slabs, a.D, dbeta, st) : VQHIP_OK;
}

// what act == VQHIP_ROW_ACT_SWIGLU refuses on top of vit_rows: x is [R, 2 D] and there is no bias
static int swiglu_rows(const char *what, int64_t R, int64_t D, const void *bias, const void *dbias, const void *ws) {
    if (R > ((1ll << 31) - 1) / (2 * D)) return fail(VQHIP_EINVAL, what, "SwiGLU: R * 2 D must be below 2^31");
    if (bias || dbias || ws) return fail(VQHIP_EINVAL, what, "SwiGLU has no bias: bias, dbias and ws must be NULL");
    return VQHIP_OK;
}

int64_t vqhip_row_bias_act_slabs(int64_t R, int64_t D) {
    if (vit_rows("vqhip_row_bias_act_slabs", R, D)) return -1;
    return (R + VQ_SG2_ROWS_SLAB - 1) / VQ_SG2_ROWS_SLAB;
}

int vqhip_row_bias_act_fwd(const void *x, int dtype, int64_t R, int64_t D, const float *bias, int act, void *y, void *stream) {
    if (int rc = vit_rows("vqhip_row_bias_act_fwd", R, D)) return rc;
    VQ_REQUIRE(vq_float_dtype(dtype), "vqhip_row_bias_act_fwd: dtype");
    VQ_REQUIRE(act == VQHIP_ROW_ACT_GELU || act == VQHIP_ROW_ACT_TANH || act == VQHIP_ROW_ACT_SWIGLU,
               "vqhip_row_bias_act_fwd: act must be 0 (GELU), 1 (tanh) or 3 (SwiGLU)");
    if (act == VQHIP_ROW_ACT_SWIGLU) {
        if (int rc = swiglu_rows("vqhip_row_bias_act_fwd", R, D, bias, nullptr, nullptr)) return rc;
        VQ_REQUIRE(x && y, "vqhip_row_bias_act_fwd: x and y are required");
    } else {
        VQ_REQUIRE(x && bias && y, "vqhip_row_bias_act_fwd: x, bias and y are required");
    }
    VqRowActArgs a = {};
    a.x = x; a.bias = bias; a.out = y; a.R = R; a.D = (int)D;
    return vq_with_dtype(dtype, [&](auto dt) { return launch_row_act<decltype(dt)::value>(a, act, false, 0, nullptr, (hipStream_t)stream); });
}

int vqhip_row_bias_act_bwd(const void *g, const void *x, int dtype, int64_t R, int64_t D, const float *bias, int act, void *gx,
                           float *dbias, float *ws, int64_t ws_bytes, void *stream) {
    if (int rc = vit_rows("vqhip_row_bias_act_bwd", R, D)) return rc;
    VQ_REQUIRE(vq_float_dtype(dtype), "vqhip_row_bias_act_bwd: dtype");
    VQ_REQUIRE(act == VQHIP_ROW_ACT_GELU || act == VQHIP_ROW_ACT_TANH || act == VQHIP_ROW_ACT_SWIGLU,
               "vqhip_row_bias_act_bwd: act must be 0 (GELU), 1 (tanh) or 3 (SwiGLU)");
    if (act == VQHIP_ROW_ACT_SWIGLU) {
        if (int rc = swiglu_rows("vqhip_row_bias_act_bwd", R, D, bias, dbias, ws)) return rc;
        VQ_REQUIRE(g && x && gx, "vqhip_row_bias_act_bwd: g, x and gx are required");
    } else {
        VQ_REQUIRE(g && x && bias && gx, "vqhip_row_bias_act_bwd: g, x, bias and gx are required");
    }
    VQ_REQUIRE(!dbias || ws, "vqhip_row_bias_act_bwd: dbias needs the workspace");
    const int64_t slabs = (R + VQ_SG2_ROWS_SLAB - 1) / VQ_SG2_ROWS_SLAB;
    if (dbias) VQ_NEED("vqhip_row_bias_act_bwd: ws too small", ws_bytes, slabs * D * (int64_t)sizeof(float));
    VqRowActArgs a = {};
    a.x = x; a.g = g; a.bias = bias; a.out = gx; a.ws = dbias ? ws : nullptr; a.R = R; a.D = (int)D;
    return vq_with_dtype(dtype, [&](auto dt) { return launch_row_act<decltype(dt)::value>(a, act, true, slabs, dbias, (hipStream_t)stream); });
}

}  // extern "C"
