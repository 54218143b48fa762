// The row-wise steps between the GEMMs of VQKDEncoder / VQKDDecoder (vq/algorithms/vqkd/autoencoder.py: a pre-norm ViT): the
// residual add fused into the LayerNorm that follows it, and bias + GELU (Mlp) / bias + tanh (task layer), each with its backward.
//
// Contract: include/vqhip.h (vqhip_add_layer_norm_fwd / _bwd, vqhip_row_bias_act_fwd / _bwd), DESIGN.md §8.  Every element is
// converted to fp32 exactly (SampleElem of the sampler); all arithmetic is fp32 IEEE without contraction; results are rounded to
// nearest even into the output dtype (ce_round of the token cross-entropy).  The pieces, the team sums, the mean and the second-pass
// M2 are the group norm's (vqhip_group_norm_kernels.h: gn_load, gn_store, gn_team_sum, gn_mean_m2), a row of D being a group of
// n = D; the second stage of every column sum is sg2_reduce_kernel (vqhip_stylegan2_kernels.h).
//
// ADD + LAYER NORM  WHO OWNS WHAT  a row of D values is cut into PIECES of PW adjacent values: PW = 8 where every tensor of the call
//   holds 16-bit elements and D % 8 == 0 (16 bytes), else 4 where D % 4 == 0 (16 bytes of fp32, 8 of a 16-bit dtype), else single
//   elements.  A TEAM of T threads owns a row; thread t holds pieces t, t + T, .., at most 32 values in registers.  D <= 2048: T = 64,
//   one wave per row, four rows per workgroup, no LDS.  2048 < D <= 8192: T = 256, one workgroup per row.
//   forward: one team per row.  s = round(x + res) in x's dtype (with res), written to sum_out and kept in registers AS ROUNDED;
//     mean and M2 by gn_mean_m2 (the order of the group norm's sums), rstd = 1 / sqrt(M2 / D + eps), y = ((s - mean) rstd) gamma[c]
//     + beta[c] rounded into y's dtype; stats[2 r] = (mean, rstd).
//   backward: a workgroup owns a SLAB of 16 consecutive rows; team w of its W = 256 / T teams takes rows w, w + W, .. of the slab in
//     that order.  Per row: xh = (s - mean) rstd, t = g gamma[c]; s1 = sum t, s2 = sum t xh (thread: increasing piece and element
//     into one accumulator from +0, then gn_team_sum); gx = rstd ((t - s1 / D) - xh (s2 / D)) (+ g_skip, one more addition).  Every
//     thread adds g xh and g of ITS columns over its team's rows, in increasing row, into accumulators from +0; the four teams of a
//     T = 64 workgroup add as (w0 + w1) + (w2 + w3) through LDS; the partial of slab b and column c goes to ws[b D + c]: every
//     (b, c) is written, so ws needs no memset; sg2_reduce_kernel adds the slabs.
//   RMS mode (beta == NULL forward, dbeta == NULL backward: the norms of LlamaTransformer): the same teams, pieces and slabs with no
//     mean: ms = sum s s / D (ln_sum_sq), rstd = 1 / sqrt(ms + eps), y = (s rstd) gamma[c], stats[2 r] = (0, rstd); backward
//     xh = s rstd, gx = rstd (t - xh (s2 / D)) (+ g_skip); only the g xh column sums are formed, ws_db is not touched.
// ROW BIAS-ACTIVATION  t = x + bias[c];  y = act(t):  GELU = (0.5 t) (1 + erff(t * fp32(2^-1/2))),  tanh = tanhf(t)
//       backward (from x and bias, y is not kept)   d = 0.5 (1 + erff(t * fp32(2^-1/2))) + t (expf(-0.5 (t t)) * fp32((2 pi)^-1/2))  (GELU)
//                                                   d = 1 - tanhf(t) tanhf(t)  (tanh);     gx = g d;   dbias[c] = sum of the fp32 gx
//   row_act_fwd_kernel: pieces of 16 bytes over the flat tensor at element alignment, as bias_act_fwd_kernel.  row_act_bwd_kernel: a
//   workgroup owns 256 consecutive rows times 64 pieces of W columns, thread (lane, group) takes rows group, group + 4, .. into W
//   accumulators, the 4 groups add as (g0 + g1) + (g2 + g3), as bias_act_bwd_rows_kernel; then sg2_reduce_kernel.
// SWIGLU  y = silu(gate) up of x = (gate | up): swiglu_kernel at the end of this file.
// Every global index is guarded: a piece beyond D is neither loaded nor stored; a row beyond R is skipped.  No atomics, no memset.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_group_norm_kernels.h"
#include "vqhip_stylegan2_kernels.h"

#define VQ_LN_THREADS 256
#define VQ_LN_SLAB 16                           // rows per workgroup of ln_bwd_kernel
#define VQ_VIT_RSQRT2 0.707106781186547524f
#define VQ_VIT_RSQRT2PI 0.398942280401432678f

struct VqLnArgs {
    const void *x;                              // forward: x; backward: the saved sum s
    const void *res;                            // forward: the branch to add, or NULL; backward: g_skip, or NULL
    const void *g;                              // backward: the gradient arriving at y
    void *sum_out;                              // forward with res: s
    void *out;                                  // y (forward) / gx (backward)
    const float *gamma, *beta;                  // [D]
    float *stats;                               // [R, 2]: mean, rstd (written forward, read backward)
    float *ws_dg, *ws_db;                       // [slabs, D] each (backward)
    int64_t R;
    int D;
    float eps;
};

// the sum of squares of the values a team holds in registers (RMS mode): thread, increasing piece and element, into one accumulator
// from +0, then gn_team_sum - the order of gn_mean_m2's second pass with mean = 0
template <int T, int NP, int PW>
__device__ __forceinline__ float ln_sum_sq(const float (&xv)[NP][PW], const int (&cnt)[NP], float *red) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < PW; ++e)
            if (e < cnt[k]) acc = acc + xv[k][e] * xv[k][e];
    return gn_team_sum<T>(acc, red);
}

// XDT: the dtype of x, sum_out (forward) / s, g_skip, gx (backward).  YDT: the dtype of res and y (forward) / g (backward).
// RMS: beta == NULL (forward) / dbeta == NULL (backward): no mean, no beta, no dbeta
template <int XDT, int YDT, int PW, int T, bool RMS>
__global__ __launch_bounds__(VQ_LN_THREADS) void ln_fwd_kernel(VqLnArgs a) {
    typedef typename SampleElem<XDT>::raw xraw;
    typedef typename SampleElem<YDT>::raw yraw;
    constexpr int NP = VQ_GN_EPT / PW;
    __shared__ float red[4];
    const int t = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * (VQ_LN_THREADS / T) + threadIdx.x / T;
    if (row >= a.R) return;                                                     // (T == 64 only: a whole wave; a T == 256 grid has no spare row)
    const uint32_t np = (uint32_t)a.D / PW;
    const xraw *in = reinterpret_cast<const xraw *>(a.x) + row * a.D;
    const yraw *res = reinterpret_cast<const yraw *>(a.res) + row * a.D;
    xraw *sum = reinterpret_cast<xraw *>(a.sum_out) + row * a.D;
    float xv[NP][PW];
    int cnt[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const uint32_t piece = (uint32_t)(k * T + t);
        cnt[k] = piece < np ? PW : 0;
        if (cnt[k] > 0) {
            gn_load<XDT, PW>(in + piece * PW, PW, xv[k]);
            if (a.res) {
                float rv[PW];
                gn_load<YDT, PW>(res + piece * PW, PW, rv);
#pragma unroll
                for (int e = 0; e < PW; ++e) xv[k][e] = SampleElem<XDT>::f32(ce_round<XDT>(xv[k][e] + rv[e]));
                gn_store<XDT, PW>(sum + piece * PW, PW, xv[k]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < PW; ++e) xv[k][e] = 0.0f;
        }
    }
    float mean = 0.0f, m2;
    if (RMS) m2 = ln_sum_sq<T, NP, PW>(xv, cnt, red);
    else gn_mean_m2<T, NP, PW>(xv, cnt, (float)a.D, red, mean, m2);
    const float rstd = 1.0f / sqrtf(m2 / (float)a.D + a.eps);
    if (t == 0) { a.stats[row * 2] = mean; a.stats[row * 2 + 1] = rstd; }
    yraw *out = reinterpret_cast<yraw *>(a.out) + row * a.D;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (cnt[k] == 0) continue;
        const uint32_t c0 = (uint32_t)(k * T + t) * PW;
        float y[PW];
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            if (RMS) y[e] = (xv[k][e] * rstd) * a.gamma[c0 + e];
            else y[e] = ((xv[k][e] - mean) * rstd) * a.gamma[c0 + e] + a.beta[c0 + e];
        }
        gn_store<YDT, PW>(out + c0, PW, y);
    }
}

template <int XDT, int YDT, int PW, int T, bool RMS>
__global__ __launch_bounds__(VQ_LN_THREADS) void ln_bwd_kernel(VqLnArgs a) {
    typedef typename SampleElem<XDT>::raw xraw;
    typedef typename SampleElem<YDT>::raw yraw;
    constexpr int NP = VQ_GN_EPT / PW, TEAMS = VQ_LN_THREADS / T;
    __shared__ float red[4];
    __shared__ float part[TEAMS > 1 ? TEAMS * VQ_GN_SMALL : 1];                 // T == 64: the teams' column sums, dgamma then dbeta
    const int t = threadIdx.x % T, team = threadIdx.x / T;
    const uint32_t np = (uint32_t)a.D / PW;
    int cnt[NP];
    float dg[NP][PW], db[NP][PW];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        cnt[k] = (uint32_t)(k * T + t) < np ? PW : 0;
#pragma unroll
        for (int e = 0; e < PW; ++e) { dg[k][e] = 0.0f; db[k][e] = 0.0f; }
    }
    for (int j = 0; j < VQ_LN_SLAB / TEAMS; ++j) {
        const int64_t row = (int64_t)blockIdx.x * VQ_LN_SLAB + j * TEAMS + team;
        if (row >= a.R) break;                                                  // (uniform in the team; T == 256: in the workgroup)
        const xraw *in = reinterpret_cast<const xraw *>(a.x) + row * a.D;
        const yraw *gin = reinterpret_cast<const yraw *>(a.g) + row * a.D;
        const float mean = RMS ? 0.0f : a.stats[row * 2], rstd = a.stats[row * 2 + 1];
        float xh[NP][PW], gu[NP][PW];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const uint32_t c0 = (uint32_t)(k * T + t) * PW;
            if (cnt[k] > 0) {
                gn_load<XDT, PW>(in + c0, PW, xh[k]);
                gn_load<YDT, PW>(gin + c0, PW, gu[k]);
#pragma unroll
                for (int e = 0; e < PW; ++e) {
                    const float h = RMS ? xh[k][e] * rstd : (xh[k][e] - mean) * rstd, tt = gu[k][e] * a.gamma[c0 + e];
                    xh[k][e] = h;
                    if (!RMS) s1 = s1 + tt;
                    s2 = s2 + tt * h;
                    dg[k][e] = dg[k][e] + gu[k][e] * h;
                    if (!RMS) db[k][e] = db[k][e] + gu[k][e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < PW; ++e) { xh[k][e] = 0.0f; gu[k][e] = 0.0f; }
            }
        }
        if (!RMS) s1 = gn_team_sum<T>(s1, red);
        s2 = gn_team_sum<T>(s2, red);
        const float m1 = s1 / (float)a.D, m2 = s2 / (float)a.D;
        xraw *out = reinterpret_cast<xraw *>(a.out) + row * a.D;
        const xraw *skip = reinterpret_cast<const xraw *>(a.res) + row * a.D;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (cnt[k] == 0) continue;
            const uint32_t c0 = (uint32_t)(k * T + t) * PW;
            float gx[PW];
#pragma unroll
            for (int e = 0; e < PW; ++e) {
                if (RMS) gx[e] = rstd * (gu[k][e] * a.gamma[c0 + e] - xh[k][e] * m2);
                else gx[e] = rstd * ((gu[k][e] * a.gamma[c0 + e] - m1) - xh[k][e] * m2);
            }
            if (a.res) {
                float sv[PW];
                gn_load<XDT, PW>(skip + c0, PW, sv);
#pragma unroll
                for (int e = 0; e < PW; ++e) gx[e] = gx[e] + sv[e];
            }
            gn_store<XDT, PW>(out + c0, PW, gx);
        }
    }
    // the slab's column sums: every (slab, column) is written, by the thread of team 0 that holds the column
    float *wdg = a.ws_dg + (int64_t)blockIdx.x * a.D, *wdb = a.ws_db + (int64_t)blockIdx.x * a.D;
    if (TEAMS == 1) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const uint32_t c0 = (uint32_t)(k * T + t) * PW;
#pragma unroll
            for (int e = 0; e < PW; ++e)
                if (e < cnt[k]) {
                    wdg[c0 + e] = dg[k][e];
                    if (!RMS) wdb[c0 + e] = db[k][e];
                }
        }
    } else {
#pragma unroll
        for (int pass = 0; pass < (RMS ? 1 : 2); ++pass) {
            __syncthreads();                                                    // the readers of the first pass are done
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const uint32_t c0 = (uint32_t)(k * T + t) * PW;
#pragma unroll
                for (int e = 0; e < PW; ++e)
                    if (e < cnt[k]) part[team * VQ_GN_SMALL + c0 + e] = pass == 0 ? dg[k][e] : db[k][e];    // c0 + e < D <= 2048
            }
            __syncthreads();
            if (team == 0) {
                float *w = pass == 0 ? wdg : wdb;
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const uint32_t c0 = (uint32_t)(k * T + t) * PW;
#pragma unroll
                    for (int e = 0; e < PW; ++e)
                        if (e < cnt[k]) {
                            const float *p = part + c0 + e;
                            w[c0 + e] = (p[0] + p[VQ_GN_SMALL]) + (p[2 * VQ_GN_SMALL] + p[3 * VQ_GN_SMALL]);
                        }
                }
            }
        }
    }
}

// ---- row bias-activation -------------------------------------------------------------------------------------------------------
struct VqRowActArgs {
    const void *x;
    const void *g;                              // backward: the incoming gradient
    const float *bias;                          // [D]
    void *out;                                  // y (forward) / gx (backward)
    float *ws;                                  // [slabs, D] (backward)
    int64_t R;
    int D;
};

template <int ACT>
__device__ __forceinline__ float vit_act(float t) {
    if (ACT == VQHIP_ROW_ACT_GELU) return (0.5f * t) * (1.0f + erff(t * VQ_VIT_RSQRT2));
    return tanhf(t);
}

template <int ACT>
__device__ __forceinline__ float vit_act_grad(float t) {
    if (ACT == VQHIP_ROW_ACT_GELU) return 0.5f * (1.0f + erff(t * VQ_VIT_RSQRT2)) + t * (expf(-0.5f * (t * t)) * VQ_VIT_RSQRT2PI);
    const float y = tanhf(t);
    return 1.0f - y * y;
}

template <int DT, int ACT>
__global__ __launch_bounds__(VQ_SG2_THREADS) void row_act_fwd_kernel(VqRowActArgs a) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    const raw *in = reinterpret_cast<const raw *>(a.x);
    raw *out = reinterpret_cast<raw *>(a.out);
    const uint32_t n = (uint32_t)(a.R * a.D), D = (uint32_t)a.D;                // R D < 2^31
    const uint32_t pieces = (n + W - 1) / W;
    for (uint32_t q = blockIdx.x * VQ_SG2_THREADS + threadIdx.x; q < pieces; q += gridDim.x * VQ_SG2_THREADS) {
        const uint32_t i0 = q * W;                                              // pieces * W < 2^31 + 8
        const int cnt = n - i0 < (uint32_t)W ? (int)(n - i0) : W;
        float x[W];
        sg2_load<DT>(in + i0, cnt, x);
        uint32_t c = i0 % D;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            x[e] = vit_act<ACT>(x[e] + a.bias[c]);
            if (++c == D) c = 0;
        }
        sg2_store<DT>(out + i0, cnt, x);
    }
}

template <int DT, int ACT>
__global__ __launch_bounds__(VQ_SG2_THREADS) void row_act_bwd_kernel(VqRowActArgs a) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    __shared__ float red[4][64][W];
    const int lane = threadIdx.x & 63, group = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * VQ_SG2_ROWS_SLAB;
    const int c0 = ((int)blockIdx.y * 64 + lane) * W;
    const int cnt = c0 >= a.D ? 0 : (a.D - c0 < W ? a.D - c0 : W);
    float acc[W], b[W];
#pragma unroll
    for (int e = 0; e < W; ++e) { acc[e] = 0.0f; b[e] = e < cnt ? a.bias[c0 + e] : 0.0f; }
    if (cnt > 0) {
        const raw *g = reinterpret_cast<const raw *>(a.g);
        const raw *x = reinterpret_cast<const raw *>(a.x);
        raw *out = reinterpret_cast<raw *>(a.out);
        for (int j = group; j < VQ_SG2_ROWS_SLAB && r0 + j < a.R; j += 4) {
            const int64_t off = (r0 + j) * a.D + c0;
            float gv[W], xv[W];
            sg2_load<DT>(g + off, cnt, gv);
            sg2_load<DT>(x + off, cnt, xv);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                gv[e] = gv[e] * vit_act_grad<ACT>(xv[e] + b[e]);
                if (e < cnt) acc[e] = acc[e] + gv[e];
            }
            sg2_store<DT>(out + off, cnt, gv);
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) red[group][lane][e] = acc[e];
    __syncthreads();
    if (group != 0 || cnt == 0 || !a.ws) return;
    for (int e = 0; e < cnt; ++e)
        a.ws[(int64_t)blockIdx.x * a.D + c0 + e] = (red[0][lane][e] + red[1][lane][e]) + (red[2][lane][e] + red[3][lane][e]);
}

// ---- SwiGLU (act == VQHIP_ROW_ACT_SWIGLU): x [R, 2F] = (gate | up), y and g [R, F], gx [R, 2F] ---------------------------------------
// One thread per 16-byte piece of the flat [R, F] side (y forward, g backward), the grid of row_act_fwd_kernel: up to 8192
// workgroups, a stride beyond.  A piece that lies inside a row (always where F % W == 0) reads its gate and its up values as two
// pieces of x; one that crosses a row end goes element by element.  No sum: nothing but the element's own (gate, up, g) enters.
#define VQ_SWIGLU_CLAMP 88.0f                   // expf sees [-88, 0]: the range VQHIP_VIT_EXP_ULPS was measured over

// e = exp(-|a|) with the argument held at -88 (a NaN passes through a itself, below)
__device__ __forceinline__ float swiglu_exp(float a) { return expf(fmaxf(-fabsf(a), -VQ_SWIGLU_CLAMP)); }

// silu(a) = a / (1 + e) for a >= 0, (a e) / (1 + e) for a < 0 (and for a NaN, which so stays one)
__device__ __forceinline__ float swiglu_silu(float a, float e) { return (a >= 0.0f ? a : a * e) / (1.0f + e); }

template <int DT, bool BWD>
__global__ __launch_bounds__(VQ_SG2_THREADS) void swiglu_kernel(VqRowActArgs a) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    const raw *in = reinterpret_cast<const raw *>(a.x);
    const raw *gin = reinterpret_cast<const raw *>(a.g);
    raw *out = reinterpret_cast<raw *>(a.out);
    const uint32_t F = (uint32_t)a.D, n = (uint32_t)(a.R * a.D);                // R 2F < 2^31
    const uint32_t pieces = (n + W - 1) / W;
    for (uint32_t q = blockIdx.x * VQ_SG2_THREADS + threadIdx.x; q < pieces; q += gridDim.x * VQ_SG2_THREADS) {
        const uint32_t i0 = q * W;
        const int cnt = n - i0 < (uint32_t)W ? (int)(n - i0) : W;
        const uint32_t r = i0 / F, c = i0 - r * F;
        const bool whole = c + (uint32_t)cnt <= F;                              // the piece ends inside its row
        const uint32_t x0 = r * 2u * F + c;                                     // its first gate; x0 + F + cnt <= R 2F
        float ga[W], up[W], gv[W];
        if (whole) {
            sg2_load<DT>(in + x0, cnt, ga);
            sg2_load<DT>(in + x0 + F, cnt, up);
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const uint32_t i = i0 + e, re = i / F, xe = re * 2u * F + (i - re * F);
                ga[e] = e < cnt ? E::f32(in[xe]) : 0.0f;
                up[e] = e < cnt ? E::f32(in[xe + F]) : 0.0f;
            }
        }
        if (BWD) sg2_load<DT>(gin + i0, cnt, gv);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const float ex = swiglu_exp(ga[e]), den = 1.0f + ex;
            const float s = swiglu_silu(ga[e], ex);
            if (!BWD) {
                ga[e] = s * up[e];
            } else {
                // sg = sigmoid(a) and qc = 1 - sg, each from e without a subtraction
                const float sg = (ga[e] >= 0.0f ? 1.0f : ex) / den, qc = (ga[e] >= 0.0f ? ex : 1.0f) / den;
                const float d = sg * (1.0f + ga[e] * qc);
                ga[e] = (gv[e] * up[e]) * d;
                up[e] = gv[e] * s;
            }
        }
        if (!BWD) {
            sg2_store<DT>(out + i0, cnt, ga);
        } else if (whole) {
            sg2_store<DT>(out + x0, cnt, ga);
            sg2_store<DT>(out + x0 + F, cnt, up);
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const uint32_t i = i0 + e, re = i / F, xe = re * 2u * F + (i - re * F);
                if (e < cnt) { out[xe] = ce_round<DT>(ga[e]); out[xe + F] = ce_round<DT>(up[e]); }
            }
        }
    }
}
