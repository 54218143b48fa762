// libvqhip device kernels, unit 8: the column pass's copies (bf16 -> fp32, listed rows) and the verification aids.  Owned by vqhip.hip.
#pragma once
#include "vqhip_kernels.h"
#include "vqhip_proposal_kernels.h"
#include "vqhip_refine_kernels.h"
// bf16 -> fp32 copy (the column pass needs the latents as an fp32 "codebook")
__global__ void bf16_to_f32_kernel(const uint16_t *in, int64_t n, float *out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = bf16_to_f32(in[i]);
}

// out[i] = e[rows[i]] for i < count, zeros up to cap (the role-swapped pipeline reads whole 32-row blocks)
__global__ void gather_listed_rows_kernel(const float *__restrict__ e, const int32_t *__restrict__ rows,
                                          const int32_t *__restrict__ count, int64_t cap, int D, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= cap) return;
    const bool live = i < (int64_t)count[0];
    const int64_t k = live ? rows[i] : 0;
    for (int d = lane; d < D; d += 64) out[i * D + d] = live ? e[k * D + d] : 0.0f;
}

// ------------------------------------------------------------------------------------------------
// verification aid: the proposal scores of every (row, code) pair and the margin the decision uses
// ------------------------------------------------------------------------------------------------
// Same operands and MFMA sequence as coarse_kernel / rescan_kernel; one wave per (64 rows, stage).  Lets a test check
// |score - exact score| <= margin/2 for every pair against float64 (tests/test_gpu_parity.py::test_margin_holds).
template <int NSTEP, int TPS>
__global__ __launch_bounds__(256) void debug_scores_kernel(const char *__restrict__ ximg, const char *__restrict__ frag,
                                                           int64_t nstages, int64_t N, int64_t K, float *__restrict__ out) {
    constexpr int NS32 = NSTEP / 2;
    constexpr int NCH = TPS * NSTEP + VQ_AUX_CHUNKS(TPS);
    constexpr int STAGE_BYTES = NCH * VQ_CHUNK_BYTES;
    constexpr int TR = (NSTEP <= 16) ? 4 : (NSTEP <= 48 ? 2 : 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ngroups = (N + 16 * TR - 1) / (16 * TR);
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < ngroups * nstages; item += (int64_t)gridDim.x * 4) {
        const int64_t fg = item / nstages, st = item % nstages;
        half8 xf[TR][NS32];
        int64_t tok[TR];
#pragma unroll
        for (int t = 0; t < TR; ++t) {
            tok[t] = fg * 16 * TR + t * 16 + (lane & 15);
            const int64_t tk = tok[t] < N ? tok[t] : N - 1;
            const char *xsrc = ximg + (tk >> 4) * (int64_t)(NS32 * VQ_CHUNK_BYTES) + ((lane >> 4) * 16 + (int)(tk & 15)) * 16;
#pragma unroll
            for (int s = 0; s < NS32; ++s) xf[t][s] = *(const half8 *)(xsrc + s * VQ_CHUNK_BYTES);
        }
        const char *base = frag + st * (int64_t)STAGE_BYTES;
        const char *aux = base + TPS * NSTEP * VQ_CHUNK_BYTES;
#pragma unroll 1
        for (int ti = 0; ti < TPS; ++ti) {
            f32x4 acc[2][TR];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                f32x4 a4 = *(const f32x4 *)(aux + (ti * 32 + 16 * c + 4 * (lane >> 4)) * 4);
#pragma unroll
                for (int t = 0; t < TR; ++t) acc[c][t] = a4;
            }
#pragma unroll
            for (int ch = 0; ch < NSTEP; ++ch) {
                half8 a = *(const half8 *)(base + (ti * NSTEP + ch) * VQ_CHUNK_BYTES + lane * 16);
#pragma unroll
                for (int t = 0; t < TR; ++t)
                    acc[ch & 1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, xf[t][ch >> 1], acc[ch & 1][t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < TR; ++t)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int64_t k = (st * TPS + ti) * 32 + tile_row16(e, lane);
                    if (tok[t] < N && k < K) out[tok[t] * K + k] = acc[e >> 2][t][e & 3];
                }
        }
    }
}

__global__ void debug_margin_kernel(const char *cb, VqCbLayout L, int64_t N, int metric, const float *xh2, const float *rho2,
                                    float *margin, float *scale) {
    int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const VqCbStats stv = cb_stats_view((const VqCbStats *)(cb + L.off_stats));
    const VqCbStats *st = &stv;
    if (n == 0) scale[0] = cb_scale(st);
    if (n < N) margin[n] = row_margin(st, L.Dp, metric, xh2[n], rho2[n]);
}
