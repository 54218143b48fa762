// GroupNorm with an optional fused SiLU, forward and backward: the step in front of every convolution of VQGANEncoder /
// VQGANDecoder (vq/algorithms/vqgan/autoencoder.py: GroupNorm(32, C, 1e-6) -> SiLU at 25 + 35 sites of the default pair, GroupNorm alone in Attention).
//
// Contract: include/vqhip.h (vqhip_group_norm_fwd / _bwd), DESIGN.md §8.  Every element is converted to fp32 exactly (SampleElem of
// the sampler); all arithmetic is fp32 IEEE without contraction; results are rounded to nearest even into the output dtype
// (ce_round of the token cross-entropy).
//
// WHO OWNS WHAT  A group (b, g) has n = (C / G) P values.  They are numbered 0 .. n - 1 in the order of the memory: MAP (NCHW) is one
//   contiguous run, value e in channel e / P; ROWS (channels-last) takes the C / G adjacent channels of position 0, then of position
//   1, ..  The numbering is cut into PIECES of PW values that are adjacent in memory (MAP: PW = 16 bytes / element; ROWS: the
//   largest of 16, 8 or one element's bytes that divides C / G, so a piece never leaves its position) and into CHUNKS of
//   T x 32 values.  A TEAM of T threads owns one chunk: thread t holds pieces t, t + T, .. of the chunk, 32 values in registers.
//   n <= 2048: T = 64, one wave per group, four groups per workgroup, no LDS.  n > 2048: T = 256, a workgroup per chunk of 8192,
//   S = ceil(n / 8192) chunks per group.  S == 1: one launch does everything from the registers (one read, one write).  S > 1: a
//   first launch leaves one partial per chunk in the workspace, a second launch, behind the launch boundary, combines the S
//   partials of its group in a fixed order (every workgroup of the group forms the same bits) and applies them to its chunk.
// ORDER OF A TEAM'S SUM  a thread adds its values in increasing piece and element into one accumulator from +0; the 64 lanes of
//   a wave add as an xor butterfly (1, 2, .. 32); the 4 waves as (w0 + w1) + (w2 + w3).  S partials: thread t adds partials t, t + 256,
//   .. in that order, then the same team sum.  No atomics anywhere: the same input gives the same bits, run to run.
// FORWARD  mean_c = sum / n_c of the chunk; M2_c = sum (x - mean_c)^2 over the values in the registers (the second pass).  S > 1:
//   mean = sum_c n_c mean_c / n and M2 = sum_c (M2_c + n_c (mean_c - mean)^2): the exact recombination of shifted sums, every term
//   non-negative, nothing cancels.  var = M2 / n, rstd = 1 / sqrt(var + eps), u = ((x - mean) rstd) gamma[c] + beta[c],
//   y = u (act 0) or u / (1 + exp(-u)) (act 1).  stats[2 (b G + g)] = (mean, rstd).
// BACKWARD  from x and stats: xh = (x - mean) rstd, u as above, d = 1 (act 0) or s (1 + u (1 - s)) with s = 1 / (1 + exp(-u)),
//   gu = g d, t = gu gamma[c].  m1 = sum t / n, m2 = sum (t xh) / n by the team sums above (S > 1: per-chunk sums in the workspace,
//   combined in the second launch), gx = rstd ((t - m1) - xh m2).  dgamma / dbeta: the first launch writes, for its SLAB (b, chunk)
//   and every channel cl of its group, the team sum of gu xh / of gu over the values of the chunk in that channel (a channel the
//   chunk does not touch gets +0) to ws[slab C + c]: every (slab, c) is written, so ws needs no memset; sg2_reduce_kernel adds the
//   slabs (vqhip_stylegan2_kernels.h).
// Every global index is guarded: a piece beyond n is neither loaded nor stored; a team beyond B G returns before any access.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_sample_kernels.h"               // SampleElem: the exact conversion to fp32
#include "vqhip_token_ce_kernels.h"             // ce_round: nearest even into the output dtype

#define VQ_GN_THREADS 256
#define VQ_GN_EPT 32                            // values a thread holds in registers
#define VQ_GN_SMALL (64 * VQ_GN_EPT)            // n up to here: one wave per group
#define VQ_GN_CHUNK (VQ_GN_THREADS * VQ_GN_EPT) // values per workgroup beyond it
#define VQ_GN_ALL 0                             // one launch: statistics and result from the registers
#define VQ_GN_PART 1                            // first launch of a split group: the chunk's partials
#define VQ_GN_APPLY 2                           // second launch: combine the partials, apply

struct VqGnArgs {
    const void *x;
    const void *g;                              // backward: the incoming gradient
    void *out;                                  // y (forward) / gx (backward)
    const float *gamma, *beta;                  // [C]
    float *stats;                               // [B G 2]: mean, rstd (written forward, read backward)
    float *ws_grp;                              // [B G S 2] partials of split groups
    float *ws_dg, *ws_db;                       // [B S, C] each (backward)
    int64_t units;                              // B G S teams
    uint32_t n;                                 // (C / G) P < 2^31
    int B, C, P, G, cpg, S;
    float eps;
    int act, phase;
};

template <int DT, int PW>
__device__ __forceinline__ void gn_load(const typename SampleElem<DT>::raw *p, int cnt, float (&x)[PW]) {
    typename SampleElem<DT>::raw v[PW];
    if (cnt == PW) {
        __builtin_memcpy(v, p, sizeof(v));
    } else {
#pragma unroll
        for (int e = 0; e < PW; ++e) v[e] = e < cnt ? p[e] : (typename SampleElem<DT>::raw)0;
    }
#pragma unroll
    for (int e = 0; e < PW; ++e) x[e] = SampleElem<DT>::f32(v[e]);
}

template <int DT, int PW>
__device__ __forceinline__ void gn_store(typename SampleElem<DT>::raw *p, int cnt, const float (&x)[PW]) {
    typename SampleElem<DT>::raw v[PW];
#pragma unroll
    for (int e = 0; e < PW; ++e) v[e] = ce_round<DT>(x[e]);
    if (cnt == PW) {
        __builtin_memcpy(p, v, sizeof(v));
    } else {
#pragma unroll
        for (int e = 0; e < PW; ++e)
            if (e < cnt) p[e] = v[e];
    }
}

// piece k of thread t of chunk s of group (b, g): where it lies, how many of its values exist, the channel of its first value
struct GnPiece {
    int64_t off;                                // element offset into the tensor
    int cnt;                                    // 0 .. PW
    uint32_t lc, rem;                           // channel inside the group, position inside the plane (MAP) of the first value
};

template <bool ROWS, int PW, int T>
__device__ __forceinline__ GnPiece gn_piece(const VqGnArgs &a, int b, int g, uint32_t s, int k, int t) {
    GnPiece p;
    const uint32_t pi = s * (uint32_t)(T * VQ_GN_EPT / PW) + (uint32_t)(k * T + t);      // pi PW < n + chunk < 2^32
    if (ROWS) {
        const uint32_t ppp = (uint32_t)a.cpg / PW;                                          // pieces per position
        const uint32_t pos = pi / ppp, j = (pi - pos * ppp) * PW;
        p.cnt = pos < (uint32_t)a.P ? PW : 0;
        p.off = ((int64_t)b * a.P + pos) * a.C + (int64_t)g * a.cpg + j;
        p.lc = j; p.rem = 0;
    } else {
        const uint32_t e0 = pi * PW;
        p.cnt = e0 >= a.n ? 0 : (a.n - e0 < (uint32_t)PW ? (int)(a.n - e0) : PW);
        p.off = ((int64_t)b * a.C + (int64_t)g * a.cpg) * a.P + e0;
        p.lc = e0 / (uint32_t)a.P; p.rem = e0 - p.lc * (uint32_t)a.P;
    }
    return p;
}

// the channel (inside the group) of the next value of a piece: ROWS steps a channel, MAP a position of the plane
template <bool ROWS>
__device__ __forceinline__ void gn_next(const VqGnArgs &a, uint32_t &lc, uint32_t &rem) {
    if (ROWS) { ++lc; }
    else if (++rem == (uint32_t)a.P) { rem = 0; ++lc; }
}

// the team's sum, valid in every thread of the team.  T == 256: every thread of the workgroup calls it.
template <int T>
__device__ __forceinline__ float gn_team_sum(float v, float *red /* [4] in LDS */) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    if (T == 256) {
        __syncthreads();                                                        // the readers of the previous sum are done
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = (red[0] + red[1]) + (red[2] + red[3]);
    }
    return v;
}

// mean and M2 = sum (x - mean)^2 of the nc values a team holds in registers (FORWARD above; shared with the row norm of
// vqhip_vit_kernels.h): a value counts where its piece has it (e < cnt[k])
template <int T, int NP, int PW>
__device__ __forceinline__ void gn_mean_m2(const float (&xv)[NP][PW], const int (&cnt)[NP], float nc, float *red, float &mean, float &m2) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < PW; ++e)
            if (e < cnt[k]) acc = acc + xv[k][e];
    mean = gn_team_sum<T>(acc, red) / nc;
    acc = 0.0f;
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < PW; ++e)
            if (e < cnt[k]) { const float d = xv[k][e] - mean; acc = acc + d * d; }
    m2 = gn_team_sum<T>(acc, red);
}

__device__ __forceinline__ float gn_sigmoid(float u) { return 1.0f / (1.0f + expf(-u)); }

// values of chunk c of a group of n
__device__ __forceinline__ float gn_chunk_count(uint32_t n, uint32_t c) {
    const uint32_t lo = c * (uint32_t)VQ_GN_CHUNK;
    return (float)(n - lo < (uint32_t)VQ_GN_CHUNK ? n - lo : (uint32_t)VQ_GN_CHUNK);
}

template <int T>
struct GnTeam {
    int t, b, g;
    uint32_t s;
    int64_t bg, unit;
    bool live;
    __device__ __forceinline__ GnTeam(const VqGnArgs &a) {
        t = threadIdx.x % T;
        unit = (int64_t)blockIdx.x * (VQ_GN_THREADS / T) + threadIdx.x / T;
        live = unit < a.units;
        const int64_t u = live ? unit : 0;
        bg = u / a.S; s = (uint32_t)(u - bg * a.S);
        b = (int)(bg / a.G); g = (int)(bg - (int64_t)b * a.G);
    }
};

template <int DT, bool ROWS, int PW, int T>
__global__ __launch_bounds__(VQ_GN_THREADS) void gn_fwd_kernel(VqGnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    constexpr int NP = VQ_GN_EPT / PW;
    __shared__ float red[4];
    const GnTeam<T> tm(a);
    if (!tm.live) return;                                                       // (T == 64 only: a T == 256 grid has no spare team)
    const raw *in = reinterpret_cast<const raw *>(a.x);
    float xv[NP][PW];
    int cnt[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const GnPiece p = gn_piece<ROWS, PW, T>(a, tm.b, tm.g, tm.s, k, tm.t);
        cnt[k] = p.cnt;
        if (p.cnt > 0) {
            gn_load<DT, PW>(in + p.off, p.cnt, xv[k]);
        } else {
#pragma unroll
            for (int e = 0; e < PW; ++e) xv[k][e] = 0.0f;
        }
    }
    float mean, m2;
    if (a.phase != VQ_GN_APPLY) {
        gn_mean_m2<T, NP, PW>(xv, cnt, a.S == 1 ? (float)a.n : gn_chunk_count(a.n, tm.s), red, mean, m2);
        if (a.phase == VQ_GN_PART) {
            if (tm.t == 0) { a.ws_grp[tm.unit * 2] = mean; a.ws_grp[tm.unit * 2 + 1] = m2; }
            return;
        }
    } else {
        const float *part = a.ws_grp + tm.bg * a.S * 2;
        float acc = 0.0f;
        for (int c = tm.t; c < a.S; c += T) acc = acc + gn_chunk_count(a.n, (uint32_t)c) * part[2 * c];
        mean = gn_team_sum<T>(acc, red) / (float)a.n;
        acc = 0.0f;
        for (int c = tm.t; c < a.S; c += T) {
            const float d = part[2 * c] - mean;
            acc = acc + (part[2 * c + 1] + gn_chunk_count(a.n, (uint32_t)c) * (d * d));
        }
        m2 = gn_team_sum<T>(acc, red);
    }
    const float rstd = 1.0f / sqrtf(m2 / (float)a.n + a.eps);
    if (tm.t == 0 && tm.s == 0) { a.stats[tm.bg * 2] = mean; a.stats[tm.bg * 2 + 1] = rstd; }
    raw *out = reinterpret_cast<raw *>(a.out);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (cnt[k] == 0) continue;
        const GnPiece p = gn_piece<ROWS, PW, T>(a, tm.b, tm.g, tm.s, k, tm.t);
        uint32_t lc = p.lc, rem = p.rem;
        float y[PW];
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            y[e] = 0.0f;
            if (e < p.cnt) {
                const int c = tm.g * a.cpg + (int)lc;
                const float u = ((xv[k][e] - mean) * rstd) * a.gamma[c] + a.beta[c];
                y[e] = a.act ? u * gn_sigmoid(u) : u;
                gn_next<ROWS>(a, lc, rem);
            }
        }
        gn_store<DT, PW>(out + p.off, p.cnt, y);
    }
}

template <int DT, bool ROWS, int PW, int T>
__global__ __launch_bounds__(VQ_GN_THREADS) void gn_bwd_kernel(VqGnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    constexpr int NP = VQ_GN_EPT / PW;
    __shared__ float red[4];
    const GnTeam<T> tm(a);
    if (!tm.live) return;
    const raw *in = reinterpret_cast<const raw *>(a.x);
    const raw *gin = reinterpret_cast<const raw *>(a.g);
    const float mean = a.stats[tm.bg * 2], rstd = a.stats[tm.bg * 2 + 1];
    float xh[NP][PW], gu[NP][PW];                                               // xh, then g d
    int cnt[NP];
    uint32_t lc0[NP], rem0[NP];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const GnPiece p = gn_piece<ROWS, PW, T>(a, tm.b, tm.g, tm.s, k, tm.t);
        cnt[k] = p.cnt; lc0[k] = p.lc; rem0[k] = p.rem;
        if (p.cnt > 0) {
            gn_load<DT, PW>(in + p.off, p.cnt, xh[k]);
            gn_load<DT, PW>(gin + p.off, p.cnt, gu[k]);
        }
        uint32_t lc = p.lc, rem = p.rem;
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            if (e < p.cnt) {
                const int c = tm.g * a.cpg + (int)lc;
                const float gam = a.gamma[c];
                const float h = (xh[k][e] - mean) * rstd;
                float d = 1.0f;
                if (a.act) {
                    const float u = h * gam + a.beta[c];
                    const float s = gn_sigmoid(u);
                    d = s * (1.0f + u * (1.0f - s));
                }
                const float v = gu[k][e] * d, t = v * gam;
                xh[k][e] = h; gu[k][e] = v;
                s1 = s1 + t; s2 = s2 + t * h;
                gn_next<ROWS>(a, lc, rem);
            } else {
                xh[k][e] = 0.0f; gu[k][e] = 0.0f;
            }
        }
    }
    if (a.phase != VQ_GN_APPLY) {
        s1 = gn_team_sum<T>(s1, red);
        s2 = gn_team_sum<T>(s2, red);
        // dgamma / dbeta partials of slab (b, s): one team sum per channel of the group
        const uint32_t lo = tm.s * (uint32_t)(T * VQ_GN_EPT);
        const uint32_t hi = a.n - lo < (uint32_t)(T * VQ_GN_EPT) ? a.n : lo + (uint32_t)(T * VQ_GN_EPT);
        const int64_t row = ((int64_t)tm.b * a.S + tm.s) * a.C + (int64_t)tm.g * a.cpg;
        for (int cl = 0; cl < a.cpg; ++cl) {
            const bool touched = ROWS || ((uint64_t)cl * (uint32_t)a.P < hi && ((uint64_t)cl + 1) * (uint32_t)a.P > lo);   // (uniform in the team)
            float dg = 0.0f, db = 0.0f;
            if (touched) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    uint32_t lc = lc0[k], rem = rem0[k];
#pragma unroll
                    for (int e = 0; e < PW; ++e) {
                        if (e < cnt[k]) {
                            if (lc == (uint32_t)cl) { dg = dg + gu[k][e] * xh[k][e]; db = db + gu[k][e]; }
                            gn_next<ROWS>(a, lc, rem);
                        }
                    }
                }
                dg = gn_team_sum<T>(dg, red);
                db = gn_team_sum<T>(db, red);
            }
            if (tm.t == 0) { a.ws_dg[row + cl] = dg; a.ws_db[row + cl] = db; }
        }
        if (a.phase == VQ_GN_PART) {
            if (tm.t == 0) { a.ws_grp[tm.unit * 2] = s1; a.ws_grp[tm.unit * 2 + 1] = s2; }
            return;
        }
    } else {
        const float *part = a.ws_grp + tm.bg * a.S * 2;
        s1 = 0.0f; s2 = 0.0f;
        for (int c = tm.t; c < a.S; c += T) { s1 = s1 + part[2 * c]; s2 = s2 + part[2 * c + 1]; }
        s1 = gn_team_sum<T>(s1, red);
        s2 = gn_team_sum<T>(s2, red);
    }
    const float m1 = s1 / (float)a.n, m2 = s2 / (float)a.n;
    raw *out = reinterpret_cast<raw *>(a.out);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (cnt[k] == 0) continue;
        const GnPiece p = gn_piece<ROWS, PW, T>(a, tm.b, tm.g, tm.s, k, tm.t);
        uint32_t lc = p.lc, rem = p.rem;
        float gx[PW];
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            gx[e] = 0.0f;
            if (e < p.cnt) {
                const float t = gu[k][e] * a.gamma[tm.g * a.cpg + (int)lc];
                gx[e] = rstd * ((t - m1) - xh[k][e] * m2);
                gn_next<ROWS>(a, lc, rem);
            }
        }
        gn_store<DT, PW>(out + p.off, p.cnt, gx);
    }
}
