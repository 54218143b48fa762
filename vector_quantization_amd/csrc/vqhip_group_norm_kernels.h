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
#include "vqhip_elem.h"                         // SampleElem: the exact conversion to fp32; ce_round: nearest even into the output dtype

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

// y = act(u) and d = act'(u) of the batch-statistics kernels below.  LeakyReLU: u == 0 (and a NaN) takes the slope in both, as
// F.leaky_relu does; the backward calls these on the u it recomputes with the forward's own instructions, so both directions agree
// on the branch.
__device__ __forceinline__ float gn_act(float u, int act) {
    if (act == 1) return u * gn_sigmoid(u);
    if (act == VQHIP_GN_ACT_LEAKY) return u > 0.0f ? u : VQHIP_GN_LEAKY_SLOPE * u;
    return u;
}

__device__ __forceinline__ float gn_act_grad(float u, int act) {
    if (act == 1) { const float s = gn_sigmoid(u); return s * (1.0f + u * (1.0f - s)); }
    return u > 0.0f ? 1.0f : VQHIP_GN_LEAKY_SLOPE;
}

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

// ---- batch statistics (G == VQHIP_GN_BATCH): BatchNorm2d (+ LeakyReLU) of PatchGANDiscriminator ----------------------------------
// One group per channel over all B images: n = B P values, numbered b P + p.  The definition, the conversions and the value u are
// the ones above; what differs is who owns what, because a channel is not contiguous in either layout.
//
// MAP (NCHW)  a channel is B runs of P values, C P apart.  The numbering is cut into pieces of PW = 16 bytes / element values and
//   chunks of 8192 exactly as above (T = 256): S = ceil(n / 8192) workgroups per channel, C S workgroups.  A piece that lies inside
//   one run is one 16-byte access at element alignment (P = 961 in bf16 starts its runs at odd offsets); a piece that crosses the
//   end of a run - one in P / PW - is read and written element by element, hopping (C - 1) P from the end of a run to the next.
// ROWS (channels-last)  value e of channel c lies at e C + c.  A workgroup takes a TILE of 8 PW adjacent channels (PW as in the
//   rows layout above: the widest of 16 bytes, 8 bytes, one element that divides C) and a SLAB of 1024 / PW positions: lane
//   lx = t % 8 owns the PW channels (8 tile + lx) PW .., row ly = t / 8 the positions slab + ly, + 32, .. (32 / PW of them): a pass
//   of the workgroup reads 32 positions of 8 x 16 bytes each.  S = ceil(n PW / 1024) slabs per channel, ceil(C / (8 PW)) S
//   workgroups.  A thread sums down its positions per channel (32 / PW values; PW == 1: two halves of 16, then their sum), the
//   lanes of equal lx add as an xor butterfly (8, 16, 32), the 4 waves as (w0 + w1) + (w2 + w3) through LDS.
// S == 1  one launch: statistics from the registers, stats / the mean and unbiased-variance block / dgamma and dbeta written by
//   the workgroup, then the result.  S > 1: a first launch leaves the chunk's partial (mean_c, M2_c) - backward: (sum gu,
//   sum gu xh) - at part[(c S + s) 2]; n_c is a function of (n, s) and is not stored.  bn_combine_kernel, one workgroup per
//   channel, adds the S partials: thread t takes partials t, t + 256, .. (m = ceil(S / 256) of them) into an accumulator that is
//   flushed into a second after 8 terms, and that into a third after 64 (adding to +0 is exact, so m <= 8 is the plain chain of the
//   kernels above); then the team sum.  It writes stats and the block (backward: dgamma, dbeta).  A third launch applies them to
//   every chunk.  The combination is a launch of its own because a ROWS workgroup would otherwise read 8 PW S partials for
//   8192 values, several times its own traffic.
// ROUNDINGS INTO A SUM, against N = VQHIP_GN_CHAIN(n) = 56 + floor(n / 2^21)
//   MAP   32 (thread) + 6 (wave) + 2 (waves) + 1 (n_c mean_c) + combine + 8 (team) + 2 (divisions), S = ceil(n / 8192),
//         m <= n / 2^21 + 1: combine = m (m <= 8), 8 + ceil(m / 8) + 1 (m <= 64), 16 + ceil(m / 64) + 2 beyond: never above m + 4.
//   ROWS  32 / PW, or 17 for PW == 1 (thread) + 3 (wave) + 2 (waves) + 1 + combine + 8 + 2 <= 33 + combine; m <= n PW / 2^18 + 1, so
//         combine <= 18 + ceil(m / 64) <= 21 + n / 2^21.
//   The backward's two sums take the same paths without the product and with one division.
// Every global index is guarded: a piece beyond n (MAP), a position beyond n or a channel beyond C (ROWS) is neither loaded nor
// stored; the grids have no spare workgroup.
#define VQ_BN_LX 8                              // ROWS: lanes across the channels of a tile
#define VQ_BN_LY (VQ_GN_THREADS / VQ_BN_LX)     // ROWS: positions per pass

struct VqBnArgs {
    const void *x;
    const void *g;                              // backward: the incoming gradient
    void *out;                                  // y (forward) / gx (backward)
    const float *gamma, *beta;                  // [C]
    float *stats;                               // [C 2]: mean, rstd
    float *mv;                                  // [2 C]: mean, then M2 / (n - 1) (forward)
    float *part;                                // [C S 2] partials of split channels
    float *dgamma, *dbeta;                      // [C] (backward)
    uint32_t n;                                 // B P, 2 .. 2^31 - 1
    uint32_t chunk;                             // values of a channel per workgroup: 8192 (MAP) or 1024 / PW (ROWS)
    int B, C, P, S;
    float eps;
    int act, phase;
};

// values of chunk s of a channel
__device__ __forceinline__ float bn_chunk_count(const VqBnArgs &a, uint32_t s) {
    const uint32_t lo = s * a.chunk;
    return (float)(a.n - lo < a.chunk ? a.n - lo : a.chunk);
}

// thread t's share of a sum over i = t, t + 256, .. < S (COMBINE above)
template <class F>
__device__ __forceinline__ float bn_thread_sum(int S, F term) {
    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
    int i0 = 0, i1 = 0;
    for (int i = threadIdx.x; i < S; i += VQ_GN_THREADS) {
        l0 = l0 + term(i);
        if (++i0 == 8) {
            l1 = l1 + l0; l0 = 0.0f; i0 = 0;
            if (++i1 == 8) { l2 = l2 + l1; l1 = 0.0f; i1 = 0; }
        }
    }
    return l2 + (l1 + l0);
}

// one workgroup per channel: the S partials of the first launch into stats and the block (forward) or dgamma and dbeta (backward)
__global__ __launch_bounds__(VQ_GN_THREADS) void bn_combine_kernel(VqBnArgs a, int bwd) {
    __shared__ float red[4];
    const int c = blockIdx.x;
    const float *part = a.part + (int64_t)c * a.S * 2;
    if (bwd) {
        const float s1 = gn_team_sum<VQ_GN_THREADS>(bn_thread_sum(a.S, [&](int i) { return part[2 * i]; }), red);
        const float s2 = gn_team_sum<VQ_GN_THREADS>(bn_thread_sum(a.S, [&](int i) { return part[2 * i + 1]; }), red);
        if (threadIdx.x == 0) { a.dbeta[c] = s1; a.dgamma[c] = s2; }
        return;
    }
    const float mean = gn_team_sum<VQ_GN_THREADS>(bn_thread_sum(a.S, [&](int i) { return bn_chunk_count(a, (uint32_t)i) * part[2 * i]; }), red) / (float)a.n;
    const float m2 = gn_team_sum<VQ_GN_THREADS>(bn_thread_sum(a.S, [&](int i) {
        const float d = part[2 * i] - mean;
        return part[2 * i + 1] + bn_chunk_count(a, (uint32_t)i) * (d * d);
    }), red);
    if (threadIdx.x == 0) {
        a.stats[2 * c] = mean; a.stats[2 * c + 1] = 1.0f / sqrtf(m2 / (float)a.n + a.eps);
        a.mv[c] = mean; a.mv[a.C + c] = m2 / (float)(a.n - 1);
    }
}

// MAP: piece k of thread t of chunk s of channel c starts at value e0 of the channel
struct BnPiece {
    int64_t off;                                // element offset of its first value
    int cnt;                                    // 0 .. PW
    uint32_t p0;                                // position of the first value inside its run
};

template <int PW>
__device__ __forceinline__ BnPiece bn_map_piece(const VqBnArgs &a, int c, uint32_t s, int k) {
    BnPiece p;
    const uint32_t e0 = (s * (uint32_t)(VQ_GN_CHUNK / PW) + (uint32_t)(k * VQ_GN_THREADS) + threadIdx.x) * PW;   // < n + 8192 < 2^32
    p.cnt = e0 >= a.n ? 0 : (a.n - e0 < (uint32_t)PW ? (int)(a.n - e0) : PW);
    const uint32_t b = e0 / (uint32_t)a.P;
    p.p0 = e0 - b * (uint32_t)a.P;
    p.off = ((int64_t)b * a.C + c) * a.P + p.p0;
    return p;
}

template <int DT, int PW>
__device__ __forceinline__ void bn_map_load(const VqBnArgs &a, const typename SampleElem<DT>::raw *in, const BnPiece &p, float (&x)[PW]) {
    if (p.p0 + (uint32_t)p.cnt <= (uint32_t)a.P) { gn_load<DT, PW>(in + p.off, p.cnt, x); return; }
    int64_t off = p.off;
    uint32_t pos = p.p0;
#pragma unroll
    for (int e = 0; e < PW; ++e) {
        x[e] = 0.0f;
        if (e < p.cnt) {
            x[e] = SampleElem<DT>::f32(in[off]);
            ++off;
            if (++pos == (uint32_t)a.P) { pos = 0; off += (int64_t)(a.C - 1) * a.P; }
        }
    }
}

template <int DT, int PW>
__device__ __forceinline__ void bn_map_store(const VqBnArgs &a, typename SampleElem<DT>::raw *out, const BnPiece &p, const float (&x)[PW]) {
    if (p.p0 + (uint32_t)p.cnt <= (uint32_t)a.P) { gn_store<DT, PW>(out + p.off, p.cnt, x); return; }
    int64_t off = p.off;
    uint32_t pos = p.p0;
#pragma unroll
    for (int e = 0; e < PW; ++e) {
        if (e < p.cnt) {
            out[off] = ce_round<DT>(x[e]);
            ++off;
            if (++pos == (uint32_t)a.P) { pos = 0; off += (int64_t)(a.C - 1) * a.P; }
        }
    }
}

template <int DT, int PW>
__global__ __launch_bounds__(VQ_GN_THREADS) void bn_map_fwd_kernel(VqBnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    constexpr int NP = VQ_GN_EPT / PW;
    __shared__ float red[4];
    const int c = (int)(blockIdx.x / (uint32_t)a.S);
    const uint32_t s = blockIdx.x - (uint32_t)c * (uint32_t)a.S;
    const raw *in = reinterpret_cast<const raw *>(a.x);
    float xv[NP][PW];
    int cnt[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const BnPiece p = bn_map_piece<PW>(a, c, s, k);
        cnt[k] = p.cnt;
        if (p.cnt > 0) {
            bn_map_load<DT, PW>(a, in, p, xv[k]);
        } else {
#pragma unroll
            for (int e = 0; e < PW; ++e) xv[k][e] = 0.0f;
        }
    }
    float mean, rstd;
    if (a.phase != VQ_GN_APPLY) {
        float m2;
        gn_mean_m2<VQ_GN_THREADS, NP, PW>(xv, cnt, bn_chunk_count(a, s), red, mean, m2);
        if (a.phase == VQ_GN_PART) {
            if (threadIdx.x == 0) { a.part[(int64_t)blockIdx.x * 2] = mean; a.part[(int64_t)blockIdx.x * 2 + 1] = m2; }
            return;
        }
        rstd = 1.0f / sqrtf(m2 / (float)a.n + a.eps);
        if (threadIdx.x == 0) {
            a.stats[2 * c] = mean; a.stats[2 * c + 1] = rstd;
            a.mv[c] = mean; a.mv[a.C + c] = m2 / (float)(a.n - 1);
        }
    } else {
        mean = a.stats[2 * c]; rstd = a.stats[2 * c + 1];
    }
    const float gam = a.gamma[c], bet = a.beta[c];
    raw *out = reinterpret_cast<raw *>(a.out);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (cnt[k] == 0) continue;
        float y[PW];
#pragma unroll
        for (int e = 0; e < PW; ++e) y[e] = gn_act(((xv[k][e] - mean) * rstd) * gam + bet, a.act);
        bn_map_store<DT, PW>(a, out, bn_map_piece<PW>(a, c, s, k), y);
    }
}

template <int DT, int PW>
__global__ __launch_bounds__(VQ_GN_THREADS) void bn_map_bwd_kernel(VqBnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    constexpr int NP = VQ_GN_EPT / PW;
    __shared__ float red[4];
    const int c = (int)(blockIdx.x / (uint32_t)a.S);
    const uint32_t s = blockIdx.x - (uint32_t)c * (uint32_t)a.S;
    const raw *in = reinterpret_cast<const raw *>(a.x);
    const raw *gin = reinterpret_cast<const raw *>(a.g);
    const float mean = a.stats[2 * c], rstd = a.stats[2 * c + 1], gam = a.gamma[c], bet = a.beta[c];
    float xh[NP][PW], gu[NP][PW];                                               // xh, then g d
    int cnt[NP];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const BnPiece p = bn_map_piece<PW>(a, c, s, k);
        cnt[k] = p.cnt;
        if (p.cnt > 0) {
            bn_map_load<DT, PW>(a, in, p, xh[k]);
            bn_map_load<DT, PW>(a, gin, p, gu[k]);
        }
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            if (e < p.cnt) {
                const float h = (xh[k][e] - mean) * rstd;
                const float v = a.act ? gu[k][e] * gn_act_grad(h * gam + bet, a.act) : gu[k][e] * 1.0f;
                xh[k][e] = h; gu[k][e] = v;
                s1 = s1 + v; s2 = s2 + v * h;
            } else {
                xh[k][e] = 0.0f; gu[k][e] = 0.0f;
            }
        }
    }
    if (a.phase != VQ_GN_APPLY) {
        s1 = gn_team_sum<VQ_GN_THREADS>(s1, red);
        s2 = gn_team_sum<VQ_GN_THREADS>(s2, red);
        if (a.phase == VQ_GN_PART) {
            if (threadIdx.x == 0) { a.part[(int64_t)blockIdx.x * 2] = s1; a.part[(int64_t)blockIdx.x * 2 + 1] = s2; }
            return;
        }
        if (threadIdx.x == 0) { a.dbeta[c] = s1; a.dgamma[c] = s2; }
    } else {
        s1 = a.dbeta[c]; s2 = a.dgamma[c];
    }
    const float m1 = (s1 * gam) / (float)a.n, m2 = (s2 * gam) / (float)a.n;
    raw *out = reinterpret_cast<raw *>(a.out);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (cnt[k] == 0) continue;
        float gx[PW];
#pragma unroll
        for (int e = 0; e < PW; ++e) gx[e] = rstd * ((gu[k][e] * gam - m1) - xh[k][e] * m2);
        bn_map_store<DT, PW>(a, out, bn_map_piece<PW>(a, c, s, k), gx);
    }
}

// ROWS: where a thread's channels and positions lie
template <int PW>
struct BnRows {
    static constexpr int NP = VQ_GN_EPT / PW;
    int lx, c0;                                 // lane across the tile; first of the thread's PW channels
    uint32_t s, pos0;                           // slab; the thread's first position: positions pos0 + 32 k
    bool has;                                   // the channels exist
    __device__ __forceinline__ BnRows(const VqBnArgs &a) {
        const uint32_t tile = blockIdx.x / (uint32_t)a.S;
        s = blockIdx.x - tile * (uint32_t)a.S;
        lx = threadIdx.x % VQ_BN_LX;
        c0 = (int)((tile * VQ_BN_LX + lx) * PW);
        has = c0 < a.C;
        pos0 = s * a.chunk + threadIdx.x / VQ_BN_LX;                            // < n + 1024 < 2^32
    }
    __device__ __forceinline__ bool live(const VqBnArgs &a, int k) const { return has && pos0 + (uint32_t)(k * VQ_BN_LY) < a.n; }
    __device__ __forceinline__ int64_t off(const VqBnArgs &a, int k) const { return (int64_t)(pos0 + (uint32_t)(k * VQ_BN_LY)) * a.C + c0; }
};

// a thread's sums down its positions, one per channel: sequential in k; NP == 32 in two halves of 16
template <int NP, int PW, class F>
__device__ __forceinline__ void bn_rows_thread_sum(const bool (&live)[NP], float (&acc)[PW], F term) {
    constexpr int H = NP > 16 ? NP / 2 : NP;
    float hi[PW];
#pragma unroll
    for (int e = 0; e < PW; ++e) { acc[e] = 0.0f; hi[e] = 0.0f; }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (!live[k]) continue;
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            if (k < H) acc[e] = acc[e] + term(k, e);
            else hi[e] = hi[e] + term(k, e);
        }
    }
    if (NP > H) {
#pragma unroll
        for (int e = 0; e < PW; ++e) acc[e] = acc[e] + hi[e];
    }
}

// the sums over the 32 threads of equal lx, valid in every thread.  Every thread of the workgroup calls it.
template <int PW>
__device__ __forceinline__ void bn_rows_team_sum(float (&v)[PW], float (*red)[VQ_BN_LX * PW]) {
    const int lx = threadIdx.x % VQ_BN_LX;
#pragma unroll
    for (int e = 0; e < PW; ++e)
#pragma unroll
        for (int m = VQ_BN_LX; m < 64; m <<= 1) v[e] = v[e] + __shfl_xor(v[e], m, 64);
    __syncthreads();                                                            // the readers of the previous sum are done
    if ((threadIdx.x & 63) < VQ_BN_LX) {
#pragma unroll
        for (int e = 0; e < PW; ++e) red[threadIdx.x >> 6][lx * PW + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PW; ++e) v[e] = (red[0][lx * PW + e] + red[1][lx * PW + e]) + (red[2][lx * PW + e] + red[3][lx * PW + e]);
}

template <int DT, int PW>
__global__ __launch_bounds__(VQ_GN_THREADS) void bn_rows_fwd_kernel(VqBnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    constexpr int NP = VQ_GN_EPT / PW;
    __shared__ float red[4][VQ_BN_LX * PW];
    const BnRows<PW> r(a);
    const raw *in = reinterpret_cast<const raw *>(a.x);
    float xv[NP][PW];
    bool live[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        live[k] = r.live(a, k);
        if (live[k]) {
            gn_load<DT, PW>(in + r.off(a, k), PW, xv[k]);
        } else {
#pragma unroll
            for (int e = 0; e < PW; ++e) xv[k][e] = 0.0f;
        }
    }
    float mean[PW], rstd[PW];
    if (a.phase != VQ_GN_APPLY) {
        const float nc = bn_chunk_count(a, r.s);
        float m2[PW];
        bn_rows_thread_sum<NP, PW>(live, mean, [&](int k, int e) { return xv[k][e]; });
        bn_rows_team_sum<PW>(mean, red);
#pragma unroll
        for (int e = 0; e < PW; ++e) mean[e] = mean[e] / nc;
        bn_rows_thread_sum<NP, PW>(live, m2, [&](int k, int e) { const float d = xv[k][e] - mean[e]; return d * d; });
        bn_rows_team_sum<PW>(m2, red);
        const bool writer = r.has && threadIdx.x < VQ_BN_LX;
        if (a.phase == VQ_GN_PART) {
            if (writer) {
#pragma unroll
                for (int e = 0; e < PW; ++e) {
                    float *part = a.part + ((int64_t)(r.c0 + e) * a.S + r.s) * 2;
                    part[0] = mean[e]; part[1] = m2[e];
                }
            }
            return;
        }
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            rstd[e] = 1.0f / sqrtf(m2[e] / (float)a.n + a.eps);
            if (writer) {
                a.stats[2 * (r.c0 + e)] = mean[e]; a.stats[2 * (r.c0 + e) + 1] = rstd[e];
                a.mv[r.c0 + e] = mean[e]; a.mv[a.C + r.c0 + e] = m2[e] / (float)(a.n - 1);
            }
        }
    } else if (r.has) {
#pragma unroll
        for (int e = 0; e < PW; ++e) { mean[e] = a.stats[2 * (r.c0 + e)]; rstd[e] = a.stats[2 * (r.c0 + e) + 1]; }
    }
    if (!r.has) return;
    float gam[PW], bet[PW];
#pragma unroll
    for (int e = 0; e < PW; ++e) { gam[e] = a.gamma[r.c0 + e]; bet[e] = a.beta[r.c0 + e]; }
    raw *out = reinterpret_cast<raw *>(a.out);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (!live[k]) continue;
        float y[PW];
#pragma unroll
        for (int e = 0; e < PW; ++e) y[e] = gn_act(((xv[k][e] - mean[e]) * rstd[e]) * gam[e] + bet[e], a.act);
        gn_store<DT, PW>(out + r.off(a, k), PW, y);
    }
}

template <int DT, int PW>
__global__ __launch_bounds__(VQ_GN_THREADS) void bn_rows_bwd_kernel(VqBnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    constexpr int NP = VQ_GN_EPT / PW;
    __shared__ float red[4][VQ_BN_LX * PW];
    const BnRows<PW> r(a);
    const raw *in = reinterpret_cast<const raw *>(a.x);
    const raw *gin = reinterpret_cast<const raw *>(a.g);
    float mean[PW], rstd[PW], gam[PW], bet[PW];
#pragma unroll
    for (int e = 0; e < PW; ++e) {
        const int c = r.has ? r.c0 + e : 0;
        mean[e] = a.stats[2 * c]; rstd[e] = a.stats[2 * c + 1]; gam[e] = a.gamma[c]; bet[e] = a.beta[c];
    }
    float xh[NP][PW], gu[NP][PW];                                               // xh, then g d
    bool live[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        live[k] = r.live(a, k);
        if (live[k]) {
            gn_load<DT, PW>(in + r.off(a, k), PW, xh[k]);
            gn_load<DT, PW>(gin + r.off(a, k), PW, gu[k]);
        }
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            if (live[k]) {
                const float h = (xh[k][e] - mean[e]) * rstd[e];
                gu[k][e] = a.act ? gu[k][e] * gn_act_grad(h * gam[e] + bet[e], a.act) : gu[k][e] * 1.0f;
                xh[k][e] = h;
            } else {
                xh[k][e] = 0.0f; gu[k][e] = 0.0f;
            }
        }
    }
    float s1[PW], s2[PW];
    if (a.phase != VQ_GN_APPLY) {
        bn_rows_thread_sum<NP, PW>(live, s1, [&](int k, int e) { return gu[k][e]; });
        bn_rows_team_sum<PW>(s1, red);
        bn_rows_thread_sum<NP, PW>(live, s2, [&](int k, int e) { return gu[k][e] * xh[k][e]; });
        bn_rows_team_sum<PW>(s2, red);
        const bool writer = r.has && threadIdx.x < VQ_BN_LX;
        if (a.phase == VQ_GN_PART) {
            if (writer) {
#pragma unroll
                for (int e = 0; e < PW; ++e) {
                    float *part = a.part + ((int64_t)(r.c0 + e) * a.S + r.s) * 2;
                    part[0] = s1[e]; part[1] = s2[e];
                }
            }
            return;
        }
        if (writer) {
#pragma unroll
            for (int e = 0; e < PW; ++e) { a.dbeta[r.c0 + e] = s1[e]; a.dgamma[r.c0 + e] = s2[e]; }
        }
    } else if (r.has) {
#pragma unroll
        for (int e = 0; e < PW; ++e) { s1[e] = a.dbeta[r.c0 + e]; s2[e] = a.dgamma[r.c0 + e]; }
    }
    if (!r.has) return;
    raw *out = reinterpret_cast<raw *>(a.out);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (!live[k]) continue;
        float gx[PW];
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            const float m1 = (s1[e] * gam[e]) / (float)a.n, m2 = (s2[e] * gam[e]) / (float)a.n;
            gx[e] = rstd[e] * ((gu[k][e] * gam[e] - m1) - xh[k][e] * m2);
        }
        gn_store<DT, PW>(out + r.off(a, k), PW, gx);
    }
}
