// libvqhip device code: what the two forms of the all-fp32 pass over a whole batch share — the skip rule of the L2 row argmin and
// the epilogue of a work item.  exact_tiled_kernel (vqhip_exact_kernels.h, vqhip_exact.hip) and exact_stream_kernel
// (vqhip_stream_kernels.h, vqhip.hip) are compiled in different translation units; nothing here is a kernel.
#pragma once
#include "vqhip_kernels.h"

// Row argmin, L2: a lane meets its codes in increasing index order, so a later code can only replace the lane's best with a
// STRICTLY smaller distance; sqrt is correctly rounded, hence monotone: radicand t >= tb (the smallest radicand the lane has
// keyed) implies sqrt(t) >= sqrt(tb) and the code cannot win — its sqrt and key (the larger half of the epilogue's
// instructions) are skipped.  NaN radicands never compare >= and always go through (NaN sorts first in dist_key).
// tb starts at +inf ("nothing keyed yet"): a radicand of +inf (|x|^2 overflows fp32: every distance of the row is inf and
// index 0 wins) must not be skipped against that start value, or the row never produces a key and keeps its 0xFFFFFFFF.
__device__ __forceinline__ bool l2_skip(float t, float tb) { return t >= tb && tb < INFINITY; }

// ------------------------------------------------------------------------------------------------
// Epilogue of a whole-batch work item (128 rows x 256 codes: acc[c][q] = the lane's column j of code tile c), both forms of the
// pass: row argmin -> the lane's best key (returned); column argmin -> atomicMin per code; distances -> stores.
// en_lds: |e_k|^2 of the item's 256 codes (L2).
// ------------------------------------------------------------------------------------------------
// HW > 0 (distances, exact_stream_kernel): `stage` is a wave-private LDS tile of 32 rows x HW codes (32, or 16 where the wave's
// share of a consumed row block is only 2 KiB: bf16 rows) through which the distances leave as ROWS — a lane's 16 values of a code
// tile are 4 codes x 4 runs down a column of d[N, K], and stored as they lie every wave-store touched 32 lines for 8 bytes each
// (8192 x 8192 x 64: 268 MB in 0.47 ms, slower than the register form); staged, a wave-store is 8 (16) rows x 128 (64) contiguous
// bytes.  K % 4 == 0 (16-byte row segments); other K keep the element stores.
template <int MODE, int HW = 0>
__device__ __forceinline__ u64 tiled_epilogue(const f32x16 (&acc)[8], const float4 *__restrict__ en_lds, float xn, int64_t kbase,
                                              int64_t K, int metric, int h, int j, bool rvalid, int64_t row,
                                              u64 *__restrict__ keys, float *__restrict__ dout, float4 *stage = nullptr,
                                              int64_t N = 0) {
    constexpr int CT = 8;
    // A lane's code of accumulator element (c, q) is kb + o with the CONSTANT
    // o = 32 c + mfma_row(q, 0): existence is `o < krem`, the winner is kept as its o (an inline constant in the select) —
    // no per-element 64-bit index is ever formed (128 of them, computed once for both passes below and kept, were the
    // register form's spills and, under this kernel's 256 registers, 316 more)
    u64 best = ~0ull;
    const int64_t kb = kbase + 4 * h;
    const int64_t left = K - kb;
    int krem = (int)(left < 0 ? 0 : (left > CT * 32 ? CT * 32 : left));      // this lane's codes kb + o exist for o < krem
    uint32_t kb32 = (uint32_t)kb;
    asm volatile("" : "+v"(krem), "+v"(kb32));
    float enr[2][16];
    auto request_en = [&](int c, float (&dst)[16]) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 v = en_lds[c * 8 + 2 * g + h];
            dst[4 * g] = v.x; dst[4 * g + 1] = v.y; dst[4 * g + 2] = v.z; dst[4 * g + 3] = v.w;
        }
    };
    if (VQ_IS_L2(metric)) request_en(0, enr[0]);
    if (MODE == 0 && VQ_IS_L2(metric)) {
        // row argmin, L2, in the radicands (exact_tiled_kernel): smallest radicand with its lowest index and the runner-up value
        // in one pass; a runner-up within 2^-21 of the smallest (near-ties, equal radicands, NaN) sends the wave through the
        // per-code sqrt + key loop.  A code that does not exist has t = +inf: fmaxf(inf, tmin) = inf leaves t2 alone.
        float tmin = INFINITY, t2 = INFINITY, tsum = 0.0f;
        int omin = -1;
        // (a chunk that lies wholly inside the codebook — all but the last — runs the pass without the existence selects)
        auto radicand_pass = [&](auto whole_chunk) {
            constexpr bool WHOLE = decltype(whole_chunk)::value;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c + 1 < CT) request_en(c + 1, enr[(c + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int o = c * 32 + mfma_row(q, 0);
                    const bool kv = WHOLE || o < krem;
                    float t = (acc[c][q] + xn) + (kv ? enr[c & 1][q] : 0.0f);
                    t = (t < 0.0f) ? 0.0f : t;
                    t = kv ? t : INFINITY;
                    const bool upd = t < tmin;
                    t2 = fminf(t2, fmaxf(t, tmin));
                    tsum += t;                                   // NaN radicands (a code row holding inf or NaN): see below
                    omin = upd ? o : omin;
                    tmin = upd ? t : tmin;
                }
            }
        };
        if (kbase + CT * 32 <= K) radicand_pass(std::true_type{}); else radicand_pass(std::false_type{});
        // A NaN radicand must win (torch.argmin: NaN first) and is invisible to the comparisons above — fmaxf(NaN, tmin) = tmin
        // only flags it while tmin does not fall any further.  The radicands are >= 0 or NaN, so their sum is NaN exactly when
        // one of them is (round 6: a codebook row holding +inf, distances inf - inf for half the rows, lost to a NaN row of
        // higher index in a later chunk — both forms of the pass)
        const bool unique = t2 > tmin * (1.0f + 0x1p-21f) && tsum == tsum;   // (inf > inf is false: equal / all-inf radicands are not unique)
        // (no code selected although the lane has codes: every radicand is NaN or +inf — the exact loop sorts that out)
        if (__any(omin >= 0 ? !unique : krem > 0)) {
            float xn2 = xn;
            asm volatile("" : "+v"(xn2));     // the radicands are computed AGAIN: sharing them with the pass above would keep 128 values alive
            request_en(0, enr[0]);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c + 1 < CT) request_en(c + 1, enr[(c + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int o = c * 32 + mfma_row(q, 0);
                    float t = (acc[c][q] + xn2) + ((o < krem) ? enr[c & 1][q] : 0.0f);
                    t = (t < 0.0f) ? 0.0f : t;
                    if (o < krem) { const u64 key = dist_key(sqrtf(t), kb32 + (uint32_t)o); best = key < best ? key : best; }
                }
            }
        } else if (omin >= 0) {
            best = dist_key(sqrtf(tmin), kb32 + (uint32_t)omin);
        }
    } else if (MODE == 2 && HW > 0 && (K & 3) == 0) {
        constexpr int HWS = HW > 0 ? HW : 32;                // (HW == 0 never reaches this branch)
        constexpr int NPR = HWS / 4, RPP = 64 / NPR;         // 16-byte pieces of a staged row; rows per read pass
        const int lane = j + 32 * h;
        const int rr = lane / NPR, rp = lane % NPR;
        const int64_t row0 = row - j;                        // the wave's first row
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (VQ_IS_L2(metric) && c + 1 < CT) request_en(c + 1, enr[(c + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            float dv[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int o = c * 32 + mfma_row(q, 0);
                if (VQ_IS_L2(metric)) {
                    float t = (acc[c][q] + xn) + ((o < krem) ? enr[c & 1][q] : 0.0f);
                    t = (t < 0.0f) ? 0.0f : t;
                    dv[q] = sqrtf(t);
                } else {
                    dv[q] = cos_distance(acc[c][q], metric);
                }
            }
#pragma unroll
            for (int hh = 0; hh < 32 / HWS; ++hh) {           // the tile's halves (HW == 16) or the whole tile
#pragma unroll
                for (int gl = 0; gl < HWS / 8; ++gl) {        // this lane's runs of four codes: 8 g + 4 h .. + 3 of the tile
                    const int g = hh * (HWS / 8) + gl, pc = 2 * gl + h;
                    stage[j * NPR + (pc ^ (j & (NPR - 1)))] = make_float4(dv[4 * g], dv[4 * g + 1], dv[4 * g + 2], dv[4 * g + 3]);
                }
#pragma unroll
                for (int pass = 0; pass < 32 / RPP; ++pass) {
                    const int r = pass * RPP + rr;
                    const float4 v = stage[r * NPR + (rp ^ (r & (NPR - 1)))];
                    const int64_t grow = row0 + r, k = kbase + c * 32 + hh * HWS + 4 * rp;
                    if (grow < N) {
                        float *dst = dout + grow * K + k;
                        if (k + 3 < K) *(float4 *)dst = v;
                        else { if (k < K) dst[0] = v.x; if (k + 1 < K) dst[1] = v.y; if (k + 2 < K) dst[2] = v.z; }
                    }
                }
            }
        }
    } else {
        float *dp = MODE == 2 ? dout + row * K + kb : nullptr;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (VQ_IS_L2(metric) && c + 1 < CT) request_en(c + 1, enr[(c + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int o = c * 32 + mfma_row(q, 0);
                const bool kv = o < krem;
                float d;
                if (VQ_IS_L2(metric)) {
                    float t = (acc[c][q] + xn) + (kv ? enr[c & 1][q] : 0.0f);
                    t = (t < 0.0f) ? 0.0f : t;
                    d = sqrtf(t);
                } else {
                    d = cos_distance(acc[c][q], metric);
                }
                if (MODE == 0) {
                    if (kv) { u64 key = dist_key(d, kb32 + (uint32_t)o); best = key < best ? key : best; }
                } else if (MODE == 1) {
                    u64 key = (rvalid && kv) ? dist_key(d, (uint32_t)row) : ~0ull;
#pragma unroll
                    for (int off = 16; off >= 1; off >>= 1) {
                        u64 o2 = __shfl_xor(key, off, 64);
                        key = o2 < key ? o2 : key;
                    }
                    if (j == 0 && kv && key != ~0ull) atomicMin(&keys[kb + o], key);
                } else {
                    if (rvalid && kv) dp[o] = d;
                }
            }
        }
    }
    return best;
}
