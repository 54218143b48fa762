// The attention step of cached generation (include/vqhip.h, "static KV cache"): rope_append_kernel writes the rotated keys and the
// values of L new tokens into the caches, decode_attention_kernel does that for one token and attends over the positions stored -
// at a position passed by value or, for a launch that a captured graph replays, read from device memory (VqAttnArgs::pos), where
// decode_advance_kernel counts it at the end of a step.
//
// decode_attention_kernel: one workgroup of four wave64s per (batch row, kv head); it serves the G = Hq / Hkv query heads of the group
// from one pass over K and V.  A cache row of Dh elements is C = Dh / E pieces of 16 bytes (E = 4 fp32 or 8 16-bit elements); LP, the
// next power of two >= C, lanes share a position and a wave holds PP = 64 / LP positions at once, so workgroup sweep `it` covers
// positions (4 it + w) PP + p for wave w and slot p.  Every (wave, slot) keeps an online softmax per query head (running maximum,
// running sum, Dh accumulators spread over its lanes); the slots of a wave merge by an xor butterfly, the four waves through LDS in
// wave order.  No array is sized by the length, nothing is atomic: the order of every sum is fixed by (seen, Dh, dtype) alone.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip_elem.h"

#define VQ_ATTN_THREADS 256
#define VQ_ATTN_WAVES 4

struct VqAttnArgs {
    const void *q, *k, *v;              // rows of the new tokens, [R, H * Dh] with these row strides (elements)
    int64_t q_stride, k_stride, v_stride;
    const float *cos, *sin;             // [L, Dh]
    void *k_cache, *v_cache;            // [B, Hkv, cap, Dh]
    void *out;                          // decode: [B, Hq * Dh]; append: q' [B, Hq, L, Dh]
    int64_t seen, cap, L;
    const int32_t *pos;                 // decode only: where not null, the position is *pos and cos, sin are [cap, Dh] tables
    int64_t table_stride;               // elements between the tables' rows (0 without pos)
    float scale;
    int Hq, Hkv, Dh, G;
};

// x c + y s to within one rounding of the exact value (the caller negates y for the first half): the two products with their
// exact remainders (fma), a two-sum of the products, the three small terms added last.  Plain fp32 would lose the bits a
// cancellation between the products exposes.
__device__ __forceinline__ float rope_pair(float x, float c, float y, float s) {
    const float p1 = x * c, e1 = fmaf(x, c, -p1);
    const float p2 = y * s, e2 = fmaf(y, s, -p2);
    const float t = p1 + p2, z = t - p1;
    const float et = (p1 - (t - z)) + (p2 - z);
    return t + (et + (e1 + e2));
}

// element i of a rotated row: x' = x cos + rotate_half(x) sin, rotate_half(x) = (-x[half:], x[:half])
template <int DT>
__device__ __forceinline__ float rope_elem(const typename SampleElem<DT>::raw *row, const float *cos, const float *sin, int i, int half) {
    const float x = SampleElem<DT>::f32(row[i]);
    const float y = SampleElem<DT>::f32(row[i < half ? i + half : i - half]);
    return rope_pair(x, cos[i], i < half ? -y : y, sin[i]);
}

// ---- prefill: L >= 1 new tokens.  One workgroup per (b, t) row; threads walk the row's (Hq + 2 Hkv) Dh elements -----------------
template <int DT>
__global__ __launch_bounds__(VQ_ATTN_THREADS) void rope_append_kernel(VqAttnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    const int64_t r = blockIdx.x, b = r / a.L, t = r % a.L;
    const int Dh = a.Dh, half = Dh / 2;
    const float *cos = a.cos + t * Dh, *sin = a.sin + t * Dh;
    const raw *q = (const raw *)a.q + r * a.q_stride, *k = (const raw *)a.k + r * a.k_stride, *v = (const raw *)a.v + r * a.v_stride;
    raw *qo = (raw *)a.out, *kc = (raw *)a.k_cache, *vc = (raw *)a.v_cache;
    const int nq = a.Hq * Dh, nk = a.Hkv * Dh;
    for (int e = threadIdx.x; e < nq + 2 * nk; e += VQ_ATTN_THREADS) {
        if (e < nq) {
            const int h = e / Dh, i = e % Dh;
            qo[((b * a.Hq + h) * a.L + t) * Dh + i] = ce_round<DT>(rope_elem<DT>(q + h * Dh, cos, sin, i, half));
        } else {
            const int f = e - nq, g = f < nk ? f : f - nk, h = g / Dh, i = g % Dh;
            const int64_t at = ((b * a.Hkv + h) * a.cap + a.seen + t) * Dh + i;
            if (f < nk) kc[at] = ce_round<DT>(rope_elem<DT>(k + h * Dh, cos, sin, i, half));
            else vc[at] = v[g];
        }
    }
}

// ---- decode: one new token ------------------------------------------------------------------------------------------------
template <int DT> struct AttnPiece;                                              // 16 bytes of a cache row as E floats
template <> struct AttnPiece<VQHIP_DTYPE_F32> {
    static constexpr int E = 4;
    static __device__ __forceinline__ void f32(const uint4 &u, float *f) {
        f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
    }
};
template <int DT> struct AttnPiece {
    static constexpr int E = 8;
    static __device__ __forceinline__ void f32(const uint4 &u, float *f) {
        const uint32_t word[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = SampleElem<DT>::f32((uint16_t)(word[i] & 0xFFFFu));
            f[2 * i + 1] = SampleElem<DT>::f32((uint16_t)(word[i] >> 16));
        }
    }
};

// the merge of two online-softmax states; an empty one is (-FLT_MAX, 0, 0)
__device__ __forceinline__ void attn_merge_factors(float m1, float m2, float &m, float &f1, float &f2) {
    m = fmaxf(m1, m2);
    f1 = expf(m1 - m);
    f2 = expf(m2 - m);
}

template <int DT, int GMAX>
__global__ __launch_bounds__(VQ_ATTN_THREADS) void decode_attention_kernel(VqAttnArgs a) {
    typedef typename SampleElem<DT>::raw raw;
    constexpr int E = AttnPiece<DT>::E;
    __shared__ float qs[GMAX * VQHIP_ATTN_MAX_HEAD_DIM];                          // q' of the group, fp32
    __shared__ float ms[VQ_ATTN_WAVES][GMAX][2];                                  // each wave's (maximum, sum) per head
    __shared__ float accs[VQ_ATTN_WAVES][GMAX][VQHIP_ATTN_MAX_HEAD_DIM];            // and its accumulators

    const int Dh = a.Dh, half = Dh / 2, G = a.G;
    const int64_t b = blockIdx.x / a.Hkv;
    const int kvh = blockIdx.x % a.Hkv;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // the position: by value, or loaded once from device memory - the same for every thread of every workgroup, so a position
    // outside the cache ends the whole launch here, in front of the first store and the first barrier
    int64_t seen = a.seen;
    const float *cos = a.cos, *sin = a.sin;
    if (a.pos) {
        seen = *a.pos;
        if (seen < 0 || seen >= a.cap) return;
        cos += seen * a.table_stride;
        sin += seen * a.table_stride;
    }
    raw *kc = (raw *)a.k_cache + ((b * a.Hkv + kvh) * a.cap) * Dh;              // this (b, kv head)'s [cap, Dh]
    raw *vc = (raw *)a.v_cache + ((b * a.Hkv + kvh) * a.cap) * Dh;

    // the new token: k' rounded into the cache at `seen`, v copied, q' of the G heads to LDS
    {
        const raw *q = (const raw *)a.q + b * a.q_stride + (int64_t)kvh * G * Dh;
        const raw *k = (const raw *)a.k + b * a.k_stride + (int64_t)kvh * Dh;
        const raw *v = (const raw *)a.v + b * a.v_stride + (int64_t)kvh * Dh;
        for (int e = tid; e < (G + 2) * Dh; e += VQ_ATTN_THREADS) {
            const int h = e / Dh, i = e % Dh;
            if (h < G) qs[h * Dh + i] = rope_elem<DT>(q + h * Dh, cos, sin, i, half);
            else if (h == G) kc[seen * Dh + i] = ce_round<DT>(rope_elem<DT>(k, cos, sin, i, half));
            else vc[seen * Dh + i] = v[i];
        }
    }
    __syncthreads();                                                              // the stores above are read back below: same workgroup

    const int C = Dh / E;                                                         // 16-byte pieces of a row
    int LP = 2;
    while (LP < C) LP <<= 1;                                                      // lanes that share a position: 2 .. 32
    const int PP = 64 / LP, c = lane & (LP - 1), p = lane / LP;
    const bool mine = c < C;
    const int64_t n = seen + 1;

    float qf[GMAX][E], acc[GMAX][E], m[GMAX], l[GMAX];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        m[g] = -FLT_MAX;
        l[g] = 0.0f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            acc[g][e] = 0.0f;
            qf[g][e] = (g < G && mine) ? qs[g * Dh + c * E + e] : 0.0f;
        }
    }

    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const int64_t sweep = (int64_t)VQ_ATTN_WAVES * PP;
    int64_t j = (int64_t)w * PP + p;                                              // this lane's position of the current sweep
    uint4 kr = zero, vr = zero;
    if (mine && j < n) {
        kr = *(const uint4 *)(kc + j * Dh + c * E);
        vr = *(const uint4 *)(vc + j * Dh + c * E);
    }
    for (int64_t base = (int64_t)w * PP; base < n; base += sweep, j += sweep) {   // wave-uniform trip count
        const bool valid = j < n;
        const int64_t jn = j + sweep;
        uint4 kn = zero, vn = zero;
        if (mine && jn < n) {                                                     // the next sweep's rows, in flight under this one's arithmetic
            kn = *(const uint4 *)(kc + jn * Dh + c * E);
            vn = *(const uint4 *)(vc + jn * Dh + c * E);
        }
        float kf[E], vf[E];
        AttnPiece<DT>::f32(kr, kf);
        AttnPiece<DT>::f32(vr, vf);
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
            if (g < G) {
                float d = 0.0f;
#pragma unroll
                for (int e = 0; e < E; ++e) d += qf[g][e] * kf[e];
                for (int off = LP >> 1; off; off >>= 1) d += __shfl_xor(d, off);  // every lane of the position holds the same bits
                if (valid) {
                    const float s = a.scale * d, mn = fmaxf(m[g], s);
                    const float alpha = expf(m[g] - mn), pj = expf(s - mn);
                    m[g] = mn;
                    l[g] = l[g] * alpha + pj;
#pragma unroll
                    for (int e = 0; e < E; ++e) acc[g][e] = acc[g][e] * alpha + pj * vf[e];
                }
            }
        }
        kr = kn;
        vr = vn;
    }

    // the slots of a wave, by an xor butterfly over the lanes that hold the same piece (both partners compute the same bits)
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        if (g < G) {
            for (int off = LP; off < 64; off <<= 1) {
                const float m2 = __shfl_xor(m[g], off), l2 = __shfl_xor(l[g], off);
                float mn, f1, f2;
                attn_merge_factors(m[g], m2, mn, f1, f2);
                m[g] = mn;
                l[g] = l[g] * f1 + l2 * f2;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float a2 = __shfl_xor(acc[g][e], off);
                    acc[g][e] = acc[g][e] * f1 + a2 * f2;
                }
            }
            if (p == 0 && mine) {
                if (c == 0) {
                    ms[w][g][0] = m[g];
                    ms[w][g][1] = l[g];
                }
#pragma unroll
                for (int e = 0; e < E; ++e) accs[w][g][c * E + e] = acc[g][e];
            }
        }
    }
    __syncthreads();

    // the four waves, in wave order; out[b][(kvh G + g) Dh + i], rounded once
    raw *out = (raw *)a.out + (b * a.Hq + (int64_t)kvh * G) * Dh;
    for (int e = tid; e < G * Dh; e += VQ_ATTN_THREADS) {
        const int g = e / Dh, i = e % Dh;
        float mx = ms[0][g][0];
#pragma unroll
        for (int ww = 1; ww < VQ_ATTN_WAVES; ++ww) mx = fmaxf(mx, ms[ww][g][0]);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int ww = 0; ww < VQ_ATTN_WAVES; ++ww) {
            const float f = expf(ms[ww][g][0] - mx);
            den += ms[ww][g][1] * f;
            num += accs[ww][g][i] * f;
        }
        out[e] = ce_round<DT>(num / den);
    }
}

// ---- the end of a replayed step: record the sampled tokens, feed them to the next step, count the position -------------------
// One workgroup.  Every thread reads the position before the barrier and thread 0 stores the new one behind it, so no thread sees
// the count it is about to become.  At the last column (or a position outside the sequence) nothing is written.
__global__ __launch_bounds__(VQ_ATTN_THREADS) void decode_advance_kernel(const int64_t *token, int64_t *next, int64_t *sequence, int64_t R,
                                                                         int64_t length, int32_t *pos) {
    const int64_t s = *pos;
    __syncthreads();
    if (s < 0 || s + 1 >= length) return;
    for (int64_t r = threadIdx.x; r < R; r += VQ_ATTN_THREADS) {
        const int64_t t = token[r];
        sequence[r * length + s + 1] = t;                                         // a bad row's -1 stays visible
        next[r] = t < 0 ? 0 : t;                                                  // and gathers embedding row 0 in the next step
    }
    if (threadIdx.x == 0) *pos = (int32_t)(s + 1);
}
