// Fused tail of the LPIPS perceptual loss (vq/tasks/image_reconstruction/losses.py:142-178): for ONE feature layer, the channel
// normalisation of both maps, the squared difference, dropout, the bias-free 1 x 1 convolution and the spatial mean -> the
// per-image value, four floats per pixel for the backward, and the gradient over pred.  The VGG16 convolutions in front stay
// with the framework.  pred and target are read in their own dtypes; nothing of the size of the features is written except
// the gradient.
//
// Contract: include/vqhip.h (vqhip_lpips_fwd / vqhip_lpips_bwd / vqhip_lpips_keep_mask), DESIGN.md §8.  Every element is converted
// to fp32 exactly (SampleElem of the sampler); all arithmetic is fp32 IEEE without contraction, division and sqrtf correctly
// rounded, except the spatial mean, which is a double sum rounded once.  Per pixel (b, p), with e = 1e-10f:
//       ff = sum_c f_c^2        nf = sqrtf(ff), e where nf < e (a NaN stays a NaN)        inf = 1 / nf      a_c = f_c * inf
//       gg = sum_c g_c^2        ng likewise                                              ing = 1 / ng      b_c = g_c * ing
//       d_c = a_c - b_c         mw_c = m_c * w_c (w_c itself without dropout)             s = sum_c mw_c * (d_c * d_c)
//       u_c = 2 * (mw_c * d_c)  sua = sum_c u_c * a_c, +0 where nf was clamped (the norm is then a constant: no projection)
//       stats[b P + p] = (inf, ing, sua, s)
//       grad_c = (g_out[b] / (float)P) * ((u_c - a_c * sua) * inf)
// TWO PASSES over the channels of a pixel inside ONE launch: the norms first, the differences second.  The second pass reads
// what the same workgroup has just read (a tile of 64 x C or 16 x C elements per operand: L1 / L2), so HBM sees each operand once.
// Why not one pass (sum w f^2, sum w g^2, sum w f g): it forms s as a difference of three sums of size |w|, so its error does not
// shrink with s, an identical pair does not give 0, and s can come out negative; the loss is small exactly where it is trained.
// Here d_c is formed per channel: the error of s is proportional to |d| (see ERROR BOUND in vqhip.h), an identical pair of one
// dtype gives s == 0 and a zero gradient exactly.
//
// MAP layout (NCHW-contiguous [B, C, P]): a workgroup owns 64 consecutive positions of ONE image (lane = position: a wave reads
// 64 consecutive elements of a channel plane) times 4 channel groups (the wave index).  Channel c belongs to group c % 4, which
// takes its channels in increasing c into ONE accumulator per sum (from +0, the product rounded first); the groups add through
// LDS as (g0 + g1) + (g2 + g3).
// ROWS layout (channels-last dense [B, P, C]): 16 lanes own a row (16 rows per workgroup).  The row is cut by the index into
// pieces of 4 elements, piece q = [4 q, 4 q + 4) for q < C / 4 (one 16- or 8-byte load per operand at element alignment), then
// C % 4 single elements; piece q belongs to lane q % 16, which takes its pieces in increasing q and adds element by element in
// increasing c; its single element (4 (C / 4) + lane, lane < C % 4) last; the 16 lanes add as the tree xor 1, 2, 4, 8.
// Longest chain of one sum, the product's rounding counted as one: map ceil(C / 4) + 1 + 2; rows 4 ceil(C / 64) + 1 + 1 + 4.  Both
// are at most VQHIP_LPIPS_CHAIN(C) = C / 4 + 12.
// In both layouts a pixel's four stats are a function of C, the dtypes, the weights and the mask alone: not of B, P, the other
// pixels or the address.  The two layouts add in different orders and need not agree bit for bit.
// lpips_reduce_kernel, ONE workgroup per image (the second launch): t_j = +0.0 (double); for p = j, j + 256, .. < P:
//   t_j += (double)s(b, p); the xor tree over the 64 lanes of a wave, then (w0 + w1) + (w2 + w3); v = (float)(t / (double)P);
//   value[b] = accumulate ? value[b] + v : v - a plain fp32 add by the one thread that owns image b.
// DROPOUT  keep(seed, layer, i) for the LOGICAL index i = (b C + c) P + p (the same in both layouts):
//       mix(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16                    (uint32)
//       h = mix(seed[0] ^ lo32(i));   h = mix(h ^ (seed[1] + hi32(i) * 0x9E3779B9 + layer * 0x85EBCA77));   keep iff h >= thr,
//       thr = ceil(p * 2^32) formed on the host.  m = 1 / (1 - p) in fp32 where kept, 0 where dropped.  No mask is stored: forward,
//       backward and vqhip_lpips_keep_mask call the same function.
// No atomics of any kind, no memset.  Every index is a pixel below B P and a channel below C.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_elem.h"                         // SampleElem: the exact conversion to fp32; ce_round: nearest even into the output dtype

#define VQ_LPIPS_THREADS 256
#define VQ_LPIPS_MAP_POS 64
#define VQ_LPIPS_MAP_GROUPS (VQ_LPIPS_THREADS / VQ_LPIPS_MAP_POS)
#define VQ_LPIPS_ROW_LANES 16
#define VQ_LPIPS_ROWS (VQ_LPIPS_THREADS / VQ_LPIPS_ROW_LANES)
#define VQ_LPIPS_EPS 1e-10f

struct VqLpipsArgs {
    const void *pred, *target;
    const float *w;                             // [C]
    const uint32_t *seed;                       // two words on the device, or null: no dropout
    int64_t B, P, tiles;                        // tiles = ceil(P / 64) workgroups per image (map layout)
    int C;
    uint32_t layer, thr;                        // keep iff hash >= thr
    float scale;                                // 1 / (1 - p)
};

__device__ __forceinline__ uint32_t lpips_mix(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ bool lpips_keep(uint32_t s0, uint32_t s1, uint32_t layer, uint32_t thr, uint64_t i) {
    uint32_t h = lpips_mix(s0 ^ (uint32_t)i);
    h = lpips_mix(h ^ (s1 + (uint32_t)(i >> 32) * 0x9E3779B9u + layer * 0x85EBCA77u));
    return h >= thr;
}

// what a thread needs of the dropout: the two seed words (read once) and the weight of a channel with the mask applied
struct LpipsDrop {
    uint32_t s0, s1, layer, thr;
    float scale;
    bool on;
    __device__ __forceinline__ void init(const VqLpipsArgs &a) {
        on = a.seed != nullptr;
        s0 = on ? a.seed[0] : 0u; s1 = on ? a.seed[1] : 0u;
        layer = a.layer; thr = a.thr; scale = a.scale;
    }
    __device__ __forceinline__ float weigh(float w, uint64_t i) const {
        if (!on) return w;
        const float m = lpips_keep(s0, s1, layer, thr, i) ? scale : 0.0f;
        return m * w;
    }
};

struct LpipsNorm {
    float inf, ing;
    bool clamped;                               // nf was below e: the norm of pred is the constant e
};

__device__ __forceinline__ LpipsNorm lpips_norms(float ff, float gg) {
    LpipsNorm n;
    float nf = sqrtf(ff), ng = sqrtf(gg);
    n.clamped = nf < VQ_LPIPS_EPS;
    if (n.clamped) nf = VQ_LPIPS_EPS;                                           // (a NaN compares false and stays)
    if (ng < VQ_LPIPS_EPS) ng = VQ_LPIPS_EPS;
    n.inf = 1.0f / nf; n.ing = 1.0f / ng;
    return n;
}

// one channel of the second pass: s and sua take their term
__device__ __forceinline__ void lpips_term(float x, float y, float mw, const LpipsNorm &n, float &s, float &sua) {
    const float av = x * n.inf, bv = y * n.ing;
    const float d = av - bv;
    const float d2 = d * d;
    const float t = mw * d2;
    s = s + t;
    const float md = mw * d;
    const float uu = 2.0f * md;
    const float ua = uu * av;
    sua = sua + ua;
}

// one element of the gradient before the scale of the image
__device__ __forceinline__ float lpips_grad(float x, float y, float mw, float inf, float ing, float sua) {
    const float av = x * inf, bv = y * ing;
    const float d = av - bv;
    const float md = mw * d;
    const float uu = 2.0f * md;
    const float pr = av * sua;
    const float df = uu - pr;
    return df * inf;
}

// 4 consecutive elements from element alignment: one 16-byte (fp32) or 8-byte (16-bit) access
template <int DT>
__device__ __forceinline__ void lpips_load4(const typename SampleElem<DT>::raw *p, float (&x)[4]) {
    typename SampleElem<DT>::raw v[4];
    __builtin_memcpy(v, p, sizeof(v));
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = SampleElem<DT>::f32(v[e]);
}

template <int DT>
__device__ __forceinline__ void lpips_store4(typename SampleElem<DT>::raw *p, const float (&x)[4]) {
    typename SampleElem<DT>::raw v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ce_round<DT>(x[e]);
    __builtin_memcpy(p, v, sizeof(v));
}

// ---- map layout ------------------------------------------------------------------------------------------------------------
struct LpipsMapAt {
    int64_t b, pos, r, base;                    // image, position, pixel b P + pos, offset of (b, channel 0, pos)
    int lane, group;
};

__device__ __forceinline__ bool lpips_map_at(const VqLpipsArgs &a, LpipsMapAt *at) {
    at->lane = threadIdx.x % VQ_LPIPS_MAP_POS;
    at->group = threadIdx.x / VQ_LPIPS_MAP_POS;
    at->b = (int64_t)blockIdx.x / a.tiles;
    at->pos = ((int64_t)blockIdx.x - at->b * a.tiles) * VQ_LPIPS_MAP_POS + at->lane;
    at->r = at->b * a.P + at->pos;
    at->base = at->b * a.C * a.P + at->pos;
    return at->pos < a.P;
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_LPIPS_THREADS) void lpips_map_fwd_kernel(VqLpipsArgs a, float *__restrict__ stats) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    __shared__ float part[2][VQ_LPIPS_MAP_GROUPS][VQ_LPIPS_MAP_POS];
    LpipsMapAt at;
    const bool live = lpips_map_at(a, &at);
    const typename EP::raw *f = reinterpret_cast<const typename EP::raw *>(a.pred) + at.base;
    const typename ET::raw *g = reinterpret_cast<const typename ET::raw *>(a.target) + at.base;
    const int C = a.C;
    float ff = 0.0f, gg = 0.0f;
    if (live) {
#pragma unroll 4
        for (int c = at.group; c < C; c += VQ_LPIPS_MAP_GROUPS) {
            const float x = EP::f32(f[(int64_t)c * a.P]), y = ET::f32(g[(int64_t)c * a.P]);
            const float x2 = x * x, y2 = y * y;
            ff = ff + x2;
            gg = gg + y2;
        }
    }
    part[0][at.group][at.lane] = ff;
    part[1][at.group][at.lane] = gg;
    __syncthreads();
    ff = (part[0][0][at.lane] + part[0][1][at.lane]) + (part[0][2][at.lane] + part[0][3][at.lane]);
    gg = (part[1][0][at.lane] + part[1][1][at.lane]) + (part[1][2][at.lane] + part[1][3][at.lane]);
    const LpipsNorm n = lpips_norms(ff, gg);
    float s = 0.0f, sua = 0.0f;
    if (live) {
        LpipsDrop drop;
        drop.init(a);
        const uint64_t i0 = (uint64_t)at.base;                                  // the logical index of (b, 0, pos)
#pragma unroll 4
        for (int c = at.group; c < C; c += VQ_LPIPS_MAP_GROUPS) {
            const float x = EP::f32(f[(int64_t)c * a.P]), y = ET::f32(g[(int64_t)c * a.P]);
            lpips_term(x, y, drop.weigh(a.w[c], i0 + (uint64_t)c * (uint64_t)a.P), n, s, sua);
        }
    }
    __syncthreads();                                                            // every thread has read the norms' partials
    part[0][at.group][at.lane] = s;
    part[1][at.group][at.lane] = sua;
    __syncthreads();
    if (!live || at.group != 0) return;
    s = (part[0][0][at.lane] + part[0][1][at.lane]) + (part[0][2][at.lane] + part[0][3][at.lane]);
    sua = (part[1][0][at.lane] + part[1][1][at.lane]) + (part[1][2][at.lane] + part[1][3][at.lane]);
    float *o = stats + 4 * at.r;
    o[0] = n.inf; o[1] = n.ing; o[2] = n.clamped ? 0.0f : sua; o[3] = s;
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_LPIPS_THREADS) void lpips_map_bwd_kernel(VqLpipsArgs a, const float *__restrict__ stats,
                                                                         const float *__restrict__ g_out, void *__restrict__ grad) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    LpipsMapAt at;
    if (!lpips_map_at(a, &at)) return;                                          // (no barrier in this kernel)
    const typename EP::raw *f = reinterpret_cast<const typename EP::raw *>(a.pred) + at.base;
    const typename ET::raw *g = reinterpret_cast<const typename ET::raw *>(a.target) + at.base;
    typename EP::raw *out = reinterpret_cast<typename EP::raw *>(grad) + at.base;
    const float *st = stats + 4 * at.r;
    const float inf = st[0], ing = st[1], sua = st[2];
    const float cr = g_out[at.b] / (float)a.P;
    LpipsDrop drop;
    drop.init(a);
    const uint64_t i0 = (uint64_t)at.base;
    const int C = a.C;
#pragma unroll 4
    for (int c = at.group; c < C; c += VQ_LPIPS_MAP_GROUPS) {
        const int64_t off = (int64_t)c * a.P;
        const float mw = drop.weigh(a.w[c], i0 + (uint64_t)c * (uint64_t)a.P);
        const float v = lpips_grad(EP::f32(f[off]), ET::f32(g[off]), mw, inf, ing, sua);
        out[off] = ce_round<DP>(cr * v);
    }
}

// ---- rows layout -----------------------------------------------------------------------------------------------------------
struct LpipsRowAt {
    int64_t r, b, pos, base;                    // pixel, image, position, offset of (pixel, channel 0)
    int sub;
};

__device__ __forceinline__ bool lpips_row_at(const VqLpipsArgs &a, LpipsRowAt *at) {
    at->sub = threadIdx.x % VQ_LPIPS_ROW_LANES;
    at->r = (int64_t)blockIdx.x * VQ_LPIPS_ROWS + threadIdx.x / VQ_LPIPS_ROW_LANES;
    const bool live = at->r < a.B * a.P;
    const int64_t r = live ? at->r : 0;
    at->b = r / a.P;
    at->pos = r - at->b * a.P;
    at->base = r * a.C;
    return live;
}

// the tree over the 16 lanes of a row (xor 1, 2, 4, 8 never leaves the 16 lanes)
__device__ __forceinline__ float lpips_row_sum(float v) {
#pragma unroll
    for (int o = 1; o < VQ_LPIPS_ROW_LANES; o <<= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_LPIPS_THREADS) void lpips_rows_fwd_kernel(VqLpipsArgs a, float *__restrict__ stats) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    LpipsRowAt at;
    const bool live = lpips_row_at(a, &at);                                     // a dead row reads row 0 and writes nothing
    const typename EP::raw *f = reinterpret_cast<const typename EP::raw *>(a.pred) + at.base;
    const typename ET::raw *g = reinterpret_cast<const typename ET::raw *>(a.target) + at.base;
    const int C = a.C, npiece = C / 4, tail = 4 * npiece + at.sub;
    float ff = 0.0f, gg = 0.0f;
#pragma unroll 2
    for (int q = at.sub; q < npiece; q += VQ_LPIPS_ROW_LANES) {
        float x[4], y[4];
        lpips_load4<DP>(f + 4 * q, x);
        lpips_load4<DT>(g + 4 * q, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x2 = x[e] * x[e], y2 = y[e] * y[e];
            ff = ff + x2;
            gg = gg + y2;
        }
    }
    if (tail < C) {
        const float x = EP::f32(f[tail]), y = ET::f32(g[tail]);
        const float x2 = x * x, y2 = y * y;
        ff = ff + x2;
        gg = gg + y2;
    }
    ff = lpips_row_sum(ff);
    gg = lpips_row_sum(gg);
    const LpipsNorm n = lpips_norms(ff, gg);
    LpipsDrop drop;
    drop.init(a);
    const uint64_t P = (uint64_t)a.P;
    const uint64_t i0 = (uint64_t)at.b * (uint64_t)C * P + (uint64_t)at.pos;    // the logical index of (b, 0, pos)
    float s = 0.0f, sua = 0.0f;
#pragma unroll 2
    for (int q = at.sub; q < npiece; q += VQ_LPIPS_ROW_LANES) {
        float x[4], y[4], w[4];
        lpips_load4<DP>(f + 4 * q, x);
        lpips_load4<DT>(g + 4 * q, y);
        lpips_load4<VQHIP_DTYPE_F32>(a.w + 4 * q, w);
#pragma unroll
        for (int e = 0; e < 4; ++e) lpips_term(x[e], y[e], drop.weigh(w[e], i0 + (uint64_t)(4 * q + e) * P), n, s, sua);
    }
    if (tail < C) lpips_term(EP::f32(f[tail]), ET::f32(g[tail]), drop.weigh(a.w[tail], i0 + (uint64_t)tail * P), n, s, sua);
    s = lpips_row_sum(s);
    sua = lpips_row_sum(sua);
    if (!live || at.sub != 0) return;
    float *o = stats + 4 * at.r;
    o[0] = n.inf; o[1] = n.ing; o[2] = n.clamped ? 0.0f : sua; o[3] = s;
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_LPIPS_THREADS) void lpips_rows_bwd_kernel(VqLpipsArgs a, const float *__restrict__ stats,
                                                                          const float *__restrict__ g_out, void *__restrict__ grad) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    LpipsRowAt at;
    if (!lpips_row_at(a, &at)) return;                                          // (no barrier and no shuffle in this kernel)
    const typename EP::raw *f = reinterpret_cast<const typename EP::raw *>(a.pred) + at.base;
    const typename ET::raw *g = reinterpret_cast<const typename ET::raw *>(a.target) + at.base;
    typename EP::raw *out = reinterpret_cast<typename EP::raw *>(grad) + at.base;
    const float *st = stats + 4 * at.r;
    const float inf = st[0], ing = st[1], sua = st[2];
    const float cr = g_out[at.b] / (float)a.P;
    LpipsDrop drop;
    drop.init(a);
    const int C = a.C, npiece = C / 4, tail = 4 * npiece + at.sub;
    const uint64_t P = (uint64_t)a.P;
    const uint64_t i0 = (uint64_t)at.b * (uint64_t)C * P + (uint64_t)at.pos;
#pragma unroll 2
    for (int q = at.sub; q < npiece; q += VQ_LPIPS_ROW_LANES) {
        float x[4], y[4], w[4], o[4];
        lpips_load4<DP>(f + 4 * q, x);
        lpips_load4<DT>(g + 4 * q, y);
        lpips_load4<VQHIP_DTYPE_F32>(a.w + 4 * q, w);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = lpips_grad(x[e], y[e], drop.weigh(w[e], i0 + (uint64_t)(4 * q + e) * P), inf, ing, sua);
            o[e] = cr * v;
        }
        lpips_store4<DP>(out + 4 * q, o);
    }
    if (tail < C) {
        const float v = lpips_grad(EP::f32(f[tail]), ET::f32(g[tail]), drop.weigh(a.w[tail], i0 + (uint64_t)tail * P), inf, ing, sua);
        out[tail] = ce_round<DP>(cr * v);
    }
}

// ---- the spatial mean of one image, and the mask for tests -----------------------------------------------------------------
__global__ __launch_bounds__(VQ_LPIPS_THREADS) void lpips_reduce_kernel(const float *__restrict__ stats, int64_t P, int accumulate,
                                                                        float *__restrict__ value) {
    __shared__ double ws[VQ_LPIPS_THREADS / 64];
    const int tid = threadIdx.x;
    const float *st = stats + 4 * (int64_t)blockIdx.x * P;
    double t = 0.0;
    for (int64_t p = tid; p < P; p += VQ_LPIPS_THREADS) t = t + (double)st[4 * p + 3];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) t = t + __shfl_xor(t, o, 64);
    if ((tid & 63) == 0) ws[tid >> 6] = t;
    __syncthreads();
    if (tid != 0) return;
    const double total = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    const float v = (float)(total / (double)P);
    value[blockIdx.x] = accumulate ? value[blockIdx.x] + v : v;
}

__global__ __launch_bounds__(VQ_LPIPS_THREADS) void lpips_keep_mask_kernel(const uint32_t *__restrict__ seed, uint32_t layer, uint32_t thr,
                                                                           int64_t n, uint8_t *__restrict__ out) {
    const uint32_t s0 = seed[0], s1 = seed[1];
    for (int64_t i = (int64_t)blockIdx.x * VQ_LPIPS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * VQ_LPIPS_THREADS)
        out[i] = lpips_keep(s0, s1, layer, thr, (uint64_t)i) ? 1 : 0;
}
