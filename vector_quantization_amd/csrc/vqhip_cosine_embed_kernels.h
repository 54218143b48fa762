// Fused CosineEmbeddingLoss of VQ-KD distillation (target +1): pred against a frozen teacher's target -> per-row loss, the three
// per-row statistics the backward needs, the two scalars, and the gradient over pred.  pred and target are read ONCE in the
// forward and once in the backward, each in its own dtype.
//
// Contract: include/vqhip.h (vqhip_cosine_embed_fwd / vqhip_cosine_embed_bwd), DESIGN.md §8.  Every element is converted to fp32
// exactly (SampleElem of the sampler); all arithmetic is fp32 IEEE without contraction, division and sqrtf correctly rounded.
//       dot = sum_j p_j t_j     pp = sum_j p_j^2 + 1e-12f     tt = sum_j t_j^2 + 1e-12f
//       den = sqrtf(pp * tt)     cos = dot / den     inv = 1 / den     ipp = 1 / pp     loss = 1 - cos
//       stats[r] = (inv, cos, ipp): the backward does no second reduction
//       grad_j = c_r * ((cos * ipp) * p_j - t_j * inv),   c_r = g (g / (float)R for the mean, a true division)
//
// ROWS layout: pred [R, C], unit column stride, row stride >= C.  ONE WAVE OWNS A ROW (four rows per 256-thread workgroup).
//   Why a wave and not a workgroup: at the shipped widths a row is 64 .. 160 pieces of 16 bytes (C = 512 .. 1280, bf16), one to
//   three per lane of a wave; a 256-thread workgroup would leave three of four lanes without a piece and pay an LDS round and a
//   barrier per row.  With a wave per row the three sums never leave registers, a 64 x 196 batch is 12 544 waves - more than
//   the 8 192 the 256 CUs hold at eight per SIMD (the rows kernels use 40 .. 76 VGPRs and no LDS: six to eight waves per SIMD) -
//   and nothing waits on a barrier.
//   PW = max(W_pred, W_target), W = 16 / sizeof(element): a PIECE is PW elements by the index j, never by the address: piece q
//   is elements [PW q, PW q + PW) for q < C / PW - one or two 16-byte loads of each operand at element alignment - followed
//   by C % PW pieces of one element.  Piece q belongs to lane q % 64; a lane takes its pieces in increasing q, its single
//   element (element PW (C / PW) + lane, for lane < C % PW) last, and adds element by element in increasing j:
//       dot = dot + p_j * t_j;   pp = pp + p_j * p_j;   tt = tt + t_j * t_j            (from +0)
//   The 64 lanes add as the balanced tree xor 1, 2, 4, 8, 16, 32 (x + y is commutative: every lane holds the same bits);
//   then pp = pp + 1e-12f, tt = tt + 1e-12f.
// MAP layout: pred [B, C, P] NCHW-contiguous, target rows [B P, C].  A workgroup owns 32 consecutive positions r = b P + p
//   (lane % 32; consecutive lanes read consecutive addresses of a channel plane) times 8 channel groups (thread / 32).
//   Channels are cut into QUADS [4 k, 4 k + 4), k < C / 4; quad k belongs to group k % 8, which takes its quads in increasing k
//   (target: one 16- or 8-byte load of the position's row; pred: four loads along P).  A thread keeps four accumulator triples,
//   triple e for channel 4 k + e; the C % 4 last channels 4 (C / 4) + e go to group 0's triple e after its quads.  A thread's
//   triples add as (a0 + a1) + (a2 + a3), the 8 groups through LDS as ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)).
//   No transpose, no [R, C] copy; the gradient is written in the same layout by the same assignment of channels to threads.
// In both layouts a row's outputs are a function of C and the two dtypes alone: not of R, of the other rows, of the address or
// alignment of a row, and run to run the same bits.  The two layouts add in different orders and need not agree bit for bit.
// Longest chain of additions of one sum, the product's own rounding counted as one: rows C / 64 + 8 (a lane's pieces) + 1 (its
// single element) + 6 (the tree) + 1; map C / 32 + 1 (a triple) + 1 (a tail channel) + 2 + 3 (the merges) + 1.  Both are below
// VQHIP_COSINE_EMBED_CHAIN(C) = C / 32 + 16.
// cosine_embed_reduce_kernel, ONE workgroup of 256 threads (a second launch behind the first on the same stream):
//   s_j = +0;  for r = j, j + 256, .. < R:  s_j = s_j + loss_r;  the xor tree over j, then (w0 + w1) + (w2 + w3).
//   out[0] = that sum, out[1] = out[0] / (float)R.  The order is a function of R alone.
// The backward writes every element of every row of grad (columns below C; the padding of a strided row is not touched),
// rounded to nearest even into pred's dtype.
// No atomics of any kind.  Every index is a row below R and a column below C.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_elem.h"                         // SampleElem: the exact conversion to fp32; ce_round: nearest even into the output dtype

#define VQ_COSE_THREADS 256
#define VQ_COSE_WAVES (VQ_COSE_THREADS / 64)
#define VQ_COSE_MAP_POS 32
#define VQ_COSE_MAP_GROUPS (VQ_COSE_THREADS / VQ_COSE_MAP_POS)
#define VQ_COSE_EPS 1e-12f

struct VqCoseArgs {
    const void *pred, *target;
    int64_t pred_stride, target_stride;         // elements between rows (rows layout: pred and grad each their own)
    int64_t R, P;                               // R = B P rows; P positions per image (map layout)
    int C;
};

struct CoseAcc {
    float dot, pp, tt;
};

__device__ __forceinline__ void cose_add(CoseAcc &a, float p, float t) {
    const float pt = p * t, p2 = p * p, t2 = t * t;
    a.dot = a.dot + pt;
    a.pp = a.pp + p2;
    a.tt = a.tt + t2;
}

__device__ __forceinline__ CoseAcc cose_sum(const CoseAcc &a, const CoseAcc &b) {
    CoseAcc o;
    o.dot = a.dot + b.dot; o.pp = a.pp + b.pp; o.tt = a.tt + b.tt;
    return o;
}

// N consecutive elements from element alignment, in 16-byte loads (N a multiple of W) or one narrower load (N < W)
template <int DT, int N>
__device__ __forceinline__ void cose_load(const typename SampleElem<DT>::raw *p, float (&x)[N]) {
    typedef SampleElem<DT> E;
    typename E::raw v[N];
    if constexpr (N >= E::W) {
#pragma unroll
        for (int k = 0; k < N; k += E::W) __builtin_memcpy(v + k, p + k, 16);
    } else {
        __builtin_memcpy(v, p, N * sizeof(typename E::raw));
    }
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = E::f32(v[e]);
}

template <int DT, int N>
__device__ __forceinline__ void cose_store(typename SampleElem<DT>::raw *p, const float (&x)[N]) {
    typedef SampleElem<DT> E;
    typename E::raw v[N];
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = ce_round<DT>(x[e]);
#pragma unroll
    for (int k = 0; k < N; k += E::W) __builtin_memcpy(p + k, v + k, 16);
}

// (inv, cos, ipp) and the loss of a row from its three finished sums
__device__ __forceinline__ void cose_finish(CoseAcc c, int64_t r, float *__restrict__ loss, float *__restrict__ stats) {
    const float pp = c.pp + VQ_COSE_EPS, tt = c.tt + VQ_COSE_EPS;
    const float prod = pp * tt;
    const float den = sqrtf(prod);
    const float cs = c.dot / den;
    stats[3 * r + 0] = 1.0f / den;
    stats[3 * r + 1] = cs;
    stats[3 * r + 2] = 1.0f / pp;
    loss[r] = 1.0f - cs;
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_COSE_THREADS) void cosine_embed_rows_fwd_kernel(VqCoseArgs a, float *__restrict__ loss,
                                                                                float *__restrict__ stats) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    constexpr int PW = EP::W > ET::W ? EP::W : ET::W;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * VQ_COSE_WAVES + (threadIdx.x >> 6);
    if (r >= a.R) return;                                                       // (no barrier below: a wave is on its own)
    const typename EP::raw *p = reinterpret_cast<const typename EP::raw *>(a.pred) + r * a.pred_stride;
    const typename ET::raw *t = reinterpret_cast<const typename ET::raw *>(a.target) + r * a.target_stride;
    const int C = a.C, npiece = C / PW;
    CoseAcc c = {0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int q = lane; q < npiece; q += 64) {
        float x[PW], y[PW];
        cose_load<DP, PW>(p + q * PW, x);
        cose_load<DT, PW>(t + q * PW, y);
#pragma unroll
        for (int e = 0; e < PW; ++e) cose_add(c, x[e], y[e]);
    }
    if (lane < C - npiece * PW) {                                               // C % PW < PW <= 8 single elements
        const int j = npiece * PW + lane;
        cose_add(c, EP::f32(p[j]), ET::f32(t[j]));
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        CoseAcc b;
        b.dot = __shfl_xor(c.dot, o, 64); b.pp = __shfl_xor(c.pp, o, 64); b.tt = __shfl_xor(c.tt, o, 64);
        c = cose_sum(c, b);
    }
    if (lane == 0) cose_finish(c, r, loss, stats);
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_COSE_THREADS) void cosine_embed_rows_bwd_kernel(VqCoseArgs a, const float *__restrict__ stats,
                                                                                const float *__restrict__ g, int g_per_row, int mean,
                                                                                void *__restrict__ grad, int64_t grad_stride) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    constexpr int PW = EP::W > ET::W ? EP::W : ET::W;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * VQ_COSE_WAVES + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const typename EP::raw *p = reinterpret_cast<const typename EP::raw *>(a.pred) + r * a.pred_stride;
    const typename ET::raw *t = reinterpret_cast<const typename ET::raw *>(a.target) + r * a.target_stride;
    typename EP::raw *out = reinterpret_cast<typename EP::raw *>(grad) + r * grad_stride;
    const float inv = stats[3 * r + 0], cs = stats[3 * r + 1], ipp = stats[3 * r + 2];
    float cr = g[g_per_row ? r : 0];
    if (mean) cr = cr / (float)a.R;
    const float k2 = cs * ipp;
    const int C = a.C, npiece = C / PW;
#pragma unroll 2
    for (int q = lane; q < npiece; q += 64) {
        float x[PW], y[PW], o[PW];
        cose_load<DP, PW>(p + q * PW, x);
        cose_load<DT, PW>(t + q * PW, y);
#pragma unroll
        for (int e = 0; e < PW; ++e) {
            const float b = k2 * x[e], s = y[e] * inv;
            const float d = b - s;
            o[e] = cr * d;
        }
        cose_store<DP, PW>(out + q * PW, o);
    }
    if (lane < C - npiece * PW) {
        const int j = npiece * PW + lane;
        const float b = k2 * EP::f32(p[j]), s = ET::f32(t[j]) * inv;
        const float d = b - s;
        out[j] = ce_round<DP>(cr * d);
    }
}

// the position and channel group of a thread of the map kernels; false where the tile hangs over the last row
struct CoseMapAt {
    int64_t r, base;                            // the row b P + p, and the offset of (b, channel 0, p) in the map
    int group;
};

__device__ __forceinline__ bool cose_map_at(const VqCoseArgs &a, CoseMapAt *at) {
    at->group = threadIdx.x / VQ_COSE_MAP_POS;
    at->r = (int64_t)blockIdx.x * VQ_COSE_MAP_POS + (threadIdx.x % VQ_COSE_MAP_POS);
    if (at->r >= a.R) return false;
    const int64_t b = at->r / a.P, pos = at->r - b * a.P;
    at->base = b * a.C * a.P + pos;
    return true;
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_COSE_THREADS) void cosine_embed_map_fwd_kernel(VqCoseArgs a, float *__restrict__ loss,
                                                                               float *__restrict__ stats) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    __shared__ CoseAcc part[VQ_COSE_MAP_GROUPS][VQ_COSE_MAP_POS];
    CoseMapAt at;
    const bool live = cose_map_at(a, &at);
    CoseAcc acc[4] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    if (live) {
        const typename EP::raw *p = reinterpret_cast<const typename EP::raw *>(a.pred) + at.base;
        const typename ET::raw *t = reinterpret_cast<const typename ET::raw *>(a.target) + at.r * a.target_stride;
        const int C = a.C, nquad = C / 4;
        for (int k = at.group; k < nquad; k += VQ_COSE_MAP_GROUPS) {
            float y[4];
            cose_load<DT, 4>(t + 4 * k, y);
#pragma unroll
            for (int e = 0; e < 4; ++e) cose_add(acc[e], EP::f32(p[(int64_t)(4 * k + e) * a.P]), y[e]);
        }
        if (at.group == 0) {
            for (int e = 0; e < C - 4 * nquad; ++e) {                           // (e < 3: acc[e] with a constant index after unrolling)
                const int ch = 4 * nquad + e;
                const float pv = EP::f32(p[(int64_t)ch * a.P]), tv = ET::f32(t[ch]);
                if (e == 0) cose_add(acc[0], pv, tv);
                else if (e == 1) cose_add(acc[1], pv, tv);
                else cose_add(acc[2], pv, tv);
            }
        }
    }
    part[at.group][threadIdx.x % VQ_COSE_MAP_POS] = cose_sum(cose_sum(acc[0], acc[1]), cose_sum(acc[2], acc[3]));
    __syncthreads();
    if (!live || at.group != 0) return;
    const int i = threadIdx.x;                                                  // group 0: the position inside the tile
    const CoseAcc c = cose_sum(cose_sum(cose_sum(part[0][i], part[1][i]), cose_sum(part[2][i], part[3][i])),
                               cose_sum(cose_sum(part[4][i], part[5][i]), cose_sum(part[6][i], part[7][i])));
    cose_finish(c, at.r, loss, stats);
}

template <int DP, int DT>
__global__ __launch_bounds__(VQ_COSE_THREADS) void cosine_embed_map_bwd_kernel(VqCoseArgs a, const float *__restrict__ stats,
                                                                               const float *__restrict__ g, int g_per_row, int mean,
                                                                               void *__restrict__ grad) {
    typedef SampleElem<DP> EP;
    typedef SampleElem<DT> ET;
    CoseMapAt at;
    if (!cose_map_at(a, &at)) return;                                           // (no barrier in this kernel)
    const typename EP::raw *p = reinterpret_cast<const typename EP::raw *>(a.pred) + at.base;
    const typename ET::raw *t = reinterpret_cast<const typename ET::raw *>(a.target) + at.r * a.target_stride;
    typename EP::raw *out = reinterpret_cast<typename EP::raw *>(grad) + at.base;
    const float inv = stats[3 * at.r + 0], cs = stats[3 * at.r + 1], ipp = stats[3 * at.r + 2];
    float cr = g[g_per_row ? at.r : 0];
    if (mean) cr = cr / (float)a.R;
    const float k2 = cs * ipp;
    const int C = a.C, nquad = C / 4;
    auto one = [&](int ch, float tv) {
        const int64_t off = (int64_t)ch * a.P;
        const float b = k2 * EP::f32(p[off]), s = tv * inv;
        const float d = b - s;
        out[off] = ce_round<DP>(cr * d);
    };
    for (int k = at.group; k < nquad; k += VQ_COSE_MAP_GROUPS) {
        float y[4];
        cose_load<DT, 4>(t + 4 * k, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) one(4 * k + e, y[e]);
    }
    if (at.group == 0)
        for (int ch = 4 * nquad; ch < C; ++ch) one(ch, ET::f32(t[ch]));
}

// out[0] = sum_r loss_r, out[1] = out[0] / (float)R
__global__ __launch_bounds__(VQ_COSE_THREADS) void cosine_embed_reduce_kernel(const float *__restrict__ loss, int64_t R,
                                                                              float *__restrict__ out) {
    __shared__ float ws[VQ_COSE_WAVES];
    const int tid = threadIdx.x;
    float s = 0.0f;
    for (int64_t r = tid; r < R; r += VQ_COSE_THREADS) s = s + loss[r];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) ws[tid >> 6] = s;
    __syncthreads();
    if (tid != 0) return;
    const float L = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    out[0] = L;
    out[1] = L / (float)R;
}
