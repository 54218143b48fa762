// The two memory-bound ops between the convolutions of StyleGAN2Discriminator (vq/algorithms/vqgan/discriminators/stylegan2.py):
// bias-activation (mmcv's FusedBiasLeakyReLU) and the 4-tap FIR blur (mmcv's upfirdn2d with k = outer([1, 3, 3, 1]) / 64), each
// with its backward, and the fused form blur(act(x + bias)) that reads the convolution's output once.
//
// Contract: include/vqhip.h (vqhip_bias_act_fwd / _bwd, vqhip_fir4_fwd / _bwd), DESIGN.md §8.  Every element is converted to fp32
// exactly (SampleElem of the sampler); all arithmetic is fp32 IEEE without contraction; results are rounded to nearest even into
// the output dtype (ce_round of the token cross-entropy).
//
// BIAS-ACTIVATION     t = x + bias[c];   l = t > 0 ? t : t * slope;   y = l * scale          (slope = 0.2f, scale = (float)sqrt(2))
//       backward     f = y > 0 ? scale : scale * slope (one rounded product);   gx = g * f;   gbias[c] = sum of the fp32 gx
//   The logical tensor is [B, C, P]; the memory is MAP (NCHW: channel stride P) or ROWS (channels-last: rows of C).
//   bias_act_fwd_kernel: a thread owns PIECES of W = 16 / sizeof(element) consecutive elements, piece q = [W q, W q + W), 16
//   bytes at element alignment (copied as a block: the compiler picks the accesses, and without a proof of alignment it emits
//   one dwordx4 load in the forward and splits the stores and the backward's loads); the last piece may be short.  The channel of an element is (i / P) % C (map), i % C (rows).
//   bias_act_bwd_map_kernel: a workgroup owns one CHUNK of 4096 consecutive positions of one (b, c) plane; thread t takes the
//   chunk's pieces t, t + 256, .. in that order, their elements in increasing index, into one accumulator from +0.
//   bias_act_bwd_rows_kernel: a workgroup owns 256 consecutive rows times 64 pieces of W channels; thread (lane, group) takes rows
//   group, group + 4, .. of the slab into W accumulators, the 4 groups add as (g0 + g1) + (g2 + g3).
//   Either writes the partial of its SLAB s and channel c to ws[s C + c]: every (s, c) is written, so ws needs no memset.
// sg2_reduce_kernel (the second stage, shared with the fused blur backward): 16 channels x 16 slab groups per workgroup; group j
//   adds slabs j, j + 16, .. in increasing s from +0; the 16 groups add as a balanced binary tree in order.  No atomics: gbias is a
//   function of the shape and the values alone, the same bits run to run.
//
// FIR  One kernel serves the blur and its adjoint as upfirdn: out[o] = sum_{i < 4} k[i] src(o * DOWN + i - off), where src(S) is
//   in[S / up] for S a multiple of up with 0 <= S / up < the input's size, and +0 elsewhere (zero padding, zero insertion).
//       forward   up = 1, DOWN = d, off = pad0            adjoint   up = d, DOWN = 1, off = 3 - pad0  (k is symmetric: flipped = k)
//   A workgroup owns CB channels x TOH x TOW outputs of one image: map CB = 1, 16 x 64; rows CB = 32, 8 x 8.  The source tile with
//   its halo, (TOH DOWN + 3) x (TOW DOWN + 3) x CB, is staged in LDS as fp32 (in the fused forward: AFTER bias-activation, the
//   padding staying +0).  Thread (cc, ox, rg) owns output column (cc, ox) and RPT consecutive output rows (map: 4 of 16; rows: all
//   8): it walks the source rows of its column top down, forms the horizontal sum of each
//       h(r) = ((k0 s(r, 0) + k1 s(r, 1)) + k2 s(r, 2)) + k3 s(r, 3)          k = (1/8, 3/8, 3/8, 1/8), every product rounded once
//   and from the last four the output  v = ((k0 h(r - 3) + k1 h(r - 2)) + k2 h(r - 1)) + k3 h(r).  With DOWN = 2 only the kept
//   outputs are formed.  An output is a function of its 4 x 4 sources alone: not of the tile, the layout or the address.
//   Fused backward: v is multiplied by f = (x + bias[c] > 0 ? scale : scale * slope) of the SAVED conv output x at the same index,
//   and the thread adds its fp32 products in increasing row into one accumulator; threads of one channel add as a balanced tree
//   through LDS (stride 128, 64, .. CB); the partial goes to ws[slab C + c], slab = blockIdx (per channel block), then sg2_reduce.
// Every global index is guarded: b < B, c < C, source and output coordinates inside their planes.  No atomics, no memset.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_elem.h"                         // SampleElem: the exact conversion to fp32; ce_round: nearest even into the output dtype
#include "vqhip_slab_reduce.h"                  // VQ_SG2_THREADS, VQ_SG2_ROWS_SLAB, sg2_reduce_kernel: the second stage of the bias gradient

#define VQ_SG2_SLOPE 0.2f
#define VQ_SG2_SCALE 1.41421356237309515f
#define VQ_SG2_MAP_CHUNK 4096                   // positions of a plane per workgroup of bias_act_bwd_map_kernel

struct VqBiasActArgs {
    const void *x;                              // forward: the input; backward: the incoming gradient g
    const void *y;                              // backward: the saved output
    const float *bias;                          // [C] (forward)
    void *out;                                  // y (forward) / gx (backward)
    float *ws;                                  // [slabs, C] (backward)
    int64_t n;                                  // B C P < 2^31
    int B, C, P;
    int chunks;                                 // ceil(P / 4096) (map backward)
};

__device__ __forceinline__ float sg2_act(float x, float b) {
    const float t = x + b;
    const float l = t > 0.0f ? t : t * VQ_SG2_SLOPE;
    return l * VQ_SG2_SCALE;
}

__device__ __forceinline__ float sg2_factor(float y) { return y > 0.0f ? VQ_SG2_SCALE : VQ_SG2_SCALE * VQ_SG2_SLOPE; }

// up to W consecutive elements from element alignment: a 16-byte block copy when the piece is whole
template <int DT>
__device__ __forceinline__ void sg2_load(const typename SampleElem<DT>::raw *p, int cnt, float (&x)[SampleElem<DT>::W]) {
    constexpr int W = SampleElem<DT>::W;
    typename SampleElem<DT>::raw v[W];
    if (cnt == W) {
        __builtin_memcpy(v, p, sizeof(v));
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = e < cnt ? p[e] : (typename SampleElem<DT>::raw)0;
    }
#pragma unroll
    for (int e = 0; e < W; ++e) x[e] = SampleElem<DT>::f32(v[e]);
}

template <int DT>
__device__ __forceinline__ void sg2_store(typename SampleElem<DT>::raw *p, int cnt, const float (&x)[SampleElem<DT>::W]) {
    constexpr int W = SampleElem<DT>::W;
    typename SampleElem<DT>::raw v[W];
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = ce_round<DT>(x[e]);
    if (cnt == W) {
        __builtin_memcpy(p, v, sizeof(v));
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e)
            if (e < cnt) p[e] = v[e];
    }
}

template <int DT, bool ROWS>
__global__ __launch_bounds__(VQ_SG2_THREADS) void bias_act_fwd_kernel(VqBiasActArgs a) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    const raw *in = reinterpret_cast<const raw *>(a.x);
    raw *out = reinterpret_cast<raw *>(a.out);
    const uint32_t n = (uint32_t)a.n, C = (uint32_t)a.C, P = ROWS ? 1u : (uint32_t)a.P;
    const uint32_t pieces = (n + W - 1) / W;
    for (uint32_t q = blockIdx.x * VQ_SG2_THREADS + threadIdx.x; q < pieces; q += gridDim.x * VQ_SG2_THREADS) {
        const uint32_t i0 = q * W;                                              // pieces * W < 2^31 + 8
        const int cnt = n - i0 < (uint32_t)W ? (int)(n - i0) : W;
        float x[W];
        sg2_load<DT>(in + i0, cnt, x);
        uint32_t plane = i0 / P, rem = i0 - plane * P, c = plane % C;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            x[e] = sg2_act(x[e], a.bias[c]);
            if (++rem == P) { rem = 0; if (++c == C) c = 0; }
        }
        sg2_store<DT>(out + i0, cnt, x);
    }
}

// (w0 + w1) + (w2 + w3) of the four waves' xor-tree sums; the result is valid in thread 0
__device__ __forceinline__ float sg2_block_sum(float v, float *red /* [4] in LDS */) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int DT>
__global__ __launch_bounds__(VQ_SG2_THREADS) void bias_act_bwd_map_kernel(VqBiasActArgs a) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    __shared__ float red[4];
    const int64_t blk = blockIdx.x;                                             // (b C + c) chunks + chunk
    const int64_t plane = blk / a.chunks;
    const int chunk = (int)(blk - plane * a.chunks);
    const int b = (int)(plane / a.C), c = (int)(plane - (int64_t)b * a.C);
    const int p0 = chunk * VQ_SG2_MAP_CHUNK;
    const int len = a.P - p0 < VQ_SG2_MAP_CHUNK ? a.P - p0 : VQ_SG2_MAP_CHUNK;
    const int64_t base = plane * a.P + p0;
    const raw *g = reinterpret_cast<const raw *>(a.x) + base;
    const raw *y = reinterpret_cast<const raw *>(a.y) + base;
    raw *out = reinterpret_cast<raw *>(a.out) + base;
    float acc = 0.0f;
    for (int i0 = threadIdx.x * W; i0 < len; i0 += VQ_SG2_THREADS * W) {
        const int cnt = len - i0 < W ? len - i0 : W;
        float gv[W], yv[W];
        sg2_load<DT>(g + i0, cnt, gv);
        sg2_load<DT>(y + i0, cnt, yv);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            gv[e] = gv[e] * sg2_factor(yv[e]);
            if (e < cnt) acc = acc + gv[e];
        }
        sg2_store<DT>(out + i0, cnt, gv);
    }
    const float s = sg2_block_sum(acc, red);
    if (threadIdx.x == 0 && a.ws) a.ws[((int64_t)b * a.chunks + chunk) * a.C + c] = s;
}

template <int DT>
__global__ __launch_bounds__(VQ_SG2_THREADS) void bias_act_bwd_rows_kernel(VqBiasActArgs a) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    __shared__ float red[4][64][W];
    const int lane = threadIdx.x & 63, group = threadIdx.x >> 6;
    const int64_t R = (int64_t)a.B * a.P;
    const int64_t r0 = (int64_t)blockIdx.x * VQ_SG2_ROWS_SLAB;
    const int c0 = ((int)blockIdx.y * 64 + lane) * W;
    const int cnt = c0 >= a.C ? 0 : (a.C - c0 < W ? a.C - c0 : W);
    float acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.0f;
    if (cnt > 0) {
        const raw *g = reinterpret_cast<const raw *>(a.x);
        const raw *y = reinterpret_cast<const raw *>(a.y);
        raw *out = reinterpret_cast<raw *>(a.out);
        for (int j = group; j < VQ_SG2_ROWS_SLAB && r0 + j < R; j += 4) {
            const int64_t off = (r0 + j) * a.C + c0;
            float gv[W], yv[W];
            sg2_load<DT>(g + off, cnt, gv);
            sg2_load<DT>(y + off, cnt, yv);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                gv[e] = gv[e] * sg2_factor(yv[e]);
                acc[e] = acc[e] + gv[e];                                        // (beyond cnt: g = +0, a zero that is never stored)
            }
            sg2_store<DT>(out + off, cnt, gv);
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) red[group][lane][e] = acc[e];
    __syncthreads();
    if (group != 0 || cnt == 0 || !a.ws) return;
    for (int e = 0; e < cnt; ++e)
        a.ws[(int64_t)blockIdx.x * a.C + c0 + e] = (red[0][lane][e] + red[1][lane][e]) + (red[2][lane][e] + red[3][lane][e]);
}

// ---- FIR -------------------------------------------------------------------------------------------------------------------
#define VQ_FIR_NONE 0
#define VQ_FIR_ACT_IN 1                         // forward: bias-activation on the way into the tile
#define VQ_FIR_MASK_OUT 2                       // backward: the factor of the saved conv output on the way out, and gbias partials

struct VqFirArgs {
    const void *in;                             // [B, C, IH, IW] in the layout
    void *out;                                  // [B, C, OH, OW]
    const void *x;                              // MASK_OUT: the saved conv output, shaped and laid out like out
    const float *bias;                          // [C] (ACT_IN, MASK_OUT)
    float *ws;                                  // [slabs, C] (MASK_OUT)
    int B, C, IH, IW, OH, OW;
    int up, offy, offx;                         // source coordinate S = o DOWN + i - off in the zero-inserted input
    int cblocks, tiles_y, tiles_x;              // blockIdx.x = ((b cblocks + cb) tiles_y + ty) tiles_x + tx
};

template <bool ROWS> struct FirTile;
template <> struct FirTile<false> { static constexpr int CB = 1, TOH = 16, TOW = 64, RPT = 4; };
template <> struct FirTile<true> { static constexpr int CB = 32, TOH = 8, TOW = 8, RPT = 8; };

template <int DT, bool ROWS, int DOWN, int FUSED>
__global__ __launch_bounds__(VQ_SG2_THREADS) void fir4_kernel(VqFirArgs a) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    typedef FirTile<ROWS> T;
    constexpr int CB = T::CB, TOH = T::TOH, TOW = T::TOW, RPT = T::RPT;
    constexpr int TIH = TOH * DOWN + 3, TIW = TOW * DOWN + 3;
    static_assert(CB * TOW * (TOH / RPT) == VQ_SG2_THREADS, "one thread per output column and row group");
    __shared__ float tile[TIH * TIW * CB];
    __shared__ float red[FUSED == VQ_FIR_MASK_OUT ? VQ_SG2_THREADS : 1];
    int64_t blk = blockIdx.x;
    const int tx = (int)(blk % a.tiles_x); blk /= a.tiles_x;
    const int ty = (int)(blk % a.tiles_y); blk /= a.tiles_y;
    const int cb = (int)(blk % a.cblocks);
    const int b = (int)(blk / a.cblocks);
    const int c_base = cb * CB, oy_base = ty * TOH, ox_base = tx * TOW;
    const int sy_base = oy_base * DOWN - a.offy, sx_base = ox_base * DOWN - a.offx;   // source coordinate of tile row / column 0
    const raw *in = reinterpret_cast<const raw *>(a.in);
    // plane strides of the two layouts, in elements
    const int64_t in_c = ROWS ? 1 : (int64_t)a.IH * a.IW, in_p = ROWS ? a.C : 1;
    const int64_t in_b = (int64_t)a.C * a.IH * a.IW;
    for (int idx = threadIdx.x; idx < TIH * TIW * CB; idx += VQ_SG2_THREADS) {
        const int cc = idx % CB, col = (idx / CB) % TIW, row = idx / (CB * TIW);
        const int c = c_base + cc, sy = sy_base + row, sx = sx_base + col;
        float v = 0.0f;
        if (c < a.C && sy >= 0 && sx >= 0) {
            const int iy = sy / a.up, ix = sx / a.up;
            if (iy * a.up == sy && ix * a.up == sx && iy < a.IH && ix < a.IW) {
                v = E::f32(in[b * in_b + c * in_c + ((int64_t)iy * a.IW + ix) * in_p]);
                if (FUSED == VQ_FIR_ACT_IN) v = sg2_act(v, a.bias[c]);
            }
        }
        tile[idx] = v;
    }
    __syncthreads();
    const int cc = threadIdx.x % CB, oxl = (threadIdx.x / CB) % TOW, rg = threadIdx.x / (CB * TOW);
    const int c = c_base + cc, ox = ox_base + oxl;
    const bool live = c < a.C && ox < a.OW;
    const float k0 = 0.125f, k1 = 0.375f;
    const int64_t out_c = ROWS ? 1 : (int64_t)a.OH * a.OW, out_p = ROWS ? a.C : 1;
    const int64_t out_base = (int64_t)b * a.C * a.OH * a.OW + c * out_c;
    raw *out = reinterpret_cast<raw *>(a.out);
    float acc = 0.0f, bias_c = 0.0f;
    if (FUSED == VQ_FIR_MASK_OUT && live) bias_c = a.bias[c];
    if (live) {
        float h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float *src = tile + ((rg * RPT * DOWN) * TIW + oxl * DOWN) * CB + cc;
#pragma unroll
        for (int rr = 0; rr < RPT * DOWN + 3; ++rr) {
            const float *s = src + rr * TIW * CB;
            const float p0 = k0 * s[0], p1 = k1 * s[CB], p2 = k1 * s[2 * CB], p3 = k0 * s[3 * CB];
            h[0] = h[1]; h[1] = h[2]; h[2] = h[3];
            h[3] = ((p0 + p1) + p2) + p3;
            if (rr >= 3 && (rr - 3) % DOWN == 0) {
                const int oy = oy_base + rg * RPT + (rr - 3) / DOWN;
                if (oy < a.OH) {
                    const float q0 = k0 * h[0], q1 = k1 * h[1], q2 = k1 * h[2], q3 = k0 * h[3];
                    float v = ((q0 + q1) + q2) + q3;
                    const int64_t off = out_base + ((int64_t)oy * a.OW + ox) * out_p;
                    if (FUSED == VQ_FIR_MASK_OUT) {
                        const float xv = E::f32(reinterpret_cast<const raw *>(a.x)[off]);
                        v = v * sg2_factor(xv + bias_c);
                        acc = acc + v;
                    }
                    out[off] = ce_round<DT>(v);
                }
            }
        }
    }
    if (FUSED == VQ_FIR_MASK_OUT) {
        red[threadIdx.x] = acc;
        __syncthreads();
#pragma unroll
        for (int stride = VQ_SG2_THREADS / 2; stride >= CB; stride >>= 1) {
            if ((int)threadIdx.x < stride) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + stride];
            __syncthreads();
        }
        if ((int)threadIdx.x < CB && c < a.C) {
            const int64_t slab = ((int64_t)b * a.tiles_y + ty) * a.tiles_x + tx;
            a.ws[slab * a.C + c] = red[threadIdx.x];
        }
    }
}
