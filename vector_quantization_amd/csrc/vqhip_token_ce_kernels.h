// Fused token cross-entropy of stage-2 training: logits [R, >= end] against one target per row -> per-row loss, lse and hit,
// the weighted scalar, and the gradient over the logits.  The logits are read ONCE in the forward and once in the backward.
//
// Contract: include/vqhip.h (vqhip_token_ce_fwd / vqhip_token_ce_bwd), DESIGN.md §8.  V = end - start, T = VQ_CE_THREADS,
// W = 16 / sizeof(element) (4 for fp32, 8 for bf16 / fp16).  Every element is converted to fp32 exactly (SampleElem of the
// sampler); all arithmetic is fp32 IEEE without contraction, expf / logf at <= 1 ulp.
//
// token_ce_fwd_kernel, one workgroup per row.  The slice is cut into PIECES by the index j inside the slice, never by the
// address: piece q is elements [W q, W q + W) for q < V / W, followed by V % W pieces of one element.  Piece q belongs to
// thread q % T, a thread takes its pieces in increasing q, the single-element pieces (q = V / W + i for thread i) last.  A
// whole piece is one 16-byte load at element alignment (global loads need none on gfx950), so what a thread adds up, and in
// which order, does not depend on where the row lies in memory: a strided view and its copy give the same bits.  (The
// sampler's SampleRow cuts rows at 16-byte boundaries - exact there because its sums are integers, not reusable here.)
//   per thread   m = -inf, s = +0, sa = +0, bi = INT_MAX.  For a piece x_0 .. x_{n-1} at index i0:
//                  pm = fmaxf(.. fmaxf(x_0, x_1) .., x_{n-1});
//                  if (pm > m) { s = s * expf(m - pm); m = pm; bi = i0 + (first e with x_e == pm); }
//                  mm = (m == -inf) ? 0 : m;   for e = 0 .. n-1:  s = s + expf(x_e - mm);  sa = sa + x_e;
//   merge(A, B)  M = fmaxf(A.m, B.m);  f_X = (X.m == M) ? 1 : expf(X.m - M);  s = A.s * f_A + B.s * f_B;  sa = A.sa + B.sa;
//                bi = the bi of the larger m, the smaller bi where the two m are equal.   (merge(A, B) == merge(B, A) bit for bit.)
//   tree         lanes of a wave by xor 1, 2, 4, 8, 16, 32 (a balanced tree over the lanes in their order), the four waves
//                through LDS as merge(merge(w0, w1), merge(w2, w3)).
//   row          lse = (M == -inf) ? NaN : M + logf(s);   a_t by one element load;   d1 = lse - a_t;
//                eps == 0: loss = d1;   else loss = (float)(1 - (double)eps) * d1 + eps * (lse - sa / (float)V);
//                hit = (lse == lse && bi == t - start).  An ignored row: loss 0, hit 0 (lse as for any row).  A target outside
//                [start, end): loss NaN, hit 0; nothing is read at the target.
// token_ce_reduce_kernel, ONE workgroup of T threads (a second launch behind the first on the same stream):
//   s_j = +0;  for r = j, j + T, j + 2T, .. < R, skipping ignored rows:  s_j = s_j + w_r * loss_r;  (W and the hits likewise)
//   then the same xor tree over j and ((w0 + w1) + (w2 + w3)).  The order is a function of R alone.
// token_ce_bwd_kernel, one workgroup per row: p = expf(a_j - lse_r), grad = c_r * ((p - oh_j) - eps / (float)V), oh_j =
//   (float)(1 - (double)eps) at the target and 0 elsewhere, c_r = g * w_r (/ W for the mean, a true division), rounded to
//   nearest even into the logits' dtype.  Columns [0, cols) outside the slice, and every column of an ignored row, are written
//   as zeros; pieces here are cut by the column index and stored with 16-byte stores at element alignment.
// No atomics of any kind.  Every index is a row below R, an element below V inside the slice, or a column below cols.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_elem.h"                         // SampleElem: the exact conversion to fp32; ce_round: nearest even into the output dtype

#define VQ_CE_THREADS 256
#define VQ_CE_WAVES (VQ_CE_THREADS / 64)
#define VQ_CE_MAX_V (1 << 20)

struct VqCeArgs {
    const void *logits;
    int64_t row_stride, start;
    int V;
    int64_t R;
    const void *targets;
    int64_t shift_len, ignore_index;
    float eps, one_minus_eps, eps_over_v;       // (float)(1 - (double)eps), eps / (float)V
    const float *weight;                        // [R] or null
};

#define VQ_CE_CLASS 0
#define VQ_CE_IGNORED 1
#define VQ_CE_OUTSIDE 2

// what row r is held to: VQ_CE_CLASS with *j = target - start in [0, V), VQ_CE_IGNORED, or VQ_CE_OUTSIDE
template <bool I64>
__device__ __forceinline__ int ce_target(const VqCeArgs &a, int64_t r, int *j) {
    int64_t at = r;
    if (a.shift_len > 0) {
        if (r % a.shift_len == a.shift_len - 1) return VQ_CE_IGNORED;          // the last position of a sequence
        at = r + 1;                                                           // (inside the same sequence: at < R)
    }
    const int64_t t = I64 ? reinterpret_cast<const int64_t *>(a.targets)[at] : (int64_t)reinterpret_cast<const int32_t *>(a.targets)[at];
    if (t == a.ignore_index) return VQ_CE_IGNORED;
    if (t < a.start || t - a.start >= a.V) return VQ_CE_OUTSIDE;
    *j = (int)(t - a.start);
    return VQ_CE_CLASS;
}

struct CeAcc {
    float m, s, sa;
    int bi;
};

__device__ __forceinline__ CeAcc ce_merge(const CeAcc &A, const CeAcc &B) {
    CeAcc o;
    o.m = fmaxf(A.m, B.m);                                                      // (m is never NaN)
    const float fa = (A.m == o.m) ? 1.0f : expf(A.m - o.m);
    const float fb = (B.m == o.m) ? 1.0f : expf(B.m - o.m);
    const float l = A.s * fa, r = B.s * fb;
    o.s = l + r;
    o.sa = A.sa + B.sa;
    o.bi = (A.m > B.m) ? A.bi : ((B.m > A.m) ? B.bi : (A.bi < B.bi ? A.bi : B.bi));
    return o;
}

template <int N>
__device__ __forceinline__ void ce_piece(CeAcc &c, const float (&x)[N], int i0) {
    float pm = x[0];
#pragma unroll
    for (int e = 1; e < N; ++e) pm = fmaxf(pm, x[e]);
    if (pm > c.m) {
        c.s = c.s * expf(c.m - pm);
        c.m = pm;
        int first = N - 1;
#pragma unroll
        for (int e = N - 2; e >= 0; --e) first = (x[e] == pm) ? e : first;
        c.bi = i0 + first;
    }
    const float mm = (c.m == -__builtin_inff()) ? 0.0f : c.m;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        c.s = c.s + expf(x[e] - mm);
        c.sa = c.sa + x[e];
    }
}

template <int DT, bool I64>
__global__ __launch_bounds__(VQ_CE_THREADS) void token_ce_fwd_kernel(VqCeArgs a, float *__restrict__ loss, float *__restrict__ lse,
                                                                     int32_t *__restrict__ hit) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    __shared__ CeAcc wave_acc[VQ_CE_WAVES];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const raw *p = reinterpret_cast<const raw *>(a.logits) + r * a.row_stride + a.start;
    const int V = a.V, npiece = V / W;
    CeAcc c;
    c.m = -__builtin_inff(); c.s = 0.0f; c.sa = 0.0f; c.bi = 0x7fffffff;
#pragma unroll 2
    for (int q = tid; q < npiece; q += VQ_CE_THREADS) {
        raw v[W];
        __builtin_memcpy(v, p + (int64_t)q * W, 16);                            // one 16-byte load, element alignment
        float x[W];
#pragma unroll
        for (int e = 0; e < W; ++e) x[e] = E::f32(v[e]);
        ce_piece<W>(c, x, q * W);
    }
    if (tid < V - npiece * W) {                                                 // V % W < W <= T single elements
        const int i = npiece * W + tid;
        const float x[1] = {E::f32(p[i])};
        ce_piece<1>(c, x, i);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        CeAcc b;
        b.m = __shfl_xor(c.m, o, 64); b.s = __shfl_xor(c.s, o, 64); b.sa = __shfl_xor(c.sa, o, 64); b.bi = __shfl_xor(c.bi, o, 64);
        c = ce_merge(c, b);
    }
    if ((tid & 63) == 0) wave_acc[tid >> 6] = c;
    __syncthreads();
    if (tid != 0) return;
    c = ce_merge(ce_merge(wave_acc[0], wave_acc[1]), ce_merge(wave_acc[2], wave_acc[3]));
    const float nan = __uint_as_float(0x7FC00000u);
    const float l = (c.m == -__builtin_inff()) ? nan : c.m + logf(c.s);
    lse[r] = l;
    int j = 0;
    const int kind = ce_target<I64>(a, r, &j);
    float out = 0.0f;
    int h = 0;
    if (kind == VQ_CE_OUTSIDE) {
        out = nan;
    } else if (kind == VQ_CE_CLASS) {
        const float d1 = l - E::f32(p[j]);
        if (a.eps == 0.0f) {
            out = d1;
        } else {
            const float mean = c.sa / (float)V;
            const float d2 = l - mean;
            const float t1 = a.one_minus_eps * d1, t2 = a.eps * d2;
            out = t1 + t2;
        }
        h = (l == l && c.bi == j) ? 1 : 0;
    }
    loss[r] = out;
    if (hit) hit[r] = h;
}

// out[0] = sum w_r loss_r, out[1] = W = sum w_r, out[2] = (float)(sum hit_r), out[3] = out[0] / out[1]; ignored rows skipped
template <bool I64>
__global__ __launch_bounds__(VQ_CE_THREADS) void token_ce_reduce_kernel(VqCeArgs a, const float *__restrict__ loss,
                                                                        const int32_t *__restrict__ hit, float *__restrict__ out) {
    __shared__ float wl[VQ_CE_WAVES], ww[VQ_CE_WAVES];
    __shared__ long long wh[VQ_CE_WAVES];
    const int tid = threadIdx.x;
    float sl = 0.0f, sw = 0.0f;
    long long sh = 0;
    for (int64_t r = tid; r < a.R; r += VQ_CE_THREADS) {
        int j;
        if (ce_target<I64>(a, r, &j) == VQ_CE_IGNORED) continue;
        const float w = a.weight ? a.weight[r] : 1.0f;
        const float wl_r = w * loss[r];
        sl = sl + wl_r;
        sw = sw + w;
        if (hit) sh += hit[r];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        sl = sl + __shfl_xor(sl, o, 64);
        sw = sw + __shfl_xor(sw, o, 64);
        sh += __shfl_xor(sh, o, 64);
    }
    if ((tid & 63) == 0) { wl[tid >> 6] = sl; ww[tid >> 6] = sw; wh[tid >> 6] = sh; }
    __syncthreads();
    if (tid != 0) return;
    const float L = (wl[0] + wl[1]) + (wl[2] + wl[3]);
    const float Wt = (ww[0] + ww[1]) + (ww[2] + ww[3]);
    out[0] = L;
    out[1] = Wt;
    out[2] = (float)((wh[0] + wh[1]) + (wh[2] + wh[3]));
    out[3] = L / Wt;
}

template <int DT, bool I64>
__global__ __launch_bounds__(VQ_CE_THREADS) void token_ce_bwd_kernel(VqCeArgs a, const float *__restrict__ lse,
                                                                     const float *__restrict__ g, int g_per_row,
                                                                     const float *__restrict__ wsum, void *__restrict__ grad,
                                                                     int cols, int64_t row_stride_out) {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    constexpr int W = E::W;
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const raw *in = reinterpret_cast<const raw *>(a.logits) + r * a.row_stride;   // column 0 of the row; read inside the slice only
    raw *out = reinterpret_cast<raw *>(grad) + r * row_stride_out;
    int j = -1;
    const int kind = ce_target<I64>(a, r, &j);
    const bool live = kind != VQ_CE_IGNORED;
    float c = 0.0f, l = 0.0f;
    if (live) {
        const float w = a.weight ? a.weight[r] : 1.0f;
        c = g[g_per_row ? r : 0] * w;
        if (wsum) c = c / wsum[0];
        l = (kind == VQ_CE_OUTSIDE) ? __uint_as_float(0x7FC00000u) : lse[r];
    }
    const int lo = (int)a.start, hi = lo + a.V, t = (kind == VQ_CE_CLASS) ? lo + j : -1;
    auto value = [&](float x, int col) -> raw {
        const float pr = expf(x - l);
        const float d = pr - (col == t ? a.one_minus_eps : 0.0f);
        const float e = d - a.eps_over_v;
        return ce_round<DT>(c * e);
    };
    const int npiece = cols / W;
#pragma unroll 2
    for (int q = tid; q < npiece; q += VQ_CE_THREADS) {
        const int c0 = q * W;
        raw o[W];
        if (!live || c0 + W <= lo || c0 >= hi) {
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] = (raw)0;
        } else if (c0 >= lo && c0 + W <= hi) {
            raw v[W];
            __builtin_memcpy(v, in + c0, 16);
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] = value(E::f32(v[e]), c0 + e);
        } else {                                                                // a piece that straddles an end of the slice
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const int col = c0 + e;
                o[e] = (col >= lo && col < hi) ? value(E::f32(in[col]), col) : (raw)0;
            }
        }
        __builtin_memcpy(out + c0, o, 16);
    }
    if (tid < cols - npiece * W) {
        const int col = npiece * W + tid;
        out[col] = (live && col >= lo && col < hi) ? value(E::f32(in[col]), col) : (raw)0;
    }
}
