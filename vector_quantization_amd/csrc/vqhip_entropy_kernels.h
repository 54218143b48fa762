// EntropyLoss on a row block of the distance matrix (vq/algorithms/vq/losses.py:130-153) — kernels of vqhip_entropy_rows,
// vqhip_entropy_finish and vqhip_entropy_grad.  The caller owns an [R, K] fp32 tile of distances (vqhip_distance on a row
// slice) that is small enough to stay cache-resident between its producer and the sweeps here; no [N, K] object exists.
//
//   a = d / T,  p = softmax(a),  H_n = lse_n - sum_k p_nk a_nk,  q_k = (1/N) sum_n p_nk,
//   L = (1/N) sum_n H_n + sum_k q_k log(q_k + 1e-5),  c_k = log(q_k + 1e-5) + q_k / (q_k + 1e-5),
//   dL/da_nj = (p_nj / N) (c_j - a_nj - S_n),  S_n = sum_k p_nk c_k - sum_k p_nk a_nk.
//
// Every sum over more than a handful of terms is accumulated in double and reduced in a fixed order (no atomics): the loss
// and both gradients are bit-reproducible run to run, and the fp32 roundings that remain are per element (tests/entropy_ref.py
// counts them from this file).  A row is owned by one wave (64 lanes, 16-byte loads where K % 4 == 0, xor-shuffle tree);
// column sums are taken per chunk of VQ_ENT_CHUNK rows into double partials which one more kernel adds up chunk by chunk.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define VQ_ENT_CHUNK 32        // rows per column-partial chunk
#define VQ_ENT_COLS 1024       // columns per workgroup of the column kernel (256 threads x 4)
#define VQ_ENT_EPS 1e-5        // the reference's epsilon inside log(q + eps)

__device__ __forceinline__ double ent_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float ent_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// the lane's elements of a row, four at a time: f(k, d_k) for every k < K this lane owns (the same k in every sweep)
template <bool VEC, typename F>
__device__ __forceinline__ void ent_row_sweep(const float *row, int K, int lane, F f) {
    if (VEC) {
        for (int k = lane * 4; k < K; k += 256) {
            const float4 v = *(const float4 *)(row + k);
            f(k, v.x); f(k + 1, v.y); f(k + 2, v.z); f(k + 3, v.w);
        }
    } else {
        for (int k = lane; k < K; k += 64) f(k, row[k]);
    }
}

// lse[r] = log sum_k exp(a_rk), spa[r] = sum_k p_rk a_rk: one wave per row, max first, then both sums in double
template <bool VEC>
__global__ __launch_bounds__(256) void entropy_rows_kernel(const float *__restrict__ tile, int R, int K, float T,
                                                           float *__restrict__ lse, float *__restrict__ spa) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
        const float *row = tile + (int64_t)r * K;
        float m = -INFINITY;
        ent_row_sweep<VEC>(row, K, lane, [&](int, float d) { m = fmaxf(m, d / T); });
        m = ent_wave_max(m);
        double s = 0.0, sa = 0.0;
        ent_row_sweep<VEC>(row, K, lane, [&](int, float d) {
            const float a = d / T;
            const float w = expf(a - m);
            s += (double)w;
            sa += (double)w * (double)a;
        });
        s = ent_wave_sum(s);
        sa = ent_wave_sum(sa);
        if (lane == 0) {
            lse[r] = (float)((double)m + log(s));
            spa[r] = (float)(sa / s);
        }
    }
}

// Column sums of one chunk of rows, four columns per thread, in double, rows in ascending order.
// MODE 0: of p_rk = exp(d_rk / T - lse_r);  MODE 1: of the tile's own values (G after entropy_grad_kernel).
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void entropy_colsum_kernel(const float *__restrict__ tile, int R, int K, float T,
                                                             const float *__restrict__ lse, double *__restrict__ partial) {
    const int k0 = blockIdx.x * VQ_ENT_COLS + threadIdx.x * 4;
    if (k0 >= K) return;
    const int nchunks = (R + VQ_ENT_CHUNK - 1) / VQ_ENT_CHUNK;
    for (int c = blockIdx.y; c < nchunks; c += gridDim.y) {
        const int r0 = c * VQ_ENT_CHUNK, r1 = (r0 + VQ_ENT_CHUNK < R) ? r0 + VQ_ENT_CHUNK : R;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = r0; r < r1; ++r) {
            const float *p = tile + (int64_t)r * K + k0;
            float v[4];
            if (VEC) {
                const float4 t = *(const float4 *)p;
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (k0 + i < K) ? p[i] : 0.0f;
            }
            const float l = MODE == 0 ? lse[r] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] += (double)(MODE == 0 ? expf(v[i] / T - l) : v[i]);
        }
        double *out = partial + (int64_t)c * K + k0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (k0 + i < K) out[i] = acc[i];
    }
}

// acc[k] (+)= the chunk partials of column k, chunk by chunk
__global__ __launch_bounds__(256) void entropy_colreduce_kernel(const double *__restrict__ partial, int nchunks, int K,
                                                                double *__restrict__ acc, int init) {
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
        double s = init ? 0.0 : acc[k];
        for (int c = 0; c < nchunks; ++c) s += partial[(int64_t)c * K + k];
        acc[k] = s;
    }
}

__device__ __forceinline__ double ent_block_sum(double v, double *sh) {
    v = ent_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One workgroup: q = qacc / N, c = log(q + eps) + q / (q + eps), loss = mean_n (lse_n - spa_n) + sum_k q_k log(q_k + eps).
__global__ __launch_bounds__(256) void entropy_finish_kernel(const float *__restrict__ lse, const float *__restrict__ spa,
                                                             const double *__restrict__ qacc, int N, int K,
                                                             float *__restrict__ q, float *__restrict__ c, float *__restrict__ loss) {
    __shared__ double sh[4];
    double h = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) h += (double)lse[n] - (double)spa[n];
    h = ent_block_sum(h, sh);
    double ql = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const double qk = qacc[k] / (double)N;
        const double lg = log(qk + VQ_ENT_EPS);
        ql += qk * lg;
        q[k] = (float)qk;
        c[k] = (float)(lg + qk / (qk + VQ_ENT_EPS));
    }
    ql = ent_block_sum(ql, sh);
    if (threadIdx.x == 0) loss[0] = (float)(h / (double)N + ql);
}

// One wave per row: S_r = sum_k p_rk c_k - spa_r, then the tile is overwritten with g_rk = p_rk * scale * (c_k - a_rk - S_r)
// (Cosine) or G_rk = g_rk / d_rk, 0 where d_rk == 0 (L2); rowsum[r] = sum_k of what was written.
// scale = inv_nt * upstream = (dL_total / dL) / (N T).
template <bool VEC, bool L2>
__global__ __launch_bounds__(256) void entropy_grad_kernel(float *__restrict__ tile, int R, int K, float T,
                                                           const float *__restrict__ lse, const float *__restrict__ spa,
                                                           const float *__restrict__ c, float inv_nt,
                                                           const float *__restrict__ upstream, float *__restrict__ rowsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float scale = upstream ? inv_nt * upstream[0] : inv_nt;
    for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
        float *row = tile + (int64_t)r * K;
        const float l = lse[r];
        double pc = 0.0;
        ent_row_sweep<VEC>(row, K, lane, [&](int k, float d) { pc += (double)expf(d / T - l) * (double)c[k]; });
        pc = ent_wave_sum(pc);
        const float S = (float)(pc - (double)spa[r]);
        double rs = 0.0;
        auto one = [&](int k, float d) -> float {
            const float a = d / T;
            const float p = expf(a - l);
            const float t = (c[k] - a) - S;
            float g = (p * scale) * t;
            if (L2) g = d > 0.0f ? g / d : 0.0f;
            rs += (double)g;
            return g;
        };
        if (VEC) {
            for (int k = lane * 4; k < K; k += 256) {
                const float4 v = *(const float4 *)(row + k);
                float4 o;
                o.x = one(k, v.x); o.y = one(k + 1, v.y); o.z = one(k + 2, v.z); o.w = one(k + 3, v.w);
                *(float4 *)(row + k) = o;
            }
        } else {
            for (int k = lane; k < K; k += 64) row[k] = one(k, row[k]);
        }
        rs = ent_wave_sum(rs);
        if (lane == 0) rowsum[r] = (float)rs;
    }
}
