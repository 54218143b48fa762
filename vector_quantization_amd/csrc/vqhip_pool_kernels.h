// Pooled code features (the linear probe of vq/tasks/image_classification/models.py:101-109): tokens [B, HW] -> the mean over
// the positions of the decoded rows, [B, D], without the decoded rows ever existing in memory.
//
// Arithmetic contract (include/vqhip.h).  For image b, channel c, with v_p the decoded value of position p:
//   s_j = +0.0f;  for p = j, j + 8, j + 16, .. < HW (increasing):  s_j = s_j + v_p            (j = 0 .. 7)
//   out[b, c] = (((s_0 + s_1) + (s_2 + s_3)) + ((s_4 + s_5) + (s_6 + s_7))) / (float)HW       (a true division)
// The order depends on HW alone: not on B, D, the grid or the token dtype.  No float atomics in the forward.
//
// decode_pool_kernel: a GROUP of 8 * CW threads owns one (image, chunk of channels): thread t of the group is partial j = t / CW
// and column col = t % CW of the chunk (CW a power of two, <= 64; a column is 4 channels and one 16-byte load on the vector
// path, 1 channel on the scalar path).  D = 256 is CW = 64: a wave per partial, one 16-byte load per lane per 1 KiB row.  Small D
// packs the partials into one wave (D = 32: 8 lanes per row, 8 rows per wave-load; D = 8: 2 lanes per row) and several images
// into one workgroup, so no lane strides through memory.  Each thread keeps VQ_POOL_UNROLL independent row loads in flight in
// front of the dependent adds, with the next batch's tokens already requested.  The eight partials of a column meet in LDS.
// ------------------------------------------------------------------------------------------------
#pragma once
#include "vqhip_fsq_kernels.h"      // VqFsqConsts, VQ_FSQ_MAX_C (owned by vqhip_fsq.hip, like this header)

#define VQ_POOL_PARTIALS 8
#define VQ_POOL_UNROLL 8
#define VQ_POOL_MAX_THREADS 512

template <bool I64>
__device__ __forceinline__ int64_t pool_token(const void *quant, int64_t n) {
    return I64 ? reinterpret_cast<const int64_t *>(quant)[n] : (int64_t)reinterpret_cast<const int32_t *>(quant)[n];
}

template <bool VEC> struct PoolCol;
template <> struct PoolCol<true> {
    typedef float4 T;
    static constexpr int W = 4;
    static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ T load(const float *p) { return *reinterpret_cast<const float4 *>(p); }
    static __device__ __forceinline__ void store(float *p, T v) { *reinterpret_cast<float4 *>(p) = v; }
    static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
    static __device__ __forceinline__ T div(T a, float h) { return make_float4(a.x / h, a.y / h, a.z / h, a.w / h); }
    static __device__ __forceinline__ T fill(float v) { return make_float4(v, v, v, v); }
};
template <> struct PoolCol<false> {
    typedef float T;
    static constexpr int W = 1;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T load(const float *p) { return *p; }
    static __device__ __forceinline__ void store(float *p, T v) { *p = v; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
    static __device__ __forceinline__ T div(T a, float h) { return a / h; }
    static __device__ __forceinline__ T fill(float v) { return v; }
};

// out [B, D] of tokens quant [B, HW] and the codebook e [K, D].  cw_log2: log2(CW); nchunks = ceil(D / (CW * W)); a block holds
// blockDim.x / (8 * CW) groups.  A token outside [0, K) is never dereferenced and makes every channel of its image NaN.
template <bool I64, bool VEC>
__global__ __launch_bounds__(VQ_POOL_MAX_THREADS) void decode_pool_kernel(const float *__restrict__ e, int64_t K, int D,
                                                                         const void *__restrict__ quant, int64_t B, int HW,
                                                                         int cw_log2, int nchunks, float *__restrict__ out) {
    typedef PoolCol<VEC> C;
    typedef typename C::T T;
    __shared__ T part[VQ_POOL_MAX_THREADS];
    __shared__ int bad_flag[VQ_POOL_MAX_THREADS];
    const int CW = 1 << cw_log2;
    const int tg_log2 = cw_log2 + 3;                                    // threads per group = 8 * CW
    const int t = threadIdx.x & ((1 << tg_log2) - 1);
    const int j = t >> cw_log2, col = t & (CW - 1);
    const int64_t group = (int64_t)blockIdx.x * (blockDim.x >> tg_log2) + (threadIdx.x >> tg_log2);
    const int64_t b = group / nchunks;
    const int chunk = (int)(group - b * nchunks);
    const int c0 = (chunk * CW + col) * C::W;                           // first channel of this thread's column
    const bool live = b < B && c0 < D;                                  // (D % 4 == 0 on the vector path: a live column is whole)
    T s = C::zero();
    int bad = 0;
    if (live) {
        const int64_t n0 = b * HW;
        const float *ec = e + c0;
        int64_t tok[VQ_POOL_UNROLL];
#pragma unroll
        for (int u = 0; u < VQ_POOL_UNROLL; ++u) {
            const int p = j + VQ_POOL_PARTIALS * u;
            tok[u] = p < HW ? pool_token<I64>(quant, n0 + p) : 0;
        }
        for (int p0 = j; p0 < HW; p0 += VQ_POOL_PARTIALS * VQ_POOL_UNROLL) {
            T v[VQ_POOL_UNROLL];
            bool ok[VQ_POOL_UNROLL];
#pragma unroll
            for (int u = 0; u < VQ_POOL_UNROLL; ++u) {                  // the batch's row loads, all in flight together
                const int p = p0 + VQ_POOL_PARTIALS * u;
                const bool in_range = tok[u] >= 0 && tok[u] < K;
                ok[u] = p < HW && in_range;
                bad |= (p < HW && !in_range) ? 1 : 0;
                v[u] = C::load(ec + (ok[u] ? tok[u] : 0) * D);          // (row 0 stands in where nothing is added: no branch)
            }
#pragma unroll
            for (int u = 0; u < VQ_POOL_UNROLL; ++u) {                  // the next batch's tokens, requested behind them
                const int p = p0 + VQ_POOL_PARTIALS * (VQ_POOL_UNROLL + u);
                tok[u] = p < HW ? pool_token<I64>(quant, n0 + p) : 0;
            }
#pragma unroll
            for (int u = 0; u < VQ_POOL_UNROLL; ++u) {                  // the dependent chain, in increasing p
                const T a = C::add(s, v[u]);
                if (ok[u]) s = a;
            }
        }
    }
    part[threadIdx.x] = s;
    bad_flag[threadIdx.x] = bad;
    __syncthreads();
    if (live && j == 0) {
        const int base = (int)threadIdx.x;                              // partial jj of this column sits jj * CW further on
        T p[VQ_POOL_PARTIALS];
        int any_bad = 0;
#pragma unroll
        for (int jj = 0; jj < VQ_POOL_PARTIALS; ++jj) {
            p[jj] = part[base + (jj << cw_log2)];
            any_bad |= bad_flag[base + (jj << cw_log2)];
        }
        const T sum = C::add(C::add(C::add(p[0], p[1]), C::add(p[2], p[3])), C::add(C::add(p[4], p[5]), C::add(p[6], p[7])));
        const T r = any_bad ? C::fill(__uint_as_float(0x7FC00000u)) : C::div(sum, (float)HW);
        C::store(out + b * D + c0, r);
    }
}

// grad_e[quant[b, p], c] += g[b, c] / (float)HW with float atomics (as vq_backward_kernel's grad_w); tokens outside [0, K) are
// skipped.  LP = 1 << lp_log2 lanes sweep a token's row (64 / LP tokens per wave): an atomic wave-instruction adds 256
// contiguous bytes at D >= 64, whole rows side by side below.
template <bool I64>
__global__ __launch_bounds__(256) void decode_pool_bwd_kernel(const float *__restrict__ g, const void *__restrict__ quant,
                                                              int64_t N, int HW, int64_t K, int D, int lp_log2,
                                                              float *__restrict__ grad_e) {
    const int LP = 1 << lp_log2;
    const int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> lp_log2;
    const int lane = threadIdx.x & (LP - 1);
    if (n >= N) return;
    const int64_t k = pool_token<I64>(quant, n);
    if (k < 0 || k >= K) return;
    const int64_t b = n / HW;
    const float h = (float)HW;
    for (int d = lane; d < D; d += LP) atomicAdd(&grad_e[k * D + d], g[b * D + d] / h);
}

// FiniteScalarQuantizer: v_p of channel c is fsq_decode_kernel's value of the token, bit for bit (floor division, non-negative
// remainder, digit / h - 1 with fsq_div_h).  Lanes run along positions: the 8 lanes of an (image, channel) are the 8 partials,
// 8 (image, channel) pairs per wave; the partials meet by xor-shuffles (lane 0 of the eight ends with the contract's tree).
template <bool I64>
__global__ __launch_bounds__(256) void fsq_decode_pool_kernel(VqFsqConsts q, const void *__restrict__ quant, int64_t B, int HW,
                                                              float *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int)(gid & (VQ_POOL_PARTIALS - 1));
    const int64_t bc = gid >> 3;
    const int C = q.C;
    const bool live = bc < B * C;
    const int64_t b = live ? bc / C : 0;
    const int c = live ? (int)(bc - b * C) : 0;
    int cum = 1, level = 1;
    float half = 1.f, rhalf = 0.f;
#pragma unroll
    for (int i = 0; i < VQ_FSQ_MAX_C; ++i) {                            // the channel's constants by selects: no runtime-indexed array
        if (i == c) { cum = q.cum[i]; level = q.level[i]; half = q.half[i]; rhalf = q.rhalf[i]; }
    }
    float s = 0.f;
    if (live) {
        const int64_t n0 = b * HW;
        for (int p = j; p < HW; p += VQ_POOL_PARTIALS) {
            const int64_t token = pool_token<I64>(quant, n0 + p);
            int digit;
            if (token >= 0 && token < q.K) {
                digit = (int)(((uint32_t)token / (uint32_t)cum) % (uint32_t)level);
            } else {
                const int64_t cc = cum;
                int64_t f = token / cc;
                if (token % cc != 0 && token < 0) f -= 1;
                int64_t m = f % level;
                if (m < 0) m += level;
                digit = (int)m;
            }
            const float v = (rhalf != 0.f ? (float)digit * rhalf : (float)digit / half) - 1.0f;
            s = s + v;
        }
    }
    s = s + __shfl_xor(s, 1, 64);                                       // lane 0 of the eight: s0 + s1
    s = s + __shfl_xor(s, 2, 64);                                       // (s0 + s1) + (s2 + s3)
    s = s + __shfl_xor(s, 4, 64);                                       // ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))
    if (live && j == 0) out[bc] = s / (float)HW;
}
