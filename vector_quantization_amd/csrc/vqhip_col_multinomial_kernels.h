// Fused MultinomialAnchor (vq/algorithms/cvqvae/anchors.py:88-104): one latent per code, drawn from softmax(+d) down the code's
// column of the distance matrix, on row blocks of that matrix — kernels of vqhip_col_multinomial_max / _mass / _pick / _resolve.
//
// Contract: include/vqhip.h (vqhip_col_multinomial_*), DESIGN.md §8.  The caller owns an [R, K] fp32 tile of distances
// (vqhip_distance of a row slice) and walks the row blocks in order; no [N, K] object exists.
//   max      running column maximum over the blocks walked so far; a column that met a NaN or a +inf holds a NaN from then on
//   mass     the block's column masses: sum over its rows of trunc(expf(d - m_k) 2^40) as 64-bit integers, one [K] row per block
//   pick     Z_k = the sum of the blocks' masses, T_k = min(floor(u_k Z_k), Z_k - 1), the block that holds the crossing and the
//            residual target inside it; col_idx[k] = -1 until a block resolves it (a bad column keeps the -1)
//   resolve  the columns whose crossing lies in this block walk it in row order to the first running sum beyond the residual
// Every sum of masses is an integer sum: exact, independent of the order and of the block size, so the result is a pure function
// of (d, u).  No float atomics, no atomics at all: the blocks are sequential on the stream and a column is owned by one lane.
// Access: one lane per column, rows in the loop — a wave instruction reads 256 contiguous bytes of a row of the tile.
// Every global index is a column below K (checked per lane), a row below R, or a block below the count the host validated.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"

#define VQ_CM_COLS 64                           // columns per workgroup of the max / mass kernels: one lane per column
#define VQ_CM_WAVES 4                           // their row groups: wave w takes rows w, w + 4, ..
#define VQ_CM_WALK 16                           // rows a resolving lane loads ahead of its running sum
#define VQ_CM_FRAC_BITS 40                      // a mass <= 1 is an integer <= 2^40; 2^20 of them sum below 2^61

typedef unsigned long long cm_u64;

// a column's maximum as the max pass leaves it: NaN = the column holds a NaN or a +inf.  (A distance is never -inf; a column of
// nothing else would have no mass and counts as bad as well.)
__device__ __forceinline__ bool cm_bad(float m) { return !(fabsf(m) < __builtin_inff()); }

// exp(d - m) as a fixed-point integer: fp32 subtraction, expf (<= 1 ulp), times 2^40 exactly, truncated
__device__ __forceinline__ cm_u64 cm_mass(float d, float m) {
    const float w = expf(d - m);
    return (cm_u64)((double)w * (double)(1ull << VQ_CM_FRAC_BITS));
}

// colmax[k] = max(colmax[k], max_r tile[r, k]) (init != 0: the first block, colmax is overwritten); NaN is sticky
__global__ __launch_bounds__(VQ_CM_COLS * VQ_CM_WAVES) void col_multinomial_max_kernel(const float *__restrict__ tile, int R, int64_t K,
                                                                                       float *__restrict__ colmax, int init) {
    __shared__ float sm[VQ_CM_WAVES][VQ_CM_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * VQ_CM_COLS + lane;
    float m = -__builtin_inff();
    bool bad = false;
    if (k < K) {
        const float *p = tile + k;
#pragma unroll 8
        for (int r = wave; r < R; r += VQ_CM_WAVES) {
            const float d = p[(int64_t)r * K];
            bad |= !(d < __builtin_inff());                                     // NaN or +inf
            m = fmaxf(m, d);
        }
    }
    sm[wave][lane] = bad ? __builtin_nanf("") : m;
    __syncthreads();
    if (wave == 0 && k < K) {
        float v = init ? -__builtin_inff() : colmax[k];
#pragma unroll
        for (int w = 0; w < VQ_CM_WAVES; ++w) {
            const float s = sm[w][lane];
            v = (v != v || s != s) ? __builtin_nanf("") : fmaxf(v, s);
        }
        colmax[k] = v;
    }
}

// mass[k] = sum_r trunc(expf(tile[r, k] - colmax[k]) 2^40) of this block's rows; 0 for a bad column
__global__ __launch_bounds__(VQ_CM_COLS * VQ_CM_WAVES) void col_multinomial_mass_kernel(const float *__restrict__ tile, int R, int64_t K,
                                                                                        const float *__restrict__ colmax,
                                                                                        cm_u64 *__restrict__ mass) {
    __shared__ cm_u64 sm[VQ_CM_WAVES][VQ_CM_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * VQ_CM_COLS + lane;
    cm_u64 s = 0;
    if (k < K) {
        const float m = colmax[k];
        if (!cm_bad(m)) {
            const float *p = tile + k;
#pragma unroll 8
            for (int r = wave; r < R; r += VQ_CM_WAVES) s += cm_mass(p[(int64_t)r * K], m);
        }
    }
    sm[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && k < K) mass[k] = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
}

// Z_k, T_k, the block of the crossing and the residual target inside it; col_idx[k] = -1 (a bad column keeps it)
__global__ __launch_bounds__(256) void col_multinomial_pick_kernel(const cm_u64 *__restrict__ mass, int blocks, int64_t K,
                                                                   const float *__restrict__ colmax, const float *__restrict__ u,
                                                                   int32_t *__restrict__ sel, cm_u64 *__restrict__ resid,
                                                                   int64_t *__restrict__ col_idx) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    col_idx[k] = -1;
    sel[k] = -1;
    resid[k] = 0;
    if (cm_bad(colmax[k])) return;
    cm_u64 z = 0;
    for (int b = 0; b < blocks; ++b) z += mass[(int64_t)b * K + k];
    if (z == 0) return;                                                          // (cannot happen: the maximal row has mass 2^40)
    float uk = u[k];
    if (!(uk >= 0.0f)) uk = 0.0f;
    cm_u64 t = (cm_u64)((double)uk * (double)z);
    if (t >= z) t = z - 1;
    cm_u64 c = 0;
    for (int b = 0; b < blocks; ++b) {
        const cm_u64 mb = mass[(int64_t)b * K + k];
        if (c + mb > t) {
            sel[k] = b;
            resid[k] = t - c;
            return;
        }
        c += mb;
    }
}

// the columns whose crossing lies in block `b` walk its rows in order: col_idx[k] = row0 + the first r whose running mass
// exceeds the residual target.  The masses are those of the mass pass, bit for bit (same tile bits, same maximum, same
// instructions), so the crossing exists.
__global__ __launch_bounds__(64) void col_multinomial_resolve_kernel(const float *__restrict__ tile, int R, int64_t K, int b, int64_t row0,
                                                                     const float *__restrict__ colmax, const int32_t *__restrict__ sel,
                                                                     const cm_u64 *__restrict__ resid, int64_t *__restrict__ col_idx) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= K || sel[k] != b) return;
    const float m = colmax[k];
    const cm_u64 target = resid[k];
    const float *p = tile + k;
    cm_u64 c = 0;
    for (int r0 = 0; r0 < R; r0 += VQ_CM_WALK) {
        float d[VQ_CM_WALK];
#pragma unroll
        for (int i = 0; i < VQ_CM_WALK; ++i) d[i] = (r0 + i < R) ? p[(int64_t)(r0 + i) * K] : -__builtin_inff();   // mass 0 past the block
#pragma unroll
        for (int i = 0; i < VQ_CM_WALK; ++i) {
            c += cm_mass(d[i], m);
            if (c > target) {
                col_idx[k] = row0 + r0 + i;
                return;
            }
        }
    }
}
