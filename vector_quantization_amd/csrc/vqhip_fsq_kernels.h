// FiniteScalarQuantizer (vq/algorithms/fsq/quantizers.py:74-150): element-wise encode, decode and the backward of the
// encode, one launch each.  Per channel i with level L_i the host passes (vqhip_fsq_t, computed with the reference's own
// torch expressions) c_i = atanh(odd_i / M_i) and M_i = (L_i - 1) * (1 - eps), and derives the integers odd_i = (L_i - 1) % 2,
// h_i = L_i // 2 and cumprod_i = L_0 * .. * L_{i-1}.  Nothing of these is recomputed here.
//
//   t = (tanh(x + c) * M - odd) / 2;  r = rint(t);  zst = t + (r - t);  z = zst / h
//   quant = int32(sum_i (zst_i + h_i) * cumprod_i)        fp32 sum of exact integers (K <= 2^24); NaN -> INT32_MIN
//   decode: digit_i = floor(q / cumprod_i) mod L_i (non-negative);  z = digit / h - 1
//   dL/dx = (((g / h) / 2) * M) * (1 - y * y),  y = tanh(x + c)       (autograd's order), cast to x's dtype
//
// Two layouts.  ROWS: token-major [N, C].  A block's 256 tokens are one contiguous run of 256*C elements: it is moved between
// global memory and LDS with 16-byte vectors (4 fp32 / 8 bf16 per lane; 256*C*2 bytes is a multiple of 16, so every tile
// starts aligned when the tensor does), and each lane reads its own row from LDS — lanes never stride C elements through
// global memory.  MAP: the NCHW-contiguous map [B, C, HW] with N = B*HW; lane n reads x[b, i, p] (b = n / HW, p = n % HW),
// i.e. neighbouring lanes touch neighbouring words of one channel row.  Token-major by-products of the map form (x_rows,
// z rows) go out through the same LDS tile.  Owned by vqhip_fsq.hip.
// ------------------------------------------------------------------------------------------------
#pragma once
#include "vqhip_kernels.h"
#define VQ_FSQ_MAX_C 16
#define VQ_FSQ_TILE 256

struct VqFsqConsts {           // by value in the kernel arguments
    int C;
    int K;
    float shift[VQ_FSQ_MAX_C];  // c
    float scale[VQ_FSQ_MAX_C];  // M
    float odd[VQ_FSQ_MAX_C];
    float half[VQ_FSQ_MAX_C];   // h
    float rhalf[VQ_FSQ_MAX_C];  // 1 / h where h is a power of two (x / h == x * (1 / h) exactly there), else 0
    float cumf[VQ_FSQ_MAX_C];   // cumprod as fp32 (exact: <= 2^24)
    int level[VQ_FSQ_MAX_C];
    int cum[VQ_FSQ_MAX_C];
};

// x / h, a true division; a product with the exact reciprocal where h is a power of two (the same correctly rounded value,
// a tenth of the instructions)
__device__ __forceinline__ float fsq_div_h(float v, const VqFsqConsts &q, int i) {
    return q.rhalf[i] != 0.f ? v * q.rhalf[i] : v / q.half[i];
}

// vec flags of the launches: which global pointers are 16-byte aligned (else the tile moves element by element)
#define VQ_FSQ_VEC_X 1
#define VQ_FSQ_VEC_Z 2
#define VQ_FSQ_VEC_ROWS 4
#define VQ_FSQ_VEC_G 8

template <int DT> struct FsqElem;
template <> struct FsqElem<0> {
    typedef float S;
    static __device__ __forceinline__ float load(S v) { return v; }
    static __device__ __forceinline__ S store(float v) { return v; }
};
template <> struct FsqElem<1> {
    typedef uint16_t S;
    static __device__ __forceinline__ float load(S v) { return bf16_to_f32(v); }
    static __device__ __forceinline__ S store(float v) {          // round to nearest even; NaN -> the canonical 0x7FC0 (c10::BFloat16)
        uint32_t b = __float_as_uint(v);
        if (v != v) return (S)0x7FC0u;
        b += 0x7FFFu + ((b >> 16) & 1u);
        return (S)(b >> 16);
    }
};

// global -> LDS and LDS -> global copies of `elems` contiguous elements by the whole block
template <typename S>
__device__ __forceinline__ void fsq_tile_in(S *__restrict__ lds, const S *__restrict__ g, int elems, bool vec) {
    constexpr int V = 16 / sizeof(S);
    const int nv = vec ? elems / V : 0;
    for (int j = threadIdx.x; j < nv; j += VQ_FSQ_TILE) reinterpret_cast<uint4 *>(lds)[j] = reinterpret_cast<const uint4 *>(g)[j];
    for (int j = nv * V + threadIdx.x; j < elems; j += VQ_FSQ_TILE) lds[j] = g[j];
}

template <typename S>
__device__ __forceinline__ void fsq_tile_out(S *__restrict__ g, const S *__restrict__ lds, int elems, bool vec) {
    constexpr int V = 16 / sizeof(S);
    const int nv = vec ? elems / V : 0;
    for (int j = threadIdx.x; j < nv; j += VQ_FSQ_TILE) reinterpret_cast<uint4 *>(g)[j] = reinterpret_cast<const uint4 *>(lds)[j];
    for (int j = nv * V + threadIdx.x; j < elems; j += VQ_FSQ_TILE) g[j] = lds[j];
}

// element (token n, channel 0) of the map and the channel stride: n = b * HW + p  ->  b * C * HW + p, stride HW
__device__ __forceinline__ int64_t fsq_map_base(uint32_t n, uint32_t HW, int C) {
    const uint32_t b = n / HW;
    return (int64_t)b * C * HW + (n - b * HW);
}

// quant [N] int32 always; z (fp32, nullable) in x's layout, or token-major when z_rows; x_rows (x's dtype, nullable, MAP only)
// the token-major copy of x; hist (nullable) += the tokens in [0, K).
template <int DT, bool MAP>
__global__ __launch_bounds__(VQ_FSQ_TILE) void fsq_encode_kernel(VqFsqConsts q, const void *__restrict__ xv, int N, int HW,
                                                                 int32_t *__restrict__ quant, float *__restrict__ z, int z_rows,
                                                                 void *__restrict__ rows_v, int32_t *__restrict__ hist, int vec) {
    typedef FsqElem<DT> E;
    typedef typename E::S S;
    __shared__ float4 tile4[VQ_FSQ_TILE * VQ_FSQ_MAX_C / 4];
    float *tf = reinterpret_cast<float *>(tile4);
    S *ts = reinterpret_cast<S *>(tile4);
    const S *x = reinterpret_cast<const S *>(xv);
    const int C = q.C;
    const int n0 = blockIdx.x * VQ_FSQ_TILE;
    const int rows = min(VQ_FSQ_TILE, N - n0);
    const int n = n0 + threadIdx.x;
    const bool live = (int)threadIdx.x < rows;
    const int row = threadIdx.x * C;
    int64_t base = 0;
    float xf[VQ_FSQ_MAX_C];
    if (!MAP) {
        fsq_tile_in(ts, x + (int64_t)n0 * C, rows * C, vec & VQ_FSQ_VEC_X);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VQ_FSQ_MAX_C; ++i)
            if (i < C) xf[i] = live ? E::load(ts[row + i]) : 0.f;
        __syncthreads();                                        // the tile is reused for z below
    } else {
        if (live) base = fsq_map_base((uint32_t)n, (uint32_t)HW, C);
#pragma unroll
        for (int i = 0; i < VQ_FSQ_MAX_C; ++i) {
            if (i < C) {
                const S v = live ? x[base + (int64_t)i * HW] : S(0);
                xf[i] = E::load(v);
                if (rows_v) ts[row + i] = v;
            }
        }
        if (rows_v) {
            __syncthreads();
            fsq_tile_out(reinterpret_cast<S *>(rows_v) + (int64_t)n0 * C, ts, rows * C, vec & VQ_FSQ_VEC_ROWS);
            __syncthreads();
        }
    }
    float zo[VQ_FSQ_MAX_C];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VQ_FSQ_MAX_C; ++i) {
        if (i < C) {
            const float y = tanhf(xf[i] + q.shift[i]);
            const float t = (y * q.scale[i] - q.odd[i]) / 2.0f;
            const float r = rintf(t);                           // half to even, as torch.round
            const float zst = t + (r - t);                      // ste(r, t)
            zo[i] = fsq_div_h(zst, q, i);
            s = s + (zst + q.half[i]) * q.cumf[i];
        }
    }
    if (live) {
        const int32_t token = (s != s) ? INT32_MIN : (int32_t)s;     // the CPU's conversion of NaN
        quant[n] = token;
        if (hist && token >= 0 && token < q.K) atomicAdd(&hist[token], 1);
    }
    if (!z) return;
    if (!MAP || z_rows) {
#pragma unroll
        for (int i = 0; i < VQ_FSQ_MAX_C; ++i)
            if (i < C) tf[row + i] = zo[i];
        __syncthreads();
        fsq_tile_out(z + (int64_t)n0 * C, tf, rows * C, vec & VQ_FSQ_VEC_Z);
    } else if (live) {
#pragma unroll
        for (int i = 0; i < VQ_FSQ_MAX_C; ++i)
            if (i < C) z[base + (int64_t)i * HW] = zo[i];
    }
}

// grad_x (x's dtype and layout) from the upstream gradient g (fp32, x's layout); y is recomputed from x
template <int DT, bool MAP>
__global__ __launch_bounds__(VQ_FSQ_TILE) void fsq_backward_kernel(VqFsqConsts q, const void *__restrict__ xv,
                                                                   const float *__restrict__ g, int N, int HW,
                                                                   void *__restrict__ gx_v, int vec) {
    typedef FsqElem<DT> E;
    typedef typename E::S S;
    __shared__ float4 tile4[VQ_FSQ_TILE * VQ_FSQ_MAX_C / 4];
    __shared__ float4 gtile4[MAP ? 1 : VQ_FSQ_TILE * VQ_FSQ_MAX_C / 4];
    S *ts = reinterpret_cast<S *>(tile4);
    float *gt = reinterpret_cast<float *>(gtile4);
    const S *x = reinterpret_cast<const S *>(xv);
    S *gx = reinterpret_cast<S *>(gx_v);
    const int C = q.C;
    const int n0 = blockIdx.x * VQ_FSQ_TILE;
    const int rows = min(VQ_FSQ_TILE, N - n0);
    const int n = n0 + threadIdx.x;
    const bool live = (int)threadIdx.x < rows;
    const int row = threadIdx.x * C;
    int64_t base = 0;
    float xf[VQ_FSQ_MAX_C], gf[VQ_FSQ_MAX_C];
    if (!MAP) {
        fsq_tile_in(ts, x + (int64_t)n0 * C, rows * C, vec & VQ_FSQ_VEC_X);
        fsq_tile_in(gt, g + (int64_t)n0 * C, rows * C, vec & VQ_FSQ_VEC_G);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VQ_FSQ_MAX_C; ++i) {
            if (i < C) {
                xf[i] = live ? E::load(ts[row + i]) : 0.f;
                gf[i] = live ? gt[row + i] : 0.f;
            }
        }
        __syncthreads();                                        // the x tile is reused for grad_x below
    } else {
        if (live) base = fsq_map_base((uint32_t)n, (uint32_t)HW, C);
#pragma unroll
        for (int i = 0; i < VQ_FSQ_MAX_C; ++i) {
            if (i < C) {
                xf[i] = live ? E::load(x[base + (int64_t)i * HW]) : 0.f;
                gf[i] = live ? g[base + (int64_t)i * HW] : 0.f;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < VQ_FSQ_MAX_C; ++i) {
        if (i < C) {
            const float y = tanhf(xf[i] + q.shift[i]);
            float d = fsq_div_h(gf[i], q, i);                   // z = zst / h
            d = d / 2.0f;                                       // t = (...) / 2
            d = d * q.scale[i];                                 // tanh(.) * M - odd
            d = d * (1.0f - y * y);                             // tanh_backward
            if (!MAP) ts[row + i] = E::store(d);
            else if (live) gx[base + (int64_t)i * HW] = E::store(d);
        }
    }
    if (!MAP) {
        __syncthreads();
        fsq_tile_out(gx + (int64_t)n0 * C, ts, rows * C, vec & VQ_FSQ_VEC_Z);
    }
}

// z (fp32, ROWS [N, C] or the MAP) of int32 / int64 tokens: the reference's from_decimal for any token, negative and >= K ones
// included (floor division, non-negative remainder)
template <bool I64, bool MAP>
__global__ __launch_bounds__(VQ_FSQ_TILE) void fsq_decode_kernel(VqFsqConsts q, const void *__restrict__ quant_v, int N, int HW,
                                                                 float *__restrict__ z, int vec) {
    __shared__ float4 tile4[MAP ? 1 : VQ_FSQ_TILE * VQ_FSQ_MAX_C / 4];
    float *tf = reinterpret_cast<float *>(tile4);
    const int C = q.C;
    const int n0 = blockIdx.x * VQ_FSQ_TILE;
    const int rows = min(VQ_FSQ_TILE, N - n0);
    const int n = n0 + threadIdx.x;
    const bool live = (int)threadIdx.x < rows;
    const int row = threadIdx.x * C;
    int64_t token = 0;
    int64_t base = 0;
    if (live) {
        token = I64 ? reinterpret_cast<const int64_t *>(quant_v)[n] : (int64_t)reinterpret_cast<const int32_t *>(quant_v)[n];
        if (MAP) base = fsq_map_base((uint32_t)n, (uint32_t)HW, C);
    }
    const bool in_range = token >= 0 && token < q.K;
#pragma unroll
    for (int i = 0; i < VQ_FSQ_MAX_C; ++i) {
        if (i < C) {
            int digit;
            if (in_range) {
                digit = (int)(((uint32_t)token / (uint32_t)q.cum[i]) % (uint32_t)q.level[i]);
            } else {
                const int64_t c = q.cum[i];
                int64_t f = token / c;
                if (token % c != 0 && token < 0) f -= 1;
                int64_t m = f % q.level[i];
                if (m < 0) m += q.level[i];
                digit = (int)m;
            }
            const float v = fsq_div_h((float)digit, q, i) - 1.0f;
            if (!MAP) tf[row + i] = v;
            else if (live) z[base + (int64_t)i * HW] = v;
        }
    }
    if (!MAP) {
        __syncthreads();
        fsq_tile_out(z + (int64_t)n0 * C, tf, rows * C, vec & VQ_FSQ_VEC_Z);
    }
}
