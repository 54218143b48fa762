// Element traits of the fused ops: how a value of a public dtype (fp32, bf16, fp16) is read as fp32 — exactly — and how an fp32
// result is rounded into it, nearest even.  Shared by the sampler, the token cross-entropy, the image and distillation losses and
// the activation ops: the one definition of what "the op's dtype" means on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"

template <int DT> struct SampleElem;
template <> struct SampleElem<VQHIP_DTYPE_F32> {
    typedef float raw;
    static constexpr int W = 4;
    static __device__ __forceinline__ float f32(raw v) { return v; }
};
template <> struct SampleElem<VQHIP_DTYPE_BF16> {
    typedef uint16_t raw;
    static constexpr int W = 8;
    static __device__ __forceinline__ float f32(raw v) { return __uint_as_float(((uint32_t)v) << 16); }
};
template <> struct SampleElem<VQHIP_DTYPE_F16> {
    typedef uint16_t raw;
    static constexpr int W = 8;
    static __device__ __forceinline__ float f32(raw v) {
        _Float16 h;
        __builtin_memcpy(&h, &v, 2);
        return (float)h;
    }
};

template <int DT> __device__ __forceinline__ typename SampleElem<DT>::raw ce_round(float v);
template <> __device__ __forceinline__ float ce_round<VQHIP_DTYPE_F32>(float v) { return v; }
template <> __device__ __forceinline__ uint16_t ce_round<VQHIP_DTYPE_BF16>(float v) {
    const uint32_t b = __float_as_uint(v);
    if (v != v) return (uint16_t)0x7FC0u;
    return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);                  // round to nearest even (inf stays inf)
}
template <> __device__ __forceinline__ uint16_t ce_round<VQHIP_DTYPE_F16>(float v) {
    const _Float16 h = (_Float16)v;                                             // v_cvt_f16_f32: round to nearest even
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}
