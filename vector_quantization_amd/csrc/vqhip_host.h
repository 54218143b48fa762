// libvqhip — the host-side helpers every translation unit uses: how an entry point refuses (the text vqhip_last_error returns),
// checks a launch, sizes a grid and turns a dtype into a template argument.  fail and ensure_dyn_lds are defined once, in
// vqhip_common.hip; they cross translation units inside the library only (hidden visibility: the library exports its C ABI alone).
#pragma once
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <type_traits>

#define VQ_HIDDEN __attribute__((visibility("hidden")))

// records "what[: detail]" as the calling host thread's last error and returns `code`
VQ_HIDDEN int fail(int code, const char *what, const char *detail = "");

#define VQ_CHECK_LAUNCH(name)                                            \
    do {                                                                 \
        hipError_t err__ = hipGetLastError();                            \
        if (err__ != hipSuccess) return fail(VQHIP_ELAUNCH, name, hipGetErrorString(err__)); \
    } while (0)

#define VQ_HIP(call)                                                     \
    do {                                                                 \
        hipError_t err__ = (call);                                       \
        if (err__ != hipSuccess) return fail(VQHIP_ELAUNCH, #call, hipGetErrorString(err__)); \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember what was set for (kernel, device).
// Devices beyond the cache simply set the attribute on every call.
#define VQ_MAX_DEVICES 64
typedef std::atomic<size_t> LdsCache[VQ_MAX_DEVICES];
VQ_HIDDEN int ensure_dyn_lds(const void *kern, size_t bytes, LdsCache &set);

// caller-owned buffers carry their size: an undersized workspace or image is refused here instead of becoming silent
// device-memory corruption inside a kernel
#define VQ_NEED(what, have, need)                                                                         \
    do {                                                                                                  \
        const int64_t need__ = (need);                                                                    \
        if ((have) < need__) {                                                                            \
            char msg__[160];                                                                              \
            snprintf(msg__, sizeof(msg__), "%lld bytes given, %lld needed", (long long)(have), (long long)need__); \
            return fail(VQHIP_EINVAL, what, msg__);                                                       \
        }                                                                                                 \
    } while (0)

// a refusal with a fixed text ("entry point: what"), and what most entry points refuse
#define VQ_REQUIRE(cond, text) do { if (!(cond)) return fail(VQHIP_EINVAL, text); } while (0)
static inline bool vq_public_metric(int m) { return m == VQHIP_METRIC_L2 || m == VQHIP_METRIC_COS || m == VQHIP_METRIC_COS_BF16; }
static inline bool vq_row_dtype(int t) { return t == VQHIP_DTYPE_F32 || t == VQHIP_DTYPE_BF16; }
static inline bool vq_float_dtype(int t) { return vq_row_dtype(t) || t == VQHIP_DTYPE_F16; }       // what the activation ops read
static inline bool vq_dense_layout(int l) { return l == VQHIP_LAYOUT_ROWS || l == VQHIP_LAYOUT_MAP; }
static inline bool vq_fits_i31(int64_t N, int64_t K) { return N < (1ll << 31) && K < (1ll << 31); }

static inline int waves_grid(int64_t rows, int waves_per_block) {
    return (int)((rows + waves_per_block - 1) / waves_per_block);
}

// A float dtype that vq_float_dtype has let through, as a template argument: `fn` is a generic lambda, `decltype(its parameter)
// ::value` the constant.  Two dtypes nest two calls.  Anything but F32 and BF16 goes to F16.
template <class Fn>
static int vq_with_dtype(int dtype, Fn &&fn) {
    switch (dtype) {
    case VQHIP_DTYPE_F32: return fn(std::integral_constant<int, VQHIP_DTYPE_F32>{});
    case VQHIP_DTYPE_BF16: return fn(std::integral_constant<int, VQHIP_DTYPE_BF16>{});
    default: return fn(std::integral_constant<int, VQHIP_DTYPE_F16>{});
    }
}
