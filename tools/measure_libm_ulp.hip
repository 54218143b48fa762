// The accuracy of the device library's erff, tanhf and expf, the one kind of constant the error bounds of the row ops of
// include/vqhip.h (VQHIP_VIT_ERF_ULPS, _TANH_ULPS, _EXP_ULPS) cannot derive: every fp32 value of a range against the float64
// function, the largest error in ulps of the exact result.  Ranges: erff [-6, 6] (beyond it the result is +-1 to the last
// bit), tanhf [-12, 12] (likewise), expf [-88, 0] (the arguments -t^2 / 2 of the GELU derivative).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/measure_libm_ulp.hip -o measure_libm_ulp && ./measure_libm_ulp
// Results: profiles/vqkd_autoencoder.txt.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define THREADS 256
#define BLOCKS 4096

// error of `got` in ulps of the exact value `want` (an ulp of a result below the normal range is 2^-149)
__device__ double ulps(float got, double want) {
    const double a = fabs(want);
    int e = a > 0.0 ? ilogb(a) : -126;
    if (e < -126) e = -126;
    return fabs((double)got - want) / ldexp(1.0, e - 23);
}

// bit patterns lo .. hi of the positive floats, both signs; one maximum per thread, no atomics
template <int FN>
__global__ __launch_bounds__(THREADS) void measure(uint32_t lo, uint32_t hi, double *worst, float *where) {
    double w = 0.0;
    float at = 0.0f;
    const uint32_t tid = blockIdx.x * THREADS + threadIdx.x, step = BLOCKS * THREADS;
    for (uint64_t b = (uint64_t)lo + tid; b <= hi; b += step) {
        for (int sign = 0; sign < 2; ++sign) {
            if (FN == 2 && sign == 0) continue;                                 // expf: negative arguments only
            const uint32_t bits = (uint32_t)b | (sign ? 0x80000000u : 0u);
            float x;
            memcpy(&x, &bits, 4);
            const float got = FN == 0 ? erff(x) : FN == 1 ? tanhf(x) : expf(x);
            const double want = FN == 0 ? erf((double)x) : FN == 1 ? tanh((double)x) : exp((double)x);
            const double u = ulps(got, want);
            if (u > w) { w = u; at = x; }
        }
    }
    worst[tid] = w;
    where[tid] = at;
}

static uint32_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

template <int FN>
static int run(const char *name, float top, double *dw, float *da) {
    static double hw[BLOCKS * THREADS];
    static float ha[BLOCKS * THREADS];
    measure<FN><<<BLOCKS, THREADS>>>(0u, bits_of(top), dw, da);
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "%s: launch failed\n", name); return 1; }
    if (hipMemcpy(hw, dw, sizeof(hw), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (hipMemcpy(ha, da, sizeof(ha), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double w = 0.0;
    float at = 0.0f;
    for (int i = 0; i < BLOCKS * THREADS; ++i)
        if (hw[i] > w) { w = hw[i]; at = ha[i]; }
    printf("%s: every fp32 value of magnitude 0 .. %g (%u bit patterns per sign): max error %.4f ulp at x = %.9g\n", name, top,
           bits_of(top) + 1u, w, at);
    return 0;
}

int main() {
    double *dw;
    float *da;
    if (hipMalloc(&dw, BLOCKS * THREADS * sizeof(double)) != hipSuccess || hipMalloc(&da, BLOCKS * THREADS * sizeof(float)) != hipSuccess) {
        fprintf(stderr, "no device memory\n");
        return 1;
    }
    int rc = run<0>("erff", 6.0f, dw, da) || run<1>("tanhf", 12.0f, dw, da) || run<2>("expf", 88.0f, dw, da);
    hipFree(dw);
    hipFree(da);
    return rc;
}
