// The second stage of every column sum of the activation ops (bias gradients of StyleGAN2, dgamma / dbeta of the norms, dbias of
// the row ops): a first kernel leaves one fp32 partial per (slab, channel) in ws[slab C + c], sg2_reduce_kernel adds the slabs of
// a channel in a fixed order.  No atomics, no memset.
// One translation unit only (vqhip_act.hip, through the activation ops' kernel headers): sg2_reduce_kernel is not a template, so a
// second unit including this header would emit the kernel twice.  The launch sits beside its kernel, hence vqhip_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip_host.h"

#define VQ_SG2_THREADS 256
#define VQ_SG2_ROWS_SLAB 256                    // rows per workgroup of bias_act_bwd_rows_kernel (and of row_act_bwd_kernel)
#define VQ_SG2_RED 16                           // channels and slab groups per workgroup of sg2_reduce_kernel

// second stage: gbias[c] = sum_s ws[s C + c] in a fixed order
__global__ __launch_bounds__(VQ_SG2_THREADS) void sg2_reduce_kernel(const float *__restrict__ ws, int64_t S, int C, float *__restrict__ gbias) {
    __shared__ float red[VQ_SG2_RED][VQ_SG2_RED];
    const int cl = threadIdx.x % VQ_SG2_RED, sg = threadIdx.x / VQ_SG2_RED;
    const int c = (int)blockIdx.x * VQ_SG2_RED + cl;
    float acc = 0.0f;
    if (c < C) {
#pragma unroll 4
        for (int64_t s = sg; s < S; s += VQ_SG2_RED) acc = acc + ws[s * C + c];
    }
    red[sg][cl] = acc;
    __syncthreads();
#pragma unroll
    for (int stride = VQ_SG2_RED / 2; stride >= 1; stride >>= 1) {
        if (sg < stride) red[sg][cl] = red[sg][cl] + red[sg + stride][cl];
        __syncthreads();
    }
    if (sg == 0 && c < C) gbias[c] = red[0][cl];
}

static int launch_sg2_reduce(const float *ws, int64_t slabs, int C, float *gbias, hipStream_t s) {
    sg2_reduce_kernel<<<(unsigned)((C + VQ_SG2_RED - 1) / VQ_SG2_RED), VQ_SG2_THREADS, 0, s>>>(ws, slabs, C, gbias);
    VQ_CHECK_LAUNCH("sg2_reduce_kernel");
    return VQHIP_OK;
}
