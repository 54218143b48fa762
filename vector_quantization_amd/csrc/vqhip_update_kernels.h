// libvqhip device kernels, unit 6: scatter-add, row gather, VQ-KD and CVQ-VAE updates.  Owned by vqhip_update.hip.
#pragma once
#include "vqhip_kernels.h"
// wave per source row; lanes sweep the row so each atomic wave-instruction adds 256 contiguous bytes
__global__ void scatter_add_rows_kernel(const float *src, const int64_t *idx, int64_t N, int64_t K, int D, float *dst) {
    int64_t n = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (n >= N) return;
    int64_t k = idx[n];
    if (k < 0 || k >= K) return;
    for (int d = lane; d < D; d += 64) atomicAdd(&dst[k * D + d], src[n * D + d]);
}

template <int DT>
__global__ void gather_rows_kernel(const void *x, const int64_t *row_idx, int64_t K, int D, float *out) {
    int64_t k = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (k >= K) return;
    int64_t n = row_idx[k];
    for (int d = lane; d < D; d += 64) out[k * D + d] = load_elem<DT>(x, n * D + d);
}

// VQ-KD codebook update, wave per code (callbacks.py:66-70,126-128,73-75)
__global__ void vqkd_update_kernel(float *w, const int64_t *hist, const float *sums, int64_t K, int D, float decay,
                                   int centroid_only) {
    int64_t k = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (k >= K) return;
    int64_t occ = hist[k];
    float cnt = (float)(occ > 0 ? occ : 1);
    if (centroid_only) {   // VQKDCallback._kmeans alone (callbacks.py:66-70): where(occurred, sums/count, w)
        if (occ > 0)
            for (int d = lane; d < D; d += 64) w[k * D + d] = sums[k * D + d] / cnt;
        return;
    }
    // c = where(occurred, sums / max(count,1), w); then normalize
    float p = 0.0f;
    for (int d = lane; d < D; d += 64) {
        float c = (occ > 0) ? sums[k * D + d] / cnt : w[k * D + d];
        p = fmaf(c, c, p);
    }
    p = wave_sum_tree(p);
    float nrm = sqrtf(p), den = (nrm < 1e-12f) ? 1e-12f : nrm;
    float om = 1.0f - decay;
    float q = 0.0f;
    for (int d = lane; d < D; d += 64) {
        float c = (occ > 0) ? sums[k * D + d] / cnt : w[k * D + d];
        c = c / den;
        float v = w[k * D + d] * decay + c * om;       // todd.utils.ema
        q = fmaf(v, v, q);
    }
    q = wave_sum_tree(q);
    float nrm2 = sqrtf(q), den2 = (nrm2 < 1e-12f) ? 1e-12f : nrm2;
    for (int d = lane; d < D; d += 64) {
        float c = (occ > 0) ? sums[k * D + d] / cnt : w[k * D + d];
        c = c / den;
        float v = w[k * D + d] * decay + c * om;
        w[k * D + d] = v / den2;
    }
}

// CVQ-VAE update, wave per code (quantizer_callback.py:94-102)
__device__ __forceinline__ float cvq_decay_of(float pk, int64_t K, float ema_decay, float eps) {
    return 1.0f - expf(-pk * (float)K * 10.0f / (1.0f - ema_decay) - eps);
}

__global__ void cvq_update_kernel(float *w, float *p, const int64_t *hist, int64_t numel, const int64_t *numel_dev,
                                  const float *anchors, int64_t K, int D, float ema_decay, float eps, int stage) {
    int64_t k = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (k >= K) return;
    // stage bit 0: p = ema(p, hist/numel); stage bit 1: w = ema(w, anchors, decay(p))
    float pk = p[k];
    if (stage & 1) {
        if (numel_dev) numel = *numel_dev;      // all-reduced token count left on the device (no host sync)
        float freq = (float)hist[k] / (float)numel;
        pk = pk * ema_decay + freq * (1.0f - ema_decay);
    }
    if (stage & 2) {
        float decay = cvq_decay_of(pk, K, ema_decay, eps);
        float om = 1.0f - decay;
        for (int d = lane; d < D; d += 64) w[k * D + d] = w[k * D + d] * decay + anchors[k * D + d] * om;
    }
    if (lane == 0 && (stage & 1)) p[k] = pk;
}

// The whole one-rank CVQ-VAE update in one launch, wave per code: probability EMA from the int32 epilogue histogram,
// decay, NearestAnchor's row gather x[col_idx[k]] and the blend — the same expressions, in the same order, as stage 1,
// vqhip_gather_rows and stage 2 above (bit-identical results); w_out may alias w_in and p_out may alias p_in.
template <int DT>
__global__ void cvq_step_kernel(const float *w_in, float *w_out, const float *p_in, float *p_out, const int32_t *hist,
                                int64_t numel, const void *x, const int64_t *col_idx, int64_t K, int D, float ema_decay,
                                float eps) {
    const int64_t k = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= K) return;
    const float freq = (float)hist[k] / (float)numel;
    const float pk = p_in[k] * ema_decay + freq * (1.0f - ema_decay);
    const float decay = cvq_decay_of(pk, K, ema_decay, eps), om = 1.0f - decay;
    const int64_t row = col_idx[k];
    for (int d = lane; d < D; d += 64) w_out[k * D + d] = w_in[k * D + d] * decay + load_elem<DT>(x, row * D + d) * om;
    if (lane == 0) p_out[k] = pk;
}

// decay_k of every code (the same expression, bit for bit): decay_k == 1.0f means the code's anchor is multiplied by 0
__global__ void cvq_decay_kernel(const float *p, int64_t K, float ema_decay, float eps, float *decay) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) decay[k] = cvq_decay_of(p[k], K, ema_decay, eps);
}

// the w update restricted to the listed codes: w[rows[i]] = w[rows[i]]*decay + anchors_sub[i]*(1-decay)
__global__ void cvq_update_rows_kernel(float *w, const float *p, const int64_t *rows, const float *anchors_sub, int64_t M,
                                       int64_t K, int D, float ema_decay, float eps) {
    int64_t i = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (i >= M) return;
    const int64_t k = rows[i];
    if (k < 0 || k >= K) return;
    const float decay = cvq_decay_of(p[k], K, ema_decay, eps), om = 1.0f - decay;
    for (int d = lane; d < D; d += 64) w[k * D + d] = w[k * D + d] * decay + anchors_sub[i * D + d] * om;
}
