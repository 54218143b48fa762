// Fused reconstruction metrics of a validation pass: pred and image [B, C, H, W] -> per image L1, MSE, PSNR and SSIM, and the
// exact integer sums behind them.  Both images are read once (the 6-pixel halo of a tile comes from L2); nothing of the size of
// an image is written.
//
// Contract: include/vqhip.h (vqhip_image_metrics), DESIGN.md §8.  T = VQ_IM_T.
//
// image_metrics_tile_kernel, one workgroup of 256 threads per (image, channel, T x T tile of pixels):
//   stage    the (T + 6) x (T + 6) pixels at the tile's origin - the tile and the halo to its right and below - are decoded to
//            bytes (im_byte: the dataset's decode in the tensor's own dtype) into two LDS byte tiles, zeros beyond the image.
//            The pixels of the tile itself (each pixel of an image is in exactly one tile) add |p - q| and (p - q)^2.
//   rows     7-wide sums of p, q, p^2, q^2, p q along every staged row, for the T window origins of that row: one thread per
//            (row, 8 origins), 16 bytes of each tile read as two 8-byte loads.  Kept in LDS as {sx | sy << 16, sxx, syy, sxy}.
//   windows  the window whose top-left pixel is (y, x) of the tile is the sum of rows y .. y + 6 of the above; a thread owns
//            column x and 4 consecutive y (10 row entries for 4 windows).  A window counts when it lies inside the image
//            (y + 6 < H, x + 6 < W).  S is evaluated in double from the integer sums and llrint(S 2^40) is added to an int64.
//   partial  the four int64 of a workgroup - abs, sq, fixed-point SSIM, NaN seen - are added over the lanes by xor shuffles and
//            over the four waves through LDS, and stored to slot blockIdx.x of the workspace.  Every slot is written by
//            every launch, so the workspace needs no memset.
// image_metrics_finish_kernel, ONE workgroup (a second launch behind the first on the same stream): wave w takes the images
//   w, w + 4, ..; its lanes add the image's slots, a shuffle tree adds the lanes, lane 0 divides.  Integer additions: the order
//   cannot matter, so the result is no function of T, of the grid or of the layout.
// No atomics of any kind.  Every global load is guarded by y < H and x < W; a workgroup writes its own slot only.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_elem.h"                         // SampleElem (exact conversion to fp32), ce_round (nearest even into bf16 / fp16)

#define VQ_IM_T VQHIP_IMAGE_METRICS_TILE
#define VQ_IM_HALO 6
#define VQ_IM_ROWS (VQ_IM_T + VQ_IM_HALO)
#define VQ_IM_STRIDE (VQ_IM_T + 8)              // bytes per staged row: the 16 bytes read for origins 8 s .. 8 s + 7 end inside it
#define VQ_IM_THREADS 256
#define VQ_IM_WAVES (VQ_IM_THREADS / 64)
#define VQ_IM_SLOT 4                            // int64 per workgroup: abs, sq, fixed-point SSIM, NaN seen

static_assert(VQ_IM_T == 32, "the thread maps below are written for T = 32 and 256 threads");

struct VqImSide {
    const void *p;
    int dtype;
    int64_t sb, sc, sy, sx;                     // element strides of [B, C, H, W]
};

struct VqImArgs {
    VqImSide a, b;                              // pred, image
    int C, H, W, tiles_x, tiles_y, want_ssim;
    double c1, c2;
};

// one element -> its byte, as `((v + 1) * 127.5).clamp(0, 255).to(uint8)` gives it in the tensor's dtype; a NaN sets *nan
__device__ __forceinline__ int im_byte(const VqImSide &s, int64_t off, int *nan) {
    float t;
    switch (s.dtype) {
    case VQHIP_DTYPE_U8:
        return reinterpret_cast<const uint8_t *>(s.p)[off];
    case VQHIP_DTYPE_F32: {
        const float t1 = reinterpret_cast<const float *>(s.p)[off] + 1.0f;
        t = t1 * 127.5f;
        break;
    }
    case VQHIP_DTYPE_BF16: {
        typedef SampleElem<VQHIP_DTYPE_BF16> E;
        const float t1 = E::f32(ce_round<VQHIP_DTYPE_BF16>(E::f32(reinterpret_cast<const uint16_t *>(s.p)[off]) + 1.0f));
        t = E::f32(ce_round<VQHIP_DTYPE_BF16>(t1 * 127.5f));
        break;
    }
    default: {
        typedef SampleElem<VQHIP_DTYPE_F16> E;
        const float t1 = E::f32(ce_round<VQHIP_DTYPE_F16>(E::f32(reinterpret_cast<const uint16_t *>(s.p)[off]) + 1.0f));
        t = E::f32(ce_round<VQHIP_DTYPE_F16>(t1 * 127.5f));
        break;
    }
    }
    if (t != t) {
        *nan = 1;
        return 0;
    }
    return (int)fminf(fmaxf(t, 0.0f), 255.0f);
}

__device__ __forceinline__ long long im_wave_sum(long long v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(VQ_IM_THREADS) void image_metrics_tile_kernel(VqImArgs g, long long *__restrict__ ws) {
    __shared__ __align__(16) uint8_t tp[VQ_IM_ROWS * VQ_IM_STRIDE], tq[VQ_IM_ROWS * VQ_IM_STRIDE];
    __shared__ uint4 hs[VQ_IM_ROWS * VQ_IM_T];
    __shared__ long long red[VQ_IM_WAVES][VQ_IM_SLOT];
    const int tid = threadIdx.x;
    unsigned int blk = blockIdx.x;
    const int tx = (int)(blk % (unsigned int)g.tiles_x);
    blk /= (unsigned int)g.tiles_x;
    const int ty = (int)(blk % (unsigned int)g.tiles_y);
    blk /= (unsigned int)g.tiles_y;
    const int c = (int)(blk % (unsigned int)g.C);
    const int64_t b = blk / (unsigned int)g.C;
    const int y0 = ty * VQ_IM_T, x0 = tx * VQ_IM_T;
    const int64_t base_a = b * g.a.sb + c * g.a.sc, base_b = b * g.b.sb + c * g.b.sc;

    int abs_acc = 0, sq_acc = 0, nan = 0;       // a tile holds 1024 pixels: both sums stay below 2^27
    for (int i = tid; i < VQ_IM_ROWS * VQ_IM_STRIDE; i += VQ_IM_THREADS) {
        const int ly = i / VQ_IM_STRIDE, lx = i - ly * VQ_IM_STRIDE;
        const int gy = y0 + ly, gx = x0 + lx;
        const bool own = ly < VQ_IM_T && lx < VQ_IM_T;
        int p = 0, q = 0;
        if (gy < g.H && gx < g.W && (own || (g.want_ssim && lx < VQ_IM_ROWS))) {
            p = im_byte(g.a, base_a + gy * g.a.sy + gx * g.a.sx, &nan);
            q = im_byte(g.b, base_b + gy * g.b.sy + gx * g.b.sx, &nan);
            if (own) {
                const int d = p - q;
                abs_acc += d < 0 ? -d : d;
                sq_acc += d * d;
            }
        }
        tp[i] = (uint8_t)p;
        tq[i] = (uint8_t)q;
    }
    long long fixed = 0;
    if (g.want_ssim) {
        __syncthreads();
        if (tid < VQ_IM_ROWS * (VQ_IM_T / 8)) {
            const int r = tid / (VQ_IM_T / 8), seg = tid % (VQ_IM_T / 8);
            uint2 w[4];
            w[0] = *reinterpret_cast<const uint2 *>(tp + r * VQ_IM_STRIDE + seg * 8);
            w[1] = *reinterpret_cast<const uint2 *>(tp + r * VQ_IM_STRIDE + seg * 8 + 8);
            w[2] = *reinterpret_cast<const uint2 *>(tq + r * VQ_IM_STRIDE + seg * 8);
            w[3] = *reinterpret_cast<const uint2 *>(tq + r * VQ_IM_STRIDE + seg * 8 + 8);
            unsigned int pb[16], qb[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const unsigned int wp = (e & 4) ? w[e >> 3].y : w[e >> 3].x, wq = (e & 4) ? w[2 + (e >> 3)].y : w[2 + (e >> 3)].x;
                pb[e] = (wp >> (8 * (e & 3))) & 0xFFu;
                qb[e] = (wq >> (8 * (e & 3))) & 0xFFu;
            }
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                unsigned int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    const unsigned int p = pb[o + j], q = qb[o + j];
                    sx += p; sy += q; sxx += p * p; syy += q * q; sxy += p * q;
                }
                hs[r * VQ_IM_T + seg * 8 + o] = make_uint4(sx | (sy << 16), sxx, syy, sxy);      // sx, sy <= 7 * 255
            }
        }
        __syncthreads();
        const int x = tid & (VQ_IM_T - 1), yr = (tid / VQ_IM_T) * 4;
        uint4 rows[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) rows[k] = hs[(yr + k) * VQ_IM_T + x];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (y0 + yr + k + 6 >= g.H || x0 + x + 6 >= g.W) continue;
            unsigned int pk = 0, uxx = 0, uyy = 0, uxy = 0;                                      // 49 * 255 fits the 16-bit halves
#pragma unroll
            for (int j = 0; j < 7; ++j) { pk += rows[k + j].x; uxx += rows[k + j].y; uyy += rows[k + j].z; uxy += rows[k + j].w; }
            const int sx = (int)(pk & 0xFFFFu), sy = (int)(pk >> 16);
            const double ux = (double)sx / 12495.0, uy = (double)sy / 12495.0;                  // 49 * 255
            const double vx = (double)(49 * (int)uxx - sx * sx) / 152938800.0;                   // 49 * 48 * 255^2; below 2^28
            const double vy = (double)(49 * (int)uyy - sy * sy) / 152938800.0;
            const double vxy = (double)(49 * (int)uxy - sx * sy) / 152938800.0;
            const double a1 = 2.0 * ux * uy + g.c1, a2 = 2.0 * vxy + g.c2;
            const double b1 = ux * ux + uy * uy + g.c1, b2 = vx + vy + g.c2;
            const double S = (a1 * a2) / (b1 * b2);
            fixed += llrint(S * 1099511627776.0);                                                // 2^40
        }
    }
    long long v[VQ_IM_SLOT] = {abs_acc, sq_acc, fixed, nan};
#pragma unroll
    for (int k = 0; k < VQ_IM_SLOT; ++k) v[k] = im_wave_sum(v[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < VQ_IM_SLOT; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < VQ_IM_SLOT)
        ws[(int64_t)blockIdx.x * VQ_IM_SLOT + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// values64 [B, 4] = l1, mse, psnr, ssim; values32 the same rounded once; sums [B, 2] = abs_sum, sq_sum
__global__ __launch_bounds__(VQ_IM_THREADS) void image_metrics_finish_kernel(const long long *__restrict__ ws, int64_t B, int64_t slots,
                                                                             double n, double windows, int want_ssim,
                                                                             double *__restrict__ values64, float *__restrict__ values32,
                                                                             long long *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    for (int64_t b = threadIdx.x >> 6; b < B; b += VQ_IM_WAVES) {
        long long v[VQ_IM_SLOT] = {0, 0, 0, 0};
        for (int64_t i = lane; i < slots; i += 64) {
            const long long *p = ws + (b * slots + i) * VQ_IM_SLOT;
#pragma unroll
            for (int k = 0; k < VQ_IM_SLOT; ++k) v[k] += p[k];
        }
#pragma unroll
        for (int k = 0; k < VQ_IM_SLOT; ++k) v[k] = im_wave_sum(v[k]);
        if (lane != 0) continue;
        const double nan = __longlong_as_double(0x7FF8000000000000ll);
        double out[4];
        out[0] = (double)v[0] / (255.0 * n);
        out[1] = (double)v[1] / (65025.0 * n);
        out[2] = -10.0 * log10(out[1]);
        out[3] = want_ssim ? (double)v[2] / 1099511627776.0 / windows : nan;
        sums[2 * b] = v[0];
        sums[2 * b + 1] = v[1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double o = v[3] ? nan : out[k];
            values64[4 * b + k] = o;
            values32[4 * b + k] = (float)o;
        }
    }
}
