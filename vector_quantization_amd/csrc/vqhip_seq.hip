// libvqhip — the sequence ops of stage 2: the fused token sampler and the token cross-entropy.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "vqhip_host.h"
#include "vqhip_sample_kernels.h"
#include "vqhip_token_ce_kernels.h"

// ---- fused token sampler: the launch (vqhip_sample_kernels.h) -----------------------------------------------------------
static LdsCache g_sample_lds[3];

template <int DT>
static int launch_sample(const VqSampleArgs &a, hipStream_t s) {
    if (a.V <= VQ_SAMPLE_RESIDENT_MAX) {
        const size_t lds = (size_t)a.V * sizeof(unsigned int);
        if (lds > 32768)                                                         // beyond the default budget next to the static part
            if (int rc = ensure_dyn_lds((const void *)sample_tokens_kernel<DT, true>, lds, g_sample_lds[DT == VQHIP_DTYPE_F32 ? 0 : (DT == VQHIP_DTYPE_BF16 ? 1 : 2)])) return rc;
        sample_tokens_kernel<DT, true><<<(unsigned)a.Ro, VQ_SAMPLE_THREADS, lds, s>>>(a);
    } else {
        sample_tokens_kernel<DT, false><<<(unsigned)a.Ro, VQ_SAMPLE_THREADS, 0, s>>>(a);
    }
    VQ_CHECK_LAUNCH("sample_tokens_kernel");
    return VQHIP_OK;
}

// ---- fused token cross-entropy: the launches (vqhip_token_ce_kernels.h) ---------------------------------------------------
template <int DT, bool I64>
static int launch_token_ce_fwd(const VqCeArgs &a, float *loss, float *lse, int32_t *hit, float *out, hipStream_t s) {
    token_ce_fwd_kernel<DT, I64><<<(unsigned)a.R, VQ_CE_THREADS, 0, s>>>(a, loss, lse, hit);
    VQ_CHECK_LAUNCH("token_ce_fwd_kernel");
    token_ce_reduce_kernel<I64><<<1, VQ_CE_THREADS, 0, s>>>(a, loss, hit, out);
    VQ_CHECK_LAUNCH("token_ce_reduce_kernel");
    return VQHIP_OK;
}

template <int DT, bool I64>
static int launch_token_ce_bwd(const VqCeArgs &a, const float *lse, const float *g, int g_per_row, const float *wsum, void *grad,
                               int cols, int64_t row_stride_out, hipStream_t s) {
    token_ce_bwd_kernel<DT, I64><<<(unsigned)a.R, VQ_CE_THREADS, 0, s>>>(a, lse, g, g_per_row, wsum, grad, cols, row_stride_out);
    VQ_CHECK_LAUNCH("token_ce_bwd_kernel");
    return VQHIP_OK;
}

extern "C" {

// ---- fused token sampler (vqhip_sample_kernels.h) ---------------------------------------------------------------------------
int vqhip_sample_tokens(const void *logits, int dtype, int64_t R, int64_t row_stride, int64_t start, int64_t end, float cfg_alpha,
                        int cfg, float temperature, int top_k, float top_p, const float *u, int64_t *tokens,
                        vqhip_sample_cut_t *cut, void *stream) {
    VQ_REQUIRE(logits && u && tokens, "vqhip_sample_tokens: logits, u and tokens are required");
    VQ_REQUIRE(vq_float_dtype(dtype), "vqhip_sample_tokens: dtype");
    VQ_REQUIRE(R >= 1 && R < (1ll << 31), "vqhip_sample_tokens: R must be in 1 .. 2^31 - 1");
    VQ_REQUIRE(!cfg || R % 2 == 0, "vqhip_sample_tokens: R must be even under CFG");
    VQ_REQUIRE(start >= 0 && start < end && end <= row_stride, "vqhip_sample_tokens: need 0 <= start < end <= row_stride");
    VQ_REQUIRE(end - start <= VQ_SAMPLE_MAX_V, "vqhip_sample_tokens: end - start is beyond 2^20");
    VQ_REQUIRE(temperature - temperature == 0.0f && temperature > 0.0f, "vqhip_sample_tokens: the temperature must be finite and > 0");
    VQ_REQUIRE(!cfg || cfg_alpha - cfg_alpha == 0.0f, "vqhip_sample_tokens: alpha must be finite");
    VqSampleArgs a;
    a.logits = logits; a.row_stride = row_stride; a.start = start;
    a.V = (int)(end - start);
    a.Ro = (int)(cfg ? R / 2 : R);
    a.cfg = cfg ? 1 : 0;
    a.w_uncond = (float)(1.0 - (double)cfg_alpha); a.w_cond = cfg_alpha;
    a.temperature = temperature;
    a.k = top_k <= 0 ? 0 : (top_k < a.V ? top_k : a.V);
    a.use_top_p = (top_p >= 0.0f && top_p <= 1.0f) ? 1 : 0;
    a.one_minus_p = 1.0 - (double)top_p;
    a.u = u; a.tokens = tokens; a.cut = cut;
    return vq_with_dtype(dtype, [&](auto dt) { return launch_sample<decltype(dt)::value>(a, (hipStream_t)stream); });
}

// ---- fused token cross-entropy (vqhip_token_ce_kernels.h) -----------------------------------------------------------------
// what the two entry points refuse alike, and the arguments the kernels share
static int token_ce_setup(const char *what, const void *logits, int dtype, int64_t R, int64_t row_stride, int64_t start, int64_t end,
                          const void *targets, int target_dtype, int64_t shift_len, int64_t ignore_index, float eps,
                          const float *weight, VqCeArgs *a) {
    if (!logits || !targets) return fail(VQHIP_EINVAL, what, "logits and targets are required");
    if (!vq_float_dtype(dtype)) return fail(VQHIP_EINVAL, what, "dtype");
    if (target_dtype != VQHIP_DTYPE_I32 && target_dtype != VQHIP_DTYPE_I64) return fail(VQHIP_EINVAL, what, "target_dtype");
    if (R < 1 || R >= (1ll << 31)) return fail(VQHIP_EINVAL, what, "R must be in 1 .. 2^31 - 1");
    if (!(start >= 0 && start < end && end <= row_stride)) return fail(VQHIP_EINVAL, what, "need 0 <= start < end <= row_stride");
    if (end - start > VQ_CE_MAX_V) return fail(VQHIP_EINVAL, what, "end - start is beyond 2^20");
    if (!(eps >= 0.0f && eps < 1.0f)) return fail(VQHIP_EINVAL, what, "label_smoothing must be in [0, 1)");
    if (shift_len < 0 || (shift_len > 0 && R % shift_len != 0)) return fail(VQHIP_EINVAL, what, "shift_len must be 0 or divide R");
    a->logits = logits; a->row_stride = row_stride; a->start = start;
    a->V = (int)(end - start);
    a->R = R;
    a->targets = targets; a->shift_len = shift_len; a->ignore_index = ignore_index;
    a->eps = eps; a->one_minus_eps = (float)(1.0 - (double)eps); a->eps_over_v = eps / (float)a->V;
    a->weight = weight;
    return VQHIP_OK;
}

int vqhip_token_ce_fwd(const void *logits, int dtype, int64_t R, int64_t row_stride, int64_t start, int64_t end, const void *targets,
                       int target_dtype, int64_t shift_len, int64_t ignore_index, float label_smoothing, const float *weight,
                       float *loss, float *lse, int32_t *hit, float *out, void *stream) {
    VqCeArgs a;
    if (int rc = token_ce_setup("vqhip_token_ce_fwd", logits, dtype, R, row_stride, start, end, targets, target_dtype, shift_len,
                                ignore_index, label_smoothing, weight, &a)) return rc;
    VQ_REQUIRE(loss && lse && out, "vqhip_token_ce_fwd: loss, lse and out are required");
    hipStream_t s = (hipStream_t)stream;
    return vq_with_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return target_dtype == VQHIP_DTYPE_I64 ? launch_token_ce_fwd<DT, true>(a, loss, lse, hit, out, s)
                                               : launch_token_ce_fwd<DT, false>(a, loss, lse, hit, out, s);
    });
}

int vqhip_token_ce_bwd(const void *logits, int dtype, int64_t R, int64_t row_stride, int64_t start, int64_t end, const void *targets,
                       int target_dtype, int64_t shift_len, int64_t ignore_index, float label_smoothing, const float *weight,
                       const float *lse, const float *g, int g_per_row, const float *wsum, void *grad, int64_t cols,
                       int64_t row_stride_out, void *stream) {
    VqCeArgs a;
    if (int rc = token_ce_setup("vqhip_token_ce_bwd", logits, dtype, R, row_stride, start, end, targets, target_dtype, shift_len,
                                ignore_index, label_smoothing, weight, &a)) return rc;
    VQ_REQUIRE(lse && g && grad, "vqhip_token_ce_bwd: lse, g and grad are required");
    VQ_REQUIRE(end <= cols && cols <= row_stride_out && cols < (1ll << 31), "vqhip_token_ce_bwd: need end <= cols <= row_stride_out, cols < 2^31");
    hipStream_t s = (hipStream_t)stream;
    return vq_with_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return target_dtype == VQHIP_DTYPE_I64 ? launch_token_ce_bwd<DT, true>(a, lse, g, g_per_row ? 1 : 0, wsum, grad, (int)cols, row_stride_out, s)
                                               : launch_token_ce_bwd<DT, false>(a, lse, g, g_per_row ? 1 : 0, wsum, grad, (int)cols, row_stride_out, s);
    });
}

}  // extern "C"
