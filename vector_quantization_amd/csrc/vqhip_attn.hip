// libvqhip — the attention step of cached generation: rotary embedding + append to a static KV cache, and the one-token
// attention over it, with the position by value or in device memory; the end of a replayed step.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "vqhip_host.h"
#include "vqhip_attn_kernels.h"

// what the entry points refuse alike (every clause before any HIP call), and the arguments the kernels share
static int attn_setup(const char *what, const void *q, int64_t q_stride, const void *k, int64_t k_stride, const void *v, int64_t v_stride,
                      int dtype, const float *cos, const float *sin, void *k_cache, void *v_cache, int64_t seen, int64_t cap,
                      int64_t B, int64_t L, int Hq, int Hkv, int Dh, void *out, VqAttnArgs *a) {
    if (!q || !k || !v || !cos || !sin || !k_cache || !v_cache || !out)
        return fail(VQHIP_EINVAL, what, "q, k, v, cos, sin, k_cache, v_cache and the output are required");
    if (!vq_float_dtype(dtype)) return fail(VQHIP_EINVAL, what, "dtype");
    if (!(Dh >= 16 && Dh <= VQHIP_ATTN_MAX_HEAD_DIM && Dh % 8 == 0))
        return fail(VQHIP_EINVAL, what, "Dh must be a multiple of 8 in 16 .. VQHIP_ATTN_MAX_HEAD_DIM");
    if (!(Hkv >= 1 && Hq >= 1 && Hq % Hkv == 0)) return fail(VQHIP_EINVAL, what, "Hq must be a positive multiple of Hkv");
    if (Hq / Hkv > VQHIP_ATTN_MAX_GROUP) return fail(VQHIP_EINVAL, what, "Hq / Hkv is beyond VQHIP_ATTN_MAX_GROUP");
    if (!(cap >= 1 && cap <= VQHIP_ATTN_MAX_LEN)) return fail(VQHIP_EINVAL, what, "cap must be in 1 .. VQHIP_ATTN_MAX_LEN");
    if (!(B >= 1 && L >= 1 && B * L < (1ll << 31) && B * Hkv < (1ll << 31))) return fail(VQHIP_EINVAL, what, "B and L must be >= 1, B L and B Hkv < 2^31");
    if (!(seen >= 0 && seen + L <= cap)) return fail(VQHIP_EINVAL, what, "need 0 <= seen and seen + L <= cap");
    if (q_stride < (int64_t)Hq * Dh || k_stride < (int64_t)Hkv * Dh || v_stride < (int64_t)Hkv * Dh)
        return fail(VQHIP_EINVAL, what, "a row stride is below H Dh");
    const uintptr_t elem = dtype == VQHIP_DTYPE_F32 ? 4 : 2;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % elem || ((uintptr_t)cos | (uintptr_t)sin) % 4)
        return fail(VQHIP_EINVAL, what, "q, k, v, cos, sin and the output need the alignment of their element type");
    if (((uintptr_t)k_cache | (uintptr_t)v_cache) % 16) return fail(VQHIP_EINVAL, what, "k_cache and v_cache must be 16-byte aligned");
    a->q = q; a->k = k; a->v = v;
    a->q_stride = q_stride; a->k_stride = k_stride; a->v_stride = v_stride;
    a->cos = cos; a->sin = sin;
    a->k_cache = k_cache; a->v_cache = v_cache; a->out = out;
    a->seen = seen; a->cap = cap; a->L = L;
    a->pos = nullptr; a->table_stride = 0;
    a->scale = 0.0f;
    a->Hq = Hq; a->Hkv = Hkv; a->Dh = Dh; a->G = Hq / Hkv;
    return VQHIP_OK;
}

template <int DT, int GMAX>
static int launch_decode_attention(const VqAttnArgs &a, int64_t B, hipStream_t s) {
    decode_attention_kernel<DT, GMAX><<<(unsigned)(B * a.Hkv), VQ_ATTN_THREADS, 0, s>>>(a);
    VQ_CHECK_LAUNCH("decode_attention_kernel");
    return VQHIP_OK;
}

static int launch_decode(const VqAttnArgs &a, int dtype, int64_t B, hipStream_t s) {
    return vq_with_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return a.G == 1 ? launch_decode_attention<DT, 1>(a, B, s) : a.G == 2 ? launch_decode_attention<DT, 2>(a, B, s)
             : a.G <= 4 ? launch_decode_attention<DT, 4>(a, B, s) : launch_decode_attention<DT, 8>(a, B, s);
    });
}

template <int DT>
static int launch_rope_append(const VqAttnArgs &a, int64_t B, hipStream_t s) {
    rope_append_kernel<DT><<<(unsigned)(B * a.L), VQ_ATTN_THREADS, 0, s>>>(a);
    VQ_CHECK_LAUNCH("rope_append_kernel");
    return VQHIP_OK;
}

extern "C" {

int vqhip_decode_attention(const void *q, int64_t q_stride, const void *k, int64_t k_stride, const void *v, int64_t v_stride, int dtype,
                           const float *cos, const float *sin, void *k_cache, void *v_cache, int64_t seen, int64_t cap, float scale,
                           int64_t B, int Hq, int Hkv, int Dh, void *out, void *hip_stream) {
    VqAttnArgs a;
    if (int rc = attn_setup("vqhip_decode_attention", q, q_stride, k, k_stride, v, v_stride, dtype, cos, sin, k_cache, v_cache, seen, cap,
                            B, 1, Hq, Hkv, Dh, out, &a)) return rc;
    VQ_REQUIRE(scale - scale == 0.0f, "vqhip_decode_attention: scale must be finite");
    a.scale = scale;
    return launch_decode(a, dtype, B, (hipStream_t)hip_stream);
}

int vqhip_decode_attention_at(const void *q, int64_t q_stride, const void *k, int64_t k_stride, const void *v, int64_t v_stride, int dtype,
                              const float *cos_table, const float *sin_table, void *k_cache, void *v_cache, const int32_t *pos, int64_t cap,
                              float scale, int64_t B, int Hq, int Hkv, int Dh, void *out, void *hip_stream) {
    VqAttnArgs a;
    // (seen = 0 with L = 1 passes the seen clause for every cap the cap clause admits: the position is the kernel's to check)
    if (int rc = attn_setup("vqhip_decode_attention_at", q, q_stride, k, k_stride, v, v_stride, dtype, cos_table, sin_table, k_cache, v_cache,
                            0, cap, B, 1, Hq, Hkv, Dh, out, &a)) return rc;
    VQ_REQUIRE(scale - scale == 0.0f, "vqhip_decode_attention_at: scale must be finite");
    VQ_REQUIRE(pos != nullptr, "vqhip_decode_attention_at: pos is required");
    VQ_REQUIRE((uintptr_t)pos % 4 == 0, "vqhip_decode_attention_at: pos must be 4-byte aligned");
    a.scale = scale;
    a.pos = pos;
    a.table_stride = Dh;
    return launch_decode(a, dtype, B, (hipStream_t)hip_stream);
}

int vqhip_decode_advance(const int64_t *token, int64_t *next, int64_t *sequence, int64_t R, int64_t length, int32_t *pos, void *hip_stream) {
    VQ_REQUIRE(token && next && sequence && pos, "vqhip_decode_advance: token, next, sequence and pos are required");
    VQ_REQUIRE(R >= 1 && R < (1ll << 31), "vqhip_decode_advance: R must be in 1 .. 2^31 - 1");
    VQ_REQUIRE(length >= 2 && length <= VQHIP_ATTN_MAX_LEN, "vqhip_decode_advance: length must be in 2 .. VQHIP_ATTN_MAX_LEN");
    VQ_REQUIRE(((uintptr_t)token | (uintptr_t)next | (uintptr_t)sequence) % 8 == 0 && (uintptr_t)pos % 4 == 0,
               "vqhip_decode_advance: token, next and sequence must be 8-byte aligned, pos 4-byte aligned");
    decode_advance_kernel<<<1, VQ_ATTN_THREADS, 0, (hipStream_t)hip_stream>>>(token, next, sequence, R, length, pos);
    VQ_CHECK_LAUNCH("decode_advance_kernel");
    return VQHIP_OK;
}

int vqhip_rope_append(const void *q, int64_t q_stride, const void *k, int64_t k_stride, const void *v, int64_t v_stride, int dtype,
                      const float *cos, const float *sin, void *k_cache, void *v_cache, int64_t seen, int64_t cap, int64_t B, int64_t L,
                      int Hq, int Hkv, int Dh, void *q_out, void *hip_stream) {
    VqAttnArgs a;
    if (int rc = attn_setup("vqhip_rope_append", q, q_stride, k, k_stride, v, v_stride, dtype, cos, sin, k_cache, v_cache, seen, cap,
                            B, L, Hq, Hkv, Dh, q_out, &a)) return rc;
    return vq_with_dtype(dtype, [&](auto dt) { return launch_rope_append<decltype(dt)::value>(a, B, (hipStream_t)hip_stream); });
}

}  // extern "C"
