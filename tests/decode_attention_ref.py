"""The float64 restatement of vqhip_decode_attention / vqhip_rope_append (include/vqhip.h, "static KV cache") and the error bounds the
GPU tests hold the kernels to.  Nothing here imports the package's own restatement: the lines below are the header's definition.

Bounds (derivation: DESIGN.md §8, the header's ERROR paragraph).  u = 2^-24 (1 + 2^-9), the project's fp32 unit roundoff with its
slack for products of (1 + u) factors.
  k', q' of rope_append   one ulp of the storage dtype at the exact value (the kernel's rotary is exact to one fp32 rounding, then
                          rounds once into the dtype: half an ulp of the dtype plus half an ulp of fp32).
  a score                 S = 17 u scale A,  A = max_j sum_i |q'_i K_j,i|.
  out                     eta = expm1(S) + (6 (n // 8 + 10) + 10) u;  2 eta / (1 - eta) vmax + u |out| + n 2^-126 vmax in fp32,
                          then the store: half an ulp of the dtype relative to |out| (fp16: 2^-25 absolute besides, the subnormals).
"""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24 * (1.0 + 2.0 ** -9)
MANTISSA = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
MIN_EXPONENT = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
STORE_U = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def rope64(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x' = x cos + rotate_half(x) sin in float64; x [..., Dh], cos and sin broadcast against it."""
    x, cos, sin = x.to(F64), cos.to(F64), sin.to(F64)
    half = x.shape[-1] // 2
    return x * cos + torch.cat((-x[..., half:], x[..., :half]), -1) * sin


def ulp(exact: torch.Tensor, dtype) -> torch.Tensor:
    """The spacing of ``dtype`` at the magnitude of each float64 value (the subnormal spacing below the smallest normal)."""
    e = torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -300))).clamp_min(MIN_EXPONENT[dtype])
    return torch.pow(torch.tensor(2.0, dtype=F64), e - MANTISSA[dtype])


def attend64(q_rot: torch.Tensor, keys: torch.Tensor, values: torch.Tensor, scale: float):
    """softmax(scale q' K^T) V with grouped-query heads in float64.  q_rot [B, Hq, Dh], keys and values [B, Hkv, n, Dh] (the cache as
    stored).  Returns (out [B, Hq, Dh], A [B, Hq] = max_j sum_i |q'_i K_j,i|, vmax [B, Hq] = max |V|)."""
    q_rot, keys, values = q_rot.to(F64), keys.to(F64), values.to(F64)
    G = q_rot.shape[1] // keys.shape[1]
    keys, values = keys.repeat_interleave(G, dim=1), values.repeat_interleave(G, dim=1)
    s = torch.einsum('bhd,bhnd->bhn', q_rot, keys) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    out = torch.einsum('bhn,bhnd->bhd', p, values) / p.sum(-1, keepdim=True)
    A = torch.einsum('bhd,bhnd->bhn', q_rot.abs(), keys.abs()).amax(-1)
    return out, A, values.abs().amax((-1, -2))


def decode64(q, k, v, cos, sin, k_cache, v_cache, seen: int, scale: float):
    """One step on float64 caches [B, Hkv, cap, Dh] (in place): the whole definition without any rounding.  Rows [B, H Dh]."""
    B, Hkv, _, Dh = k_cache.shape
    k_cache[:, :, seen] = rope64(k.reshape(B, Hkv, Dh), cos.reshape(1, 1, Dh), sin.reshape(1, 1, Dh))
    v_cache[:, :, seen] = v.reshape(B, Hkv, Dh).to(F64)
    q_rot = rope64(q.reshape(B, -1, Dh), cos.reshape(1, 1, Dh), sin.reshape(1, 1, Dh))
    out, _, _ = attend64(q_rot, k_cache[:, :, :seen + 1], v_cache[:, :, :seen + 1], scale)
    return out.reshape(B, -1)


def append64(q, k, v, cos, sin, k_cache, v_cache, seen: int):
    """L tokens on float64 caches (in place); rows [B L, H Dh], cos and sin [L, Dh].  Returns q' [B, Hq, L, Dh]."""
    B, Hkv, _, Dh = k_cache.shape
    L = q.shape[0] // B
    cos, sin = cos.reshape(1, L, 1, Dh), sin.reshape(1, L, 1, Dh)
    k_cache[:, :, seen:seen + L] = rope64(k.reshape(B, L, Hkv, Dh), cos, sin).transpose(1, 2)
    v_cache[:, :, seen:seen + L] = v.reshape(B, L, Hkv, Dh).to(F64).transpose(1, 2)
    return rope64(q.reshape(B, L, -1, Dh), cos, sin).transpose(1, 2)


def score_bound(scale: float, A):
    """|kernel score - exact score| for a query whose largest sum_i |q'_i K_j,i| is A."""
    return 17.0 * U * scale * A


def merge_chain(n: int) -> float:
    """The rescales and merges a weight passes through at length n: its slot's later positions, the butterfly, the four waves."""
    return float(n // 8 + 10)


def out_bound(n: int, scale: float, A, vmax, out_abs, dtype):
    """|kernel out - exact out| on the same stored cache, after the store into ``dtype``; A, vmax, out_abs: tensors or numbers."""
    eta = torch.expm1(torch.as_tensor(score_bound(scale, A), dtype=F64)) + (6.0 * merge_chain(n) + 10.0) * U
    fp32 = 2.0 * eta / (1.0 - eta) * vmax + U * out_abs + n * 2.0 ** -126 * vmax
    return fp32 + STORE_U[dtype] * (out_abs + fp32) + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def ln_weight(n: int) -> float:
    """ln n: what the argument roundings of the exponentials weigh in the mean (inside the 10 u of ``out_bound``)."""
    return math.log(max(n, 1))
