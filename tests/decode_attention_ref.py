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


# ---- the lane geometry of decode_attention_kernel, restated from the header and the kernel's comment (not imported from the
#      package), the lengths at which its control flow changes, and what the geometry tests build from them ----

def geometry(Dh: int, dtype):
    """(E, C, LP, PP, sweep): E elements per 16-byte piece, C = Dh / E pieces per row, LP = the next power of two >= C (at least 2)
    lanes share a position, a wave holds PP = 64 / LP positions, the four waves sweep 4 PP positions."""
    E = 16 // torch.empty((), dtype=dtype).element_size()
    C = Dh // E
    LP = 2
    while LP < C:
        LP *= 2
    PP = 64 // LP
    return E, C, LP, PP, 4 * PP


def edge_lengths(Dh: int, dtype):
    """The lengths n = seen + 1 at which that geometry's control flow changes: one position, a full first wave and one more, the
    fourth wave's first position (3 PP + 1), one sweep (the prefetch guard, the ragged tail), a third sweep, a fourth that ends in its second wave."""
    _, _, _, PP, sweep = geometry(Dh, dtype)
    return sorted({1, PP, PP + 1, 3 * PP + 1, sweep - 1, sweep, sweep + 1, 2 * sweep + 1, 3 * sweep + PP + 1})


def attend64_grouped(q_rot: torch.Tensor, keys: torch.Tensor, values: torch.Tensor, scale: float):
    """``attend64`` without the G copies of the cache (query head h reads kv head h // G, as there): the same three results, and
    the scores [B, Hq, n] besides."""
    q_rot, keys, values = q_rot.to(F64), keys.to(F64), values.to(F64)
    B, Hq, Dh = q_rot.shape
    Hkv = keys.shape[1]
    qg = q_rot.reshape(B, Hkv, Hq // Hkv, Dh)
    s = torch.einsum('bkgd,bknd->bkgn', qg, keys) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    out = torch.einsum('bkgn,bknd->bkgd', p, values) / p.sum(-1, keepdim=True)
    A = torch.einsum('bkgd,bknd->bkgn', qg.abs(), keys.abs()).amax(-1)
    vmax = values.abs().amax((-1, -2))[:, :, None].expand(B, Hkv, Hq // Hkv)
    return out.reshape(B, Hq, Dh), A.reshape(B, Hq), vmax.reshape(B, Hq), s.reshape(B, Hq, -1)


def drop_one_shift(q_rot: torch.Tensor, keys: torch.Tensor, values: torch.Tensor, scale: float, j: int) -> torch.Tensor:
    """The float64 output with position j removed from the softmax, minus the float64 output with it: [B, Hq, Dh].  With one
    position stored nothing remains and the output without it counts as zero (the kernel would divide 0 by 0)."""
    full = attend64_grouped(q_rot, keys, values, scale)[0]
    keep = torch.ones(keys.shape[2], dtype=torch.bool)
    keep[j] = False
    if not bool(keep.any()):
        return -full
    return attend64_grouped(q_rot, keys[:, :, keep], values[:, :, keep], scale)[0] - full


def power_positions(PP: int, n: int):
    """The positions whose loss the matrix must be able to see: both sides of the first wave's edge, the last two."""
    return sorted({j for j in (0, PP - 1, PP, n - 2, n - 1) if 0 <= j < n})


def power_ratio(q_rot, keys, values, scale: float, dtype, PP: int) -> float:
    """min over the positions of ``power_positions`` and the heads of |drop_one_shift|_max / (2 max out_bound of the head): above 1,
    a kernel that skips or double-counts one of these positions leaves the bound.  Computed from the reference alone."""
    n = keys.shape[2]
    out, A, vmax, _ = attend64_grouped(q_rot, keys, values, scale)
    bound = out_bound(n, scale, A[..., None], vmax[..., None], out.abs(), dtype).amax(-1)
    return min(float((drop_one_shift(q_rot, keys, values, scale, j).abs().amax(-1) / (2.0 * bound)).min()) for j in power_positions(PP, n))


def rope_tables(positions, Dh: int, theta: float = 10000.0):
    """cos, sin fp32 [len(positions), Dh] as LlamaRotaryEmbedding computes them (the CPU twin of the GPU tests' ``tables``)"""
    inv = 1.0 / (theta ** (torch.arange(0, Dh, 2, dtype=torch.float32) / Dh))
    f = torch.as_tensor(positions, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((f, f), -1)
    return emb.cos(), emb.sin()


def host_problem(shape, dtype, seed: int = 0, L: int = 1, amp: float = 1.0, tail: float = 777.0):
    """The values of tests/test_gpu_decode_attention.py's ``problem(shape, dtype, True, seed, L, amp)`` on the CPU, draw for draw (the
    GPU tests compare the two), so that what a CPU test establishes about the inputs holds for the GPU tests' inputs."""
    B, Hq, Hkv, Dh, seen, cap = shape
    gen = torch.Generator().manual_seed(100 + seed)
    nq, nk = Hq * Dh, Hkv * Dh
    rows = (amp * torch.randn(B * L, nq + 2 * nk, generator=gen)).to(dtype)
    store = torch.full((2, 2, B, Hkv, cap, Dh), tail, dtype=dtype)
    store[0, :, :, :, :seen] = (amp * torch.randn(2, B, Hkv, seen, Dh, generator=gen)).to(dtype)
    cos, sin = rope_tables(range(seen, seen + L), Dh)
    return dict(q=rows[:, :nq], k=rows[:, nq:nq + nk], v=rows[:, nq + nk:], cos=cos, sin=sin, store=store, kc=store[0, 0], vc=store[0, 1])


def matrix_shape(Dh: int, G: int, n: int):
    """(B, Hq, Hkv, Dh, seen, cap) of the geometry matrix: two batch rows and two kv heads, so the batch stride and kvh G Dh are live."""
    return (2, 2 * G, 2, Dh, n - 1, n + 2)


def matrix_seed(G: int, n: int) -> int:
    return 1000 * G + n


# The matrix draws q, k, v and the cache at this amplitude.  At unit variance the scores are N(0, 1) and a position's weight ranges
# over e^+-3.5 around 1 / n: the lightest of the watched positions then moves a head by a fifth of twice its bound (fp32, Dh = 16,
# n = 209) and the power condition fails.  At 0.5 the scores are N(0, 1 / 16), every weight is within a factor of two of 1 / n, and
# the condition holds at every case (weakest: 1.22 in bf16 at Dh = 16, n = 417); a query read from the wrong head still moves the
# weights by a third.  Values and bound scale alike.
MATRIX_AMP = 0.5


# ---- the full length, by probes: at n = 4096 the bound is a tenth of |out| for random data, so each batch row holds two chosen
#      positions with one key, bit for bit, whose score is more than 150 above every other: the exact output is the mean of their
#      two value rows to 1e-60, and a dropped, doubled or misaddressed row moves it by O(|V|) ----

PROBE_Q_AMP = 32.0                                        # with keys of norm 16 a probe scores about 512, a random key below 180


def probe_pairs(Dh: int, dtype, n: int):
    """One (a, b) per batch row: across two waves, across two sweeps, one (wave, slot) twice, the last sweep, and - the last row -
    position 0 with n - 1, the token the launch itself writes."""
    _, _, _, PP, sweep = geometry(Dh, dtype)
    return [(PP - 1, PP), (sweep - 1, sweep), (1, 1 + sweep), (n - sweep, n - 2), (0, n - 1)]


def probe_problem(Dh: int, G: int, dtype, n: int, cap: int, stored_key, seed: int = 0, tail: float = 777.0):
    """The inputs of one probe launch, on the CPU, keyed like ``host_problem``'s (packed rows, Hkv = 2).  ``stored_key(q, k, v, cos,
    sin)`` returns k' [B, Hkv, Dh] as the implementation under test stores it for these rows: the probe key of row b, planted at
    both of its positions - so the key that the last row's launch writes at n - 1 is the key planted at position 0, bit for bit."""
    pairs = probe_pairs(Dh, dtype, n)
    B, Hkv, Hq, seen = len(pairs), 2, 2 * G, n - 1
    gen = torch.Generator().manual_seed(4000 + seed)
    nq, nk = Hq * Dh, Hkv * Dh
    u = torch.randint(0, 2, (B, Hkv, 1, Dh), generator=gen).to(torch.float32) * 2.0 - 1.0
    q = PROBE_Q_AMP * (u + 0.25 * torch.randn(B, Hkv, G, Dh, generator=gen))
    rows = torch.randn(B, nq + 2 * nk, generator=gen)
    rows[:, :nq] = q.reshape(B, nq)
    k_probe = (16.0 * Dh ** -0.5 * u).reshape(B, nk)
    rows[B - 1, nq:nq + nk] = k_probe[B - 1]
    rows = rows.to(dtype)
    store = torch.full((2, 2, B, Hkv, cap, Dh), tail, dtype=dtype)
    store[0, :, :, :, :seen] = torch.randn(2, B, Hkv, seen, Dh, generator=gen).to(dtype)
    cos, sin = rope_tables([seen], Dh)
    p = dict(q=rows[:, :nq], k=rows[:, nq:nq + nk], v=rows[:, nq + nk:], cos=cos, sin=sin, store=store, kc=store[0, 0], vc=store[0, 1])
    key = stored_key(p['q'], k_probe.to(dtype), p['v'], cos, sin).reshape(B, Hkv, Dh)
    for b, pair in enumerate(pairs):
        for j in pair:
            if j != seen:
                store[0, 0, b, :, j] = key[b]
    return p, pairs


def probe_expectation(p, pairs, n: int, scale: float, dtype):
    """(the float64 output on the cache as stored [B, Hq, Dh], its bound) after the launch; asserts what the construction promises:
    one key at both positions bit for bit, more than 150 of score above every other position, an exact output at the mean of the
    two value rows, and both value rows more than 20 bounds away from it in every head."""
    kc, vc = p['kc'][:, :, :n].cpu(), p['vc'][:, :, :n].cpu()
    B, Hkv, _, Dh = kc.shape
    Hq = p['q'].shape[1] // Dh
    q_rot = rope64(p['q'].reshape(B, Hq, Dh).cpu(), p['cos'].cpu().reshape(1, 1, Dh), p['sin'].cpu().reshape(1, 1, Dh))
    want, A, vmax, s = attend64_grouped(q_rot, kc, vc, scale)
    bound = out_bound(n, scale, A[..., None], vmax[..., None], want.abs(), dtype)
    for b, (i, j) in enumerate(pairs):
        assert torch.equal(kc[b, :, i].view(torch.uint8), kc[b, :, j].view(torch.uint8)), f'row {b}: the keys at {i} and {j} differ'
        rest = torch.ones(n, dtype=torch.bool)
        rest[[i, j]] = False
        gap = torch.minimum(s[b, :, i], s[b, :, j]) - s[b][:, rest].amax(-1)
        assert float(gap.min()) > 150.0, (b, float(gap.min()))
        va, vb = (vc[b, :, t].to(F64).repeat_interleave(Hq // Hkv, dim=0) for t in (i, j))
        assert float((want[b] - (va + vb) / 2).abs().max()) <= 1e-12
        apart = (va - vb).abs() / 2                                              # the mean's distance to either row, per element
        assert bool((apart.amax(-1) > 20.0 * bound[b].amax(-1)).all()), (b, float((apart.amax(-1) / bound[b].amax(-1)).min()))
    return want, bound
