"""A float64 restatement of the CosineEmbeddingLoss contract of include/vqhip.h (vqhip_cosine_embed_fwd / _bwd), the case
generators of the GPU tests and the header's error bounds.  Written from the definition in the header: numpy only, torch for the
dtypes."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
EPS = float(np.float32(1e-12))              # ATen's EPSILON is a float constant, in float64 arithmetic too
CS = [1, 7, 8, 33, 511, 512, 520, 768, 1029, 4104]
RS = [1, 5, 300]
PADS = [0, 3]                                  # row stride C and C + 3 (a sliced view)
DTYPES = [(torch.bfloat16, torch.float32), (torch.float16, torch.float16), (torch.float32, torch.float32),
          (torch.float32, torch.bfloat16)]
MAP_SHAPES = [(1, 1, 1), (3, 7, 49), (2, 33, 65), (2, 512, 196), (1, 1029, 5)]
MAP_DTYPES = [(torch.bfloat16, torch.float32), (torch.float32, torch.float32)]
KINDS = 6
GARBAGE = 1.0e4                                # what the padding columns hold: must not be read


def chain(C: int) -> float:
    """VQHIP_COSINE_EMBED_CHAIN(C)."""
    return float(C // 32 + 16)


def bound(C: int) -> float:
    """VQHIP_COSINE_EMBED_BOUND(C): |kernel - exact| of a row's cos and loss."""
    return (2.0 * chain(C) + 6.0) * U * (1.0 + 2.0 ** -9)


def grad_bound(C: int, h):
    """VQHIP_COSINE_EMBED_GRAD_BOUND(C, h): a gradient element in fp32 per unit |c_r|, h = 1 / sqrt(|p|^2 + 1e-12)."""
    return (4.0 * chain(C) + 21.0) * U * (1.0 + 2.0 ** -9) * h


def sum_chain(R: int) -> float:
    """The header's chain of the scalars: (R / 256 + 10) u sum |loss_r|."""
    return float(R // 256 + 10)


def half_ulp(x: np.ndarray, dtype) -> np.ndarray:
    """Half a unit in the last place of ``dtype`` at the magnitude of x (the rounding of the gradient into pred's dtype)."""
    bits, emin = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -140)))
    return 2.0 ** (np.maximum(e, emin) - bits)


def cases():
    """(C, R, pad, (pred dtype, target dtype), seed): the full product of the rows grid."""
    out = []
    for C in CS:
        for R in RS:
            for pad in PADS:
                for dtypes in DTYPES:
                    out.append((C, R, pad, dtypes, len(out)))
    return out


def map_cases():
    """(B, C, P, (pred dtype, target dtype), seed)."""
    return [(B, C, P, dtypes, 1000 + i) for i, ((B, C, P), dtypes) in
            enumerate((s, d) for s in MAP_SHAPES for d in MAP_DTYPES)]


def _strided(values: torch.Tensor, pad: int) -> torch.Tensor:
    R, C = values.shape
    if not pad:
        return values.contiguous()
    buf = torch.full((R, C + pad), GARBAGE, dtype=values.dtype)
    buf[:, :C] = values
    return buf[:, :C]


@functools.lru_cache(maxsize=None)
def make_case(C, R, pad, dtypes, seed):
    """(pred [R, C], target [R, C]) on the CPU in the two dtypes, both views of row stride C + pad.  Row r is of kind
    (r + seed) % 6: 0, 1, 2 normal draws at scale 2^-8, 1, 2^8; 3 target = pred up to bf16 rounding (cos near 1: the cancellation
    of 1 - cos); 4 target = -pred; 5 target orthogonal to pred by construction (pairs swapped and negated; C = 1: a zero target)."""
    g = np.random.default_rng(7000 + seed)
    pd, td = dtypes
    p = g.normal(size=(R, C))
    t = g.normal(size=(R, C))
    for r in range(R):
        kind = (r + seed) % KINDS
        if kind < 3:
            s = (2.0 ** -8, 1.0, 2.0 ** 8)[kind]
            p[r] *= s
            t[r] *= s
    pred = torch.from_numpy(p).to(torch.float32).to(pd)
    p = pred.double().numpy()
    for r in range(R):
        kind = (r + seed) % KINDS
        if kind == 3:
            t[r] = torch.from_numpy(p[r]).to(torch.float32).to(torch.bfloat16).double().numpy()
        elif kind == 4:
            t[r] = -p[r]
        elif kind == 5:
            t[r] = 0.0
            even = (C // 2) * 2
            t[r, 0:even:2] = -p[r, 1:even:2]
            t[r, 1:even:2] = p[r, 0:even:2]
    target = torch.from_numpy(t).to(torch.float32).to(td)
    return _strided(pred, pad), _strided(target, pad)


@functools.lru_cache(maxsize=None)
def make_map_case(B, C, P, dtypes, seed):
    """(pred_map [B, C, P] NCHW-contiguous, pred_rows [B P, C], target [B, P, C]): the rows case of R = B P with pred permuted."""
    pred, target = make_case(C, B * P, 0, dtypes, seed)
    return pred.reshape(B, P, C).permute(0, 2, 1).contiguous(), pred, target.reshape(B, P, C)


def reference(p64: np.ndarray, t64: np.ndarray) -> dict:
    """The definition in float64 on the converted operands [R, C]: ``loss`` [R], ``grad_unit`` [R, C] = dloss_r / dp,
    ``total`` = sum_r loss_r, and ``cos``, ``h`` = 1 / sqrt(pp) [R]."""
    with np.errstate(all='ignore'):
        dot = (p64 * t64).sum(-1)
        pp = (p64 * p64).sum(-1) + EPS
        tt = (t64 * t64).sum(-1) + EPS
        den = np.sqrt(pp * tt)
        cos = dot / den
        loss = 1.0 - cos
        gu = (cos / pp)[:, None] * p64 - t64 / den[:, None]
        return dict(loss=loss, grad_unit=gu, total=loss.sum(), cos=cos, h=1.0 / np.sqrt(pp))


def as64(t: torch.Tensor) -> np.ndarray:
    return t.reshape(-1, t.shape[-1]).to(torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def expected(case) -> dict:
    """The float64 reference of a rows case, computed once and shared."""
    pred, target = make_case(*case)
    return reference(as64(pred), as64(target))


@functools.lru_cache(maxsize=None)
def expected_map(case) -> dict:
    _, pred, target = make_map_case(*case)
    return reference(as64(pred), as64(target))
