"""A float64 restatement of the token cross-entropy contract of include/vqhip.h (vqhip_token_ce_fwd / _bwd), the case generators
of the GPU tests and the header's error bounds.  Written from the definition in the header: numpy only, torch for the dtypes."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
VS = [1, 2, 63, 64, 65, 257, 1024, 4099, 16384]
STARTS = [0, 1, 1001]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
RS = [1, 2, 6]
# one V just past every boundary of the kernel's forms: a 16-byte piece (4 fp32 / 8 16-bit elements) and one round of the 256
# threads over the pieces (1024 / 2048 elements)
BOUNDARY_VS = [5, 9, 1025, 2049]
LONG_V = 64000
PAD = 7                                       # row stride = end + 7: rows at every element alignment
IGNORE = -100


def chain(n: int) -> float:
    return float(n // 256 + 20)


def lse_bound(V: int, amax: float) -> float:
    return (5.0 * amax + 44.0 + 4.0 * chain(V)) * U * (1.0 + 2.0 ** -9)


def bound(V: int, amax: float) -> float:
    """VQHIP_TOKEN_CE_BOUND: |kernel - exact| of lse and of the per-row loss."""
    return lse_bound(V, amax) + ((chain(V) + 11.0) * amax + 70.0) * U


def grad_bound(V: int, amax: float) -> float:
    """VQHIP_TOKEN_CE_GRAD_BOUND: a gradient element in fp32 per unit |c_r|."""
    return lse_bound(V, amax) + (2.0 * amax + 22.0) * U


def half_ulp(x: np.ndarray, dtype) -> np.ndarray:
    """Half a unit in the last place of ``dtype`` at the magnitude of x (the rounding of the gradient into the logits' dtype)."""
    bits, emin = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -140)))
    return 2.0 ** (np.maximum(e, emin) - bits)


def cases():
    """(V, start, R, dtype, seed): every V with the three dtypes, the starts rotating, R cycling; not the full product."""
    out, n = [], 0
    for i, V in enumerate(VS + BOUNDARY_VS):
        for k, dtype in enumerate(DTYPES):
            out.append((V, STARTS[(i + k) % 3], RS[n % 3], dtype, n))
            n += 1
    for k, dtype in enumerate(DTYPES):
        out.append((LONG_V, STARTS[k], 2, dtype, n))
        n += 1
    return out


@functools.lru_cache(maxsize=None)
def make_case(V, start, R, dtype, seed):
    """logits [R, end + 7] in ``dtype`` (CPU) and int64 targets [R].  Row r is of kind (r + seed) % 4: 0 normal draws, 1 a wide
    spread (|a| up to 60), 2 exact ties at the maximum, 3 all values equal.  The columns outside the slice hold large values
    that must not be read.  With R = 6 the last row's target is ignored."""
    g = np.random.default_rng(1000 + seed)
    end = start + V
    x = g.normal(0, 3, size=(R, end + PAD))
    x[:, :start] = 90.0
    x[:, end:] = 95.0
    t = g.integers(start, end, size=R)
    for r in range(R):
        kind = (r + seed) % 4
        sl = x[r, start:end]
        if kind == 1:
            sl[:] = g.uniform(-60, 60, size=V)
            sl[g.integers(0, V)] = 60.0
        elif kind == 2:
            top = sl.max() + 0.5
            tied = g.choice(V, size=min(V, 3), replace=False)
            sl[tied] = top
            t[r] = start + (tied.min() if r % 2 == 0 else tied.max())        # a hit on the lowest tied index, a miss on a higher
        elif kind == 3:
            sl[:] = 1.5
    if R == 6:
        t[R - 1] = IGNORE
    return torch.from_numpy(x).to(torch.float32).to(dtype), torch.from_numpy(t.astype(np.int64))


def row_targets(targets: np.ndarray, start: int, V: int, shift_len: int = 0, ignore_index: int = IGNORE):
    """Per row: the index inside the slice, -1 for an ignored row, -2 for a target outside the slice."""
    R = len(targets)
    out = np.empty(R, dtype=np.int64)
    for r in range(R):
        if shift_len and r % shift_len == shift_len - 1:
            out[r] = -1
            continue
        t = int(targets[r + 1] if shift_len else targets[r])
        out[r] = -1 if t == ignore_index else (t - start if start <= t < start + V else -2)
    return out


def reference(a: np.ndarray, tj: np.ndarray, eps: float, w=None):
    """The definition in float64 on the converted slice a [R, V]: dict of lse, loss, hit [R], wsum, total, hits, and
    ``grad_unit`` [R, V] = p - (1 - e)[j = t] - e / V (zero rows where ignored, NaN rows where the target is outside)."""
    R, V = a.shape
    e = float(np.float32(eps))
    ome = float(np.float32(1.0 - e))
    w = np.ones(R) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all='ignore'):
        m = a.max(-1, keepdims=True)
        lse = (m + np.log(np.exp(a - m).sum(-1, keepdims=True)))[:, 0]
        loss, hit, gu = np.zeros(R), np.zeros(R, dtype=np.int64), np.zeros((R, V))
        for r in range(R):
            if tj[r] == -1:
                continue
            if tj[r] == -2:
                loss[r], gu[r] = np.nan, np.nan
                continue
            d1 = lse[r] - a[r, tj[r]]
            loss[r] = d1 if e == 0 else ome * d1 + e * (lse[r] - a[r].sum() / V)
            hit[r] = int(not math.isnan(lse[r]) and int(np.argmax(a[r])) == tj[r])        # argmax: the lowest index
            gu[r] = np.exp(a[r] - lse[r]) - e / V
            gu[r, tj[r]] -= ome
        live = tj != -1
        wsum = w[live].sum()
        total = (w[live] * loss[live]).sum()
    return dict(lse=lse, loss=loss, hit=hit, wsum=wsum, total=total, hits=int(hit.sum()), grad_unit=gu, live=live, w=w)


def slice64(logits: torch.Tensor, start: int, V: int) -> np.ndarray:
    return logits.reshape(-1, logits.shape[-1])[:, start:start + V].to(torch.float64).numpy()
