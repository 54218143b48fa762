"""numpy restatement of the fused MultinomialAnchor's contract (include/vqhip.h, vqhip_col_multinomial_*), shared by
test_col_multinomial_cpu.py and test_gpu_col_multinomial.py.

``pick`` is the definition itself: integer masses trunc(exp32(d - m) 2^40) down each column, exact integer sums, the first row
whose running sum exceeds T = min(floor(u Z), Z - 1).  Its float32 ``exp`` is numpy's, the kernel's is the device's: both are
within an ulp of the exact value, so the two need not pick the same row where u falls within delta of a boundary —
``check_pick`` is the rule both are held to, in float64 and free of either ``exp``.
"""
from typing import NamedTuple

import numpy as np

F32 = np.float32
FRAC = float(1 << 40)
MASS_FLOOR = -28.0          # exp(x) 2^40 < 1 for x < -27.73: a row further below the maximum has mass 0 and is never picked


def delta(N: int) -> float:
    """VQHIP_SAMPLE_DELTA(N): 2^-18 + N 2^-39 (derived in include/vqhip.h next to vqhip_col_multinomial_*)."""
    return 2.0 ** -18 + N * 2.0 ** -39


def bad_columns(d: np.ndarray) -> np.ndarray:
    """bool [K]: the column holds a NaN or a +inf."""
    d = np.asarray(d, dtype=F32)
    return (np.isnan(d) | (d == np.inf)).any(0)


def pick(d_fp32: np.ndarray, u: np.ndarray) -> np.ndarray:
    """col_idx int64 [K] of the definition on d [N, K] fp32 and u [K] fp32; -1 for a bad column."""
    d = np.asarray(d_fp32, dtype=F32)
    u = np.asarray(u, dtype=F32)
    N, K = d.shape
    assert u.shape == (K,)
    bad = bad_columns(d)
    safe = np.where(bad[None, :], F32(0.0), d)
    m = safe.max(0)
    with np.errstate(under='ignore'):
        w = np.exp((safe - m[None, :]).astype(F32)).astype(F32)                  # float32 exp of the float32 difference
    M = np.trunc(w.astype(np.float64) * FRAC).astype(np.int64)                   # the product is exact in float64
    C = np.cumsum(M, axis=0)                                                     # exact: below 2^61 for N <= 2^20
    Z = C[-1]
    assert (Z >= (1 << 40)).all()
    uu = np.where(u >= 0, u, F32(0.0)).astype(np.float64)
    T = np.minimum(np.floor(uu * Z.astype(np.float64)).astype(np.int64), Z - 1)
    idx = (C > T[None, :]).argmax(0).astype(np.int64)
    idx[bad] = -1
    return idx


class Check(NamedTuple):
    ok: np.ndarray           # bool [K]: the column meets the acceptance rule
    worst: float             # the largest |share error| / delta over the columns that are not bad (0: every u inside its interval)


def check_pick(d_fp32: np.ndarray, u: np.ndarray, idx: np.ndarray, dlt: float) -> Check:
    """The acceptance rule, per column.  Bad column: idx == -1 is required.  Any other column, with s_n = exp64(d[n, k] - m_k),
    S = sum_n s_n and j = idx[k] in [0, N):  d[j, k] - m_k >= -28;  sum_{n < j} s_n / S <= u_k + delta;
    sum_{n <= j} s_n / S >= u_k - delta.  No column is excused."""
    d = np.asarray(d_fp32, dtype=F32)
    u = np.where(np.asarray(u, dtype=F32) >= 0, np.asarray(u, dtype=F32), F32(0.0)).astype(np.float64)
    idx = np.asarray(idx).astype(np.int64)
    N, K = d.shape
    assert u.shape == (K,) and idx.shape == (K,)
    bad = bad_columns(d)
    ok = np.zeros(K, dtype=bool)
    ok[bad] = idx[bad] == -1
    good = ~bad
    in_range = good & (idx >= 0) & (idx < N)
    worst = 0.0
    if in_range.any():
        cols = np.nonzero(in_range)[0]
        d64 = d[:, cols].astype(np.float64)
        m = d64.max(0)
        with np.errstate(under='ignore'):
            s = np.exp(d64 - m[None, :])
        Cs = np.cumsum(s, axis=0)
        S = Cs[-1]
        j = idx[cols]
        a = np.arange(cols.size)
        hi = Cs[j, a] / S
        lo = (Cs[j, a] - s[j, a]) / S
        lo = np.where(j == 0, 0.0, lo)
        uc = u[cols]
        err = np.maximum(np.maximum(lo - uc, uc - hi), 0.0)
        worst = float(err.max() / dlt)
        ok[cols] = (d64[j, a] - m >= MASS_FLOOR) & (lo <= uc + dlt) & (hi >= uc - dlt)
    return Check(ok, worst)


def shares64(d_fp32: np.ndarray) -> np.ndarray:
    """float64 softmax down the columns, [K, N]: row k is the distribution code k draws its latent from."""
    d64 = np.asarray(d_fp32, dtype=F32).astype(np.float64).T
    with np.errstate(under='ignore'):
        s = np.exp(d64 - d64.max(1, keepdims=True))
    return s / s.sum(1, keepdims=True)


def uniforms(K: int, seed: int) -> np.ndarray:
    """u fp32 [K] in [0, 1): what torch.rand hands the kernel, from a seed."""
    u = np.random.default_rng(seed).random(K, dtype=F32)
    return np.minimum(u, np.nextafter(F32(1.0), F32(0.0)))
