"""Seeded hostile input families for the index-exactness tests (TEST INFRASTRUCTURE — numpy only, PCG64 streams like
oracle/synth.py).

The fp16 proposal pass of the library sees the codebook through ONE power-of-two scale per codebook (max|e| -> [2^13, 2^14),
anything below 2^-14 after scaling flushed to zero) and the latents through NO scale at all (above 65 504: inf, below 2^-14:
zero).  ``synth.make_inputs`` never reaches either edge; the families below sit on them.  Every family starts from `planted`
data (x = W[i] + 0.3 eps), so a row has one clearly nearest code in real arithmetic and a wrong index is a wrong answer, not
a coin toss between near ties (except `ulp_pairs`, whose point is the tie).

``make(kind, seed, N, K, D, **params) -> (x, w)`` fp32.  ``CASES`` names the (kind, params) pairs the tests run.
``bare_fp16_argmin`` is the library WITHOUT its margin: the argmax of the fp16 proposal score.  ``image_shares`` restates
the image rules as statistics (share of entries flushed / overflowed).
"""
from __future__ import annotations

import numpy as np

from . import synth

F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0


def _planted(seed: int, N: int, K: int, D: int, codes=None, w=None):
    """x = W[pick] + 0.3 eps with pick drawn from `codes` (default: all K)."""
    if w is None:
        w = synth.normal(seed + 1, K, D)
    g = synth.rng(seed + 2)
    pick = g.integers(0, K, N) if codes is None else np.asarray(codes)[g.integers(0, len(codes), N)]
    x = (w[pick] + np.float32(0.3) * synth.normal(seed, N, D)).astype(np.float32)
    return x, w, pick


def _f32(a) -> np.ndarray:
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return np.ascontiguousarray(a, dtype=np.float32)


# ---- the families ----------------------------------------------------------------------------------------------------

def channel_scale(seed, N, K, D, c=None, p=12, two=False, p2=-12):
    """Channel c of x and W times 2^p (two=True: a second channel times 2^p2 as well)."""
    x, w, _ = _planted(seed, N, K, D)
    c = D // 3 if c is None else c
    x[:, c] *= np.float32(2.0 ** p); w[:, c] *= np.float32(2.0 ** p)
    if two:
        c2 = (c + D // 2) % D
        x[:, c2] *= np.float32(2.0 ** p2); w[:, c2] *= np.float32(2.0 ** p2)
    return x, w


def channel_offset(seed, N, K, D, c=None, offset=3000.0):
    """Channel c of x and W shifted by +offset (a ViT "massive activation": same sign everywhere).  At 3000 the fp16
    image rounds the hot channel by more than the planted noise; at 2^28 every other channel falls below 2^-14 of the scale
    and is flushed (a cosine codebook's normalised rows then all round to the same unit vector in fp32 as well)."""
    x, w, _ = _planted(seed, N, K, D)
    c = D // 3 if c is None else c
    x[:, c] += np.float32(offset); w[:, c] += np.float32(offset)
    return x, w


def _outlier_codebook(seed, K, D, s, every=97):
    w = synth.normal(seed + 1, K, D)
    out = np.arange(every - 1, K, every)
    w[out] *= np.float32(2.0 ** s)
    return w, out


def code_outliers(seed, N, K, D, s=28, every=97):
    """Every `every`-th code times 2^s; latents planted on the small codes and, for a tenth of the rows, on the outliers."""
    w, out = _outlier_codebook(seed, K, D, s, every)
    small = np.setdiff1d(np.arange(K), out)
    x, _, _ = _planted(seed, N, K, D, codes=small, w=w)
    if len(out):
        xo, _, _ = _planted(seed + 7, N, K, D, codes=out, w=w)
        x[9::10] = xo[9::10]
    return x, w


def row_scales(seed, N, K, D, lo=-20, hi=20):
    """Row n of x times 2^U{lo..hi}."""
    x, w, _ = _planted(seed, N, K, D)
    e = synth.rng(seed + 3).integers(lo, hi + 1, N)
    return _f32(x * np.ldexp(np.float32(1), e)[:, None].astype(np.float32)), w


def huge_rows(seed, N, K, D, factor=1e6, every=5):
    """Every `every`-th row times `factor`: 1e6 overflows fp16 only (1e5 leaves one row in a thousand at D = 8 without an
    entry above 65 504; at 1e6 every row has one), 1e16 passes the margin's magnitude guard (1e30 in
    squared units), 3e19 overflows |x|^2 in fp32 (the definition's distance is inf / NaN there)."""
    x, w, _ = _planted(seed, N, K, D)
    x[::every] = _f32(x[::every] * np.float32(factor))
    return x, w


def tiny_rows(seed, N, K, D, p=-18, every=3):
    """Every `every`-th row times 2^p (every=1: all rows): whole rows below fp16's smallest normal number."""
    x, w, _ = _planted(seed, N, K, D)
    x[::every] *= np.float32(2.0 ** p)
    return x, w


def codebook_scale(seed, N, K, D, s=90, subnormal=False, scale_x=True):
    """W times 2^s, x scaled alike where that is finite and unscaled otherwise (the codebook scale's shift is clamped at
    +-100).  subnormal=True: W is scaled so that its entries are fp32 subnormals (and x is left alone).  scale_x=False with
    s = 55: |e|^2 is finite in fp32 and above the margin's magnitude guard (1e30), the token image finite."""
    x, w, _ = _planted(seed, N, K, D)
    if subnormal:
        return x, _f32(w * np.float32(2.0 ** -100) * np.float32(2.0 ** -30))
    f = np.float32(2.0 ** s)
    w = _f32(w * f)
    if not scale_x:
        return x, w
    xs = _f32(x * f)
    return (xs if np.isfinite(xs).all() and np.isfinite(w).all() else x), w


def ulp_pairs(seed, N, K, D):
    """K/2 codes, each followed somewhere in the second half of the codebook by a copy that differs by ONE fp32 ulp in one
    coordinate (even codes: the copy is larger, odd: smaller).  A third of the latents sit exactly on codes, a third on the
    fp32 midpoint of a pair, a third are planted with noise: the fp32 definition ties or differs in its last bit, and the
    lowest index must win where it ties."""
    H = K // 2
    base = synth.normal(seed + 1, H, D)
    g = synth.rng(seed + 4)
    perm = g.permutation(H)
    coord = g.integers(0, D, H)
    copy = base.copy()
    r = np.arange(H)
    toward = np.where(r % 2 == 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    copy[r, coord] = np.nextafter(base[r, coord], toward)
    w = np.empty((K, D), np.float32)
    w[:H] = base
    w[H:2 * H] = copy[perm]                     # copy of code i lies at H + where(perm == i)
    if K > 2 * H:
        w[2 * H:] = synth.normal(seed + 5, K - 2 * H, D)
    pick = g.integers(0, H, N)
    x = base[pick].copy()
    mid = ((base[pick].astype(np.float64) + copy[pick].astype(np.float64)) * 0.5).astype(np.float32)
    x[1::3] = mid[1::3]
    x[2::3] = (base[pick] + np.float32(0.3) * synth.normal(seed, N, D))[2::3]
    return x.astype(np.float32), w


def count_ulp_pairs(w: np.ndarray) -> int:
    """Number of codes of the first half with a copy in the second half at one fp32 ulp in exactly one coordinate."""
    H = w.shape[0] // 2
    # adjacent fp32 numbers of one sign have adjacent bit patterns: a pair's rows differ by 1 in the sum of their patterns
    ka = np.ascontiguousarray(w[:H]).view(np.int32).astype(np.int64)
    kb = np.ascontiguousarray(w[H:2 * H]).view(np.int32).astype(np.int64)
    at = {}
    for i, s in enumerate(ka.sum(1).tolist()):
        at.setdefault(s, []).append(i)
    n = 0
    for j, s in enumerate(kb.sum(1).tolist()):
        for i in at.get(s - 1, []) + at.get(s + 1, []):
            d = np.abs(ka[i] - kb[j])
            if d.sum() == 1:
                n += 1
                break
    return n


def mixed(seed, N, K, D, s=28):
    """One batch against a `code_outliers` codebook whose rows come from four families — of every 8 consecutive rows one has
    a channel times 2^12, one a row scale 2^U{-20..20}, one is huge (x 1e6), one tiny (x 2^-18), four are plain planted
    rows: 16-token tiles, 32-code tiles and shared epilogues see hot and ordinary rows side by side."""
    w, out = _outlier_codebook(seed, K, D, s)
    small = np.setdiff1d(np.arange(K), out)
    x, _, _ = _planted(seed, N, K, D, codes=small, w=w)
    r = np.arange(N)
    x[r % 8 == 0, D // 3] *= np.float32(4096.0)
    e = synth.rng(seed + 3).integers(-20, 21, N)
    m = r % 8 == 1
    x[m] = _f32(x[m] * np.ldexp(np.float32(1), e[m])[:, None].astype(np.float32))
    x[r % 8 == 2] = _f32(x[r % 8 == 2] * np.float32(1e6))
    x[r % 8 == 3] *= np.float32(2.0 ** -18)
    return x, w


KINDS = {'channel_scale': channel_scale, 'channel_offset': channel_offset, 'code_outliers': code_outliers,
         'row_scales': row_scales, 'huge_rows': huge_rows, 'tiny_rows': tiny_rows, 'codebook_scale': codebook_scale,
         'ulp_pairs': ulp_pairs, 'mixed': mixed}

# name -> (kind, params): the cases the tests run.  family = the number the kind has in the test plan.
CASES = {
    'channel_scale': ('channel_scale', {}),
    'channel_scale_two': ('channel_scale', {'two': True}),
    'channel_offset': ('channel_offset', {}),
    'channel_offset_2p28': ('channel_offset', {'offset': 2.0 ** 28}),
    'code_outliers_s12': ('code_outliers', {'s': 12}),
    'code_outliers_s28': ('code_outliers', {'s': 28}),
    'row_scales': ('row_scales', {}),
    'huge_rows': ('huge_rows', {}),
    'huge_rows_1e16': ('huge_rows', {'factor': 1e16}),
    'huge_rows_3e19': ('huge_rows', {'factor': 3e19}),
    'tiny_rows': ('tiny_rows', {}),
    'tiny_rows_all': ('tiny_rows', {'every': 1}),
    'codebook_scale_m120': ('codebook_scale', {'s': -120}),
    'codebook_scale_m90': ('codebook_scale', {'s': -90}),
    'codebook_scale_p90': ('codebook_scale', {'s': 90}),
    'codebook_scale_p110': ('codebook_scale', {'s': 110}),
    'codebook_scale_subnormal': ('codebook_scale', {'subnormal': True}),
    'codebook_scale_p55_w': ('codebook_scale', {'s': 55, 'scale_x': False}),
    'ulp_pairs': ('ulp_pairs', {}),
    'mixed': ('mixed', {}),
}
FAMILY = {'channel_scale': 1, 'channel_offset': 2, 'code_outliers': 3, 'row_scales': 4, 'huge_rows': 5, 'tiny_rows': 6,
          'codebook_scale': 7, 'ulp_pairs': 8, 'mixed': 9}


def make(kind: str, seed: int, N: int, K: int, D: int, **params):
    """(x[N, D], w[K, D]) fp32 of a hostile family; `kind` is a family (with its parameters) or a name of CASES."""
    if kind in CASES and not params:
        kind, params = CASES[kind]
    x, w = KINDS[kind](seed, N, K, D, **params)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32)


def family_of(case: str) -> int:
    return FAMILY[CASES[case][0] if case in CASES else case]


# ---- the fp16 images, restated ---------------------------------------------------------------------------------------

def cb_scale(w: np.ndarray, metric: str = 'L2') -> float:
    """The codebook image's power-of-two scale: max|e| -> [2^13, 2^14), shift clamped at +-100; 1 for an empty or non-finite
    codebook (non-finite includes a row whose fp32 |e|^2 overflows); cosine images (unit rows) use the constant 2^13."""
    if metric != 'L2':
        return 2.0 ** 13
    with np.errstate(over='ignore', invalid='ignore'):
        e2 = (w.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    m = float(np.abs(w).max()) if w.size else 0.0
    if not (m > 0.0) or not np.isfinite(w).all() or not np.isfinite(e2).all():
        return 1.0
    _, ex = np.frexp(np.float32(m))
    return float(np.ldexp(1.0, int(np.clip(14 - int(ex), -100, 100))))


def f16_image(v: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """RNE to fp16 of v * scale (the product rounded to fp32 first, as the kernels form it), results below 2^-14 flushed to
    zero, overflow to inf; returned as float64 values of the fp16 numbers."""
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        q = (v.astype(np.float32) * np.float32(scale)).astype(np.float16).astype(np.float64)
    q[np.abs(q) < F16_MIN_NORMAL] = 0.0
    return q


def image_shares(x: np.ndarray, w: np.ndarray, metric: str = 'L2') -> dict:
    """Shares of non-zero input entries the images lose: cb_flushed, x_flushed, x_inf; x_inf_rows: rows with an inf entry;
    x_zero_rows: non-zero rows whose image is all zeros; cb_scale and the largest residual norm of a code's image."""
    se = cb_scale(w, metric)
    wi = f16_image(w, se)
    xi = f16_image(x)
    wnz, xnz = w != 0, x != 0
    with np.errstate(over='ignore', invalid='ignore'):
        resid = np.sqrt(((w.astype(np.float64) - wi / se) ** 2).sum(1))
    return {
        'cb_scale': se,
        'cb_resid_max': float(resid.max()),       # max_k |e_k - image of e_k|, unscaled units
        'cb_flushed': float(((wi == 0) & wnz).sum() / max(1, wnz.sum())),
        'x_flushed': float(((xi == 0) & xnz).sum() / max(1, xnz.sum())),
        'x_inf': float(np.isinf(xi).sum() / max(1, xnz.sum())),
        'x_inf_rows': int(np.isinf(xi).any(1).sum()),
        'x_zero_rows': int(((xi == 0).all(1) & xnz.any(1)).sum()),
    }


def bare_fp16_argmin(x: np.ndarray, w: np.ndarray, metric: str = 'L2') -> np.ndarray:
    """Argmax of the proposal score with NO margin behind it: the "subtly wrong kernel" of the test plan.  Images as above;
    score = xh . eh 2^p - 2^p |e|^2 / 2 (L2) or the dot product (cosine: x and w are the normalised rows), accumulated in
    float64; lowest index on ties; a row whose scores contain a NaN (inf image entries) returns -1 — counted as wrong."""
    se = cb_scale(w, metric)
    wi, xi = f16_image(w, se), f16_image(x)
    with np.errstate(over='ignore', invalid='ignore'):
        s = np.zeros((x.shape[0], w.shape[0]))
        fin = np.isfinite(xi).all(1)
        s[fin] = xi[fin] @ wi.T
        if metric == 'L2':
            s -= 0.5 * se * (w.astype(np.float64) ** 2).sum(1)[None, :]
    idx = s.argmax(1).astype(np.int64)
    idx[~fin | np.isnan(s).any(1)] = -1
    return idx
