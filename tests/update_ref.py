"""Float64 references, derived error bounds, the case table and the mutations of the codebook-update tests.

A plain helper module (not a conftest, no pytest settings), in the pattern of ``tests/backward_ref.py``, whose ``compare``,
``tree``, ``U`` and ``FLOOR`` it reuses.  ``tests/test_update_reference_cpu.py`` proves the bounds on the CPU (ATen's fp32
evaluation and the C oracle stay inside, every mutation falls outside); ``tests/test_gpu_updates.py`` holds the HIP update
kernels (``vqhip_update_kernels.h``, ``vqhip_exchange_kernels.h``) to the same bounds through the same ``compare``.

Every reference is the ``oracle.torch_ref`` composition (``frequency``, ``ema``, ``kmeans``, ``vqkd_after_encode``,
``cvq_after_encode``) evaluated in float64 from the exact fp32 input values.  The hyperparameters enter at the fp32 values
the C ABI receives (``f32(g)``), so a comparison measures the kernel and not the rounding of its argument.  The centroid sums
and the (all-reduced) anchor sums are INPUTS here: the scatter-add and the collective have tests of their own.

Rounding counts (u = 2^-24 per fp32 operation, relative to the magnitude expression of its result; the library is built with
``-ffp-contract=off``, so no product and sum share a rounding).  ``lt`` = 1 where g < 0.5 (``1.0f - g`` is exact for
g >= 0.5, one rounding below), ``cv`` = the int -> float conversions that round (a count or token count above 2^24):

* ``p' = p g + (float(h) / float(n)) (1 - g)`` (``cvq_update_kernel``, ``cvq_step_kernel``, ``cvq_apply_kernel``): the
  longest path is conversion(s), quotient, [1 - g], product, sum: **c = 3 + lt + cv** on A = |p| g + (h/n)(1 - g).
* the exponent ``-p' K 10 / (1 - g) - eps`` (``cvq_decay_of``, ``cvq_may_need_anchor``): product with K, product with 10,
  [1 - g], quotient, difference: **c = 4 + lt** on A = |p'| K 10/(1 - g) + eps, plus the error p' brings along times K 10/(1-g).
* ``expf``: |d exp(a)| <= exp(a) (expm1(|d a|) + ulps 2u).  No accuracy table of the device's ``expf`` is at hand, so the bound
  is ASSUMED: **EXPF_ULPS = 1**; 1 ulp is at most 2u of the value.
* ``decay = 1 - exp``: **1** on 1 + exp.  ``om = 1 - decay``: **1** on 1 + |decay|, on top of decay's own error.
* the blend ``w decay + a om``: product, sum: **c = 2** on |w||decay| + |a||om|, plus |w| d(decay) + |a| d(om); the packed
  form's ``a = S / world`` adds **1** on the anchor term.
* VQ-KD (``vqkd_update_kernel``): ``c0 = sums / float(count)``: conversion, quotient: **2**.  A normalisation
  ``v / max(|v|, 1e-12f)`` costs tree(D)/2 + 1 for the norm (sum of non-negative terms, sqrt halves), 1 for the quotient and
  1 for ``1e-12f`` not being the double 1e-12: **tree(D)/2 + 2** (+ 1 for the constant), on top of what its input carries: an
  elementwise error d v moves the norm by at most |d v|_2.  The EMA ``w g + cn (1 - g)``: product(s) [1 - g], sum:
  **2 + lt**.  Two normalisations and the EMA are chained by ``_normalize_tol`` / ``vqkd_tolerance``, term by term.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from backward_ref import EPS, FLOOR, U, compare, tree          # noqa: F401  (re-exported: the tests use ur.compare)
from oracle import synth, torch_ref as tr

EXPF_ULPS = 1                  # assumed: see the docstring
C_BLEND = 2
SURE_ARG = 20.0                # VQ_CVQ_SURE_ARG of vqhip_exchange_kernels.h
F64 = torch.float64


def f32(v: float) -> float:
    """The value the C ABI's ``float`` argument holds."""
    return float(np.float32(v))


def lt(g: float) -> int:
    return 1 if f32(g) < 0.5 else 0


def c_exponent(g: float) -> int:
    """Roundings of the exponent's own chain (x K, x 10, [1 - g], /, - eps)."""
    return 4 + lt(g)


# ------------------------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (5, 8), (1027, 24), (257, 63), (130, 65), (64, 256), (33, 1030)]
SETTINGS = [(0.99, 1e-3), (0.9, 1e-2), (0.5, 0.0), (0.999, 1e-3), (0.25, 0.5)]
KD_DECAYS = [0.99, 0.9, 0.5, 0.999, 0.25, 0.0, 1.0]
KINDS = ('uniform', 'one', 'big')
TOKENS = (300, 777, 1500, 3000, 1021)
BIG_A, BIG_B = 2 ** 24 + 1, 2 ** 40


@dataclass
class CvqCase:
    name: str
    K: int
    D: int
    N: int
    g: float
    eps: float
    kind: str                  # histogram: 'uniform', 'one' (one code holds every token), 'big' (counts of 2^24 + 1 and 2^40)
    seed: int


@dataclass
class KdCase:
    name: str
    K: int
    D: int
    N: int
    g: float
    kind: str
    seed: int


CVQ_CASES = [CvqCase(f'k{K}_d{D}_g{g}_e{eps}_{KINDS[(i + j) % 3]}', K, D, TOKENS[(i + j) % 5], g, eps, KINDS[(i + j) % 3], 900 + 10 * i + j)
             for i, (K, D) in enumerate(SHAPES) for j, (g, eps) in enumerate(SETTINGS)]
KD_CASES = [KdCase(f'kd_k{K}_d{D}_g{g}_{KINDS[(i + j) % 3]}', K, D, TOKENS[(i + j) % 5], g, KINDS[(i + j) % 3], 1900 + 10 * i + j)
            for i, (K, D) in enumerate(SHAPES) for j, g in enumerate(KD_DECAYS)]


def threshold_p(K: int, g: float, eps: float) -> float:
    """p* with p* g K 10 / (1 - g) + eps = 20: the probability at which a code leaves the listed set."""
    g, eps = f32(g), f32(eps)
    return (SURE_ARG - eps) * (1.0 - g) / (g * K * 10.0)


def histogram(kind: str, seed: int, N: int, K: int):
    """(int64 histogram [K], token count).  'uniform': a random assignment with code 1 left empty; 'big': the same with a count
    of 2^24 + 1 and one of 2^40 planted (an all-reduced histogram of a very large world: only the int64 entry points take it)."""
    g = synth.rng(seed)
    if kind == 'one' or K == 1:
        h = np.zeros(K, np.int64)
        h[K - 1] = N
        return torch.from_numpy(h), N
    tok = g.integers(0, K, N)
    if K > 2:
        tok[tok == 1] = 0
    h = np.bincount(tok, minlength=K).astype(np.int64)
    if kind == 'big' and K >= 5:
        h[K - 2], h[K - 3] = BIG_A, BIG_B
    return torch.from_numpy(h), int(h.sum())


def cvq_inputs(c: CvqCase) -> dict:
    """w [K, D], p [K], hist int64 [K], numel, and three ranks' latents / column indices / int32 histograms (rank 0 is the
    one-rank data; 'big' counts exist in ``hist`` only).  Planted, where K leaves room: p in {0, a subnormal, the threshold,
    1.0, NaN} on the last codes, w rows at 2^60 and 2^-60 on the first two."""
    K, D, N = c.K, c.D, c.N
    g = synth.rng(c.seed)
    w = (g.standard_normal((K, D), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    span = 12.0 * (1.0 - f32(c.g)) / (K * 10.0)                      # exponents between -12 and 0 before the histogram's share
    p = (g.random(K, dtype=np.float32) * np.float32(span)).astype(np.float32)
    planted = [0.0, 1e-40, threshold_p(K, c.g, c.eps), 1.0, float('nan')]
    for i, v in enumerate(planted[:max(0, K - 1)]):
        p[K - 1 - i] = np.float32(v)
    if K >= 8:
        w[0] = np.float32(2.0 ** 60) * np.sign(w[0] + np.float32(0.1))
        w[1] = np.float32(2.0 ** -60) * w[1]
    hist, numel = histogram(c.kind, c.seed + 1, N, K)
    ranks = []
    for r in range(3):
        x = g.standard_normal((N, D), dtype=np.float32)
        col = g.integers(0, N, K).astype(np.int64)
        h = hist if (r == 0 and c.kind != 'big') else histogram('uniform', c.seed + 2 + r, N, K)[0]
        ranks.append(dict(x=torch.from_numpy(x), col=torch.from_numpy(col), hist32=h.to(torch.int32), numel=N))
    return dict(w=torch.from_numpy(w), p=torch.from_numpy(p), hist=hist, numel=numel, ranks=ranks)


def kd_inputs(c: KdCase) -> dict:
    """w [K, D] unit rows, hist int64 [K], sums [K, D].  Planted, where K leaves room: code 1 empty; code 2 an exactly zero sum
    with count 2 (two antipodal rows); code 3 empty with a zero codebook row; rows at 2^60 and 2^-60; 'big' counts."""
    K, D, N = c.K, c.D, c.N
    g = synth.rng(c.seed)
    w = synth.unit_rows(g.standard_normal((K, D), dtype=np.float32))
    hist, _ = histogram(c.kind, c.seed + 1, N, K)
    # a sum of `count` unit rows scattered around a direction: its norm is well below count
    dirs = synth.unit_rows(g.standard_normal((K, D), dtype=np.float32))
    sums = (dirs * np.minimum(hist.numpy(), 10 ** 6).astype(np.float32)[:, None] * np.float32(0.7)
            + g.standard_normal((K, D), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    sums[hist.numpy() == 0] = g.standard_normal((int((hist == 0).sum()), D), dtype=np.float32)     # ignored by a correct kernel
    if K >= 8:
        hist = hist.clone()
        hist[2] = 2
        sums[2] = 0.0
        hist[3] = 0
        w[3] = 0.0
        w[4] = np.float32(2.0 ** 60) * w[4]
        w[5] = np.float32(2.0 ** -60) * w[5]
    return dict(w=torch.from_numpy(w), hist=hist, sums=torch.from_numpy(sums))


# ------------------------------------------------------------------------------------------------------------------
# CVQ-VAE: reference and tolerance
# ------------------------------------------------------------------------------------------------------------------

def nan_codes(p: torch.Tensor) -> torch.Tensor:
    return torch.isnan(p)


def cvq_reference(w, p, hist, numel, x, col, g, eps, world: int = 1, dtype=F64, stage: int = 3, swap: bool = False,
                  freq_div=None) -> dict:
    """``tr.cvq_after_encode`` on (w, p) with the histogram ``hist`` / ``numel`` and the anchors ``x[col]`` (``world`` > 1: ``x``
    holds the SUMS over the ranks, divided by ``world`` as anchors.py:65-67 does), in ``dtype``.  The [N, K] matrix handed to
    NearestAnchor is built so that its column argmin is ``col``.  A NaN p is evaluated as 0 (``compare`` wants a finite
    reference); the caller checks those codes on their own (``nan_codes``).  ``stage`` 1 / 2 as ``ops.cvq_update_``.
    ``swap`` / ``freq_div``: mutations.  Returns dict(p, decay, w)."""
    K = w.shape[0]
    g, eps = f32(g), f32(eps)
    w, x = w.to(dtype), x.to(dtype)
    p = torch.nan_to_num(p, nan=0.0).to(dtype)
    n = x.shape[0]
    d = torch.ones(n, K, dtype=torch.float32)
    d[col, torch.arange(K)] = 0.0
    if dtype == F64:                                   # int64 / int64 would be ATen's fp32 quotient: exact operands instead
        h, nm = hist.to(F64), torch.tensor(float(numel if freq_div is None else freq_div), dtype=F64)
    else:
        h, nm = hist, torch.tensor(int(numel if freq_div is None else freq_div))
    if stage & 1:
        new_w, new_p, anchors, _, decay = tr.cvq_after_encode(x, None, d, w, p, g, eps, world_hist=h, world_numel=nm,
                                                              world_size=world, other_anchors=[] if world > 1 else None)
    else:                                              # stage 2 alone: the decay line and the blend from the current p
        new_p = p
        anchors = x[col] / world if world > 1 else x[col]
        decay = 1 - torch.exp(-p.reshape(K, 1) * K * 10 / (1 - g) - eps)
        new_w = tr.ema(w, anchors, decay)
    if swap:
        new_w = tr.ema(w, anchors, 1 - decay)
    if not stage & 2:
        new_w = w
    return dict(p=new_p, decay=decay.reshape(K), w=new_w)


def cvq_tolerance(w, p, hist, numel, a_abs, g, eps, stage: int = 3, c_anchor: int = 0) -> dict:
    """Tolerances (float64) of p', decay and w' as counted in the module docstring.  ``a_abs``: |anchor| per element [K, D]
    (after the division by the world size); ``c_anchor``: roundings the anchor itself carries (1 for S / world)."""
    K = w.shape[0]
    g, eps = f32(g), f32(eps)
    w64 = w.to(F64).abs()
    p64 = torch.nan_to_num(p, nan=0.0).to(F64)
    h = hist.to(F64)
    s = K * 10.0 / (1.0 - g)
    if stage & 1:
        freq = h / float(numel)
        cv = (h > 2 ** 24).to(F64) + (1.0 if numel > 2 ** 24 else 0.0)
        a_p = p64.abs() * g + freq * (1.0 - g)
        tol_p = (3 + lt(g) + cv) * U * a_p
        p_new = p64 * g + freq * (1.0 - g)
    else:
        tol_p = torch.zeros_like(p64)
        p_new = p64
    arg = -p_new * s - eps
    tol_arg = c_exponent(g) * U * (p_new.abs() * s + eps) + tol_p * s
    e = torch.exp(arg)
    tol_e = e * (torch.expm1(tol_arg) * (1 + 2 * EXPF_ULPS * U) + 2 * EXPF_ULPS * U)
    tol_decay = tol_e + U * (1 + e)
    decay = 1 - e
    tol_om = tol_decay + U * (1 + decay.abs())
    a_abs = a_abs.to(F64)
    dk, ok = decay.abs().unsqueeze(1), e.abs().unsqueeze(1)
    tol_w = (w64 * tol_decay.unsqueeze(1) + a_abs * tol_om.unsqueeze(1) + C_BLEND * U * (w64 * dk + a_abs * ok)
             + c_anchor * U * a_abs * ok)
    if not stage & 2:
        tol_w = torch.zeros_like(tol_w)
    return dict(p=tol_p, decay=tol_decay, w=tol_w, arg=arg, tol_arg=tol_arg)


# ------------------------------------------------------------------------------------------------------------------
# VQ-KD: reference and tolerance
# ------------------------------------------------------------------------------------------------------------------

def kd_reference(w, hist, sums, g, mode: str = 'full', dtype=F64) -> torch.Tensor:
    """``tr.vqkd_after_encode`` (mode 'full') / ``tr.kmeans`` ('centroid') from the given histogram and centroid sums."""
    w, sums = w.to(dtype), sums.to(dtype)
    if mode == 'centroid':
        return tr.kmeans(None, None, w, hist, sums)
    return tr.vqkd_after_encode(torch.zeros(1, w.shape[1], dtype=dtype), None, w, f32(g), hist, sums)


def _normalize_tol(v: torch.Tensor, tol_v: torch.Tensor, D: int):
    """(F.normalize(v), its tolerance) in float64 for fp32 rows that carry the elementwise error ``tol_v``."""
    nrm = v.norm(dim=1, keepdim=True)
    den = nrm.clamp_min(EPS)
    # (a square below 2^-126 is a subnormal: each of the D squares may lose up to 2^-149 absolutely, whatever its size)
    d_nrm = tol_v.norm(dim=1, keepdim=True) + (tree(D) / 2 + 1) * U * nrm + D * 2.0 ** -149 / (2 * nrm.clamp_min(2.0 ** -74))
    d_den = torch.where(nrm + d_nrm < EPS, torch.full_like(den, U * EPS), d_nrm + U * den)
    out = v / den
    return out, tol_v / den + out.abs() * d_den / den + U * out.abs()


def kd_tolerance(w, hist, sums, g, mode: str = 'full', tol_sums=None) -> torch.Tensor:
    g = f32(g)
    D = w.shape[1]
    w64, s64 = w.to(F64), sums.to(F64)
    occ = (hist > 0).reshape(-1, 1)
    cnt = hist.clamp_min(1).to(F64).reshape(-1, 1)
    c0 = torch.where(occ, s64 / cnt, w64)
    tol_c0 = 2 * U * c0.abs()
    if tol_sums is not None:
        tol_c0 = tol_c0 + tol_sums / cnt
    tol_c0 = torch.where(occ, tol_c0, torch.zeros_like(tol_c0))
    if mode == 'centroid':
        return tol_c0
    cn, tol_cn = _normalize_tol(c0, tol_c0, D)
    a_v = w64.abs() * g + cn.abs() * (1.0 - g)
    tol_v = U * (w64.abs() * g + cn.abs() * (1.0 - g) * (1 + lt(g))) + tol_cn * (1.0 - g) + U * a_v
    v = w64 * g + cn * (1.0 - g)
    return _normalize_tol(v, tol_v, D)[1]


# ------------------------------------------------------------------------------------------------------------------
# small float64 restatements of what torch_ref has no piece for
# ------------------------------------------------------------------------------------------------------------------

def listed_arg(p: torch.Tensor, K: int, g: float, eps: float) -> torch.Tensor:
    """The exponent ``cvq_may_need_anchor`` tests, in float64 from the fp32 product fl(p g): listed iff not (arg <= -20)."""
    g32 = torch.tensor(g, dtype=torch.float32)
    lower = (p.to(torch.float32) * g32).to(F64)                      # the kernel's own first rounding: an fp32 product
    return -lower * K * 10.0 / (1.0 - f32(g)) - f32(eps)


def listed(p: torch.Tensor, K: int, g: float, eps: float) -> torch.Tensor:
    return ~(listed_arg(p, K, g, eps) <= -SURE_ARG)


def pack_header(hist: torch.Tensor, numel: int) -> torch.Tensor:
    """The packed buffer's header (vqhip_exchange_kernels.h): counts as two 16-bit pieces, the token count as three, a zero."""
    h = hist.to(torch.int64)
    head = torch.tensor([numel & 0xFFFF, (numel >> 16) & 0xFFFF, numel >> 32, 0], dtype=torch.int64)
    return torch.cat([h & 0xFFFF, h >> 16, head]).to(torch.float32)


def unpack_header(packed: torch.Tensor, K: int) -> torch.Tensor:
    """int64 [K + 1] = counts, token count, from a (summed) header: exact while every piece stays below 2^24."""
    q = packed.to(F64)
    counts = q[K:2 * K] * 65536 + q[:K]
    numel = (q[2 * K + 2] * 65536 + q[2 * K + 1]) * 65536 + q[2 * K]
    return torch.cat([counts, numel.reshape(1)]).to(torch.int64)


# ------------------------------------------------------------------------------------------------------------------
# mutations: deliberately wrong float64 restatements that the bound must reject
# ------------------------------------------------------------------------------------------------------------------

CVQ_MUTATIONS = {'g_0.99', 'eps_dropped', 'freq_over_K', 'decay_swapped', 'last_K%4_unchanged', 'd_tail_unchanged',
                 'world_division_omitted', 'p_not_written'}
KD_MUTATIONS = {'g_0.99', 'decay_swapped', 'count_clamp_omitted', 'second_normalize_omitted', 'first_normalize_omitted',
                'unoccupied_zero_centroid', 'last_K%4_unchanged', 'd_tail_unchanged'}


def _keep_tail_codes(new: torch.Tensor, old: torch.Tensor) -> torch.Tensor:
    K = new.shape[0]
    out = new.clone()
    out[K - K % 4:] = torch.nan_to_num(old[K - K % 4:].to(new.dtype), nan=0.0)
    return out


def _keep_tail_elems(new: torch.Tensor, old: torch.Tensor) -> torch.Tensor:
    D = new.shape[1]
    out = new.clone()
    out[:, 64 * (D // 64):] = old[:, 64 * (D // 64):].to(new.dtype)
    return out


def cvq_mutations(c: CvqCase, inp: dict, x, col, hist, numel, world: int = 1) -> dict:
    """name -> dict(p, w) of every wrong restatement that applies to the case."""
    w, p = inp['w'], inp['p']
    base = cvq_reference(w, p, hist, numel, x, col, c.g, c.eps, world)
    out = {}
    if f32(c.g) != f32(0.99):
        out['g_0.99'] = cvq_reference(w, p, hist, numel, x, col, 0.99, c.eps, world)
    if c.eps != 0:
        out['eps_dropped'] = cvq_reference(w, p, hist, numel, x, col, c.g, 0.0, world)
    if numel != c.K:
        out['freq_over_K'] = cvq_reference(w, p, hist, numel, x, col, c.g, c.eps, world, freq_div=c.K)
    out['decay_swapped'] = cvq_reference(w, p, hist, numel, x, col, c.g, c.eps, world, swap=True)
    if c.K % 4:
        out['last_K%4_unchanged'] = dict(p=_keep_tail_codes(base['p'], p), w=_keep_tail_codes(base['w'], w))
    if c.D % 64:
        out['d_tail_unchanged'] = dict(p=base['p'], w=_keep_tail_elems(base['w'], w))
    if world > 1:
        out['world_division_omitted'] = cvq_reference(w, p, hist, numel, x, col, c.g, c.eps, 1)
    out['p_not_written'] = dict(p=torch.nan_to_num(p, nan=0.0).to(F64), w=base['w'])
    return out


def kd_mutations(c: KdCase, inp: dict) -> dict:
    """name -> the full-mode result of every wrong restatement that applies to the case."""
    import torch.nn.functional as F
    w, hist, sums = inp['w'].to(F64), inp['hist'], inp['sums'].to(F64)
    g = f32(c.g)
    base = kd_reference(inp['w'], hist, sums, g)
    occ = (hist > 0).reshape(-1, 1)
    cnt = hist.clamp_min(1).to(F64).reshape(-1, 1)
    cent = torch.where(occ, sums / cnt, w)
    out = {}
    if g != f32(0.99):
        out['g_0.99'] = kd_reference(inp['w'], hist, sums, 0.99)
    out['decay_swapped'] = F.normalize(tr.ema(w, F.normalize(cent), 1.0 - g))
    if bool((hist == 0).any()):
        # with `where` the clamp is dead code; it is live in the branchless select m c + (1 - m) w, where 0 * (0 / 0) is NaN
        m = occ.to(F64)
        raw = m * (sums / hist.to(F64).reshape(-1, 1)) + (1 - m) * w
        out['count_clamp_omitted'] = F.normalize(tr.ema(w, F.normalize(raw), g))
        zero = torch.where(occ, sums / cnt, torch.zeros_like(w))
        out['unoccupied_zero_centroid'] = F.normalize(tr.ema(w, F.normalize(zero), g))
    out['second_normalize_omitted'] = tr.ema(w, F.normalize(cent), g)
    out['first_normalize_omitted'] = F.normalize(tr.ema(w, cent, g))
    if c.K % 4:
        out['last_K%4_unchanged'] = _keep_tail_codes(base, w)
    if c.D % 64:
        out['d_tail_unchanged'] = _keep_tail_elems(base, w)
    return out


def not_vacuous(ref: torch.Tensor, tol: torch.Tensor) -> bool:
    """Some element has a tolerance above the floor and a non-zero reference: the comparison is not one of zeros with zeros."""
    return bool(((tol.expand_as(ref) > FLOOR) & (ref != 0)).any())


# ------------------------------------------------------------------------------------------------------------------
# the known difference: 1 - g formed in double and rounded (oracle.c_oracle.cvq_decay, the reference) against the
# kernels' fp32 ``1.0f - g``
# ------------------------------------------------------------------------------------------------------------------

def double_g_figure(g: float) -> dict:
    """Largest |decay(double g) - decay(fp32 g)| over the CVQ cases, in units of decay's bound, both in float64.  'double g':
    the denominator fl32(1 - g) with g the DOUBLE value (what ``np.float32(1 - 0.99)`` gives); 'fp32 g': 1 - f32(g)."""
    worst, where = 0.0, ''
    den_double = float(np.float32(1.0 - g))
    den_f32 = 1.0 - f32(g)
    for c in CVQ_CASES:
        inp = cvq_inputs(c)
        p = torch.nan_to_num(inp['p'], nan=0.0).to(F64)
        eps = f32(c.eps)
        d_a = 1 - torch.exp(-p * c.K * 10 / den_double - eps)
        d_b = 1 - torch.exp(-p * c.K * 10 / den_f32 - eps)
        tol = cvq_tolerance(inp['w'], inp['p'], inp['hist'], inp['numel'], torch.zeros_like(inp['w']), g, c.eps, stage=2)['decay']
        r = ((d_a - d_b).abs() / tol.clamp_min(FLOOR)).max().item()
        if r > worst:
            worst, where = r, c.name
    return dict(g=g, ratio=worst, case=where, denominators_differ_by_u=abs(den_double - den_f32) / (U * den_f32))


# ------------------------------------------------------------------------------------------------------------------
# the kernels' expressions restated in numpy fp32, operation by operation in the kernels' order (-ffp-contract=off: every
# product, sum and quotient rounds on its own; exp is the correctly rounded one, not the device's expf).  CPU stand-ins for
# what the kernels compute: tests/test_update_reference_cpu.py runs them through the same bounds and the same listed-set
# assertions as the GPU tests, and profiles/update_parity.txt records their figures next to the device's.
# ------------------------------------------------------------------------------------------------------------------

_F = np.float32


def k_decay(p: np.ndarray, K: int, g: float, eps: float) -> np.ndarray:
    """cvq_decay_of."""
    g, eps = _F(g), _F(eps)
    with np.errstate(all='ignore'):
        arg = ((-p * _F(K)) * _F(10.0)) / (_F(1.0) - g) - eps
        return (_F(1.0) - np.exp(arg.astype(np.float64)).astype(np.float32)).astype(np.float32)


def k_pnew(p: np.ndarray, hist: np.ndarray, numel: int, g: float) -> np.ndarray:
    """p' of cvq_update_kernel / cvq_step_kernel / cvq_apply_kernel."""
    g = _F(g)
    with np.errstate(all='ignore'):
        freq = (hist.astype(np.float32) / _F(numel)).astype(np.float32)
        return ((p * g).astype(np.float32) + (freq * (_F(1.0) - g)).astype(np.float32)).astype(np.float32)


def k_blend(w: np.ndarray, a: np.ndarray, decay: np.ndarray) -> np.ndarray:
    with np.errstate(all='ignore'):
        om = (_F(1.0) - decay).astype(np.float32)
        return ((w * decay[:, None]).astype(np.float32) + (a * om[:, None]).astype(np.float32)).astype(np.float32)


def k_cvq(w, p, hist, numel, a, g, eps, world: int = 1) -> dict:
    """The whole CVQ-VAE update (stage 3 / cvq_step / cvq_apply; ``world`` > 1: a = S / world first) from torch inputs."""
    K = w.shape[0]
    pk = k_pnew(p.numpy(), hist.numpy(), numel, g)
    a = a.numpy() if world == 1 else (a.numpy() / _F(world)).astype(np.float32)
    decay = k_decay(pk, K, g, eps)
    return dict(p=torch.from_numpy(pk), decay=torch.from_numpy(decay), w=torch.from_numpy(k_blend(w.numpy(), a, decay)))


def k_vqkd(w, hist, sums, g, mode: str = 'full') -> torch.Tensor:
    """vqkd_update_kernel (the row sums of squares as numpy's fp32 pairwise sums, not the wave tree)."""
    W, h, s = w.numpy(), hist.numpy(), sums.numpy()
    occ = h > 0
    cnt = np.where(occ, h, 1).astype(np.float32)[:, None]
    with np.errstate(all='ignore'):
        c = np.where(occ[:, None], (s / cnt).astype(np.float32), W)
        if mode == 'centroid':
            return torch.from_numpy(c)

        def den(v):
            n = np.sqrt((v * v).astype(np.float32).sum(1, dtype=np.float32)).astype(np.float32)
            return np.where(n < _F(1e-12), _F(1e-12), n)[:, None]
        c = (c / den(c)).astype(np.float32)
        d = _F(g)
        v = ((W * d).astype(np.float32) + (c * (_F(1.0) - d)).astype(np.float32)).astype(np.float32)
        return torch.from_numpy((v / den(v)).astype(np.float32))


def k_listed(p: np.ndarray, K: int, g: float, eps: float) -> np.ndarray:
    """cvq_may_need_anchor."""
    g = _F(g)
    with np.errstate(all='ignore'):
        lower = (p * g).astype(np.float32)
        arg = ((-lower * _F(K)) * _F(10.0) / (_F(1.0) - g) - _F(eps)).astype(np.float32)
        return ~(arg <= _F(-SURE_ARG))


# ------------------------------------------------------------------------------------------------------------------
# the listed set: settings, probabilities around the threshold, and the assertions on a listed set however it was computed
# ------------------------------------------------------------------------------------------------------------------

ROWS_SETTINGS = [(16384, 0.99, 1e-3), (7, 0.5, 0.0), (1000, 0.9, 0.5), (70000, 0.999, 1e-3), (4001, 0.25, 1e-3), (4000, 0.99, 1e-3),
                 (1023, 0.99, 1e-3), (65536, 0.99, 1e-3), (65537, 0.99, 1e-3)]
ROWS_N = 1000                  # token count of the soundness check: freq in {0, 1/N, 1}


def rows_p(K: int, g: float, eps: float) -> torch.Tensor:
    """min(K, 8193) consecutive fp32 values centred on the threshold, planted values in the remaining slots, shuffled.  Where K
    leaves no slot (K <= 8193) the outermost of the consecutive values, those farthest from the threshold, give way to the planted
    ones (K // 3 of them at most), so that NaN and negative p meet every path of the kernel."""
    n = min(K, 8193)
    ps = np.array([threshold_p(K, g, eps)], np.float32)
    vals = (ps.view(np.int32)[0] + np.arange(n, dtype=np.int64) - n // 2).astype(np.int32).view(np.float32)
    planted = np.array([np.nan, -1.0, 0.0, 1e-40, 1.0, -1e-30, ps[0] * 0.5, ps[0] * 2], np.float32)
    if K - n < len(planted):
        m = min(len(planted), K // 3)
        vals[:m // 2] = planted[:m // 2]
        vals[n - (m - m // 2):] = planted[m // 2:m]
    p = np.concatenate([vals, np.resize(planted, K - n)]).astype(np.float32)
    synth.rng(4242).shuffle(p)
    return torch.from_numpy(p)


def check_listed_set(p: torch.Tensor, K: int, g: float, eps: float, is_listed: torch.Tensor, p_freq0: torch.Tensor) -> str:
    """Agreement of a listed set (bool [K]) with the float64 predicate outside the band the exponent's counted roundings leave,
    NaN / negative p listed, and the margin: ``p_freq0`` is p' for freq = 0 as the update computed it.  Returns the record line."""
    hostile = torch.isnan(p) | (p < 0)
    assert bool(torch.isnan(p).any()) and bool((p < 0).any())
    assert bool(is_listed[hostile].all()), 'NaN and negative p must be listed'
    arg = listed_arg(p, K, g, eps)
    band = (arg + SURE_ARG).abs() <= c_exponent(g) * U * SURE_ARG
    differs = is_listed != listed(p, K, g, eps)
    assert not bool((differs & ~band).any()), 'the listed set differs from the float64 predicate outside the band'
    assert int(differs.sum()) <= int(band.sum())
    worst_exp = 0.0
    if bool((~is_listed).any()):
        worst_exp = float(torch.exp(-p_freq0[~is_listed].to(F64) * K * 10.0 / (1.0 - f32(g)) - f32(eps)).max())
    margin = 2.0 ** -25 / worst_exp if worst_exp > 0 else float('inf')
    assert margin > 1.0
    return (f'cvq_rows K={K} g={g} eps={eps}: listed={int(is_listed.sum())} in_band={int(band.sum())} differ={int(differs.sum())} '
            f'largest exp(arg) unlisted={worst_exp:.4g} margin to 2^-25: factor {margin:.4g}')
