"""Float64 references, derived error bounds, the comparison function and the case table of the backward tests.

A plain helper module (not a conftest, no pytest settings).  It imports numpy, torch and ``oracle/torch_ref.py`` only, so it
travels with the tree; ``tests/test_backward_reference_cpu.py`` proves the bounds on the CPU (the reference in fp32 stays inside,
every deliberate mutation falls outside) and ``tests/test_gpu_backward.py`` holds every HIP backward kernel to the same bounds
through the same ``compare``.

Every reference is the ``oracle.torch_ref`` composition evaluated in float64 on the CPU from the exact input values and
differentiated by torch autograd.  Every tolerance is ``c * 2^-24 * A`` per element: ``A`` is the kernel's formula evaluated in
float64 with every term replaced by its absolute value (so cancellation cannot shrink it), ``c`` the number of fp32 roundings on
the longest path of the kernel, counted from the code in ``vector_quantization_amd/csrc`` and written down below.  Nothing here
is tuned to what a kernel returns.

Rounding counts (u = 2^-24, one unit per fp32 operation, relative to the magnitude expression of its result):

* ``tree(D) = ceil(D / 64) + 6``: a dot product of a row — ceil(D/64) fma per lane, then the 6-level halving tree over 64 lanes
  (``wave_sum_tree``; the L-lane group sums of the D <= 32 kernels are the same tree without its all-zero upper levels).
  A norm is sqrt of such a sum of non-negative terms: tree/2 + 1; ``v / max(|v|, eps)``: tree/2 + 2 (one more for 1e-12f, which
  is not the double 1e-12, is added once per kernel below).
* ``vq_backward_kernel`` / ``vq_backward_map256_kernel`` grad_x = g - kx (z - x):  kx = (g_cm + beta g_comb) * (2 / (N D)) is 4
  (product, sum, quotient, product; N D < 2^24 is exact), z - x 1, kx * d 1, g - . 1: **c = 7**.  The bf16 map store adds half a
  bf16 ulp of the result.
* grad_W[k] = sum over the m tokens of code k of kw (e_k - x_n):  kw 3 (sum, quotient, product), e - x 1, product 1, then m - 1
  additions in any order (fp32 atomics) or in the fixed order of the ordered route (at most m additions of partial sums):
  **c = m + 4**.  It is the worst case over summation orders, hence loose for a code with thousands of tokens; the case table
  plants the tokens a broken grid-stride tail would lose as outliers so that one missing contribution still exceeds it.
* ``normalize_bwd_kernel`` gv = (g - y (y.g)) / den, y = v / den:  y tree/2 + 2; the dot product adds tree to its terms' y;
  product, difference, quotient by den (tree/2 + 1): **c = 2.5 tree + 9**.
* ``vqkd_backward*`` and the normalised VQ tail chain these; ``vqkd_count`` / ``vq_norm_count`` add the same units step by step.
* ``diff_kernel`` out = (a - b) * (scale * scale_dev): **c = 3**; its sum of squares is a double sum of fp32 squares of fp32
  differences: 2 for the squared difference, 1 for the product: **c = 3** (plus n 2^-53 for the double sum).
* ``ste_kernel`` x + (z - x): **c = 2**.

ATen's fp32 evaluation of the same compositions (condition 1 of the CPU test) was counted too: its mse backward is
(2/numel * g) * (a - b) per loss term and the terms are accumulated one by one — 2 per term plus the accumulations, at most 8
for the three loss terms plus the straight-through gradient, so grad_x uses **c = 8** for kernel and ATen alike; its row sums
are vectorised cascades with fewer roundings per element than tree(D) + the chain counted here.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import synth, torch_ref as tr

U = 2.0 ** -24
FLOOR = 2.0 ** -126            # smallest normal fp32: absolute floor of every tolerance
EPS = 1e-12
OUTLIER = 4096.0               # |x - e| of a planted token against ~1 of an ordinary one (2^12)
SWEEP = 8192                   # rows one sweep of vq_backward_kernel's capped grid covers (2048 workgroups x 4 waves)


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------

@dataclass
class Verdict:
    ok: bool
    worst: float                # largest err / tol (inf where the result is not finite)
    pos: tuple                  # its position
    bad: int                    # elements outside the bound
    floor_needed: bool          # some element passed only because of the 2^-126 floor

    def line(self, name: str) -> str:
        return (f'{name}: err/tol={self.worst:.4g} at {self.pos} outside={self.bad}'
                f'{" floor-needed" if self.floor_needed else ""}')


def compare(got, ref, tol) -> Verdict:
    """|got - ref| <= max(tol, 2^-126) element by element; a NaN or Inf in ``got`` where ``ref`` is finite is outside."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64)
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    tol = torch.as_tensor(tol).detach().cpu().to(torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(tol).all()) and bool((tol >= 0).all())
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    ratio = err / tol.clamp_min(FLOOR)
    if ratio.numel() == 0:
        return Verdict(True, 0.0, (), 0, False)
    flat = int(ratio.reshape(-1).argmax())
    pos = tuple(int(v) for v in np.unravel_index(flat, tuple(ratio.shape))) if ratio.dim() else ()
    bad = int((ratio > 1).sum())
    floor_needed = bool(((err > tol) & (err <= FLOOR)).any())
    return Verdict(bad == 0, float(ratio.reshape(-1)[flat]), pos, bad, floor_needed)


def tree(D: int) -> float:
    return math.ceil(D / 64) + 6


C_GRAD_X = 8                   # 7 for the kernel, 8 for ATen's term-by-term accumulation: the larger one for both
C_DIFF = 3
C_SSE = 3
C_STE = 2


def c_grad_w(m: torch.Tensor) -> torch.Tensor:
    return m.to(torch.float64) + 4


def c_normalize_bwd(D: int) -> float:
    return 2.5 * tree(D) + 9


def vq_norm_count(D: int) -> float:
    """normalize_rows -> vq_backward on the normalised rows (+ g_xn) -> normalize_rows_bwd."""
    t = tree(D)
    e_xn = t / 2 + 2                                   # the rows the tail works on are fp32 outputs of normalize_rows
    e_gr = C_GRAD_X + e_xn + 1                         # grad of the rows, one more for adding g_xn
    e_y = t / 2 + 2
    e_dot = e_y + e_gr + t
    return max(e_gr, e_y + e_dot + 1) + 1 + (t / 2 + 1) + 1 + 1      # difference, quotient by den, eps


def vqkd_count(D: int) -> float:
    """vqkd_backward_kernel, step by step (see the kernel): the longest path runs through both dot products."""
    t = tree(D)
    e_xn = t / 2 + 2                                   # xn is an fp32 output of normalize_rows, the reference's is exact
    e_dn = e_xn + t / 2 + 1                            # |xn|
    e_t = e_xn + e_dn + 1                              # t = xn / dn
    e_z = t / 2 + 2                                    # zn = w / dz
    e_gt = max(e_t, e_z) + 4                           # sc (2), difference, product
    e_d1 = e_t + e_gt + t                              # dot1 = sum t gt
    e_g1 = max(e_gt, e_t + e_d1 + 1) + 1 + e_dn + 1    # (gt - t dot1) / dn
    e_gxn = e_g1 + 1                                   # + g_zste
    e_y = t / 2 + 2                                    # y = x / dx
    e_d2 = e_y + e_gxn + t                             # dot2 = sum y gxn
    return max(e_gxn, e_y + e_d2 + 1) + 1 + (t / 2 + 1) + 1 + 1      # (gxn - y dot2) / dx, eps


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------

def to_dtype(a: np.ndarray, dtype: str) -> torch.Tensor:
    """fp32 values as a tensor of the case's dtype; bf16 inputs are rounded HERE, once, and are exact from then on."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return t.bfloat16() if dtype == 'bf16' else t


def tokens(kind: str, seed: int, N: int, K: int) -> np.ndarray:
    g = synth.rng(seed)
    if kind == 'same':
        return np.full(N, K - 1, np.int64)
    if kind == 'distinct':
        assert N <= K
        return g.permutation(K)[:N].astype(np.int64)
    if kind == 'zipf':
        return np.minimum(g.zipf(1.3, N) - 1, K - 1).astype(np.int64)
    if kind == 'uniform':
        return g.integers(0, K, N).astype(np.int64)
    raise ValueError(kind)


def upstream(mix: str, seed: int, N: int, D: int) -> Optional[np.ndarray]:
    """Gradient of the straight-through output: None (loss only), at the scale of the loss term (commensurate) or N(0,1)."""
    if mix == 'loss':
        return None
    g = synth.normal(seed, N, D)
    if mix == 'commensurate':
        return (g * np.float32(2.0 / (N * D))).astype(np.float32)
    assert mix in ('ste', 'normal')
    return g


def planted_tokens(N: int) -> list:
    """Tokens a broken grid-stride tail would lose: the last one, and the first of the second sweep (the 8 193rd)."""
    out = [N - 1]
    if N > SWEEP:
        out.append(SWEEP)
    return out


# ------------------------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------------------------

@dataclass
class VqCase:
    """ops.vq_backward (form 'tok'), ops.vq_backward_map ('map') or the normalised tail of _VqStep ('norm')."""
    name: str
    N: int
    K: int
    D: int
    dtype: str = 'f32'
    tok: str = 'zipf'
    mix: str = 'commensurate'
    scal: tuple = (1.0, 1.0, 1.0)          # g_cb, g_cm, g_comb (None = not passed)
    beta: float = 0.25
    need_x: bool = True
    need_w: bool = True
    ordered: Optional[bool] = None
    form: str = 'tok'
    hw: int = 0                            # map form: positions per image
    out_dtype: str = 'f32'                 # map form
    g_xn: bool = False                     # norm form: a second consumer of the normalised rows
    seed: int = 100
    zero_rows: tuple = ()                  # norm form: planted rows (all zero / |x| = 1e-13)
    tiny_rows: tuple = ()


def _pat(i: int) -> tuple:
    v = (0.7, 1.3, 0.9)
    return tuple(v[j] if (i >> j) & 1 else None for j in range(3))


VQ_CASES = [
    VqCase('n1_d1', 1, 1, 1, tok='same'),
    VqCase('n3_d3_bf16_lossonly', 3, 7, 3, 'bf16', mix='loss', scal=(1.0, 1.0, None), beta=0.0),
    VqCase('n5_d6_ste_only', 5, 7, 6, tok='distinct', mix='ste', scal=(None, None, None)),
    VqCase('n3_d260_bf16_distinct_ordered', 3, 4096, 260, 'bf16', tok='distinct', ordered=True),
    VqCase('n8191_k1_d30_bf16', 8191, 1, 30, 'bf16', tok='same', scal=(None, None, 1.0)),
    VqCase('n8192_d4_ordered_beta1', 8192, 7, 4, scal=(1.0, None, 1.0), beta=1.0, ordered=True),
    VqCase('n8193_d8_bf16_k4096', 8193, 4096, 8, 'bf16', ordered=False),
    VqCase('n8193_k1_d1', 8193, 1, 1, tok='same'),
    VqCase('n70001_d8_policy', 70001, 7, 8),                                   # policy default: the ordered route
    VqCase('n70001_k1_d6_bf16_lossonly', 70001, 1, 6, 'bf16', tok='same', mix='loss'),
    VqCase('n70001_d3', 70001, 7, 3, scal=(1.0, 1.0, None)),
    VqCase('n8193_k1_d1030', 8193, 1, 1030, tok='same', scal=(None, 1.0, 1.0)),
    VqCase('n8193_d1024_bf16_ordered', 8193, 7, 1024, 'bf16', ordered=True),
    VqCase('n1024_k4096_d256_atomics', 1024, 4096, 256, ordered=False),
    VqCase('n8191_d64_normal_g', 8191, 4096, 64, mix='normal'),
    VqCase('n8193_d64_bf16_x_alone', 8193, 7, 64, 'bf16', need_w=False),
    VqCase('n8193_d64_w_alone_atomics', 8193, 7, 64, need_x=False, ordered=False),
    VqCase('n8193_d64_w_alone_ordered', 8193, 7, 64, need_x=False, ordered=True, mix='loss'),
    VqCase('n5_d1030_bf16', 5, 7, 1030, 'bf16', tok='uniform', mix='loss'),
    VqCase('n8192_d260', 8192, 4096, 260, beta=0.0, scal=(1.0, 1.0, 1.0)),
] + [
    # every None / non-None pattern of (g_cb, g_cm, g_comb), beta and route rotating
    VqCase(f'pattern{i}_{"ordered" if i & 1 else "atomics"}', 8192, 7, 8, 'bf16' if i & 2 else 'f32', scal=_pat(i),
           beta=(0.0, 0.25, 1.0)[i % 3], ordered=bool(i & 1), mix='commensurate' if i else 'ste')
    for i in range(8)
] + [
    VqCase('pattern0_ordered', 8192, 7, 8, scal=(None, None, None), ordered=True, mix='ste'),     # kw == 0 on the ordered route
    VqCase('pattern_cm_only_ordered', 8193, 7, 8, scal=(None, 1.0, None), ordered=True),
]

MAP_CASES = [
    VqCase('map_csplit1_d32', 512, 64, 32, form='map', hw=256, tok='uniform', scal=(None, 1.0, 1.0)),
    VqCase('map_csplit2_d64_bf16x_lossonly', 512, 64, 64, 'bf16', form='map', hw=512, tok='uniform', mix='loss', scal=(None, 1.0, None)),
    VqCase('map_csplit4_d128_bf16out', 768, 64, 128, form='map', hw=256, out_dtype='bf16', tok='uniform', scal=(None, None, 1.0)),
    VqCase('map_csplit8_d256_bf16_bf16', 2048, 64, 256, 'bf16', form='map', hw=1024, out_dtype='bf16', tok='uniform', scal=(None, 1.0, 1.0)),
    VqCase('map_1100tiles_d32_bf16out', 1100 * 256, 64, 32, form='map', hw=256, out_dtype='bf16', tok='uniform', scal=(None, 1.0, 1.0)),
    VqCase('map_odd_d96_bf16x_ste_only', 512, 64, 96, 'bf16', form='map', hw=256, tok='uniform', mix='ste', scal=(None, None, None)),
    VqCase('map_odd_d96_hw512', 1024, 64, 96, form='map', hw=512, tok='uniform', scal=(None, 1.0, None), beta=1.0),
]

NORM_CASES = [       # _VqStep on normalised rows: normalize_rows -> vq_backward -> (+ g_xn) -> normalize_rows_bwd
    VqCase('norm_d8_gxn', 1000, 16, 8, form='norm', tok='uniform', g_xn=True, zero_rows=(0,), tiny_rows=(1,)),
    VqCase('norm_d30_bf16_lossonly', 257, 16, 30, 'bf16', form='norm', tok='uniform', mix='loss', zero_rows=(5,)),
    VqCase('norm_d256_gxn_lossonly', 300, 16, 256, form='norm', tok='uniform', mix='loss', g_xn=True, tiny_rows=(7,)),
]


@dataclass
class KdCase:
    """train_step.vqkd_backward; ``g_xn``: the extra gradient _VqkdStep adds into g_zste."""
    name: str
    N: int
    D: int
    dtype: str = 'f32'
    mix: str = 'commensurate'              # 'loss' = g_zste None, 'ste' = g_loss None
    g_xn: bool = False
    K: int = 16
    seed: int = 300
    plant: bool = True                     # rows 0..3: all zero, |x| = 1e-13, a zero code, a row equal to its code


KD_CASES = [
    KdCase('kd_n1_d5', 1, 5, plant=False),
    KdCase('kd_n7_d8_bf16', 7, 8, 'bf16'),
    KdCase('kd_n31_d8_lossonly', 31, 8, mix='loss'),
    KdCase('kd_n33_d5_bf16', 33, 5, 'bf16'),
    KdCase('kd_n65569_d8_sweep', 2048 * 32 + 33, 8),                  # more than one sweep of the capped grid, L = 8
    KdCase('kd_n15_d12', 15, 12, mix='ste'),
    KdCase('kd_n17_d16_bf16', 17, 16, 'bf16', g_xn=True),
    KdCase('kd_n7_d24_bf16_lossonly', 7, 24, 'bf16', mix='loss'),
    KdCase('kd_n9_d32', 9, 32),
    KdCase('kd_n2048_d32_bf16_gxn', 2048, 32, 'bf16', g_xn=True),
    KdCase('kd_n7_d33', 7, 33),
    KdCase('kd_n5_d64_bf16_ste', 5, 64, 'bf16', mix='ste'),
    KdCase('kd_n8197_d100_sweep', 8197, 100),                         # more than one sweep, wave form
    KdCase('kd_n7_d768_bf16', 7, 768, 'bf16'),
    KdCase('kd_n2049_d768_lossonly_gxn', 2049, 768, mix='loss', g_xn=True),
]


@dataclass
class NbCase:
    name: str
    R: int
    D: int
    dtype: str = 'f32'
    seed: int = 500


NB_CASES = [NbCase('nb_r1_d1', 1, 1), NbCase('nb_r3_d8_bf16', 3, 8, 'bf16'), NbCase('nb_r4_d63', 4, 63),
            NbCase('nb_r5_d64_bf16', 5, 64, 'bf16'), NbCase('nb_r4097_d65', 4097, 65), NbCase('nb_r5_d256', 5, 256),
            NbCase('nb_r3_d1030_bf16', 3, 1030, 'bf16'), NbCase('nb_r4097_d8_bf16', 4097, 8, 'bf16')]


@dataclass
class ElCase:
    name: str
    n: int
    da: str
    db: str
    seed: int = 700


EL_CASES = [ElCase('el_n1_ff', 1, 'f32', 'f32'), ElCase('el_n255_fb', 255, 'f32', 'bf16'), ElCase('el_n255_bf', 255, 'bf16', 'f32'),
            ElCase('el_n255_bb', 255, 'bf16', 'bf16'), ElCase('el_stride_ff', 256 * 2048 + 1, 'f32', 'f32'),
            ElCase('el_stride_bb', 256 * 2048 + 1, 'bf16', 'bf16'), ElCase('el_stride_fb', 256 * 2048 + 1, 'f32', 'bf16'),
            ElCase('el_n1_bf', 1, 'bf16', 'f32')]
EL_SCALE, EL_SCALE_DEV = 0.37, 1.9


# ------------------------------------------------------------------------------------------------------------------
# VQ tail (vq_backward_kernel, vq_backward_map256_kernel, the ordered grad_W kernels, the normalised tail)
# ------------------------------------------------------------------------------------------------------------------

def vq_inputs(c: VqCase) -> dict:
    x, w = synth.make_inputs('normal', c.seed, c.N, c.K, c.D)
    idx = tokens(c.tok, c.seed + 7, c.N, c.K)
    if c.form != 'norm':
        for n in planted_tokens(c.N):                 # the token's whole row sits 2^12 away from its code
            x[n] = w[idx[n]] + np.float32(OUTLIER) * np.sign(x[n] + np.float32(0.5))
    for r in c.zero_rows:
        x[r] = 0.0
    for r in c.tiny_rows:
        x[r] = 0.0
        x[r, 0] = 1e-13
    gz = upstream(c.mix, c.seed + 11, c.N, c.D)
    gxn = None
    if c.g_xn:
        gxn = (synth.normal(c.seed + 13, c.N, c.D) * np.float32(2.0 / (c.N * c.D))).astype(np.float32)
    return dict(x=to_dtype(x, c.dtype), w=torch.from_numpy(w), idx=torch.from_numpy(idx),
                g_zste=None if gz is None else torch.from_numpy(gz), g_xn=None if gxn is None else torch.from_numpy(gxn))


def _scal(v, dtype):
    return None if v is None else torch.tensor(v, dtype=dtype)


def vq_value(c: VqCase, inp: dict, dtype=torch.float64, beta: Optional[float] = None, nd: Optional[float] = None):
    """The scalar whose gradient the kernel returns, from oracle.torch_ref in ``dtype``; returns (grad_x, grad_w).
    ``beta`` / ``nd`` restate it deliberately wrong (mutations): another beta, another divisor of the squared error."""
    beta = c.beta if beta is None else beta
    x = inp['x'].to(dtype).requires_grad_(True)
    w = inp['w'].to(dtype).requires_grad_(True)
    rows = F.normalize(x) if c.form == 'norm' else x
    z = tr.decode(inp['idx'], w)
    total = (x * 0).sum() + (w * 0).sum()
    if inp['g_zste'] is not None:
        total = total + (tr.ste(z, rows) * inp['g_zste'].to(dtype)).sum()
    if inp['g_xn'] is not None:
        total = total + (rows * inp['g_xn'].to(dtype)).sum()
    fix = 1.0 if nd is None else (c.N * c.D) / nd
    g_cb, g_cm, g_comb = (_scal(v, dtype) for v in c.scal)
    if g_cb is not None:
        total = total + g_cb * tr.codebook_loss(z, rows) * fix
    if g_cm is not None:
        total = total + g_cm * tr.commitment_loss(z, rows) * fix
    if g_comb is not None:
        total = total + g_comb * tr.vqgan_loss(z, rows, beta) * fix
    gx, gw = torch.autograd.grad(total, (x, w))
    return gx, gw


def _kx_kw_abs(c: VqCase):
    g_cb, g_cm, g_comb = (0.0 if v is None else abs(v) for v in c.scal)
    s = 2.0 / (c.N * c.D)
    return (g_cm + c.beta * g_comb) * s, (g_cb + g_comb) * s


def vq_counts(c: VqCase, inp: dict) -> torch.Tensor:
    return torch.bincount(inp['idx'], minlength=c.K)


def vq_tolerance(c: VqCase, inp: dict):
    """(tol of grad_x [N, D], tol of grad_W [K, D]) in float64."""
    x = inp['x'].double()
    w = inp['w'].double()
    idx = inp['idx']
    kx, kw = _kx_kw_abs(c)
    gz = torch.zeros_like(x) if inp['g_zste'] is None else inp['g_zste'].double().abs()
    m = vq_counts(c, inp)
    if c.form != 'norm':
        a_x = gz + kx * (w[idx].abs() + x.abs())
        a_w = torch.zeros_like(w).index_add_(0, idx, kw * (w[idx].abs() + x.abs()))
        return C_GRAD_X * U * a_x, (c_grad_w(m) * U).unsqueeze(1) * a_w
    nrm = x.norm(dim=1, keepdim=True)
    den = nrm.clamp_min(EPS)
    y = (x / den).abs()
    a_r = gz + kx * (w[idx].abs() + y)
    if inp['g_xn'] is not None:
        a_r = a_r + inp['g_xn'].double().abs()
    clamped = nrm < EPS
    a_x = torch.where(clamped, a_r / den, (a_r + y * (y * a_r).sum(1, keepdim=True)) / den)
    a_w = torch.zeros_like(w).index_add_(0, idx, kw * (w[idx].abs() + y))
    c_w = c_grad_w(m) + tree(c.D) / 2 + 2                       # the rows are fp32 outputs of normalize_rows
    return vq_norm_count(c.D) * U * a_x, (c_w * U).unsqueeze(1) * a_w


def to_map(t: torch.Tensor, c: VqCase) -> torch.Tensor:
    """'(b hw) d -> b d hw': the token form rearranged as the feature map."""
    return t.reshape(c.N // c.hw, c.hw, c.D).permute(0, 2, 1).contiguous()


def half_bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """Half a bf16 ulp (8 significand bits) of |v|, at least that of the smallest normal."""
    e = torch.floor(torch.log2(v.abs().clamp_min(FLOOR)))
    return torch.exp2(e - 8)


def map_tolerance(c: VqCase, ref_tok: torch.Tensor, tol_tok: torch.Tensor) -> torch.Tensor:
    tol = to_map(tol_tok, c)
    if c.out_dtype == 'bf16':
        tol = tol + half_bf16_ulp(to_map(ref_tok, c).abs() + tol)
    return tol


# ------------------------------------------------------------------------------------------------------------------
# VQ-KD tail (vqkd_backward_small_kernel<DT, 8|16|32>, vqkd_backward_kernel<DT>)
# ------------------------------------------------------------------------------------------------------------------

def kd_inputs(c: KdCase) -> dict:
    x = synth.normal(c.seed, c.N, c.D)
    w = synth.unit_rows(synth.normal(c.seed + 1, c.K, c.D))
    idx = tokens('uniform', c.seed + 7, c.N, c.K)
    zero_rows, tiny_rows = (), ()
    if c.plant and c.N >= 7:
        x[0] = 0.0
        x[1] = 0.0
        x[1, c.D - 1] = 1e-13
        w[2] = 0.0
        idx[2] = 2
        idx[3] = 5
        x[3] = w[5]
        zero_rows, tiny_rows = (0,), (1,)
    gz = upstream(c.mix if c.mix != 'ste' else 'commensurate', c.seed + 11, c.N, c.D)
    gxn = None
    if c.g_xn:
        gxn = (synth.normal(c.seed + 13, c.N, c.D) * np.float32(2.0 / (c.N * c.D))).astype(np.float32)
    return dict(x=to_dtype(x, c.dtype), w=torch.from_numpy(w), idx=torch.from_numpy(idx),
                g_zste=None if gz is None else torch.from_numpy(gz), g_xn=None if gxn is None else torch.from_numpy(gxn),
                g_loss=None if c.mix == 'ste' else 0.8, zero_rows=zero_rows, tiny_rows=tiny_rows)


def kd_value(c: KdCase, inp: dict, dtype=torch.float64, nd: Optional[float] = None, loss_scale: float = 1.0,
             drop_gxn: bool = False) -> torch.Tensor:
    x = inp['x'].to(dtype).requires_grad_(True)
    w = inp['w'].to(dtype)
    xn = F.normalize(x)
    z = tr.decode(inp['idx'], w)
    total = (x * 0).sum()
    if inp['g_zste'] is not None:
        total = total + (tr.ste(z, xn) * inp['g_zste'].to(dtype)).sum()
    if inp['g_xn'] is not None and not drop_gxn:
        total = total + (xn * inp['g_xn'].to(dtype)).sum()
    if inp['g_loss'] is not None:
        fix = loss_scale * (1.0 if nd is None else (c.N * c.D) / nd)
        total = total + torch.tensor(inp['g_loss'], dtype=dtype) * tr.commitment_loss(z, xn, norm=True) * fix
    return torch.autograd.grad(total, x)[0]


def _abs_normalize_bwd(v: torch.Tensor, a_g: torch.Tensor) -> torch.Tensor:
    """Magnitude expression of normalize_bwd(v; g) given that of g."""
    nrm = v.norm(dim=1, keepdim=True)
    den = nrm.clamp_min(EPS)
    y = (v / den).abs()
    return torch.where(nrm < EPS, a_g / den, (a_g + y * (y * a_g).sum(1, keepdim=True)) / den)


def kd_tolerance(c: KdCase, inp: dict) -> torch.Tensor:
    x = inp['x'].double()
    w = inp['w'].double()
    xn = F.normalize(x)
    t = F.normalize(xn).abs()
    zn = F.normalize(w[inp['idx']]).abs()
    sc = 0.0 if inp['g_loss'] is None else abs(inp['g_loss']) * 2.0 / (c.N * c.D)
    a_gxn = _abs_normalize_bwd(xn, sc * (t + zn))
    for g in (inp['g_zste'], inp['g_xn']):
        if g is not None:
            a_gxn = a_gxn + g.double().abs()
    return vqkd_count(c.D) * U * _abs_normalize_bwd(x, a_gxn)


# ------------------------------------------------------------------------------------------------------------------
# F.normalize backward alone, (a - b) * scale, sum (a - b)^2, x + (z - x)
# ------------------------------------------------------------------------------------------------------------------

def nb_inputs(c: NbCase) -> dict:
    v = synth.normal(c.seed, c.R, c.D)
    zero_rows, tiny_rows = (), ()
    if c.R >= 3:
        v[0] = 0.0
        v[2] = 0.0
        v[2, c.D // 2] = 1e-13
        zero_rows, tiny_rows = (0,), (2,)
    return dict(v=to_dtype(v, c.dtype), g=torch.from_numpy(synth.normal(c.seed + 1, c.R, c.D)), zero_rows=zero_rows,
                tiny_rows=tiny_rows)


def nb_value(inp: dict, dtype=torch.float64) -> torch.Tensor:
    v = inp['v'].to(dtype).requires_grad_(True)
    return torch.autograd.grad((F.normalize(v) * inp['g'].to(dtype)).sum(), v)[0]


def nb_tolerance(c: NbCase, inp: dict) -> torch.Tensor:
    return c_normalize_bwd(c.D) * U * _abs_normalize_bwd(inp['v'].double(), inp['g'].double().abs())


def unclamped_rows(ref: torch.Tensor, v: torch.Tensor, g: torch.Tensor, rows) -> torch.Tensor:
    """Mutation: the rows' clamp branch (g / eps) replaced by the unclamped formula (g - y (y.g)) / |v|, y = v / |v|."""
    out = ref.clone()
    for r in rows:
        nrm = v[r].norm()
        y = v[r] / nrm
        out[r] = (g[r] - y * (y * g[r]).sum()) / nrm
    return out


def el_inputs(c: ElCase) -> dict:
    return dict(a=to_dtype(synth.normal(c.seed, c.n), c.da), b=to_dtype(synth.normal(c.seed + 1, c.n), c.db))


def el_values(inp: dict, dtype=torch.float64) -> dict:
    """diff = (a - b) * scale * scale_dev, sse = sum (a - b)^2 (elementwise in ``dtype``, summed in float64 as the kernel
    does), ste = a + (b - a) with a in the role of x."""
    a, b = inp['a'].to(dtype), inp['b'].to(dtype)
    scale = torch.tensor(EL_SCALE, dtype=dtype) * torch.tensor(EL_SCALE_DEV, dtype=dtype)
    d = a - b
    return dict(diff=d * scale, sse=(d * d).double().sum().reshape(1), ste=tr.ste(b, a))


def el_tolerances(c: ElCase, inp: dict) -> dict:
    a, b = inp['a'].double().abs(), inp['b'].double().abs()
    d2 = ((inp['a'].double() - inp['b'].double()) ** 2).sum().reshape(1)
    return dict(diff=C_DIFF * U * abs(EL_SCALE * EL_SCALE_DEV) * (a + b),
                sse=(C_SSE * U + c.n * 2.0 ** -53) * d2,
                ste=C_STE * U * (a + (b + a)))


# ------------------------------------------------------------------------------------------------------------------
# mutations: deliberately wrong float64 restatements that the bound must reject
# ------------------------------------------------------------------------------------------------------------------

def swap_channels(t: torch.Tensor, row: int = 0, d: int = 0) -> torch.Tensor:
    out = t.clone()
    out[row, d], out[row, d + 1] = t[row, d + 1], t[row, d]
    return out


def vq_mutations(c: VqCase, inp: dict, gx: torch.Tensor, gw: torch.Tensor) -> dict:
    """name -> (grad_x, grad_w) of every wrong restatement that applies to the case."""
    out = {}
    kx, kw = _kx_kw_abs(c)
    ste_part = torch.zeros_like(gx)
    if c.form != 'norm' and inp['g_zste'] is not None:
        ste_part = inp['g_zste'].double()
    if kx > 0 and c.need_x and c.form != 'norm':
        out['loss_term_x1.01'] = (ste_part + 1.01 * (gx - ste_part), gw)
    if kx > 0 and c.need_x and c.form == 'norm':
        base = vq_value(VqCase(**{**c.__dict__, 'scal': (None, None, None)}), inp)[0]     # everything but the loss term
        out['loss_term_x1.01'] = (base + 1.01 * (gx - base), gw)
    if c.beta == 0.25 and c.scal[2] is not None and c.need_x:
        out['beta_0.26'] = vq_value(c, inp, beta=0.26)
    if kx > 0 or kw > 0:
        out['nd_plus_one'] = vq_value(c, inp, nd=c.N * (c.D + 1.0))
    if kw > 0 and c.need_w and c.form == 'tok':
        for n in planted_tokens(c.N):
            k = int(inp['idx'][n])
            g2 = gw.clone()
            g2[k] -= kw_signed(c) * (inp['w'][k].double() - inp['x'][n].double())
            out[f'dropped_token_{n}'] = (gx, g2)
    if c.D >= 2 and c.need_x:
        out['swapped_channels'] = (swap_channels(gx, min(c.N - 1, 2)), gw)
    if c.form == 'norm':
        g_rows = vq_rows_grad(c, inp)
        if c.zero_rows:
            out['unclamped_zero_row'] = (unclamped_rows(gx, inp['x'].double(), g_rows, c.zero_rows), gw)
        if c.tiny_rows:
            out['unclamped_tiny_row'] = (unclamped_rows(gx, inp['x'].double(), g_rows, c.tiny_rows), gw)
        if c.g_xn:
            out['g_xn_dropped'] = vq_value(c, {**inp, 'g_xn': None})
    return out


def kw_signed(c: VqCase) -> float:
    g_cb, _, g_comb = (0.0 if v is None else v for v in c.scal)
    return (g_cb + g_comb) * 2.0 / (c.N * c.D)


def vq_rows_grad(c: VqCase, inp: dict) -> torch.Tensor:
    """Gradient with respect to the normalised rows (norm form), float64: what normalize_rows_bwd receives."""
    x = inp['x'].double()
    rows = F.normalize(x).requires_grad_(True)
    w = inp['w'].double()
    z = tr.decode(inp['idx'], w)
    total = (rows * 0).sum()
    if inp['g_zste'] is not None:
        total = total + (tr.ste(z, rows) * inp['g_zste'].double()).sum()
    if inp['g_xn'] is not None:
        total = total + (rows * inp['g_xn'].double()).sum()
    _, g_cm, g_comb = (_scal(v, torch.float64) for v in c.scal)
    if g_cm is not None:
        total = total + g_cm * tr.commitment_loss(z, rows)
    if g_comb is not None:
        total = total + g_comb * tr.vqgan_loss(z, rows, c.beta)
    return torch.autograd.grad(total, rows)[0]


def kd_mutations(c: KdCase, inp: dict, gx: torch.Tensor) -> dict:
    out = {}
    if inp['g_loss'] is not None:
        out['loss_term_x1.01'] = kd_value(c, inp, loss_scale=1.01)
        out['nd_plus_one'] = kd_value(c, inp, nd=c.N * (c.D + 1.0))
    if c.D >= 2:
        out['swapped_channels'] = swap_channels(gx, min(c.N - 1, 4))
    if inp['g_xn'] is not None:
        out['g_xn_dropped'] = kd_value(c, inp, drop_gxn=True)
    if inp['zero_rows'] or inp['tiny_rows']:
        # gradient with respect to xn = F.normalize(x), float64: what the second normalize backward receives
        x = inp['x'].double()
        xn = F.normalize(x).requires_grad_(True)
        z = tr.decode(inp['idx'], inp['w'].double())
        total = (xn * 0).sum()
        for g in (inp['g_zste'], inp['g_xn']):
            if g is not None:
                total = total + (xn * g.double()).sum()
        if inp['g_loss'] is not None:
            total = total + inp['g_loss'] * tr.commitment_loss(z, xn, norm=True)
        g_xn = torch.autograd.grad(total, xn)[0]
        if inp['zero_rows']:
            out['unclamped_zero_row'] = unclamped_rows(gx, x, g_xn, inp['zero_rows'])
        if inp['tiny_rows']:
            out['unclamped_tiny_row'] = unclamped_rows(gx, x, g_xn, inp['tiny_rows'])
    return out


def nb_mutations(c: NbCase, inp: dict, gv: torch.Tensor) -> dict:
    out = {}
    if c.D >= 2:
        out['swapped_channels'] = swap_channels(gv, c.R - 1)
    v, g = inp['v'].double(), inp['g'].double()
    if inp['zero_rows']:
        out['unclamped_zero_row'] = unclamped_rows(gv, v, g, inp['zero_rows'])
    if inp['tiny_rows']:
        out['unclamped_tiny_row'] = unclamped_rows(gv, v, g, inp['tiny_rows'])
    return out


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """A float64 / fp32 value rounded once to bf16 (round to nearest even), returned as float64."""
    return t.to(torch.float32).bfloat16().double() if t.dtype != torch.float64 else _round64_bf16(t)


def _round64_bf16(t: torch.Tensor) -> torch.Tensor:
    m, e = torch.frexp(t)                              # t = m 2^e, 0.5 <= |m| < 1: 8 significand bits -> multiples of 2^-8
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)
