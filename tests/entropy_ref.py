"""Float64 evaluator, derived error bounds, case table and mutations of the fused EntropyLoss tests.

A plain helper module (not a conftest, no pytest settings), in the pattern of ``tests/backward_ref.py``: it imports numpy,
torch, ``oracle`` and ``backward_ref`` only.  ``tests/test_entropy_reference_cpu.py`` proves it on the CPU,
``tests/test_gpu_entropy.py`` holds the HIP route to the same bounds through the same ``compare``.

Definitions (vq/algorithms/vq/losses.py:139-153, mirrored literally):  a = d / T,  p = softmax(a, -1),
H_n = lse_n - sum_k p_nk a_nk,  q_k = (1/N) sum_n p_nk,  L = (1/N) sum_n H_n + sum_k q_k log(q_k + 1e-5);
c_k = log(q_k + 1e-5) + q_k / (q_k + 1e-5),  S_n = sum_k p_nk (c_k - a_nk),  dL/da_nj = (p_nj / N) (c_j - a_nj - S_n),
dL/dd = dL/da / T;  L2:  G = (dL/dd) / d, 0 where d == 0,  dx = x rowsum(G) - G e,  de = e colsum(G) - G^T x;
Cosine:  g_xn = -(dL/dd) en,  g_en = -(dL/dd)^T xn on the normalised operands, then F.normalize's backward.
``evaluate`` computes all of it in float64, chunked over rows, in two sweeps (the statistics, then the gradients).

Tolerances are first-order propagated bounds ``sum |partial derivative| * (bound of the input's error)`` plus
``c * 2^-24 * A`` for the roundings of each step, A = the step's formula with every term replaced by its absolute value.
u = 2^-24.  Counted from ``vector_quantization_amd/csrc`` (nothing is tuned to what a kernel returns):

* the distance (``exact_*_kernel``, MODE 2).  L2: t = (-2 x.e + |x|^2) + |e|^2, d = sqrt(max(t, 0)).  The fp32 MFMA dot is a
  chain of D fma (D u of sum |x_i e_i|), the two norms are ``tree(D)`` sums, two additions follow:
  |dt| <= u [(2 D + 4) sum |x_i e_i| + (tree(D) + 2)(|x|^2 + |e|^2)] =: Delta.  |sqrt(t + dt) - sqrt(t)| <= min(sqrt(Delta),
  Delta / d) exactly (no first-order step: d may be arbitrarily small), plus u d for the square root itself.
  Precondition for an entry with d == 0 in float64 (x_n == e_k): the planted rows are small integers, so the three terms of t are
  exact in fp32 and the kernel's d is 0 as well; the case builder asserts it.
  Cosine: the operands are fp32 outputs of ``normalize_rows`` (tree(D) / 2 + 3 each, as in backward_ref), the dot is D fma,
  1 - s is one rounding: |dd| <= u [(D + tree(D) + 6) sum |xn_i en_i| + 1 + |s|].
* a = d / T: one rounding (IEEE division).  ATen's composition rounds a + 1e-5 once more inside log_softmax; ISSUE: "treat it as
  such and count that rounding": |da| <= |dd| / |T| + 2 u |a|.
* ``entropy_rows_kernel``: m = max a is exact; w = expf(a - m): the subtraction (u |a - m|) and expf (<= 1 ulp in the device
  library's documentation; counted as C_EXP = 2 u) act as a relative error of w.  The sums over K, the logarithm, the quotient
  sum w a / sum w run in double (2^-53 per step, not counted); lse and spa are rounded to fp32 once each.  lse is 1-Lipschitz
  in max_k |da_k|.  ATen sums the K terms in fp32: tree(K) more on lse and on the sum of p (a - lse).
* ``entropy_colsum_kernel``: p = expf(a - lse): relative error da + dlse + u (|a - lse| + C_EXP); the sums over N run in
  double; q and c are stored in fp32 (one rounding each; log in double — the C_LOG = 2 u is for ATen's logf).  ATen's mean
  over N: tree(N).
* ``entropy_grad_kernel``: S = sum p c - spa (sum in double, one rounding), t = (c - a) - S two roundings, scale = inv_nt *
  upstream two roundings, (p * scale) * t two, / d one: 3 u of |c| + |a| + |S| on t and C_MUL = 8 u on the product
  (ATen's chain through softmax_backward and div has no more factors than that).  rowsum / colsum: double sums, one rounding.
* the two contractions are library GEMMs whose summation order is not ours: the worst case over orders, K (for dx) and
  N + number of blocks (for de) additions, as backward_ref takes it for atomics.  It is loose for large K and N.
* F.normalize's backward: ``backward_ref.c_normalize_bwd(D)`` on its own formula, and the error of the incoming gradient
  propagated through the (linear) formula in absolute values.
* a bf16 grad_x adds half a bf16 ulp of the result.
* underflow: an fp32 result below 2^-126 is flushed or rounded on the denormal grid, an absolute error of at most 2^-126 that
  the relative counts above do not see.  A gradient element is a sum of K (grad_x) or N (grad_w) products, each of which —
  and each factor G or g before it, then multiplied by an operand element — can underflow: the absolute floor of the
  gradients' tolerances is 2^-126 (1 + max |operand|) times the number of terms (compare()'s own floor covers one operation).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import backward_ref as br
from oracle import synth

U = br.U
EPS = 1e-5                    # the reference's epsilon inside log(q + eps)
NORM_EPS = 1e-12
C_EXP = 2.0
C_LOG = 2.0
C_MUL = 8.0
tree = br.tree
compare = br.compare

MUTATIONS = ('T_1pct', 'no_eps_in_log', 'no_q_ratio', 'S_without_c', 'mean_over_N_plus_1', 'last_row_dropped_from_q',
             'zero_d_inv_eps', 'softmax_of_minus_a')


@dataclass
class Case:
    name: str
    N: int
    K: int
    D: int
    metric: str = 'L2'
    dtype: str = 'f32'
    T: float = 0.5
    block_rows: Optional[int] = None      # None: the default (one tile of 64 MiB); else forced
    plant: str = 'none'                   # 'equal': x_n == e_k with small integers (L2 d == 0); 'zero': an all-zero latent
    seed: int = 900
    upstream: float = 1.0


# small cases: float64 autograd of oracle.torch_ref is affordable, every mutation is tried (CPU test), and the GPU runs them too
SMALL_CASES = [
    Case('s_n1_k1_d8', 1, 1, 8),
    Case('s_n5_k7_d3_cos_bf16', 5, 7, 3, 'Cosine', 'bf16'),
    Case('s_n24_k20_d8_equal_Tm8', 24, 20, 8, T=-8.0, plant='equal'),
    Case('s_n24_k20_d8_equal_bf16', 24, 20, 8, dtype='bf16', T=-1.0, plant='equal', block_rows=5),
    Case('s_n127_k64_d30_T001', 127, 64, 30, T=0.01, block_rows=50),
    Case('s_n127_k64_d32_cos_zero_Tm1', 127, 64, 32, 'Cosine', T=-1.0, plant='zero', block_rows=127),
    Case('s_n200_k33_d8_cos_T001_bf16', 200, 33, 8, 'Cosine', 'bf16', T=0.01, block_rows=64),
    Case('s_n129_k130_d12_up', 129, 130, 12, upstream=-0.37, block_rows=31),
]

# the ISSUE's grid, pairwise: N in {1, 127, 1000, 8193}, K in {1, 64, 1000, 4096}, D in {8, 30, 32, 256, 768, 1030}, both
# metrics, both dtypes, T in {0.5, 0.01, -1}, block_rows not dividing N / one block, the two planted rows
GPU_CASES = SMALL_CASES + [
    Case('g_n1_k4096_d256_cos', 1, 4096, 256, 'Cosine', T=0.01),
    Case('g_n127_k1_d768_bf16', 127, 1, 768, dtype='bf16', T=-1.0),
    Case('g_n1000_k1000_d30_cos_bf16', 1000, 1000, 30, 'Cosine', 'bf16', T=0.5, block_rows=333),
    Case('g_n1000_k64_d1030_T001', 1000, 64, 1030, T=0.01, block_rows=1000),
    Case('g_n1000_k1000_d32_equal_Tm1', 1000, 1000, 32, T=-1.0, plant='equal', block_rows=7),
    Case('g_n8193_k4096_d256_bf16', 8193, 4096, 256, dtype='bf16', T=0.5, block_rows=3000),
    Case('g_n8193_k64_d8_cos_zero', 8193, 64, 8, 'Cosine', T=-1.0, plant='zero'),
    Case('g_n8193_k1000_d768_cos_T001', 8193, 1000, 768, 'Cosine', T=0.01, block_rows=8192),
    Case('g_n127_k4096_d1030_cos_bf16', 127, 4096, 1030, 'Cosine', 'bf16', T=-1.0, block_rows=100),
    Case('g_n1000_k4096_d8_T001_bf16', 1000, 4096, 8, dtype='bf16', T=0.01),
    Case('g_n8193_k1_d32_cos', 8193, 1, 32, 'Cosine', T=0.5, block_rows=4097),
]

PLANT_ROW, PLANT_CODE = 3, 2


def inputs(c: Case) -> dict:
    x, w = synth.make_inputs('normal', c.seed, c.N, c.K, c.D)
    zero_pairs = []
    if c.plant == 'equal':
        assert c.metric == 'L2' and c.N > PLANT_ROW and c.K > PLANT_CODE
        v = synth.rng(c.seed + 5).integers(1, 4, c.D).astype(np.float32) * np.where(np.arange(c.D) % 2, 1.0, -1.0).astype(np.float32)
        assert c.D * 9 < 2 ** 24               # |v|^2, v.v exact in fp32 in any order: the kernel's t is exactly 0
        x[PLANT_ROW] = v
        w[PLANT_CODE] = v
        zero_pairs = [(PLANT_ROW, PLANT_CODE)]
    if c.plant == 'zero':
        x[min(PLANT_ROW, c.N - 1)] = 0.0
    return dict(x=br.to_dtype(x, c.dtype), w=torch.from_numpy(w), zero_pairs=zero_pairs)


def _normalize(v: torch.Tensor):
    nrm = v.norm(dim=1, keepdim=True)
    den = nrm.clamp_min(NORM_EPS)
    return v / den, nrm, den


def _normalize_bwd(v: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    y, nrm, den = _normalize(v)
    return torch.where(nrm < NORM_EPS, g / den, (g - y * (y * g).sum(1, keepdim=True)) / den)


class _Tile:
    """The float64 distances of a row chunk against the whole codebook, with the bound of their fp32 error."""

    def __init__(self, metric: str, xo: torch.Tensor, eo: torch.Tensor, r0: int, zero_pairs, D: int, tol: bool):
        dot = xo @ eo.t()
        if metric == 'L2':
            xn, en = (xo * xo).sum(1, keepdim=True), (eo * eo).sum(1).unsqueeze(0)
            t = (xn + en - 2 * dot).clamp_min(0)
            for (n, k) in zero_pairs:
                if r0 <= n < r0 + xo.shape[0]:
                    t[n - r0, k] = 0.0
            self.d = t.sqrt()
            if tol:
                delta = U * ((2 * D + 4) * (xo.abs() @ eo.abs().t()) + (tree(D) + 2) * (xn + en))
                safe = self.d.clamp_min(1e-300)
                self.dd = torch.where(self.d > 0, torch.minimum(delta.sqrt(), delta / safe) + U * self.d, torch.zeros_like(delta))
        else:
            self.d = 1 - dot
            if tol:
                self.dd = U * ((D + tree(D) + 6) * (xo.abs() @ eo.abs().t()) + 1 + dot.abs())


def evaluate(c: Case, inp: dict, tol: bool = True, mutation: Optional[str] = None, chunk: int = 1024) -> dict:
    """loss, grad_x [N, D], grad_w [K, D] in float64 (times ``c.upstream``) and, with ``tol``, their tolerances."""
    x, w = inp['x'].double(), inp['w'].double()
    N, K, D = c.N, c.K, c.D
    T = c.T * (1.01 if mutation == 'T_1pct' else 1.0)
    Ts = -T if mutation == 'softmax_of_minus_a' else T
    Nm = N + 1.0 if mutation == 'mean_over_N_plus_1' else float(N)
    eps_log = 0.0 if mutation == 'no_eps_in_log' else EPS
    cos = c.metric == 'Cosine'
    if cos:
        xo, eo = _normalize(x)[0], _normalize(w)[0]
    else:
        xo, eo = x, w
    zp = inp['zero_pairs']
    nblocks = math.ceil(N / (c.block_rows or N))

    # ---- sweep 1: row statistics, q ----
    lse, spa = torch.empty(N, dtype=torch.float64), torch.empty(N, dtype=torch.float64)
    qsum = torch.zeros(K, dtype=torch.float64)
    e_lse, d_spa, d_h = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    dq = torch.zeros(K, dtype=torch.float64)
    for r0 in range(0, N, chunk):
        sl = slice(r0, min(N, r0 + chunk))
        tl = _Tile(c.metric, xo[sl], eo, r0, zp, D, tol)
        a = tl.d / T
        ap = tl.d / Ts
        l = torch.logsumexp(ap, 1, keepdim=True)
        p = (ap - l).exp()
        lse[sl] = l[:, 0]
        sp = (p * a).sum(1, keepdim=True)
        spa[sl] = sp[:, 0]
        pq = p.clone()
        if mutation == 'last_row_dropped_from_q' and sl.stop == N:
            pq[-1] = 0.0
        qsum += pq.sum(0)
        if tol:
            da = tl.dd / abs(T) + 2 * U * a.abs()
            m = a.max(1, keepdim=True)[0]
            el = da.max(1, keepdim=True)[0] + U * ((p * (a - m).abs()).sum(1, keepdim=True) + C_EXP + tree(K)) + U * l.abs()
            ds = ((p * (1 + a - sp).abs() * da).sum(1, keepdim=True)
                  + U * (p * (a - sp).abs() * ((a - m).abs() + C_EXP)).sum(1, keepdim=True) + U * sp.abs())
            e_lse[sl], d_spa[sl] = el[:, 0], ds[:, 0]
            d_h[sl] = (el + ds + U * (tree(K) + 4) * (p * (a - l).abs()).sum(1, keepdim=True))[:, 0]
            rho = da + el + U * ((a - l).abs() + C_EXP + 1)
            dq += (p * rho).sum(0)
    q = qsum / Nm
    lq = torch.log(q + eps_log)
    ratio = torch.zeros_like(q) if mutation == 'no_q_ratio' else q / (q + eps_log)
    cvec = lq + ratio
    H = lse - spa
    loss = H.sum() / Nm + (q * lq).sum()
    out = dict(loss=loss * c.upstream)
    if tol:
        dq = dq / N + U * (tree(N) + 2) * q
        out['tol_loss'] = abs(c.upstream) * (d_h.sum() / N + U * tree(N) * H.abs().sum() / N + (cvec.abs() * dq).sum()
                                             + U * (C_LOG + tree(K) + 3) * (q * lq).abs().sum() + 2 * U * abs(float(loss)))
        dc = (1 / (q + EPS) + EPS / (q + EPS) ** 2) * dq + U * (C_LOG + 3) * (lq.abs() + ratio)

    # ---- sweep 2: gradients ----
    gx = torch.empty(N, D, dtype=torch.float64)
    gw = torch.zeros(K, D, dtype=torch.float64)
    tx, tw = torch.zeros(N, D, dtype=torch.float64), torch.zeros(K, D, dtype=torch.float64)
    colG, colGa, coldG = (torch.zeros(K, dtype=torch.float64) for _ in range(3))
    k_up = c.upstream / (Nm * T)
    ax, ae = xo.abs(), eo.abs()
    op_err = U * (tree(D) / 2 + 3) if cos else 0.0
    for r0 in range(0, N, chunk):
        sl = slice(r0, min(N, r0 + chunk))
        tl = _Tile(c.metric, xo[sl], eo, r0, zp, D, tol)
        a = tl.d / T
        p = (tl.d / Ts - lse[sl].unsqueeze(1)).exp()
        cc = cvec.unsqueeze(0)
        S = (p * (cc - a)).sum(1, keepdim=True)
        if mutation == 'S_without_c':
            S = -(p * a).sum(1, keepdim=True)
        t = cc - a - S
        g = k_up * p * t
        if tol:
            da = tl.dd / abs(T) + 2 * U * a.abs()
            rho = da + e_lse[sl].unsqueeze(1) + U * ((a - lse[sl].unsqueeze(1)).abs() + C_EXP + 1)
            mag = cc.abs() + a.abs()
            Sabs = (p * mag).sum(1, keepdim=True)
            dS = ((p * rho * mag).sum(1, keepdim=True) + (p * dc.unsqueeze(0)).sum(1, keepdim=True) + d_spa[sl].unsqueeze(1)
                  + U * (tree(K) + 2) * Sabs)
            At = mag + Sabs
            dt = dc.unsqueeze(0) + da + dS + 3 * U * At
            gabs = abs(k_up) * p * At
            dg = abs(k_up) * p * (rho * t.abs() + dt) + C_MUL * U * gabs
        if not cos:
            pos = tl.d > 0
            safe = torch.where(pos, tl.d, torch.ones_like(tl.d))
            G = torch.where(pos, g / safe, torch.zeros_like(g))
            if mutation == 'zero_d_inv_eps' and zp:
                # what a kernel without the d == 0 guard (1 / eps in its place) returns: invisible in exact arithmetic
                # (x_n - e_k == 0), so the structure dx = x rowsum(G) - G e is evaluated in fp32 like the kernel's
                G32 = G.float()
                for (n, k) in zp:
                    if sl.start <= n < sl.stop:
                        G32[n - sl.start, k] = float(g[n - sl.start, k]) / EPS
                x32, e32 = xo[sl].float(), eo.float()
                gx[sl] = (x32 * G32.sum(1, keepdim=True) - G32 @ e32).double()
                gw += (e32 * G32.sum(0).unsqueeze(1) - G32.t() @ x32).double()
                continue
            gx[sl] = xo[sl] * G.sum(1, keepdim=True) - G @ eo
            gw -= G.t() @ xo[sl]
            colG += G.sum(0)
            if tol:
                Ga = torch.where(pos, gabs / safe, torch.zeros_like(g))
                dG = torch.where(pos, dg / safe + gabs * tl.dd / safe ** 2 + U * gabs / safe, torch.zeros_like(g))
                GaE = Ga @ ae
                tx[sl] = (ax[sl] * (dG.sum(1, keepdim=True) + 2 * U * Ga.sum(1, keepdim=True)) + dG @ ae + U * (K + 2) * GaE
                          + U * (ax[sl] * Ga.sum(1, keepdim=True) + GaE))
                tw += dG.t() @ ax[sl] + U * (N + nblocks + 2) * (Ga.t() @ ax[sl])
                colGa += Ga.sum(0)
                coldG += dG.sum(0)
        else:
            gx[sl] = -(g @ eo)
            gw -= g.t() @ xo[sl]
            if tol:
                gaE = gabs @ ae
                tx[sl] = dg @ ae + (U * (K + 1) + op_err) * gaE
                tw += dg.t() @ ax[sl] + (U * (N + nblocks + 2) + op_err) * (gabs.t() @ ax[sl])
    if not cos:
        if mutation != 'zero_d_inv_eps' or not zp:
            gw += eo * colG.unsqueeze(1)
        if tol:
            tw += ae * (coldG + 3 * U * colGa).unsqueeze(1) + U * (ae * colGa.unsqueeze(1))
    else:
        if tol:
            # F.normalize's backward: the incoming gradient's error through the linear formula, plus the kernel's own count
            tx = br._abs_normalize_bwd(x, tx) + br.c_normalize_bwd(D) * U * br._abs_normalize_bwd(x, (gx.abs()))
            tw = br._abs_normalize_bwd(w, tw) + br.c_normalize_bwd(D) * U * br._abs_normalize_bwd(w, (gw.abs()))
        gx, gw = _normalize_bwd(x, gx), _normalize_bwd(w, gw)
    out.update(grad_x=gx, grad_w=gw)
    if tol:
        tx = tx + br.FLOOR * K * (1 + float(ae.max()))
        tw = tw + br.FLOOR * N * (1 + float(ax.max()))
        if c.dtype == 'bf16':
            tx = tx + br.half_bf16_ulp(gx.abs() + tx)
        out.update(tol_x=tx, tol_w=tw)
    return out


def autograd_reference(c: Case, inp: dict, dtype=torch.float64) -> dict:
    """``oracle.torch_ref.entropy_loss`` (the reference's composition, torch autograd) in ``dtype``, times ``c.upstream``."""
    from oracle import torch_ref as tr
    r = tr.entropy_loss(inp['x'].to(dtype), inp['w'].to(dtype), c.metric, c.T)
    return dict(loss=r['loss'] * c.upstream, grad_x=r['grad_x'] * c.upstream, grad_w=r['grad_w'] * c.upstream)


def mutations_for(c: Case, inp: dict):
    """The deliberately wrong restatements that can show on the case."""
    out = ['T_1pct', 'softmax_of_minus_a', 'mean_over_N_plus_1']
    if c.K > 1:
        out += ['no_eps_in_log', 'no_q_ratio', 'S_without_c']
    if c.N > 1 and c.K > 1:
        out.append('last_row_dropped_from_q')
    if inp['zero_pairs']:
        out.append('zero_d_inv_eps')
    return out


def verdicts(got: dict, ref: dict, scale: float = 1.0) -> dict:
    """compare() of loss, grad_x, grad_w against ``ref`` (an ``evaluate`` result with tolerances, widened by ``scale``)."""
    gx = got['grad_x']
    if gx.dtype == torch.bfloat16:
        gx = gx.float()
    return dict(loss=compare(got['loss'], ref['loss'], scale * ref['tol_loss']),
                grad_x=compare(gx, ref['grad_x'], scale * ref['tol_x']),
                grad_w=compare(got['grad_w'], ref['grad_w'], scale * ref['tol_w']))
