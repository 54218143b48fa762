"""Float64 references, derived error bounds, mutations and the case table of the forward-value tests.

A plain helper module in the style of ``tests/backward_ref.py`` (not a conftest, no pytest settings).  It imports numpy,
torch, ``backward_ref`` and ``oracle/torch_ref.py`` only and makes no GPU call of its own: the evaluators run on whatever
device their arguments live on.  ``tests/test_forward_reference_cpu.py`` proves the bounds on the CPU (an fp32 restatement
stays inside, every mutation falls outside) and ``tests/test_gpu_forward.py`` holds the HIP kernels to the same bounds.

What is checked: the loss scalars (``sse`` of ``ops.gather_ste_loss``, ``mse[0..3]`` of ``ops.gather_ste_mse``, the modules'
``loss`` and ``memo['loss']`` entries), the decoded rows and the straight-through output.

**Reference.**  ``oracle.torch_ref`` (``decode``, ``ste``, ``codebook_loss``, ``commitment_loss(norm=...)``, ``vqgan_loss``) in
``torch.float64`` on the same fp32 / bf16 input values (bf16 widens exactly), on the tokens AS GIVEN (the argmin is never
re-derived).

**Exact outputs.**  ``z == e[idx]`` bit for bit.  ``z_ste == fl(x + fl(z - x))`` bit for bit: one fp32 subtraction and one fp32
addition, no product next to them, so nothing can be contracted; plain torch fp32 ``x + (z - x)`` gives the same bits.
``mse[2] == fl(mse[0] + fl(beta * mse[1]))`` bit for bit from the returned ``mse[0]`` (the library is built with
``-ffp-contract=off``: the product and the sum round separately, as the reference's two ops do).

**Bound on a loss scalar** (u = 2^-24; every summand is a square, so the bound is relative to the float64 value ``ref``):

    |got - ref| <= (c u + n 2^-53) ref + half_ulp_fp32(ref)

* ``gather_ste_loss_kernel`` vector form (D % 4 == 0), per group of four elements: ``d = fl(z - x)`` carries 1 rounding relative
  to z - x, so d^2 carries 2; ``fl(d * d)`` adds 1: 3 per square.  ``fl(d0^2 + d1^2)`` adds 1 to both of its squares, and so does
  the other pair; ``fl(pair + pair)`` adds 1: **c = 5**.  Scalar form (D % 4 != 0): the square alone, **c = 3**; so is
  ``diff_kernel``'s sum of squares that the hook-by-hook route takes (``backward_ref.C_SSE``).  ``c_plain(D)`` returns the count of
  the form the fused kernel runs at that D; it covers the hook-by-hook route, whose count is never larger.
* From there on the kernel works in double: each lane's running sum, the 6 shuffle levels, the 16 wave sums, one atomic per
  workgroup in any order, the division by N D (exact as a double product).  A sum of n non-negative terms in any order is within
  (n - 1) 2^-53 of the exact sum, relative; the division adds one more: the ``n 2^-53`` term, n = N D.  It is kept although it
  is far below c u (3e-9 at the largest case).
* The cast to fp32 (``mse[0]``, ``mse[1]``) is one rounding of the double mean: half an fp32 ulp.  It is taken at ``ref`` as the
  contract states it; where the double mean and ``ref`` sit on different sides of a power of two the exact term would be the
  ulp above it.  ``sse`` (a float64 output) has no such term.
* ``mse[2]`` against the float64 ``(1 + beta) m`` where ``mse[0]`` is not visible (a module with VQGANLoss alone): with
  m^ = m + e, |e| <= b, the two fp32 operations give (1 + beta) e + beta m^ d1 + (m^ + w) d2, |d| <= u:
  ``(1 + beta) b + 2 u (1 + beta) (m + b)`` (``combined_bound``).
* Normalised tails (``vqkd_tail_kernel``, ``vqkd_tail_small_kernel<L>``): per element ``df = fl(fl(z / den_z) - fl(x / den_x))``.
  A squared norm is ``tree(D) = ceil(D / 64) + 6`` roundings (``backward_ref.tree``: the fma chain of a lane and the halving tree; the
  L-lane groups are the same tree without its empty levels), the square root halves that and adds 1, the quotient adds 1:
  ``a = tree(D) / 2 + 2`` relative to each normalised element (a row under the eps clamp has den = eps exactly and only the
  quotient's rounding: a is an upper bound there).  The difference does not inherit a relative error (it cancels), so the bound is
  the magnitude expression: E = a u (|zn| + |xn|) + u |df| per element, and the fp32 square adds u (|df| + E)^2:
  ``sum (2 |df| E + E^2 + u (|df| + E)^2) / (N D)``, then the double sum and the cast as above.  ``zn``, ``xn`` are the float64
  ``F.normalize`` of the rows.  The rows the tail reads are the library's own fp32 normalised rows (``memo['x']``, bit-checked
  against the oracle elsewhere); the reference starts from their values, so their own roundings are not in the count.

* Two results that are each within a bound of the same truth (two routes of the library; the kernel and the C oracle) are
  compared under twice the bound (``pair_bound``, ``route_pair_bound``).

Nothing here is tuned to what a kernel returns.

**Mutations** (``mutations``): wrong float64 restatements that a bound must reject — the last row dropped, the last row counted
twice, the elements d >= 4 (D // 4) dropped (D % 4 != 0 only), the last 16-row block dropped, the divisor N D replaced by
(N - 1) D (N = 1: a division by zero, which ``compare`` counts as outside), and a sequential fp32 running sum of the fp32 squares in
place of the double accumulation.  The last one is REQUIRED outside only from N D >= 2^22 on (``SEQ_FP32_FROM``); the CPU test checks
that it is, case by case.  A case whose loss is exactly zero (``tok='exact'``) has no mutation: dropping, repeating or rescaling
summands cannot move a sum of zeros.  There the kernel must return 0.0 exactly.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import backward_ref as br
from backward_ref import Verdict, compare, to_dtype, tokens, tree      # noqa: F401  (the reporting is backward_ref's)
from oracle import synth, torch_ref as tr

U = br.U
D53 = 2.0 ** -53
C_PLAIN_VEC = 5
C_PLAIN_SCALAR = 3
ROWS_PER_BLOCK = 16            # rows one workgroup of the tail kernels takes per sweep
SEQ_FP32_FROM = 1 << 22        # N D from which the sequential fp32 sum must fall outside


def check(got, ref, tol) -> Verdict:
    """``backward_ref.compare`` on scalars: Python floats go in as float64 (``torch.as_tensor`` alone would make them fp32)."""
    f64 = lambda v: v.detach().to(torch.float64) if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64)
    return compare(f64(got).reshape(()), f64(ref).reshape(()), f64(tol).reshape(()))


def c_plain(D: int) -> int:
    return C_PLAIN_VEC if D % 4 == 0 else C_PLAIN_SCALAR


def a_normalize(D: int) -> float:
    return tree(D) / 2 + 2


def half_ulp_fp32(v: float) -> float:
    """Half an fp32 ulp of |v| (0 for 0; the subnormal spacing below 2^-126)."""
    v = abs(float(v))
    if v == 0.0:
        return 0.0
    e = math.frexp(v)[1] - 1                       # v in [2^e, 2^(e+1))
    return 2.0 ** (max(e, -126) - 24)


def loss_bound(ref: float, c: float, n: int, fp32_out: bool = True) -> float:
    """(c u + n 2^-53) ref, plus half an fp32 ulp of ref where the kernel returns the value as fp32."""
    return (c * U + n * D53) * ref + (half_ulp_fp32(ref) if fp32_out else 0.0)


def combined_bound(ref_m: float, b_m: float, beta: float) -> float:
    """Bound of fl(m^ + fl(beta m^)) against (1 + beta) ref_m, given |m^ - ref_m| <= b_m."""
    return (1.0 + beta) * b_m + 2.0 * U * (1.0 + beta) * (ref_m + b_m)


def pair_bound(ref: float, c: float, n: int) -> float:
    """Two values that are each within ``loss_bound`` of the same float64 truth differ by at most twice that bound.  ``ref`` is one
    of the two, not the truth: the truth is within 2^-20 of it, relative, so the bound is evaluated there."""
    return 2.0 * loss_bound(abs(ref) * (1.0 + 2.0 ** -20), c, n)


def route_pair_bound(loss: float, D: int, n: int) -> float:
    """``pair_bound`` for a plain loss term two routes of the library return (the mean, or VQGANLoss's combination of it): c_plain(D)
    + 2 for the combination's two roundings, and the mean's half ulp scaled by (1 + beta) <= 2 is at most one more half ulp of
    the (larger) combined value."""
    at = abs(loss) * (1.0 + 2.0 ** -20)
    return 2.0 * (loss_bound(at, c_plain(D) + 2, n) + half_ulp_fp32(at))


def combine_fp32(m0, beta: float) -> np.float32:
    """fl(m0 + fl(beta * m0)) in fp32, two roundings (VQGANLoss.forward: losses.py:126)."""
    m0 = np.float32(m0)
    return np.float32(m0 + np.float32(np.float32(beta) * m0))


# ------------------------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class FwdCase:
    """tail: 'plain' (ops.gather_ste_loss: sse), 'plain_mse' (ops.gather_ste_mse: the ticket form with beta), 'normalised' (the
    VQ-KD tails: F.normalize on both sides); the module-level kinds are the rows of MODULE_CONFIGS.
    tok: 'uniform', 'same' (K = 1: every token the same code), 'exact' (x == e[idx]: the loss is exactly 0)."""
    name: str
    N: int
    K: int
    D: int
    dtype: str = 'f32'
    tok: str = 'uniform'
    scale: float = 1.0
    tail: str = 'plain'
    beta: float = 0.25
    seed: int = 900
    zero_rows: tuple = ()
    tiny_rows: tuple = ()


def _shape(n, k, d, dtype='f32', tok='uniform', scale=1.0, beta=0.25):
    tag = f'n{n}_d{d}_{dtype}' + ('' if tok == 'uniform' else f'_{tok}') + ('' if scale == 1.0 else f'_x{scale:g}')
    return [FwdCase(f'{tag}_{tail}', n, k, d, dtype, tok, scale, tail, beta, seed=900 + 13 * i)
            for i, tail in enumerate(('plain', 'plain_mse'))]


# Geometry of gather_ste_loss_kernel: 16 rows per workgroup, at most 256 workgroups (4096 rows per sweep), 64 lanes x 4 elements
# per step.  N: one row; a partial block; one row into a second block; one row into the grid-stride sweep; two sweeps plus one.
# D: scalar form narrower than a wave; minimal vector form; scalar; vector with a partial last step; exact; one lane into a second
# step; scalar multi-step.  Every N and every D appears with either dtype.
TAIL_CASES = sum([
    _shape(1, 7, 3),
    _shape(15, 7, 4, scale=1e-3),
    _shape(17, 64, 30, scale=1e3, beta=1.0),
    _shape(4097, 512, 252),
    _shape(8193, 512, 256),
    _shape(17, 1, 260, tok='same'),
    _shape(4097, 64, 1030),
    _shape(1, 7, 256, 'bf16'),
    _shape(15, 64, 30, 'bf16', scale=1e3),
    _shape(17, 1, 4, 'bf16', tok='same', beta=0.0),
    _shape(4097, 7, 3, 'bf16'),
    _shape(8193, 512, 260, 'bf16', scale=1e-3),
    _shape(15, 7, 252, 'bf16'),
    _shape(8193, 64, 1030, 'bf16'),
    _shape(17, 64, 256, tok='exact'),
    _shape(4097, 64, 30, 'bf16', tok='exact'),
    _shape(4111, 512, 260, 'bf16'),               # beyond the named Ns: a 15-row last block in the second sweep (last block != last row)
], [])

# The streamed form: both outputs of 98 321 x 256 fp32 are 201 361 408 bytes, just over the 192 MiB (201 326 592) from which
# gather_ste_impl streams (non-temporal accesses, grid cap 512); N is 16 * 6145 + 1.
STREAM_N, STREAM_K, STREAM_D = 98321, 512, 256
STREAM_CASES = [FwdCase(f'n{STREAM_N}_d{STREAM_D}_{dt}_{tail}', STREAM_N, STREAM_K, STREAM_D, dt, tail=tail, seed=950 + i)
                for i, (dt, tail) in enumerate([('f32', 'plain'), ('f32', 'plain_mse'), ('bf16', 'plain'), ('bf16', 'plain_mse')])]

# The VQ-KD tails: L lanes per row at D = 8, 16, 24 (idle lanes), 32; a wave per row at D = 64, 768.  Row 0 has norm zero, row 1 a
# norm under the eps clamp of the FIRST normalisation (what reaches the tail is 0.1 long), as backward_ref plants them.
# Every D at every N (the one-call route runs at all three): 63 ends in a ragged group of rows (64 / L rows per wave) and a
# partial workgroup, 3000 is one sweep of several workgroups, 32769 is one row into a further sweep of the 256-workgroup grid
# (L = 8: 32768 rows per sweep; L = 16: 16384; L = 32: 8192; a wave per row: 4096).
NORM_NS, NORM_DS = (63, 3000, 32769), (8, 16, 24, 32, 64, 768)
NORM_CASES = [FwdCase(f'norm_n{n}_d{d}', n, 64, d, tail='normalised', seed=970 + i, zero_rows=(0,), tiny_rows=(1,))
              for i, (d, n) in enumerate((d, n) for d in NORM_DS for n in NORM_NS)]

ALL_CASES = TAIL_CASES + STREAM_CASES + NORM_CASES


def by_name(name: str) -> FwdCase:
    return next(c for c in ALL_CASES if c.name == name)


def inputs(c: FwdCase) -> dict:
    """x [N, D] of the case's dtype, w [K, D] fp32, idx [N] int64 — CPU tensors."""
    x, w = synth.make_inputs('normal', c.seed, c.N, c.K, c.D)
    s = np.float32(c.scale)
    x, w = x * s, w * s
    idx = tokens('same' if c.tok == 'same' else 'uniform', c.seed + 7, c.N, c.K)
    if c.tail == 'normalised':
        # rows as NormalizeCallback leaves them (fp32 unit rows near their codes), a unit codebook
        w = synth.unit_rows(w)
        x = synth.unit_rows(w[idx] + np.float32(0.3) * x)
        for r in c.zero_rows:
            x[r] = 0.0
        for r in c.tiny_rows:                        # F.normalize of a row of norm 1e-13: one element 0.1
            x[r] = 0.0
            x[r, c.D - 1] = 0.1
    if c.tok == 'exact':
        if c.dtype == 'bf16':
            w = synth.bf16_round(w)
        x = w[idx].copy()
    return dict(x=to_dtype(x, c.dtype), w=torch.from_numpy(np.ascontiguousarray(w, np.float32)), idx=torch.from_numpy(idx))


# ------------------------------------------------------------------------------------------------------------------
# float64 evaluator (any device)
# ------------------------------------------------------------------------------------------------------------------

def reference(x: torch.Tensor, w: torch.Tensor, idx: torch.Tensor, tail: str, beta: float = 0.25) -> dict:
    """oracle.torch_ref in float64 from the given values and tokens.  Plain tails: codebook, commitment and VQGAN loss; the
    normalised tail: CommitmentLoss(norm=True).  Python floats."""
    x64, w64 = x.to(torch.float64), w.to(torch.float64)
    z = tr.decode(idx, w64)
    if tail == 'normalised':
        return dict(commitment=float(tr.commitment_loss(z, x64, norm=True)))
    return dict(codebook=float(tr.codebook_loss(z, x64)), commitment=float(tr.commitment_loss(z, x64)),
                vqgan=float(tr.vqgan_loss(z, x64, beta)))


def exact_outputs(x: torch.Tensor, w: torch.Tensor, idx: torch.Tensor):
    """(z, z_ste) the kernels must return bit for bit: the fp32 gather, and plain fp32 add and sub of the same values."""
    x32 = x.to(torch.float32)
    z = tr.decode(idx, w)
    return z, tr.ste(z, x32)


def _rows64(x: torch.Tensor, w: torch.Tensor, idx: torch.Tensor, tail: str, chunk: int = 1 << 15):
    """Per-row float64 sums of the squared differences, and of their part at d >= 4 (D // 4)."""
    D = x.shape[1]
    rows, rest = [], []
    for a in range(0, x.shape[0], chunk):
        xc, zc = x[a:a + chunk].to(torch.float64), w.to(torch.float64)[idx[a:a + chunk]]
        if tail == 'normalised':
            xc, zc = F.normalize(xc), F.normalize(zc)
        sq = (zc - xc) ** 2
        rows.append(sq.sum(1))
        rest.append(sq[:, 4 * (D // 4):].sum(1))
    return torch.cat(rows), torch.cat(rest)


def fp32_squares(x: torch.Tensor, w: torch.Tensor, idx: torch.Tensor, tail: str) -> torch.Tensor:
    """The fp32 squares of the fp32 differences, [N, D], element by element as the kernels form them."""
    x32, z = x.to(torch.float32), w[idx]
    if tail == 'normalised':
        x32, z = F.normalize(x32), F.normalize(z)
    d = z - x32
    return d * d


def restate_fp32(x: torch.Tensor, w: torch.Tensor, idx: torch.Tensor, tail: str) -> float:
    """The mean with the kernel's grouping: fp32 squares, (s0 + s1) + (s2 + s3) in fp32 where the vector form runs, then a
    float64 sum and the division."""
    sq = fp32_squares(x, w, idx, tail)
    N, D = sq.shape
    if tail != 'normalised' and D % 4 == 0:
        g = sq.reshape(N, D // 4, 4)
        sq = (g[..., 0] + g[..., 1]) + (g[..., 2] + g[..., 3])
    return float(sq.to(torch.float64).sum()) / (N * D)


def normalised_bound(x: torch.Tensor, w: torch.Tensor, idx: torch.Tensor, ref: float, chunk: int = 1 << 15) -> float:
    """The magnitude-expression bound of the normalised tails (module docstring), with the double sum and the fp32 cast."""
    N, D = x.shape
    a = a_normalize(D)
    total = 0.0
    w64 = w.to(torch.float64)
    for s in range(0, N, chunk):
        xn, zn = F.normalize(x[s:s + chunk].to(torch.float64)), F.normalize(w64[idx[s:s + chunk]])
        df = (zn - xn).abs()
        E = a * U * (zn.abs() + xn.abs()) + U * df
        total += float((2 * df * E + E * E + U * (df + E) ** 2).sum())
    return total / (N * D) + N * D * D53 * ref + half_ulp_fp32(ref)


# ------------------------------------------------------------------------------------------------------------------
# mutations
# ------------------------------------------------------------------------------------------------------------------

MUTATIONS = ('last_row_dropped', 'last_row_twice', 'tail_elements_dropped', 'last_block_dropped', 'divisor_n_minus_1',
             'sequential_fp32_sum')


def mutations(x: torch.Tensor, w: torch.Tensor, idx: torch.Tensor, tail: str) -> dict:
    """name -> the wrong mean, for every mutation that applies to the shape (tail_elements_dropped: D % 4 != 0)."""
    N, D = x.shape
    rows, rest = _rows64(x, w, idx, tail)
    S = float(rows.sum())
    nd = float(N * D)
    out = {
        'last_row_dropped': (S - float(rows[-1])) / nd,
        'last_row_twice': (S + float(rows[-1])) / nd,
        'last_block_dropped': (S - float(rows[ROWS_PER_BLOCK * ((N - 1) // ROWS_PER_BLOCK):].sum())) / nd,
        'divisor_n_minus_1': S / ((N - 1.0) * D) if N > 1 else math.inf,
    }
    if D % 4 != 0:
        out['tail_elements_dropped'] = (S - float(rest.sum())) / nd
    sq = fp32_squares(x, w, idx, tail).reshape(-1).numpy()
    out['sequential_fp32_sum'] = float(np.cumsum(sq, dtype=np.float32)[-1]) / nd
    return out


def applies(name: str, c: FwdCase) -> bool:
    """The applicability rules of ``mutations``, from the case alone: none at an exactly zero loss, the dropped tail elements at
    D % 4 != 0 only."""
    return c.tok != 'exact' and (name != 'tail_elements_dropped' or c.D % 4 != 0)


def must_reject(name: str, N: int, D: int) -> bool:
    """Whether the bound is required to reject the mutation at this shape (the fp32 running sum: from N D = 2^22 on)."""
    return name != 'sequential_fp32_sum' or N * D >= SEQ_FP32_FROM


# ------------------------------------------------------------------------------------------------------------------
# module-level kinds (tests/test_gpu_forward.py builds them; listed here so that the table is in one place)
# ------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class ModuleKind:
    name: str
    distance: str              # 'L2' | 'Cosine'
    loss: str                  # 'VQGANLoss' | 'CodebookLoss'
    callback: str = ''         # '' | 'NormalizeCallback' | 'CVQVAECallback'
    train: bool = True


MODULE_KINDS = [
    ModuleKind('l2_vqgan_train', 'L2', 'VQGANLoss'),
    ModuleKind('l2_vqgan_eval', 'L2', 'VQGANLoss', train=False),
    ModuleKind('cos_codebook_train', 'Cosine', 'CodebookLoss'),
    ModuleKind('cos_codebook_eval', 'Cosine', 'CodebookLoss', train=False),
    ModuleKind('l2_codebook_normalize_train', 'L2', 'CodebookLoss', 'NormalizeCallback'),
    ModuleKind('l2_vqgan_normalize_eval', 'L2', 'VQGANLoss', 'NormalizeCallback', train=False),
    ModuleKind('cos_vqgan_normalize_train', 'Cosine', 'VQGANLoss', 'NormalizeCallback'),
    ModuleKind('cos_vqgan_normalize_eval', 'Cosine', 'VQGANLoss', 'NormalizeCallback', train=False),
    ModuleKind('cvq_l2_vqgan', 'L2', 'VQGANLoss', 'CVQVAECallback'),
    ModuleKind('cvq_cos_codebook', 'Cosine', 'CodebookLoss', 'CVQVAECallback'),
]
MODULE_SHAPES = [(777, 512, 256, 'bf16'), (1001, 300, 30, 'f32'), (3000, 2048, 64, 'f32')]      # (N, K, D, latent dtype); D = 30: the exact route
