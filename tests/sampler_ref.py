"""numpy restatement of the fused sampler's contract (include/vqhip.h, vqhip_sample_tokens), shared by test_sampler_cpu.py
and test_gpu_sampler.py, and the inputs of the GPU cases (so the CPU suite can check the conditions they rely on).

Exact parts: ``keys`` (the fp32 CFG mix and division, operation by operation as the header writes them), ``topk_set`` (pure
comparison), the order (a, -index).  float64 parts: masses exp(a - max), cumulative shares, the draw.  ``ambiguous`` names the
tokens whose float64 share lies within delta of the top-p threshold: the kernel may cut anywhere inside that run.
"""
import numpy as np

F32 = np.float32


def delta(V: int) -> float:
    """VQHIP_SAMPLE_DELTA(V): 2^-18 + V 2^-39 (derived in include/vqhip.h from the kernel's fixed-point summation)."""
    return 2.0 ** -18 + V * 2.0 ** -39


def round_to(x: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values representable in ``dtype`` ('float32', 'bfloat16', 'float16'), round to nearest even."""
    x = np.asarray(x, dtype=F32)
    if dtype == 'float32':
        return x.copy()
    if dtype == 'float16':
        return x.astype(np.float16).astype(F32)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    out = b.astype(np.uint32).view(F32).copy()
    out[~np.isfinite(x)] = x[~np.isfinite(x)]
    return out


def keys(logits: np.ndarray, cfg_alpha=None, temperature: float = 1.0) -> np.ndarray:
    """a [Ro, V] fp32 of the slice ``logits`` [R, V] (already fp32, exactly): every operation rounded to fp32 on its own."""
    x = np.asarray(logits, dtype=F32)
    with np.errstate(invalid='ignore', over='ignore'):
        if cfg_alpha is not None:
            assert x.shape[0] % 2 == 0
            alpha = F32(cfg_alpha)
            w0 = F32(1.0 - float(alpha))
            unc, cond = x[:x.shape[0] // 2], x[x.shape[0] // 2:]
            a = (w0 * unc).astype(F32) + (alpha * cond).astype(F32)
        else:
            a = x.copy()
        if F32(temperature) != F32(1.0):
            a = (a / F32(temperature)).astype(F32)
        a = (a + F32(0.0)).astype(F32)                     # -0 -> +0
    return a


def bad_rows(logits: np.ndarray, a: np.ndarray, cfg: bool) -> np.ndarray:
    """[Ro] bool: an input or a mixed value is NaN or +inf, or nothing is finite."""
    x = np.asarray(logits, dtype=F32)
    bad_in = np.isnan(x) | (x == np.inf)
    bad_in = bad_in.any(-1)
    if cfg:
        Ro = x.shape[0] // 2
        bad_in = bad_in[:Ro] | bad_in[Ro:]
    bad_a = (np.isnan(a) | (a == np.inf)).any(-1) | ~np.isfinite(a).any(-1)
    return bad_in | bad_a


def topk_set(a_row: np.ndarray, top_k: int) -> np.ndarray:
    """bool [V]: a >= the k-th largest value, k = min(top_k, V); everything when top_k <= 0."""
    V = a_row.shape[0]
    if top_k <= 0:
        return np.ones(V, dtype=bool)
    k = min(int(top_k), V)
    kth = np.partition(a_row, V - k)[V - k]
    return a_row >= kth


def ascending(a_row: np.ndarray) -> np.ndarray:
    """Token indices from the lowest rank to the highest: by a ascending, among equal values the HIGHER index first."""
    idx = np.arange(a_row.shape[0])
    return np.lexsort((-idx, a_row))


def masses(a_row: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """float64 exp(a - max) on ``mask`` (max over the row: the top-ranked token always survives), 0 elsewhere."""
    a64 = a_row.astype(np.float64)
    with np.errstate(over='ignore'):
        m = np.exp(a64 - a64.max())
    return np.where(mask, m, 0.0)


class RowCut:
    """What top-k and top-p leave of one row: ``kept`` bool [V]; ``asc`` the survivors of top-k in ascending rank; ``c`` their
    float64 cumulative shares; ``pos`` the position in ``asc`` of the lowest-ranked kept token; ``run`` = (first, last + 1)
    positions of the ambiguous run at ``delta`` (empty: first == last + 1)."""

    def __init__(self, a_row, top_k, top_p, dlt):
        V = a_row.shape[0]
        self.surv = topk_set(a_row, top_k)
        asc = ascending(a_row)
        self.asc = asc[self.surv[asc]]
        m = masses(a_row, self.surv)
        c = np.cumsum(m[self.asc])
        self.c = c / c[-1]
        n = self.asc.shape[0]
        p32 = float(F32(top_p))
        if 0.0 <= p32 <= 1.0:
            thr = 1.0 - p32
            removed = self.c <= thr
            removed[-1] = False
            self.pos = int(np.argmin(removed))              # first False (removed is a prefix: c is non-decreasing)
            amb = np.abs(self.c[:-1] - thr) <= dlt          # the top-ranked token is never in question
            where = np.nonzero(amb)[0]
            self.run = (int(where[0]), int(where[-1]) + 1) if where.size else (self.pos, self.pos)
            assert where.size == 0 or where[-1] - where[0] + 1 == where.size
        else:
            self.pos = 0
            self.run = (0, 0)
        self.kept = np.zeros(V, dtype=bool)
        self.kept[self.asc[self.pos:]] = True
        self.n = n

    @property
    def ambiguous(self) -> int:
        return self.run[1] - self.run[0]


def ambiguous(c64: np.ndarray, threshold: float, dlt: float) -> np.ndarray:
    """Positions (ascending rank) whose float64 share lies within ``dlt`` of ``threshold``; the top-ranked token excluded."""
    return np.nonzero(np.abs(np.asarray(c64)[:-1] - threshold) <= dlt)[0]


def kept_from_cut(a_row: np.ndarray, cut_value, cut_index: int) -> np.ndarray:
    """The kept set a cut record describes: {a > cut_value} + {a == cut_value, index <= cut_index}."""
    idx = np.arange(a_row.shape[0])
    return (a_row > cut_value) | ((a_row == cut_value) & (idx <= cut_index))


def draw_interval(a_row: np.ndarray, kept: np.ndarray, j: int):
    """float64 [lo, hi] of token j in the cumulative distribution over ``kept`` in index order."""
    m = masses(a_row, kept)
    C = np.cumsum(m)
    Z = C[-1]
    return (C[j] - m[j]) / Z, C[j] / Z


def draw(a_row: np.ndarray, kept: np.ndarray, u: float) -> int:
    """First kept j with C_j > u Z in float64; the last kept token if none."""
    m = masses(a_row, kept)
    C = np.cumsum(m)
    hit = np.nonzero(kept & (C > u * C[-1]))[0]
    return int(hit[0]) if hit.size else int(np.nonzero(kept)[0][-1])


# ---- the inputs of the GPU cases ------------------------------------------------------------------------------------------
VS = (1, 2, 63, 64, 65, 257, 1024, 4099, 16384)
STARTS = (0, 1, 1001)
RS = (1, 2, 6)
DTYPES = ('float32', 'bfloat16', 'float16')
RESIDENT_MAX = 32768                                        # VQ_SAMPLE_RESIDENT_MAX: rows up to this V keep their keys in LDS
BIG_VS = (RESIDENT_MAX, RESIDENT_MAX + 1, 64000)
TOP_KS = (0, 1, 2, 50, 600)                                 # + V and V + 5 per case
TOP_PS = (0.0, 0.5, 0.92, 1.0, 2.0)
TOP_P_KS = (0, 600)                                         # the top-k settings the top-p checks run under
PAD = 7                                                     # row_stride = end + PAD


def scale_of(V: int) -> float:
    """Spread of the logits: every token's share stays above delta(V), so few tokens sit within delta of a threshold."""
    return 2.0 if V <= 257 else (1.0 if V <= 1024 else (0.5 if V <= 16384 else 0.25))


def cases():
    """(V, start, R, dtype, seed): every V with every start and every dtype; R cycles through RS."""
    out, n = [], 0
    for V in VS + BIG_VS:
        for si, start in enumerate(STARTS):
            for di, dtype in enumerate(DTYPES):
                if V in BIG_VS and (si + di) % 3 != 0:      # the long rows: three (start, dtype) pairs each
                    continue
                R = RS[(si + di + n) % 3] if V not in BIG_VS else 2
                out.append((V, start, R, dtype, 3000 + n))
                n += 1
    return out


def make_logits(V, start, R, dtype, seed):
    """The whole fp32 [R, start + V + PAD] matrix of a case, rounded to ``dtype``; columns outside the slice hold large values a
    kernel that read them would show."""
    g = np.random.default_rng(seed)
    full = np.full((R, start + V + PAD), 50.0, dtype=F32)
    full[:, start:start + V] = g.normal(0.0, scale_of(V), size=(R, V)).astype(F32)
    return round_to(full, dtype)
