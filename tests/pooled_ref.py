"""The pooled-features contract (include/vqhip.h) restated in numpy fp32, the float64 mean it approximates and the
derived bound between the two.  Shared by test_pooled_cpu.py and test_gpu_pooled.py; not a test.

    s_j = +0.0f;  for p = j, j + 8, .. < HW (increasing):  s_j = s_j + v_p                 (j = 0 .. 7)
    out = (((s_0 + s_1) + (s_2 + s_3)) + ((s_4 + s_5) + (s_6 + s_7))) / (float)HW
"""
import numpy as np

PARTIALS = 8
U = 2.0 ** -24                              # unit roundoff of fp32
TINY = float(np.finfo(np.float32).tiny)     # the smallest normal fp32: the bound's absolute floor

HW_CASES = (1, 7, 8, 9, 196, 256)
KD_CASES = ((64, 1), (64, 6), (512, 8), (512, 32), (300, 100), (16384, 256), (128, 768), (64, 1028))


def pooled(v: np.ndarray) -> np.ndarray:
    """v fp32 [B, HW, C] (the decoded value of every position) -> out fp32 [B, C], every operation an fp32 IEEE one."""
    v = np.asarray(v)
    assert v.dtype == np.float32 and v.ndim == 3
    B, HW, C = v.shape
    with np.errstate(all='ignore'):
        s = np.zeros((PARTIALS, B, C), dtype=np.float32)
        for p in range(HW):
            s[p % PARTIALS] = s[p % PARTIALS] + v[:, p, :]
        total = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))
        out = total / np.float32(HW)
    assert out.dtype == np.float32
    return out


def pooled_tokens(e: np.ndarray, quant: np.ndarray) -> np.ndarray:
    """The contract on a codebook e fp32 [K, D] and tokens [B, HW]: an image with a token outside [0, K) is NaN in every channel."""
    K = e.shape[0]
    quant = np.asarray(quant).astype(np.int64)
    ok = (quant >= 0) & (quant < K)
    out = pooled(e[np.where(ok, quant, 0)])
    out[~ok.all(axis=1)] = np.nan
    return out


def mean64(v: np.ndarray) -> np.ndarray:
    """The float64 mean over the positions of v [B, HW, C]."""
    with np.errstate(all='ignore'):
        return np.asarray(v, dtype=np.float64).mean(axis=1)


def bound(v: np.ndarray) -> np.ndarray:
    """|out - mean64| <= (HW + 2) * 2^-24 * (sum_p |v_p|) / HW + the smallest normal fp32, per (b, c): at most HW - 1 rounded
    additions and one rounded division (the standard bound, with one unit to spare for the second-order terms)."""
    v = np.asarray(v, dtype=np.float64)
    HW = v.shape[1]
    return (HW + 2) * U * np.abs(v).sum(axis=1) / HW + TINY


def grad_bound(quant: np.ndarray, g: np.ndarray, K: int) -> np.ndarray:
    """Per-entry bound [K, D] of the pooled backward grad_e[k, c] = sum over the n_k contributions of g[b, c] / HW:
    (n_k + 2) * 2^-24 * sum |g[b, c]| / HW (one rounded division each, at most n_k - 1 rounded additions, in any order)."""
    quant = np.asarray(quant).astype(np.int64).reshape(quant.shape[0], -1)
    g = np.abs(np.asarray(g, dtype=np.float64))
    B, HW = quant.shape
    n = np.zeros(K)
    acc = np.zeros((K, g.shape[1]))
    for b in range(B):
        t = quant[b][(quant[b] >= 0) & (quant[b] < K)]
        np.add.at(n, t, 1.0)
        np.add.at(acc, t, g[b] / HW)
    return (n[:, None] + 2) * U * acc
