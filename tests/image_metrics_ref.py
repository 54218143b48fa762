"""The reference of the reconstruction-metric tests (vqhip_image_metrics of include/vqhip.h), in numpy and scipy:

(a) ``decode``            the reference's own expression (vq/datasets/base.py:70-73) on CPU torch, in the tensor's dtype;
(b) ``metrics``           the header's definition from exact integer sums, evaluated in float64;
(c) ``ssim_restated``     an independent line-by-line restatement of the default path of scikit-image's
                          ``structural_similarity(im1, im2, channel_axis=0, data_range=1)`` over ``scipy.ndimage.uniform_filter``
                          in float64 (scikit-image itself runs that filter in float32 for float32 images).

and the case generators the CPU and GPU tests share.  scikit-image is not needed."""
import functools

import numpy as np
import torch
from scipy import ndimage

T = 32                                        # VQHIP_IMAGE_METRICS_TILE
# the smallest shapes at which the kernel can still go wrong: one window; no multiple of anything; a tile boundary inside the
# halo; more than one tile each way; one more than a tile each way with a full halo; three tiles down, three windows across
SHAPES = [(7, 7), (8, 23), (16, 20), (33, 65), (T + 1, T + 7), (2 * T + 5, 9)]
CHANNELS = [1, 3, 4]
BATCHES = [1, 5]
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.uint8]
KINDS = ['noise', 'identical', 'black_white', 'near', 'outside', 'boundary']
C1, C2 = (0.01 * 1) ** 2, (0.03 * 1) ** 2
SSIM_BOUND = 2.0 ** -40                       # VQHIP_IMAGE_SSIM_BOUND


def decode(images: torch.Tensor) -> torch.Tensor:
    """(a): vq/datasets/base.py:70-73 as it stands; uint8 tensors are decoded already.  A NaN has no defined byte in torch:
    it is given 0 here, as the header states for the integer sums."""
    if images.dtype == torch.uint8:
        return images
    t = ((images + 1) * 127.5).clamp(0, 255)
    return torch.where(torch.isnan(t), torch.zeros_like(t), t).to(torch.uint8)


def _window_sums(a: np.ndarray) -> np.ndarray:
    """Sums over every 7 x 7 window that lies inside [..., H, W] (int64, exact): [..., H - 6, W - 6]."""
    s = np.zeros(a.shape[:-2] + (a.shape[-2] + 1, a.shape[-1] + 1), dtype=np.int64)
    s[..., 1:, 1:] = a.cumsum(-2).cumsum(-1)
    return s[..., 7:, 7:] - s[..., :-7, 7:] - s[..., 7:, :-7] + s[..., :-7, :-7]


def metrics(p: np.ndarray, q: np.ndarray, ssim: bool = True) -> dict:
    """(b): bytes p, q [B, C, H, W] -> abs_sum, sq_sum (int64), l1, mse, psnr, ssim (float64) per image."""
    p, q = p.astype(np.int64), q.astype(np.int64)
    B, C, H, W = p.shape
    n = C * H * W
    d = p - q
    abs_sum, sq_sum = np.abs(d).sum((1, 2, 3)), (d * d).sum((1, 2, 3))
    out = dict(abs_sum=abs_sum, sq_sum=sq_sum, l1=abs_sum.astype(np.float64) / np.float64(255 * n),
               mse=sq_sum.astype(np.float64) / np.float64(255 * 255 * n))
    with np.errstate(divide='ignore'):
        out['psnr'] = -10.0 * np.log10(out['mse'])
    if ssim:
        sx, sy, sxx, syy, sxy = (_window_sums(a) for a in (p, q, p * p, q * q, p * q))
        ux, uy = sx / (49.0 * 255.0), sy / (49.0 * 255.0)
        den = 49.0 * 48.0 * 255.0 * 255.0
        vx, vy, vxy = (49 * sxx - sx * sx) / den, (49 * syy - sy * sy) / den, (49 * sxy - sx * sy) / den
        S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out['ssim'] = S.mean((2, 3)).mean(1)
    else:
        out['ssim'] = np.full(B, np.nan)
    return out


def ssim_restated(im1: np.ndarray, im2: np.ndarray) -> float:
    """(c): one image pair [C, H, W], float64 in [0, 1]."""
    win_size, K1, K2, data_range = 7, 0.01, 0.03, 1
    per_channel = []
    for x, y in zip(im1.astype(np.float64), im2.astype(np.float64)):
        NP = win_size ** x.ndim
        cov_norm = NP / (NP - 1)                                  # sample covariance
        ux = ndimage.uniform_filter(x, size=win_size)
        uy = ndimage.uniform_filter(y, size=win_size)
        uxx = ndimage.uniform_filter(x * x, size=win_size)
        uyy = ndimage.uniform_filter(y * y, size=win_size)
        uxy = ndimage.uniform_filter(x * y, size=win_size)
        vx = cov_norm * (uxx - ux * ux)
        vy = cov_norm * (uyy - uy * uy)
        vxy = cov_norm * (uxy - ux * uy)
        R = data_range
        c1, c2 = (K1 * R) ** 2, (K2 * R) ** 2
        A1, A2, B1, B2 = 2 * ux * uy + c1, 2 * vxy + c2, ux ** 2 + uy ** 2 + c1, vx + vy + c2
        S = (A1 * A2) / (B1 * B2)
        pad = (win_size - 1) // 2
        per_channel.append(S[pad:-pad, pad:-pad].mean(dtype=np.float64))
    return float(np.mean(per_channel))


def _boundary_values(rng, shape) -> np.ndarray:
    """fp32 values whose decode sits on a truncation boundary: (v + 1) * 127.5 at or next to an integer, from both sides."""
    k = rng.integers(0, 257, size=shape).astype(np.float32)
    v = (k / np.float32(127.5) - np.float32(1.0)).astype(np.float32)
    step = rng.integers(-2, 3, size=shape)
    for s in (1, 2):
        v = np.where(step >= s, np.nextafter(v, np.float32(2.0)), v)
        v = np.where(step <= -s, np.nextafter(v, np.float32(-2.0)), v)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_pair(kind: str, B: int, C: int, H: int, W: int, dtype, seed: int = 0):
    """(pred, image) as NCHW-contiguous CPU tensors of ``dtype``: model-range floats, or bytes for uint8.  Read-only."""
    rng = np.random.default_rng([seed, KINDS.index(kind), B, C, H, W])
    shape = (B, C, H, W)
    if dtype == torch.uint8:
        q = rng.integers(0, 256, size=shape)
        if kind == 'identical':
            p = q.copy()
        elif kind == 'black_white':
            p, q = np.zeros(shape, dtype=np.int64), np.full(shape, 255)
        elif kind == 'near':
            p = np.clip(q + rng.integers(-6, 7, size=shape), 0, 255)
        else:                                                     # 'outside' and 'boundary' have no meaning for bytes: noise
            p = rng.integers(0, 256, size=shape)
        return torch.from_numpy(p.astype(np.uint8)), torch.from_numpy(q.astype(np.uint8))
    q = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    if kind == 'noise':
        p = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    elif kind == 'identical':
        p = q.copy()
    elif kind == 'black_white':
        p, q = np.full(shape, -1.0, dtype=np.float32), np.full(shape, 1.0, dtype=np.float32)
    elif kind == 'near':                                          # at most +-6 levels: 6 / 127.5 in the model's range
        p = (q + rng.uniform(-6.0, 6.0, size=shape).astype(np.float32) / np.float32(127.5)).astype(np.float32)
    elif kind == 'outside':
        p = rng.uniform(-3.0, 3.0, size=shape).astype(np.float32)
        q = rng.choice(np.array([-np.inf, -70000.0, -1.5, -1.0, -0.0, 0.0, 0.5, 1.0, 1.004, 1e30, np.inf], dtype=np.float32), size=shape)
    else:
        p, q = _boundary_values(rng, shape), _boundary_values(rng, shape)
    return torch.from_numpy(p).to(dtype), torch.from_numpy(q).to(dtype)


@functools.lru_cache(maxsize=None)
def expected(kind: str, B: int, C: int, H: int, W: int, dtype, seed: int = 0, ssim: bool = True) -> dict:
    """(b) on the (a)-decoded bytes of ``make_pair``: computed once, shared, read-only."""
    pred, image = make_pair(kind, B, C, H, W, dtype, seed)
    return metrics(decode(pred).numpy(), decode(image).numpy(), ssim)


def grid():
    """(B, C, H, W) over the whole product of the shapes, channels and batches."""
    return [(B, C, H, W) for (H, W) in SHAPES for C in CHANNELS for B in BATCHES]


def ulps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float64 units in the last place; 0 where both are the same infinity or both NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid='ignore'):
        return np.where(same, 0.0, np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))
