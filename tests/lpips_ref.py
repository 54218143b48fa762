"""What the LPIPS tests share: a float64 numpy restatement of the definition of vqhip_lpips_fwd / _bwd (include/vqhip.h) and of
its gradient, the bound macros restated from the header, and the case generators.

Features are post-ReLU-like: non-negative, about half of the elements zero; the pixels cycle through KINDS, among them whole
all-zero pixels (pred, target, both), pixels with a norm below 1e-10 and identical pairs.  The weights have mixed sign."""
import numpy as np
import torch

EPS = float(np.float32(1e-10))                              # the fp32 constant the kernels and ATen compare the norm with
U = 2.0 ** -24
CHANNELS = (64, 128, 256, 512, 512)

CS = (1, 3, 64, 65, 512)
BPS = ((1, 1, 1), (2, 5, 7), (3, 9, 29))                    # (B, H, W): P = 1, 35 and 16 * 16 + 5
DTYPES = ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16),
          (torch.float16, torch.float16))
LAYOUTS = ('map', 'rows')
KINDS = 10
PRECISION = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
MIN_EXP = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}


def chain(C: int) -> float:
    """VQHIP_LPIPS_CHAIN(C)."""
    return float(C // 4 + 12)


def bound(C: int, wabs: float) -> float:
    """VQHIP_LPIPS_BOUND(C, wabs)."""
    return (8.0 * chain(C) + 56.0) * U * (1.0 + 2.0 ** -9) * wabs


def grad_bound(C: int, wabs: float, h):
    """VQHIP_LPIPS_GRAD_BOUND(C, wabs, h)."""
    return (16.0 * chain(C) + 136.0) * U * (1.0 + 2.0 ** -9) * wabs * h


def plain_fp32_bound(C: int, wabs: float) -> float:
    """|fp32 evaluation by torch ops - exact| of one layer's share of the value, for ANY order of the sums: the derivation of
    VQHIP_LPIPS_BOUND with the chain replaced by its worst case, a sequential sum (C additions over the channels), one rounding
    for the division where the kernel has two (reciprocal and product), and a sequential fp32 mean over P <= 2^10 pixels of the
    CPU tests (P u of at most 4 wabs, where the kernel's double sum has one rounding)."""
    N = C + 1.0
    return (8.0 * N + 56.0 + 4.0 * 1024.0) * U * (1.0 + 2.0 ** -9) * wabs


def half_ulp(v, dtype):
    """Half a unit in the last place of ``dtype`` at the magnitude of ``v`` (numpy float64 in, out): the rounding of an fp32
    gradient into the output dtype."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    e = np.maximum(np.where(np.isfinite(e), e, 0.0), MIN_EXP[dtype])
    return 0.5 * 2.0 ** (e - (PRECISION[dtype] - 1))


def as64(t: torch.Tensor) -> np.ndarray:
    """A [B, C, *positions] tensor of any layout as float64 [B, C, P] in logical order."""
    return t.detach().cpu().double().reshape(t.shape[0], t.shape[1], -1).numpy()


def reference(f, g, w, mask=None, scale=1.0, eps=EPS):
    """The definition in float64.  f, g [B, C, P]; w [C]; mask [B, C, P] of 0 / 1 (None: all kept), scale = 1 / (1 - p) as the
    fp32 value the kernels use; eps: the fp32 constant by default (float64 torch ops compare with the double 1e-10).
    ``grad_unit`` is d value[b] / d f: multiply by g_out[b]."""
    f, g, w = np.asarray(f, np.float64), np.asarray(g, np.float64), np.asarray(w, np.float64).reshape(-1)
    B, C, P = f.shape
    m = np.ones_like(f) if mask is None else np.asarray(mask, np.float64).reshape(B, C, P) * float(scale)
    with np.errstate(all='ignore'):
        nf_raw, ng_raw = np.sqrt((f * f).sum(1)), np.sqrt((g * g).sum(1))
        clamped = nf_raw < eps                                                  # (a NaN compares false and stays a NaN)
        nf, ng = np.where(clamped, eps, nf_raw), np.where(ng_raw < eps, eps, ng_raw)
        a, b = f / nf[:, None, :], g / ng[:, None, :]
        d = a - b
        mw = m * w[None, :, None]
        s = (mw * d * d).sum(1)
        u = 2.0 * mw * d
        sua = (u * a).sum(1)
        ds = np.where(clamped[:, None, :], u / eps, (u - a * sua[:, None, :]) / nf[:, None, :])
        return dict(s=s, value=s.mean(1), grad_unit=ds / P, h=1.0 / nf, clamped=clamped, a=a, b=b)


def torch_composition(f: torch.Tensor, g: torch.Tensor, w: torch.Tensor, mask=None, scale=1.0) -> torch.Tensor:
    """The reference's lines on one layer with torch ops (vq/tasks/image_reconstruction/losses.py:148,172-176), dropout replaced
    by a given mask: [B]."""
    import torch.nn.functional as F
    a, b = F.normalize(f, p=2, dim=1, eps=1e-10), F.normalize(g, p=2, dim=1, eps=1e-10)
    loss = F.mse_loss(a, b, reduction='none')
    if mask is not None:
        loss = loss * (mask.to(loss.dtype) * scale)
    loss = F.conv2d(loss, w.reshape(1, -1, 1, 1).to(loss.dtype))
    return loss.mean(dim=(1, 2, 3))


def make_layer(C: int, B: int, H: int, W: int, dtypes=(torch.float32, torch.float32), seed: int = 0, layout: str = 'map'):
    """(pred, target, w): CPU feature maps [B, C, H, W] in ``dtypes`` and ``layout`` ('map' NCHW-contiguous, 'rows' channels-last)
    and the fp32 weights [1, C, 1, 1].  Pixel i = b P + p is of kind (i + seed) % KINDS."""
    gen = torch.Generator().manual_seed(1000 * C + 10 * B * H * W + seed)
    P = H * W
    pred = torch.randn(B, C, P, generator=gen).clamp_min(0.0) * 1.5
    target = (pred + 0.5 * torch.randn(B, C, P, generator=gen)).clamp_min(0.0)
    kind = ((torch.arange(B * P) + seed) % KINDS).view(B, 1, P)
    pred = torch.where((kind == 5) | (kind == 7), torch.zeros(()), pred)
    target = torch.where((kind == 6) | (kind == 7), torch.zeros(()), target)
    pred = torch.where(kind == 8, pred * 1e-12, pred)                           # a norm below 1e-10 (exactly zero in fp16)
    pred = pred.to(dtypes[0])
    target = torch.where(kind == 9, pred.float(), target).to(dtypes[1])         # an identical pair where the dtypes agree
    w = torch.randn(C, generator=gen).view(1, C, 1, 1)
    fmt = torch.channels_last if layout == 'rows' else torch.contiguous_format
    return (pred.view(B, C, H, W).contiguous(memory_format=fmt), target.view(B, C, H, W).contiguous(memory_format=fmt), w)


def grad_ok(got: np.ndarray, want: np.ndarray, tol: np.ndarray, dtype) -> np.ndarray:
    """Elementwise: within ``tol``, or - where the expected value is beyond the largest finite number of ``dtype`` - the infinity
    of its sign."""
    fmax = float(torch.finfo(dtype).max)
    with np.errstate(invalid='ignore'):
        near = np.abs(got - want) <= tol
        over = (np.abs(want) + tol >= fmax) & np.isinf(got) & (np.sign(got) == np.sign(want))
    return near | over
