"""Tensor-level front end of libvqhip: torch tensors in, torch tensors out, every byte of arithmetic in
the HIP library.  torch is used only for device memory and the current HIP stream.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import METRIC_COS, METRIC_COS_BF16, METRIC_L2, check

# 'CosineBF16': cosine as the reference's GPU runs evaluate it under bf16 autocast (include/vqhip.h, VQHIP_METRIC_COS_BF16)
METRICS = {'L2': METRIC_L2, 'Cosine': METRIC_COS, 'CosineBF16': METRIC_COS_BF16,
           METRIC_L2: METRIC_L2, METRIC_COS: METRIC_COS, METRIC_COS_BF16: METRIC_COS_BF16}


_METRIC_NAMES = {METRIC_L2: 'L2', METRIC_COS: 'Cosine', METRIC_COS_BF16: 'CosineBF16'}


def metric_name(metric) -> str:
    """'L2' / 'Cosine' / 'CosineBF16' for a metric given by name or by its include/vqhip.h code."""
    return _METRIC_NAMES[METRICS[metric]]


def coarse_supported(D: int) -> bool:
    """True where the fp16 proposal image exists (D <= 1024, D % 8 == 0: every shipped config)."""
    return 1 <= D <= 1024 and D % 8 == 0


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """hipStream_t of the current stream of the current device.  (The raw accessor: `torch.cuda.current_stream()`
    builds a Stream object per call — 11 us each, five calls per training step in the eager CVQ-VAE profile.)"""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_tensor_device(fn):
    """Run the wrapped op with the first device tensor argument's device current: the launches go to that device's
    current stream, and the per-device kernel attributes (dynamic LDS size) are set for the right device.  A no-op when
    the tensors already live on the current device (the usual one-process-per-GPU case)."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        for a in args:
            t = a.weight if isinstance(a, PreparedCodebook) else a
            if isinstance(t, torch.Tensor) and t.is_cuda:
                if t.device.index != torch.cuda.current_device():
                    with torch.cuda.device(t.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapper


def _require_cuda(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.VqhipError('vector_quantization_amd ops need tensors on an MI355X device (no CPU path)')


def _latents(x: torch.Tensor):
    """Dense row-major [N, D] view of the latents in a dtype the library reads (fp32 or bf16)."""
    if x.dim() != 2:
        raise ValueError(f'expected [N, D] latents, got {tuple(x.shape)}')
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    return x, (_lib.DTYPE_F32 if x.dtype == torch.float32 else _lib.DTYPE_BF16)


def _codebook(e: torch.Tensor) -> torch.Tensor:
    if e.dim() != 2:
        raise ValueError(f'expected [K, D] codebook, got {tuple(e.shape)}')
    e = e.detach()
    if e.dtype != torch.float32:
        e = e.float()
    e = e.contiguous()
    if e.data_ptr() % 16:
        e = e.clone()
    return e


def _bytes(n: int, device) -> torch.Tensor:
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=device)


@dataclass
class PreparedCodebook:
    """Device image produced by vqhip_codebook_prepare (fp16 MFMA fragments, |e|^2, error bounds)."""
    image: torch.Tensor
    weight: torch.Tensor          # the fp32 codebook the image was made from (kept alive for the re-rank)
    K: int
    D: int
    metric: int

    def exact_rows(self) -> Optional[torch.Tensor]:
        """Cosine images: the fp32 rows F.normalize(weight) the exact definition consumes, as a view into the image
        (bit-identical to ``normalize_rows(weight)``); None for L2 (the weight itself is the operand)."""
        if self.metric not in (METRIC_COS, METRIC_COS_BF16):
            return None
        off = _lib.lib().vqhip_codebook_exact_offset(self.K, self.D)
        return self.image[off:off + self.K * self.D * 4].view(torch.float32).view(self.K, self.D)


@_on_tensor_device
def prepare_codebook(e: torch.Tensor, metric='L2') -> PreparedCodebook:
    _require_cuda(e)
    e = _codebook(e)
    K, D = e.shape
    m = METRICS[metric]
    L = _lib.lib()
    image = _bytes(L.vqhip_codebook_bytes(K, D), e.device)
    check(L.vqhip_codebook_prepare(_ptr(e), K, D, m, _ptr(image), image.numel(), _stream()), 'vqhip_codebook_prepare')
    return PreparedCodebook(image, e, K, D, m)


@_on_tensor_device
def argmin(x: torch.Tensor, cb: PreparedCodebook, hist: Optional[torch.Tensor] = None,
           return_stats: bool = False):
    """idx[n] = argmin_k distance(x_n, e_k) — fused fp16 proposal + exact fp32 re-rank.

    For the cosine metric x must already be normalised (``normalize_rows``)."""
    _require_cuda(x)
    x, dt = _latents(x)
    N, D = x.shape
    if D != cb.D:
        raise ValueError(f'latent dim {D} != codebook dim {cb.D}')
    L = _lib.lib()
    idx = torch.empty(N, dtype=torch.int64, device=x.device)
    ws = _bytes(L.vqhip_workspace_bytes(N, cb.K, D), x.device)
    if hist is not None:
        assert hist.dtype == torch.int32 and hist.numel() == cb.K and hist.is_contiguous()
    check(L.vqhip_argmin(_ptr(x), dt, _ptr(cb.weight), _ptr(cb.image), cb.image.numel(), N, cb.K, D, cb.metric, _ptr(idx),
                         _ptr(hist), _ptr(ws), ws.numel(), _stream()), 'vqhip_argmin')
    if return_stats:
        st = torch.zeros(4, dtype=torch.int32, device=x.device)
        if N > 0:
            check(L.vqhip_argmin_stats(_ptr(ws), _ptr(st), _stream()), 'vqhip_argmin_stats')
        return idx, st
    return idx


@_on_tensor_device
def encode(x: torch.Tensor, e: torch.Tensor, metric='L2', hist: Optional[torch.Tensor] = None, zero_hist: bool = False):
    """``prepare_codebook`` + (cosine: ``normalize_rows(x)``) + ``argmin`` as ONE library call with two launches less:
    the training-time encode, where the codebook changes every step.  x are the latents as the quantizer receives them
    (not normalised).  Returns (idx, prepared codebook, xq) — xq = the normalised latents for cosine, None for L2;
    every value is that of the separate calls, bit for bit."""
    _require_cuda(x, e)
    x, dt = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    if D != e.shape[1]:
        raise ValueError(f'latent dim {D} != codebook dim {e.shape[1]}')
    m = METRICS[metric]
    L = _lib.lib()
    image = _bytes(L.vqhip_codebook_bytes(K, D), e.device)
    idx = torch.empty(N, dtype=torch.int64, device=x.device)
    xq = torch.empty(N, D, dtype=torch.float32, device=x.device) if m in (METRIC_COS, METRIC_COS_BF16) else None
    ws = _bytes(L.vqhip_workspace_bytes(N, K, D), x.device)
    if hist is not None:
        assert hist.dtype == torch.int32 and hist.numel() == K and hist.is_contiguous()
    # zero_hist: `hist` may be uninitialised memory — the call's first launch zeroes it (no separate fill kernel)
    check(L.vqhip_encode_ex(_ptr(x), dt, _ptr(e), N, K, D, m, _ptr(image), image.numel(), _ptr(idx), _ptr(hist), _ptr(xq),
                            _ptr(ws), ws.numel(), 1 if (zero_hist and hist is not None) else 0, _stream()), 'vqhip_encode_ex')
    return idx, PreparedCodebook(image, e, K, D, m), xq


@_on_tensor_device
def encode_map(x_map: torch.Tensor, e: torch.Tensor, metric='L2', hist: Optional[torch.Tensor] = None, zero_hist: bool = False):
    """``encode`` for latents given as the NCHW-contiguous feature map [B, D, H, W]: 'b c h w -> (b h w) c' is folded into
    the call's first launch.  Returns (idx int64 [B*H*W], prepared codebook, xrows [B*H*W, D], xq) — xrows = the
    token-major copy of the latents in x's dtype, xq = the normalised fp32 rows (cosine; None for L2)."""
    _require_cuda(x_map, e)
    if x_map.dim() != 4 or not x_map.is_contiguous() or x_map.dtype not in (torch.float32, torch.bfloat16) or x_map.data_ptr() % 16:
        raise ValueError('encode_map expects a contiguous fp32 / bf16 [B, D, H, W] map')
    e = _codebook(e)
    B, D, H, W = x_map.shape
    K = e.shape[0]
    if D != e.shape[1]:
        raise ValueError(f'latent dim {D} != codebook dim {e.shape[1]}')
    m = METRICS[metric]
    L = _lib.lib()
    N = B * H * W
    dt = _lib.DTYPE_F32 if x_map.dtype == torch.float32 else _lib.DTYPE_BF16
    image = _bytes(L.vqhip_codebook_bytes(K, D), e.device)
    idx = torch.empty(N, dtype=torch.int64, device=x_map.device)
    cos = m in (METRIC_COS, METRIC_COS_BF16)
    xrows = torch.empty(N, D, dtype=x_map.dtype, device=x_map.device)
    xq = torch.empty(N, D, dtype=torch.float32, device=x_map.device) if cos else None
    ws = _bytes(L.vqhip_workspace_bytes(N, K, D), x_map.device)
    if hist is not None:
        assert hist.dtype == torch.int32 and hist.numel() == K and hist.is_contiguous()
    check(L.vqhip_encode_map(_ptr(x_map), dt, _ptr(e), B, H * W, K, D, m, _ptr(image), image.numel(), _ptr(idx), _ptr(hist),
                             _ptr(xrows), _ptr(xq), _ptr(ws), ws.numel(), 1 if (zero_hist and hist is not None) else 0, _stream()),
          'vqhip_encode_map')
    return idx, PreparedCodebook(image, e, K, D, m), xrows, xq


@_on_tensor_device
def gather_ste_map(x_rows: Optional[torch.Tensor], e: torch.Tensor, idx: torch.Tensor, B: int, H: int, W: int, beta: float = 0.0):
    """(out_map fp32 [B, D, H, W] NCHW-contiguous, mse fp32[4] or None): the straight-through output x + (e[idx] - x) — or,
    with ``x_rows`` None, the decoded rows e[idx] — written directly as the feature map ('(b h w) c -> b c h w' folded in)."""
    _require_cuda(e, idx)
    e = _codebook(e)
    D = e.shape[1]
    idx = idx.reshape(-1).contiguous()
    N = B * H * W
    assert idx.dtype == torch.int64 and idx.numel() == N and N > 0
    out = torch.empty(B, D, H, W, dtype=torch.float32, device=e.device)
    mse = None
    dt = _lib.DTYPE_F32
    scratch = None
    if x_rows is not None:
        x_rows, dt = _latents(x_rows)
        assert tuple(x_rows.shape) == (N, D)
        mse = torch.empty(4, dtype=torch.float32, device=e.device)
        scratch = _mse_scratch(e.device)
    check(_lib.lib().vqhip_gather_ste_map(_ptr(x_rows), dt, _ptr(e), _ptr(idx), B, H * W, D, _ptr(out), _ptr(mse), float(beta),
                                          _ptr(scratch), _stream()), 'vqhip_gather_ste_map')
    return out, mse


@_on_tensor_device
def argmin_exact(x: torch.Tensor, e: torch.Tensor, metric='L2', hist: Optional[torch.Tensor] = None,
                 return_min: bool = False):
    """Same contract as ``argmin`` evaluated entirely with fp32 MFMA (x, e normalised by the caller for cosine)."""
    _require_cuda(x, e)
    x, dt = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    L = _lib.lib()
    idx = torch.empty(N, dtype=torch.int64, device=x.device)
    dmin = torch.empty(N, dtype=torch.float32, device=x.device) if return_min else None
    ws = _bytes(L.vqhip_workspace_bytes(N, K, D), x.device)
    check(L.vqhip_argmin_exact(_ptr(x), dt, _ptr(e), N, K, D, METRICS[metric], _ptr(idx), _ptr(dmin), _ptr(hist),
                               _ptr(ws), ws.numel(), _stream()), 'vqhip_argmin_exact')
    return (idx, dmin) if return_min else idx


@_on_tensor_device
def distance(x: torch.Tensor, e: torch.Tensor, metric='L2', out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Materialised d[N, K] (memo['distance']); x, e normalised by the caller for cosine.  ``out``: a dense fp32 [N, K]
    buffer to fill instead of a new one (the row blocks of ``entropy_loss``)."""
    _require_cuda(x, e)
    x, dt = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    L = _lib.lib()
    if out is not None:
        assert out.dtype == torch.float32 and tuple(out.shape) == (N, K) and out.is_contiguous() and out.device == x.device
    d = out if out is not None else torch.empty(N, K, dtype=torch.float32, device=x.device)
    ws = _bytes(L.vqhip_workspace_bytes(N, K, D), x.device)
    check(L.vqhip_distance(_ptr(x), dt, _ptr(e), N, K, D, METRICS[metric], _ptr(d), _ptr(ws), ws.numel(), _stream()),
          'vqhip_distance')
    return d


ENTROPY_TILE_BYTES = 64 << 20      # workspace cap of entropy_loss: one [R, K] fp32 tile (stays in the 256 MiB Infinity Cache)


def entropy_block_rows(N: int, K: int, tile_bytes: int = ENTROPY_TILE_BYTES) -> int:
    """Rows per block of ``entropy_loss``: as many as keep the [R, K] fp32 tile within ``tile_bytes`` (at least one)."""
    return max(1, min(int(N), int(tile_bytes) // (4 * int(K))))


def _entropy_args(x, e, metric, temperature, block_rows):
    import math
    _require_cuda(x, e)
    m = METRICS[metric]
    if m not in (METRIC_L2, METRIC_COS):
        raise ValueError(f"entropy_loss: metric must be 'L2' or 'Cosine', got {metric!r}")
    T = float(temperature)
    if T == 0.0 or not math.isfinite(T):
        raise ValueError(f'entropy_loss: the temperature must be finite and non-zero, got {temperature!r}')
    x, _ = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    if D != e.shape[1]:
        raise ValueError(f'latent dim {D} != codebook dim {e.shape[1]}')
    if N < 1 or K < 1:
        raise ValueError('entropy_loss needs N >= 1 and K >= 1')
    R = entropy_block_rows(N, K) if block_rows is None else int(block_rows)
    if R < 1:
        raise ValueError(f'entropy_loss: block_rows must be >= 1, got {block_rows!r}')
    return x, e, m, T, N, K, D, min(R, N)


@_on_tensor_device
def entropy_loss(x: torch.Tensor, e: torch.Tensor, metric='L2', temperature: float = 1.0, block_rows: Optional[int] = None):
    """EntropyLoss (vq/algorithms/vq/losses.py:139-153) of the distances of x [N, D] to e [K, D] without the [N, K] matrix:
    rows go through one [block_rows, K] fp32 tile (default: what fits ``ENTROPY_TILE_BYTES``) — ``distance`` fills it,
    vqhip_entropy_rows reduces it.  x, e normalised by the caller for cosine.  Returns (loss fp32 0-dim, saved) with
    saved = dict(lse[N], spa[N], q[K], c[K], block_rows) for ``entropy_loss_backward``; nothing in it grows with N * K."""
    x, e, m, T, N, K, D, R = _entropy_args(x, e, metric, temperature, block_rows)
    L = _lib.lib()
    dev = x.device
    tile = _bytes(R * K * 4, dev)[:R * K * 4].view(torch.float32)
    ws = _bytes(L.vqhip_entropy_workspace_bytes(R, K), dev)
    lse = torch.empty(N, dtype=torch.float32, device=dev)
    spa = torch.empty(N, dtype=torch.float32, device=dev)
    qacc = torch.empty(K, dtype=torch.float64, device=dev)
    for r0 in range(0, N, R):
        r = min(R, N - r0)
        t = tile[:r * K].view(r, K)
        distance(x[r0:r0 + r], e, m, out=t)
        check(L.vqhip_entropy_rows(_ptr(t), r, K, T, _ptr(lse[r0:]), _ptr(spa[r0:]), _ptr(qacc), 1 if r0 == 0 else 0,
                                   _ptr(ws), ws.numel(), _stream()), 'vqhip_entropy_rows')
    q = torch.empty(K, dtype=torch.float32, device=dev)
    c = torch.empty(K, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    check(L.vqhip_entropy_finish(_ptr(lse), _ptr(spa), _ptr(qacc), N, K, _ptr(q), _ptr(c), _ptr(loss), _stream()),
          'vqhip_entropy_finish')
    return loss.reshape(()), dict(lse=lse, spa=spa, q=q, c=c, block_rows=R)


@_on_tensor_device
def entropy_loss_backward(x: torch.Tensor, e: torch.Tensor, metric, temperature: float, saved: dict,
                          upstream: Optional[torch.Tensor] = None, need_x: bool = True, need_e: bool = True):
    """(grad_x fp32 [N, D], grad_e fp32 [K, D]) of ``entropy_loss`` times the device scalar ``upstream`` (None = 1); an output
    that is not needed is None.  One more sweep of the row blocks: the tile is recomputed, vqhip_entropy_grad overwrites it with
    dL/dd (cosine) or G = dL/dd / d, 0 where d == 0 (L2), and two library GEMMs per block contract it with the operands exactly
    as ``distances._L2Matrix`` / ``_DotMatrix`` do: L2  dx = x rowsum(G) - G e,  de = e colsum(G) - G^T x;
    cosine  dx = -g e,  de = -g^T x.  grad_e is accumulated block by block in block order."""
    x, e, m, T, N, K, D, R = _entropy_args(x, e, metric, temperature, saved['block_rows'])
    L = _lib.lib()
    dev = x.device
    l2 = m == METRIC_L2
    if upstream is not None:
        upstream = upstream.detach().reshape(1).to(device=dev, dtype=torch.float32).contiguous()
    tile = _bytes(R * K * 4, dev)[:R * K * 4].view(torch.float32)
    ws = _bytes(L.vqhip_entropy_workspace_bytes(R, K), dev) if l2 else None
    rowsum = torch.empty(R, dtype=torch.float32, device=dev)
    colacc = torch.empty(K, dtype=torch.float64, device=dev) if l2 else None
    gx = torch.empty(N, D, dtype=torch.float32, device=dev) if need_x else None
    ge = torch.zeros(K, D, dtype=torch.float32, device=dev) if need_e else None
    lse, spa = saved['lse'], saved['spa']
    for r0 in range(0, N, R):
        r = min(R, N - r0)
        t = tile[:r * K].view(r, K)
        xb = x[r0:r0 + r]
        distance(xb, e, m, out=t)
        check(L.vqhip_entropy_grad(_ptr(t), r, K, T, _ptr(lse[r0:]), _ptr(spa[r0:]), _ptr(saved['c']), 1.0 / (N * T),
                                   _ptr(upstream), m, _ptr(rowsum), _ptr(colacc), 1 if r0 == 0 else 0, _ptr(ws),
                                   ws.numel() if ws is not None else 0, _stream()), 'vqhip_entropy_grad')
        xb32 = xb.float()
        if need_x:
            if l2:
                torch.sub(xb32 * rowsum[:r].unsqueeze(1), t @ e, out=gx[r0:r0 + r])
            else:
                torch.neg(t @ e, out=gx[r0:r0 + r])
        if need_e:
            ge.addmm_(t.t(), xb32, alpha=-1.0)
    if need_e and l2:
        ge.add_(e * colacc.float().unsqueeze(1))
    return gx, ge


COL_MULTINOMIAL_MAX_N = _lib.COL_MULTINOMIAL_MAX_N     # rows of col_multinomial: a column's 2^40 fixed-point mass stays below 2^61


def _col_multinomial_args(x, e, metric, u, block_rows):
    """(The checks of shape, dtype and size come first and need no device: a wrong call says what is wrong on any machine.)"""
    m = METRICS[metric]
    if m not in (METRIC_L2, METRIC_COS):
        raise ValueError(f"col_multinomial: metric must be 'L2' or 'Cosine', got {metric!r}")
    x, _ = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    if D != e.shape[1]:
        raise ValueError(f'latent dim {D} != codebook dim {e.shape[1]}')
    if N < 1 or K < 1:
        raise ValueError('col_multinomial needs N >= 1 and K >= 1')
    if N > COL_MULTINOMIAL_MAX_N:
        raise ValueError(f'col_multinomial: N={N} is beyond 2^20 rows')
    if not isinstance(u, torch.Tensor) or u.dtype != torch.float32 or tuple(u.shape) != (K,):
        got = f'{u.dtype} {tuple(u.shape)}' if isinstance(u, torch.Tensor) else type(u).__name__
        raise ValueError(f'col_multinomial: u must be float32 [{K}] (one uniform in [0, 1) per code), got {got}')
    if u.device != x.device:
        raise ValueError(f'col_multinomial: u is on device {u.device}, the latents on {x.device}')
    R = entropy_block_rows(N, K) if block_rows is None else int(block_rows)
    if R < 1:
        raise ValueError(f'col_multinomial: block_rows must be >= 1, got {block_rows!r}')
    _require_cuda(x, e, u)
    return x, e, m, u.contiguous(), N, K, D, min(R, N)


@_on_tensor_device
def col_multinomial(x: torch.Tensor, e: torch.Tensor, metric='L2', *, u: torch.Tensor, block_rows: Optional[int] = None) -> torch.Tensor:
    """MultinomialAnchor indices (vq/algorithms/cvqvae/anchors.py:100) without the [N, K] matrix: for every code k one row n drawn
    with probability softmax_n(+d[n, k]) — the reference's sign: farther latents are likelier — by the inverse-CDF walk of
    include/vqhip.h (vqhip_col_multinomial_*) on the uniforms ``u`` fp32 [K] in [0, 1).  The rows go through one
    [block_rows, K] fp32 tile (default: what fits ``ENTROPY_TILE_BYTES``, as ``entropy_loss``) that ``distance`` fills: once when
    the matrix fits one tile, three times otherwise.  x, e normalised by the caller for cosine.  Returns int64 [K]; -1 for a
    code whose column holds a NaN or a +inf.  A pure function of (x, e, metric, u): not of block_rows or the run."""
    x, e, m, u, N, K, D, R = _col_multinomial_args(x, e, metric, u, block_rows)
    L = _lib.lib()
    dev = x.device
    tile = _bytes(R * K * 4, dev)[:R * K * 4].view(torch.float32)
    ws = _bytes(L.vqhip_col_multinomial_workspace_bytes(N, K, R), dev)
    col_idx = torch.empty(K, dtype=torch.int64, device=dev)
    blocks = range(0, N, R)
    single = len(blocks) == 1                    # the tile stays: one evaluation of the distances serves all three passes

    def fill(r0):
        r = min(R, N - r0)
        t = tile[:r * K].view(r, K)
        distance(x[r0:r0 + r], e, m, out=t)
        return t

    t = None
    for r0 in blocks:
        t = fill(r0)
        check(L.vqhip_col_multinomial_max(_ptr(t), r0, N, K, R, _ptr(ws), ws.numel(), _stream()), 'vqhip_col_multinomial_max')
    for r0 in blocks:
        t = t if single else fill(r0)
        check(L.vqhip_col_multinomial_mass(_ptr(t), r0, N, K, R, _ptr(ws), ws.numel(), _stream()), 'vqhip_col_multinomial_mass')
    check(L.vqhip_col_multinomial_pick(_ptr(u), N, K, R, _ptr(ws), ws.numel(), _ptr(col_idx), _stream()), 'vqhip_col_multinomial_pick')
    for r0 in blocks:
        t = t if single else fill(r0)
        check(L.vqhip_col_multinomial_resolve(_ptr(t), r0, N, K, R, _ptr(ws), ws.numel(), _ptr(col_idx), _stream()),
              'vqhip_col_multinomial_resolve')
    return col_idx


@_on_tensor_device
def col_argmin(x: torch.Tensor, e: torch.Tensor, metric='L2') -> torch.Tensor:
    """NearestAnchor indices: for every code the nearest token (lowest token on ties)."""
    _require_cuda(x, e)
    x, dt = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    L = _lib.lib()
    out = torch.empty(K, dtype=torch.int64, device=x.device)
    ws = _bytes(L.vqhip_col_workspace_bytes(N, K, D), x.device)
    check(L.vqhip_col_argmin(_ptr(x), dt, _ptr(e), N, K, D, METRICS[metric], _ptr(out), _ptr(ws), ws.numel(), _stream()),
          'vqhip_col_argmin')
    return out


@_on_tensor_device
def row_sqnorm(v: torch.Tensor) -> torch.Tensor:
    _require_cuda(v)
    v, dt = _latents(v)
    out = torch.empty(v.shape[0], dtype=torch.float32, device=v.device)
    check(_lib.lib().vqhip_row_sqnorm(_ptr(v), dt, v.shape[0], v.shape[1], _ptr(out), _stream()), 'vqhip_row_sqnorm')
    return out


@_on_tensor_device
def normalize_rows(v: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """F.normalize(v, dim=1) as fp32."""
    _require_cuda(v)
    v, dt = _latents(v)
    out = torch.empty(v.shape, dtype=torch.float32, device=v.device)
    check(_lib.lib().vqhip_normalize_rows(_ptr(v), dt, v.shape[0], v.shape[1], eps, _ptr(out), _stream()),
          'vqhip_normalize_rows')
    return out


@_on_tensor_device
def gather_ste_loss(x: torch.Tensor, e: torch.Tensor, idx: torch.Tensor, need_z: bool = True,
                    need_ste: bool = True, need_sse: bool = True):
    """(z = e[idx], z_ste = x + (z - x), sse = sum (z-x)^2 as a float64[1] tensor); unwanted outputs are None."""
    _require_cuda(x, e, idx)
    x, dt = _latents(x)
    e = _codebook(e)
    idx = idx.reshape(-1).contiguous()
    assert idx.dtype == torch.int64 and idx.numel() == x.shape[0]
    N, D = x.shape
    z = torch.empty(N, D, dtype=torch.float32, device=x.device) if need_z else None
    zs = torch.empty(N, D, dtype=torch.float32, device=x.device) if need_ste else None
    sse = torch.zeros(1, dtype=torch.float64, device=x.device) if need_sse else None
    check(_lib.lib().vqhip_gather_ste_loss(_ptr(x), dt, _ptr(e), _ptr(idx), N, D, _ptr(z), _ptr(zs), _ptr(sse),
                                           _stream()), 'vqhip_gather_ste_loss')
    return z, zs, sse


_MSE_SCRATCH: dict = {}      # (device index, stream) -> 16 zeroed bytes the kernel hands back zeroed


_MSE_SCRATCH_OWNED: list = []    # innermost `owned_mse_scratch` buffer, if any


class owned_mse_scratch:
    """While active, ``gather_ste_mse`` uses ``buf`` (16 zeroed device bytes the caller owns) instead of the per-stream
    cache.  GraphedQuantizer captures with its own buffer: two captured graphs never share a scratch (they could replay
    concurrently on different streams), and no zero-fill is captured into the graph."""

    def __init__(self, buf: torch.Tensor) -> None:
        assert buf.is_cuda and buf.numel() * buf.element_size() >= 16
        self.buf = buf

    def __enter__(self):
        _MSE_SCRATCH_OWNED.append(self.buf)
        return self.buf

    def __exit__(self, *exc):
        _MSE_SCRATCH_OWNED.pop()
        return False


def _mse_scratch(device: torch.device) -> torch.Tensor:
    if _MSE_SCRATCH_OWNED and _MSE_SCRATCH_OWNED[-1].device == device:
        return _MSE_SCRATCH_OWNED[-1]
    key = (device.index, _raw_stream(device.index) if _raw_stream is not None else torch.cuda.current_stream(device).cuda_stream)
    buf = _MSE_SCRATCH.get(key)
    if buf is None:
        buf = _MSE_SCRATCH[key] = torch.zeros(16, dtype=torch.uint8, device=device)
    return buf


@_on_tensor_device
def gather_ste_mse(x: torch.Tensor, e: torch.Tensor, idx: torch.Tensor, need_z: bool = False, need_ste: bool = True,
                   beta: float = 0.0):
    """(z or None, z_ste or None, mse fp32[4]) with mse[0] = mse[1] = mean((e[idx] - x)^2) and mse[2] = mse[0] + beta*mse[1]
    (VQGANLoss): `gather_ste_loss` with the mean finished inside the kernel (no zero-fill, division, cast, scale and add
    kernels around it)."""
    _require_cuda(x, e, idx)
    x, dt = _latents(x)
    e = _codebook(e)
    idx = idx.reshape(-1).contiguous()
    assert idx.dtype == torch.int64 and idx.numel() == x.shape[0] and x.shape[0] > 0
    N, D = x.shape
    z = torch.empty(N, D, dtype=torch.float32, device=x.device) if need_z else None
    zs = torch.empty(N, D, dtype=torch.float32, device=x.device) if need_ste else None
    mse = torch.empty(4, dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_gather_ste_mse(_ptr(x), dt, _ptr(e), _ptr(idx), N, D, _ptr(z), _ptr(zs), _ptr(mse), float(beta),
                                          _ptr(_mse_scratch(x.device)), _stream()), 'vqhip_gather_ste_mse')
    return z, zs, mse


@_on_tensor_device
def hist(idx: torch.Tensor, K: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hist[K] int32 (+)= bincount(idx) of int64 tokens, or of int32 ones (FiniteScalarQuantizer's); only 0 <= k < K counts."""
    _require_cuda(idx)
    idx = idx.reshape(-1).contiguous()
    if out is None:
        out = torch.zeros(K, dtype=torch.int32, device=idx.device)
    if idx.dtype == torch.int32:
        check(_lib.lib().vqhip_hist_i32(_ptr(idx), idx.numel(), K, _ptr(out), _stream()), 'vqhip_hist_i32')
        return out
    assert idx.dtype == torch.int64
    check(_lib.lib().vqhip_hist(_ptr(idx), idx.numel(), K, _ptr(out), _stream()), 'vqhip_hist')
    return out


# ---- FiniteScalarQuantizer (vq/algorithms/fsq/quantizers.py:74-150) --------------------------------------------------------

FSQ_MAX_K = 1 << 24          # the reference's fp32 digit sum is exact up to here


def fsq_check_levels(levels) -> tuple:
    """The levels FiniteScalarQuantizer accepts: 1 <= C <= 16 channels, each level >= 3, product <= 2^24."""
    levels = tuple(int(v) for v in levels)
    if not 1 <= len(levels) <= _lib.FSQ_MAX_C:
        raise ValueError(f'FiniteScalarQuantizer: {len(levels)} channels, expected 1..{_lib.FSQ_MAX_C}')
    bad = [v for v in levels if v < 3]
    if bad:
        raise ValueError(f'FiniteScalarQuantizer: levels {bad} < 3 (the reference divides by zero at 1 and gives NaN at 2)')
    K = 1
    for v in levels:
        K *= v
    if K > FSQ_MAX_K:
        raise ValueError(f'FiniteScalarQuantizer: prod(levels) = {K} > 2^24 (the reference\'s fp32 token sum is no longer exact)')
    return levels


def fsq_constants(levels, eps: float = 1e-3) -> _lib.FsqConstants:
    """vqhip_fsq_t of ``levels``: M and shift = atanh(odd / M) evaluated by the reference's own torch expressions on the host
    (quantizers.py:116-121, max_ = (L - 1) * (1 - eps), odd = (L - 1) % 2, both from the int32 levels tensor)."""
    levels = fsq_check_levels(levels)
    max_per_digit = torch.tensor(levels, dtype=torch.int)
    max_ = (max_per_digit - 1) * (1 - eps)
    odd = (max_per_digit - 1) % 2
    shift = torch.atanh(odd / max_)
    q = _lib.FsqConstants()
    q.struct_bytes = ctypes.sizeof(_lib.FsqConstants)
    q.C = len(levels)
    for i, v in enumerate(levels):
        q.levels[i] = v
        q.shift[i] = float(shift[i])
        q.scale[i] = float(max_[i])
    return q


def _fsq_layout(t: torch.Tensor, C: int, what: str):
    """(layout, N, HW) of fp32 / bf16 latents: [..., C] token-major, or the NCHW-contiguous map [B, C, H, W]."""
    if t.dim() == 4 and t.shape[1] == C and t.is_contiguous():
        b, _, h, w = t.shape
        return _lib.LAYOUT_MAP, b * h * w, max(h * w, 1)
    if t.shape[-1] != C or not t.is_contiguous():
        raise ValueError(f'{what}: expected contiguous [..., {C}] rows or an NCHW-contiguous [B, {C}, H, W] map, got '
                         f'{tuple(t.shape)}')
    return _lib.LAYOUT_ROWS, t.numel() // C, 0


def _float_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.DTYPE_F32
    if t.dtype == torch.bfloat16:
        return _lib.DTYPE_BF16
    raise ValueError(f'FiniteScalarQuantizer latents must be fp32 or bf16, got {t.dtype}')


@_on_tensor_device
def fsq_encode(x: torch.Tensor, q: _lib.FsqConstants, need_z: bool = True, z_rows: bool = False, want_rows: bool = False,
               hist: Optional[torch.Tensor] = None):
    """One launch: (quant int32 [N], z fp32 or None, x_rows or None).  ``x`` is [..., C] rows or an NCHW-contiguous map
    [B, C, H, W]; z comes in x's layout (``z_rows``: token-major [N, C] also for a map); ``want_rows`` (map only) adds the
    token-major copy of x in x's dtype; ``hist`` (int32 [K]) is added to."""
    _require_cuda(x)
    C = q.C
    layout, N, HW = _fsq_layout(x, C, 'fsq_encode')
    dt = _float_dtype(x)
    quant = torch.empty(N, dtype=torch.int32, device=x.device)
    z = None
    if need_z:
        z = torch.empty((N, C) if (z_rows or layout == _lib.LAYOUT_ROWS) else x.shape, dtype=torch.float32, device=x.device)
    rows = torch.empty(N, C, dtype=x.dtype, device=x.device) if (want_rows and layout == _lib.LAYOUT_MAP) else None
    if hist is not None:
        assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.is_cuda
    check(_lib.lib().vqhip_fsq_encode(ctypes.byref(q), _ptr(x), dt, layout, N, HW, _ptr(quant), _ptr(z), int(z_rows), _ptr(rows),
                                      _ptr(hist), _stream()), 'vqhip_fsq_encode')
    if z is not None and layout == _lib.LAYOUT_ROWS:
        z = z.view(x.shape)
    return quant, z, rows


@_on_tensor_device
def fsq_backward(x: torch.Tensor, g: torch.Tensor, q: _lib.FsqConstants) -> torch.Tensor:
    """dL/dx (x's dtype and layout) of the encode's z, from g = dL/dz (x's shape; read as fp32)."""
    _require_cuda(x, g)
    layout, N, HW = _fsq_layout(x, q.C, 'fsq_backward')
    dt = _float_dtype(x)
    g = g.float().contiguous()
    assert g.shape == x.shape
    gx = torch.empty_like(x)
    check(_lib.lib().vqhip_fsq_backward(ctypes.byref(q), _ptr(x), dt, layout, N, HW, _ptr(g), _ptr(gx), _stream()),
          'vqhip_fsq_backward')
    return gx


@_on_tensor_device
def fsq_decode(quant: torch.Tensor, q: _lib.FsqConstants, map_shape: Optional[tuple] = None) -> torch.Tensor:
    """z fp32 of int32 / int64 tokens: [*quant.shape, C], or (``map_shape`` = (B, H, W)) the NCHW map [B, C, H, W]."""
    _require_cuda(quant)
    if quant.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'fsq_decode: tokens must be int32 or int64, got {quant.dtype}')
    flat = quant.reshape(-1).contiguous()
    N = flat.numel()
    C = q.C
    qdt = _lib.DTYPE_I32 if quant.dtype == torch.int32 else _lib.DTYPE_I64
    if map_shape is not None:
        B, H, W = map_shape
        assert B * H * W == N
        z = torch.empty(B, C, H, W, dtype=torch.float32, device=quant.device)
        layout, HW = _lib.LAYOUT_MAP, H * W
    else:
        z = torch.empty(*quant.shape, C, dtype=torch.float32, device=quant.device)
        layout, HW = _lib.LAYOUT_ROWS, 0
    check(_lib.lib().vqhip_fsq_decode(ctypes.byref(q), _ptr(flat), qdt, layout, N, HW, _ptr(z), _stream()), 'vqhip_fsq_decode')
    return z


# ---- what the op families below decide alike about a tensor: float dtype, dense layout, row view, small arguments -----------

FLOAT_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
IMAGE_DTYPES = {**FLOAT_DTYPES, torch.uint8: _lib.DTYPE_U8}
LAYOUTS = {'rows': _lib.LAYOUT_ROWS, 'map': _lib.LAYOUT_MAP}              # channels-last dense / NCHW-contiguous
IMAGE_LAYOUTS = {'rows': _lib.IMAGE_NHWC, 'map': _lib.IMAGE_NCHW}         # the same two in vqhip_image_metrics' enum (codes reversed)


def float_dtype_refusal(name: str, t: torch.Tensor) -> str:
    """'' for fp32 / bf16 / fp16, else the sentence that says so; ``name`` is the subject with its verb ('pred is')."""
    return '' if t.dtype in FLOAT_DTYPES else f'{name} {t.dtype}, not float32, bfloat16 or float16'


def dense_layouts(t: torch.Tensor) -> tuple:
    """The layouts of include/vqhip.h ``t`` is dense in: 'map' (contiguous: NCHW, [B, C], ...) before 'rows' (4-D channels-last)."""
    found = ('map',) if t.is_contiguous() else ()
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        found += ('rows',)
    return found


def dense_layout(t: torch.Tensor):
    """The first of ``dense_layouts(t)`` ('map' where both hold, as for C == 1), None where there is none."""
    found = dense_layouts(t)
    return found[0] if found else None


def dense_refusal(name: str, t: torch.Tensor) -> str:
    """'' where ``t`` is dense in one of the two layouts, else the sentence that says so."""
    return '' if dense_layouts(t) else f'{name} with strides {t.stride()} is neither NCHW-contiguous nor channels-last dense'


def dense(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself where it is dense in one of the two layouts, else a contiguous copy: autograd hands over gradients with any
    strides (the expanded scalar of ``.sum().backward()`` has none but zeros)."""
    return t if dense_layouts(t) else t.contiguous()


def _dense_like(t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """``t`` dense in the layout the kernels read ``like`` in (a copy only where autograd handed over another memory format)."""
    if dense_layout(like) == 'rows':
        return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)
    return t if t.is_contiguous() else t.contiguous()


def _empty_like(x: torch.Tensor, shape) -> torch.Tensor:
    """An uninitialised [B, C, H, W] tensor of ``shape`` in the dtype and dense layout of ``x``."""
    fmt = torch.channels_last if dense_layout(x) == 'rows' else torch.contiguous_format
    return torch.empty(shape, dtype=x.dtype, device=x.device, memory_format=fmt)


def row_view(t: torch.Tensor, name: str):
    """``t`` [..., C] as rows [R, C] read in place: (the VIEW, its row stride in elements), or a string that says why not - no float
    dtype, a strided last dimension, leading dimensions that flatten only by a copy, rows that overlap.  Never a copy.  Nothing
    follows a single row, so its stride counts as at least C.  An empty tensor passes (R = 0 is the caller's to refuse)."""
    if t.dim() < 1 or t.dtype not in FLOAT_DTYPES:
        return f'{name}: {t.dtype} {tuple(t.shape)} is not float32, bfloat16 or float16 with at least one dimension'
    C = t.shape[-1]
    if t.stride(-1) != 1 and C > 1:
        return f'the last dimension of {name} does not have stride 1'
    try:
        rows = t if t.dim() == 2 else t.view(-1, C)
    except RuntimeError:
        return f'{name}: shape {tuple(t.shape)} with strides {t.stride()} does not flatten to rows without a copy'
    stride = rows.stride(0) if rows.shape[0] > 1 else max(rows.stride(0), C)
    if stride < C:
        return f'the rows of {name} overlap (row stride {stride} < {C})'
    return rows, stride


def _refuse(what: str, why: str) -> None:
    if why:
        raise ValueError(f'{what}: {why}')


def _grad_values(g: torch.Tensor, R: int):
    """The incoming gradient as the kernels read it: (fp32, flat, contiguous; 1 where it holds one value per row of R > 1 rows)."""
    g = g.reshape(-1).to(torch.float32).contiguous()
    return g, 1 if g.numel() == R and R > 1 else 0


def _fp32_vector(p: torch.Tensor) -> torch.Tensor:
    """A parameter as the kernels read it: fp32, flat, contiguous (a copy of its few elements only where it is not that already)."""
    return p.detach().reshape(-1).to(torch.float32).contiguous()


def _seed_refusal(seed: torch.Tensor) -> str:
    ok = seed.dtype in (torch.int32, torch.uint32) and seed.numel() == 2 and seed.is_contiguous()
    return '' if ok else f'seed must hold two contiguous 32-bit words on the device, got {seed.dtype} {tuple(seed.shape)}'


# ---- fused token sampler (stage-2 generation, vq/tasks/sequence_modeling/models/samplers.py) -----------------------------

SAMPLE_MAX_V = 1 << 20


def _logit_rows(what: str, logits: torch.Tensor, start: int, end: int):
    """``logits`` [..., V_total] as the kernels read it in place: (rows [R, V_total] as a VIEW, R, the row stride in elements).
    ValueError where ``row_view`` has a reason or [start, end) is not inside the last dimension."""
    view = row_view(logits, 'the logits')
    if not isinstance(view, str) and not 0 <= start < end <= logits.shape[-1]:
        view = f'need 0 <= start < end <= {logits.shape[-1]} (the last dimension), got [{start}, {end})'
    _refuse(what, view if isinstance(view, str) else '')
    return view[0], view[0].shape[0], view[1]


@_on_tensor_device
def sample_tokens(logits: torch.Tensor, start: int, end: int, *, u: torch.Tensor, temperature: float = 1.0, top_k: int = 0,
                  top_p: float = 2.0, cfg_alpha: Optional[float] = None, want_cut: bool = False):
    """One token per row of ``logits[..., start:end]`` in ONE launch (vqhip_sample_tokens of include/vqhip.h): CFG mix
    (``cfg_alpha`` not None: the first half of the rows is unconditional, the second conditional), temperature, top-k
    (``top_k <= 0``: off), top-p (applied iff ``0 <= top_p <= 1``) and the inverse-CDF draw with the uniforms ``u`` (fp32, one per
    OUTPUT row, in [0, 1)).  The logits are read in place, in their own dtype (fp32 / bf16 / fp16), through their row stride: any
    leading shape whose last dimension has stride 1 and which flattens to rows as a view (ValueError otherwise: never a copy);
    ``end`` may not pass the last dimension.  Returns int64 tokens shaped
    ``logits.shape[:-1]`` with ``+ start`` added and the CFG duplication done; a bad row (NaN, +inf, nothing finite) gets -1.
    ``want_cut``: also the per-output-row cut records as an int32 tensor [Ro, 6] (the 24-byte vqhip_sample_cut_t: kept,
    topk_kept, cut_value bits, cut_index, max bits, z bits)."""
    _require_cuda(logits, u)
    shape = logits.shape
    rows, R, stride = _logit_rows('sample_tokens', logits, start, end)
    cfg = cfg_alpha is not None
    Ro = R // 2 if cfg else R
    if u.dtype != torch.float32 or u.numel() != Ro or not u.is_contiguous():
        raise ValueError(f'sample_tokens: u must be {Ro} contiguous fp32 uniforms, got {u.dtype} {tuple(u.shape)}')
    tokens = torch.empty(R, dtype=torch.int64, device=logits.device)
    cut = torch.empty(Ro, 6, dtype=torch.int32, device=logits.device) if want_cut else None
    # the library checks the limits (R, the slice, V <= 2^20, temperature, alpha) before any HIP call
    check(_lib.lib().vqhip_sample_tokens(_ptr(rows), FLOAT_DTYPES[logits.dtype], R, stride, int(start), int(end),
                                         float(cfg_alpha) if cfg else 0.0, 1 if cfg else 0, float(temperature), int(top_k),
                                         float(top_p), _ptr(u), _ptr(tokens), _ptr(cut), _stream()), 'vqhip_sample_tokens')
    tokens = tokens.reshape(shape[:-1])
    return (tokens, cut) if want_cut else tokens


def sample_cut_fields(cut: torch.Tensor) -> dict:
    """The [Ro, 6] int32 records of ``sample_tokens(want_cut=True)`` as named host arrays (numpy)."""
    import numpy as np
    c = cut.cpu().numpy()
    f = np.ascontiguousarray(c).view(np.float32)
    return dict(kept=c[:, 0].copy(), topk_kept=c[:, 1].copy(), cut_value=f[:, 2].copy(), cut_index=c[:, 3].copy(),
                max=f[:, 4].copy(), z=f[:, 5].copy())


# ---- fused token cross-entropy (stage-2 training: hf.py:61-69, mage.py:107-123 / 479-489) ---------------------------------

TOKEN_DTYPES = {torch.int32: _lib.DTYPE_I32, torch.int64: _lib.DTYPE_I64}
TOKEN_CE_REDUCTIONS = ('mean', 'sum', 'none')


def _token_ce_args(what: str, logits, targets, start, end, label_smoothing, ignore_index, weight, shift):
    """The arguments vqhip_token_ce_fwd and _bwd share, from tensors that are read in place (the logits) or are [R] vectors."""
    _require_cuda(logits, targets, weight)
    end = logits.shape[-1] if end is None else end
    rows, R, stride = _logit_rows(what, logits, start, end)
    if targets.dtype not in TOKEN_DTYPES or targets.shape != logits.shape[:-1]:
        raise ValueError(f'{what}: targets must be int32 or int64 of shape {tuple(logits.shape[:-1])}, got {targets.dtype} {tuple(targets.shape)}')
    if shift and logits.dim() < 2:
        raise ValueError(f'{what}: shift needs logits [..., L, V_total]')
    targets = targets.reshape(-1).contiguous()
    if weight is not None:
        if weight.numel() != R:
            raise ValueError(f'{what}: weight must have one value per row ({R}), got {tuple(weight.shape)}')
        weight = _fp32_vector(weight)
    head = (_ptr(rows), FLOAT_DTYPES[logits.dtype], R, stride, int(start), int(end), _ptr(targets), TOKEN_DTYPES[targets.dtype],
            int(logits.shape[-2]) if shift else 0, int(ignore_index), float(label_smoothing), _ptr(weight))
    return head, R, (rows, targets, weight)


@_on_tensor_device
def token_ce_forward(logits: torch.Tensor, targets: torch.Tensor, start: int = 0, end: Optional[int] = None, *,
                     label_smoothing: float = 0.0, ignore_index: int = -100, weight: Optional[torch.Tensor] = None,
                     shift: bool = False) -> dict:
    """vqhip_token_ce_fwd of include/vqhip.h on ``logits[..., start:end]`` read in place (the view rules of ``sample_tokens``):
    fp32 ``loss`` [R], ``lse`` [R], int32 ``hit`` [R] and the device scalars ``out`` [4] = (sum w loss, W, hits, sum / W).  Two
    launches, no copy of the logits, no synchronisation."""
    head, R, keep = _token_ce_args('token_ce_forward', logits, targets, start, end, label_smoothing, ignore_index, weight, shift)
    dev = logits.device
    loss, lse = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
    hit, out = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.float32, device=dev)
    check(_lib.lib().vqhip_token_ce_fwd(*head, _ptr(loss), _ptr(lse), _ptr(hit), _ptr(out), _stream()), 'vqhip_token_ce_fwd')
    return dict(loss=loss, lse=lse, hit=hit, out=out)


@_on_tensor_device
def token_ce_backward(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor, g: torch.Tensor, start: int = 0,
                      end: Optional[int] = None, *, label_smoothing: float = 0.0, ignore_index: int = -100,
                      weight: Optional[torch.Tensor] = None, shift: bool = False, weight_sum: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vqhip_token_ce_bwd: the gradient over the logits, in their dtype and shape (contiguous), every element written by the
    kernel (zeros outside the slice and in ignored rows).  ``g``: fp32, one value (sum, mean) or one per row (none);
    ``weight_sum``: the device scalar W of the forward for the mean, None otherwise.  ``out``: a buffer to write into."""
    head, R, keep = _token_ce_args('token_ce_backward', logits, targets, start, end, label_smoothing, ignore_index, weight, shift)
    _require_cuda(lse, g, weight_sum, out)
    g, per_row = _grad_values(g, R)
    if g.numel() not in (1, R) or lse.dtype != torch.float32 or lse.numel() != R or not lse.is_contiguous():
        raise ValueError(f'token_ce_backward: g must hold 1 or {R} values and lse {R} contiguous fp32 values')
    Vt = logits.shape[-1]
    grad = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device) if out is None else out
    if grad.shape != logits.shape or grad.dtype != logits.dtype or not grad.is_contiguous():
        raise ValueError('token_ce_backward: out must be contiguous, of the shape and dtype of the logits')
    check(_lib.lib().vqhip_token_ce_bwd(*head, _ptr(lse), _ptr(g), per_row, _ptr(weight_sum), _ptr(grad), Vt, Vt, _stream()),
          'vqhip_token_ce_bwd')
    return grad


def token_cross_entropy(logits: torch.Tensor, targets: torch.Tensor, start: int = 0, end: Optional[int] = None, *,
                        label_smoothing: float = 0.0, ignore_index: int = -100, weight: Optional[torch.Tensor] = None,
                        shift: bool = False, reduction: str = 'mean', want_stats: bool = False):
    """Cross-entropy of ``logits[..., start:end]`` against ``targets`` (vocabulary indices, shape ``logits.shape[:-1]``), with
    autograd: see ``functional.token_cross_entropy``."""
    from . import functional
    return functional.token_cross_entropy(logits, targets, start, end, label_smoothing=label_smoothing, ignore_index=ignore_index,
                                          weight=weight, shift=shift, reduction=reduction, want_stats=want_stats)


# ---- fused CosineEmbeddingLoss (VQ-KD distillation: vq/algorithms/utils/losses.py:13-65) ------------------------------------

COSINE_REDUCTIONS = ('mean', 'sum', 'none')


def cosine_embedding_refusal(pred: torch.Tensor, target: torch.Tensor, layout: Optional[str] = None) -> str:
    """Why vqhip_cosine_embed_fwd would refuse this pair ('' if it would not): the clauses of its LIMITS that depend on the
    tensors' dtypes, shapes and strides.  ``layout``: 'rows' (None: the same) - pred and target both [..., C]; 'map' - pred the
    NCHW-contiguous [B, C, *positions], target [B, *positions, C] (or [B * P, C])."""
    layout = layout or 'rows'
    if layout not in LAYOUTS:
        return f'layout {layout!r} is neither rows nor map'
    why = float_dtype_refusal('pred is', pred) or float_dtype_refusal('target is', target)
    if why:
        return why
    if target.numel() == 0:                                                     # (row_view lets R = 0 pass)
        return f'target: empty tensor {tuple(target.shape)}'
    rows = row_view(target, 'target')
    if isinstance(rows, str):
        return rows
    R, C = rows[0].shape
    if layout == 'rows':
        if pred.shape != target.shape:
            return f'pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape'
        prow = row_view(pred, 'pred')
        if isinstance(prow, str):
            return prow
    else:
        if pred.dim() < 3 or pred.shape[1] != C or pred.numel() != R * C:
            return f'pred {tuple(pred.shape)} is not the [B, C, *positions] map of the target rows {tuple(target.shape)}'
        if not pred.is_contiguous():
            return f'pred with strides {pred.stride()} is not an NCHW-contiguous map'
    if not 0 < R < (1 << 31):
        return f'{R} rows are outside 1 .. 2^31-1'
    return '' if C <= _lib.COSINE_EMBED_MAX_C else f'C={C} is beyond 2^16'


def _cosine_embed_args(what: str, pred, target, layout):
    """The arguments vqhip_cosine_embed_fwd and _bwd share; both tensors are read in place."""
    _require_cuda(pred, target)
    _refuse(what, cosine_embedding_refusal(pred, target, layout))
    layout = layout or 'rows'
    trows, tstride = row_view(target, 'target')
    R, C = trows.shape
    if layout == 'rows':
        prows, pstride = row_view(pred, 'pred')
        B, P = R, 1
    else:
        prows, pstride = pred, 0
        B, P = pred.shape[0], R // pred.shape[0]
    head = (_ptr(prows), FLOAT_DTYPES[pred.dtype], LAYOUTS[layout], pstride, _ptr(trows), FLOAT_DTYPES[target.dtype], tstride, B, P, C)
    return head, R, C, (prows, trows)


@_on_tensor_device
def cosine_embedding_forward(pred: torch.Tensor, target: torch.Tensor, *, layout: Optional[str] = None) -> dict:
    """vqhip_cosine_embed_fwd of include/vqhip.h on ``pred`` and ``target`` read in place, each in its own dtype: fp32 ``loss``
    [R], ``stats`` [R, 3] = (1 / sqrt(pp tt), cos, 1 / pp) and the device scalars ``out`` [2] = (sum, mean).  ``layout``: 'rows'
    (default; both [..., C], views with unit column stride) or 'map' (``pred`` NCHW-contiguous [B, C, *positions], ``target``
    [B, *positions, C]).  Two launches, no copy, no synchronisation."""
    head, R, C, keep = _cosine_embed_args('cosine_embedding_forward', pred, target, layout)
    dev = pred.device
    loss = torch.empty(R, dtype=torch.float32, device=dev)
    stats = torch.empty(R, 3, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    check(_lib.lib().vqhip_cosine_embed_fwd(*head, _ptr(loss), _ptr(stats), _ptr(out), _stream()), 'vqhip_cosine_embed_fwd')
    return dict(loss=loss, stats=stats, out=out)


@_on_tensor_device
def cosine_embedding_backward(pred: torch.Tensor, target: torch.Tensor, stats: torch.Tensor, g: torch.Tensor, *,
                              layout: Optional[str] = None, mean: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vqhip_cosine_embed_bwd: the gradient over ``pred``, in its dtype, shape and layout, every element written by the one
    launch.  ``g``: fp32, one value (sum, mean) or one per row (none); ``mean``: divide by R on the device.  ``out``: a buffer of
    pred's shape and dtype to write into - rows layout: any view with unit column stride (the padding of its rows is not
    touched); map layout: contiguous."""
    head, R, C, keep = _cosine_embed_args('cosine_embedding_backward', pred, target, layout)
    _require_cuda(stats, g, out)
    g, per_row = _grad_values(g, R)
    if g.numel() not in (1, R) or stats.dtype != torch.float32 or stats.shape != (R, 3) or not stats.is_contiguous():
        raise ValueError(f'cosine_embedding_backward: g must hold 1 or {R} values and stats be contiguous fp32 [{R}, 3]')
    grad = torch.empty(pred.shape, dtype=pred.dtype, device=pred.device) if out is None else out
    if grad.shape != pred.shape or grad.dtype != pred.dtype:
        raise ValueError('cosine_embedding_backward: out must have the shape and dtype of pred')
    if (layout or 'rows') == 'rows':
        grows = row_view(grad, 'out')
        _refuse('cosine_embedding_backward', grows if isinstance(grows, str) else '')
        grows, gstride = grows
    else:
        _refuse('cosine_embedding_backward', '' if grad.is_contiguous() else 'out must be an NCHW-contiguous map')
        grows, gstride = grad, 0
    check(_lib.lib().vqhip_cosine_embed_bwd(*head, _ptr(stats), _ptr(g), per_row, 1 if mean else 0, _ptr(grows), gstride, _stream()),
          'vqhip_cosine_embed_bwd')
    return grad


def cosine_embedding_loss(pred: torch.Tensor, target: torch.Tensor, reduction: str = 'mean', *, layout: Optional[str] = None):
    """1 - cos(pred, target) per row with autograd to ``pred``: see ``functional.cosine_embedding_loss``."""
    from . import functional
    return functional.cosine_embedding_loss(pred, target, reduction, layout=layout)


# ---- fused LPIPS tail (the VQGAN generator's perceptual loss: vq/tasks/image_reconstruction/losses.py:99-178) ---------------

LPIPS_CHANNELS = (64, 128, 256, 512, 512)                   # the five taps of VGG16
LPIPS_MAX_LAYER = 1 << 16


def lpips_layout(pred: torch.Tensor, target: torch.Tensor):
    """The layout both feature maps share ('map' before 'rows' where both hold, as for C == 1), None if there is none."""
    both = [name for name in dense_layouts(pred) if name in dense_layouts(target)]
    return both[0] if both else None


def lpips_refusal(pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None) -> str:
    """Why vqhip_lpips_fwd would refuse this pair of feature maps ('' if it would not): the clauses of its LIMITS that depend
    on the tensors' dtypes, shapes and strides.  ``weight``: the 1 x 1 convolution's, any shape with C elements."""
    why = float_dtype_refusal('pred is', pred) or float_dtype_refusal('target is', target)
    if why:
        return why
    if pred.dim() < 3 or pred.shape != target.shape:
        return f'pred {tuple(pred.shape)} and target {tuple(target.shape)} are not two [B, C, *positions] maps of one shape'
    if pred.numel() == 0:
        return f'empty features {tuple(pred.shape)}'
    why = dense_refusal('pred', pred) or dense_refusal('target', target)
    if why:
        return why
    if lpips_layout(pred, target) is None:
        return f'pred (strides {pred.stride()}) and target (strides {target.stride()}) differ in layout'
    B, C = pred.shape[:2]
    P = pred.numel() // (B * C)
    if C > _lib.LPIPS_MAX_C:
        return f'C={C} is beyond 2^16'
    if B * P >= (1 << 31):
        return f'{B * P} pixels are outside 1 .. 2^31-1'
    if weight is not None and (weight.numel() != C or weight.dtype != torch.float32):
        return f'the weights are {weight.dtype} {tuple(weight.shape)}, not float32 with C={C} elements'
    return ''


def _lpips_args(what: str, pred, target, weight, seed, p, layer):
    """The arguments vqhip_lpips_fwd and _bwd share; both maps are read in place."""
    _require_cuda(pred, target, weight, seed)
    _refuse(what, lpips_refusal(pred, target, weight))
    if seed is not None:
        _refuse(what, _seed_refusal(seed) or ('' if 0.0 <= p < 1.0 else f'p={p!r} is outside [0, 1)'))
    _refuse(what, '' if 0 <= layer <= LPIPS_MAX_LAYER else f'layer={layer!r} is outside 0 .. 2^16')
    w = _fp32_vector(weight)
    B, C = pred.shape[:2]
    P = pred.numel() // (B * C)
    head = (_ptr(pred), FLOAT_DTYPES[pred.dtype], _ptr(target), FLOAT_DTYPES[target.dtype], LAYOUTS[lpips_layout(pred, target)],
            B, C, P, _ptr(w), _ptr(seed), float(p), int(layer))
    return head, B, C, P, (w,)


@_on_tensor_device
def lpips_layer_forward(pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, *, seed: Optional[torch.Tensor] = None,
                        p: float = 0.5, layer: int = 0, value: Optional[torch.Tensor] = None) -> dict:
    """vqhip_lpips_fwd of include/vqhip.h on one layer's feature maps ``pred`` and ``target`` [B, C, *positions], read in place, each
    in its own dtype, both NCHW-contiguous or both channels-last: fp32 ``stats`` [B, P, 4] = (1 / nf, 1 / ng, sum u a, s) per pixel
    and ``value`` [B], the spatial mean of s.  ``value``: a buffer of earlier layers to ADD this layer onto (in place).
    ``seed``: two 32-bit words on the device switch the dropout on, with probability ``p``; ``layer`` enters its hash.
    Two launches, no copy, no synchronisation."""
    head, B, C, P, keep = _lpips_args('lpips_layer_forward', pred, target, weight, seed, p, layer)
    _require_cuda(value)
    stats = torch.empty(B, P, 4, dtype=torch.float32, device=pred.device)
    accumulate = value is not None
    if accumulate and (value.dtype != torch.float32 or value.shape != (B,) or not value.is_contiguous()):
        raise ValueError(f'lpips_layer_forward: value must be contiguous fp32 [{B}]')
    value = value if accumulate else torch.empty(B, dtype=torch.float32, device=pred.device)
    check(_lib.lib().vqhip_lpips_fwd(*head, _ptr(stats), _ptr(value), 1 if accumulate else 0, _stream()), 'vqhip_lpips_fwd')
    return dict(stats=stats, value=value, s=stats[..., 3])


@_on_tensor_device
def lpips_layer_backward(pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, stats: torch.Tensor, g: torch.Tensor, *,
                         seed: Optional[torch.Tensor] = None, p: float = 0.5, layer: int = 0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vqhip_lpips_bwd: the gradient of sum_b g[b] value[b] over ``pred``, in its dtype, shape and layout, every element written
    by the one launch.  ``g``: fp32 [B]; ``seed``, ``p``, ``layer``: those of the forward (the mask is regenerated).  ``out``: a
    buffer of pred's shape, dtype and strides to write into."""
    head, B, C, P, keep = _lpips_args('lpips_layer_backward', pred, target, weight, seed, p, layer)
    _require_cuda(stats, g, out)
    g, _ = _grad_values(g, B)
    if g.numel() != B or stats.dtype != torch.float32 or stats.shape != (B, P, 4) or not stats.is_contiguous():
        raise ValueError(f'lpips_layer_backward: g must hold {B} values and stats be contiguous fp32 [{B}, {P}, 4]')
    grad = torch.empty_like(pred) if out is None else out                       # (preserve_format: pred is dense, so its strides)
    if grad.shape != pred.shape or grad.dtype != pred.dtype or grad.stride() != pred.stride():
        raise ValueError('lpips_layer_backward: out must have the shape, dtype and strides of pred')
    check(_lib.lib().vqhip_lpips_bwd(*head, _ptr(stats), _ptr(g), _ptr(grad), _stream()), 'vqhip_lpips_bwd')
    return grad


@_on_tensor_device
def lpips_keep_mask(seed: torch.Tensor, p: float, layer: int, B: int, C: int, P: int) -> torch.Tensor:
    """vqhip_lpips_keep_mask: the dropout mask uint8 [B, C, P] (1 kept, 0 dropped) the two kernels regenerate from ``seed``, by the
    same device function - what a reference needs to be held against a seeded run."""
    _require_cuda(seed)
    _refuse('lpips_keep_mask', _seed_refusal(seed))
    out = torch.empty(B, C, P, dtype=torch.uint8, device=seed.device)
    check(_lib.lib().vqhip_lpips_keep_mask(_ptr(seed), float(p), int(layer), B, C, P, _ptr(out), _stream()), 'vqhip_lpips_keep_mask')
    return out


def lpips_distance(pred_features, target_features, weights, seed: Optional[torch.Tensor] = None, p: float = 0.5) -> torch.Tensor:
    """The LPIPS distance [B] fp32 of the lists of feature maps, with autograd to the pred features: see ``functional.lpips_distance``."""
    from . import functional
    return functional.lpips_distance(pred_features, target_features, weights, seed, p)


# ---- StyleGAN2 discriminator ops (vq/algorithms/vqgan/discriminators/stylegan2.py: FusedBiasLeakyReLU and upfirdn2d) ------------

FIR4_PADS = ((2, 2), (1, 1))                                # Blur's padding for the 3 x 3 and the 1 x 1 downsampling convolution


def stylegan2_refusal(x: torch.Tensor, bias: Optional[torch.Tensor] = None, *, kernel_size: Optional[int] = None) -> str:
    """Why vqhip_bias_act_* / vqhip_fir4_* would refuse this activation ('' if they would not): the clauses of their LIMITS that
    depend on the tensor's dtype, shape and strides.  ``bias``: [C]; ``kernel_size``: of the convolution a Blur serves (3 or 1)."""
    why = float_dtype_refusal('the activation is', x) \
        or ('' if x.dim() in (2, 4) else f'the activation is {x.dim()}-D, not [B, C] or [B, C, H, W]') \
        or ('' if x.numel() else f'empty activation {tuple(x.shape)}') or dense_refusal('the activation', x)
    if why:
        return why
    if x.shape[1] > _lib.SG2_MAX_C:
        return f'C={x.shape[1]} is beyond 2^16'
    if x.numel() >= (1 << 31):
        return f'{x.numel()} elements are outside 1 .. 2^31-1'
    if bias is not None and bias.numel() != x.shape[1]:
        return f'the bias has {bias.numel()} elements, not C={x.shape[1]}'
    if kernel_size is not None and kernel_size not in (1, 3):
        return f'kernel_size={kernel_size}: the blur paddings are known for 3 and 1 only'
    return ''


def _sg2_head(what: str, x: torch.Tensor, bias=None):
    _require_cuda(x, bias)
    _refuse(what, stylegan2_refusal(x, bias))
    B, C = x.shape[:2]
    return FLOAT_DTYPES[x.dtype], LAYOUTS[dense_layout(x)], B, C, x.numel() // (B * C)


@_on_tensor_device
def bias_act(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """vqhip_bias_act_fwd: ``leaky_relu(x + bias[c], 0.2) * 2**0.5`` of a [B, C] or [B, C, H, W] activation, read in place, in its
    dtype and memory format (NCHW or channels-last).  One launch."""
    dtype, layout, B, C, P = _sg2_head('bias_act', x, bias)
    b = _fp32_vector(bias)
    y = torch.empty_like(x)
    check(_lib.lib().vqhip_bias_act_fwd(_ptr(x), dtype, layout, B, C, P, _ptr(b), _ptr(y), _stream()), 'vqhip_bias_act_fwd')
    return y


@_on_tensor_device
def bias_act_backward(g: torch.Tensor, y: torch.Tensor, need_gbias: bool = True):
    """vqhip_bias_act_bwd: ``(gx, gbias)`` from the incoming gradient and the SAVED OUTPUT ``y`` (the sign of y selects the branch;
    x is not kept).  ``gx`` in g's dtype and layout, ``gbias`` fp32 [C] from a fixed-order two-stage sum (None without
    ``need_gbias``).  Linear in ``g``: the same call on a second-order gradient is its derivative."""
    dtype, layout, B, C, P = _sg2_head('bias_act_backward', y)
    _require_cuda(g)
    if g.shape != y.shape or g.dtype != y.dtype:
        raise ValueError(f'bias_act_backward: g is {g.dtype} {tuple(g.shape)}, y {y.dtype} {tuple(y.shape)}')
    g = _dense_like(g, y)
    gx = torch.empty_like(y)
    gbias = ws = None
    if need_gbias:
        slabs = _lib.lib().vqhip_bias_act_slabs(layout, B, C, P)
        ws = torch.empty(slabs * C, dtype=torch.float32, device=y.device)
        gbias = torch.empty(C, dtype=torch.float32, device=y.device)
    check(_lib.lib().vqhip_bias_act_bwd(_ptr(g), _ptr(y), dtype, layout, B, C, P, _ptr(gx), _ptr(gbias), _ptr(ws),
                                        0 if ws is None else ws.numel() * 4, _stream()), 'vqhip_bias_act_bwd')
    return gx, gbias


def fir4_out_size(H: int, W: int, pad, down: int) -> tuple:
    """(OH, OW) of the blur of an H x W plane: ``(H + py0 + py1 - 4) // down + 1``; ``pad`` = (py0, py1, px0, px1)."""
    py0, py1, px0, px1 = pad
    return (H + py0 + py1 - 4) // down + 1, (W + px0 + px1 - 4) // down + 1


def _fir4_pad(what: str, pad, down: int) -> tuple:
    pad = (pad,) * 4 if isinstance(pad, int) else tuple(pad)
    pad = pad * 2 if len(pad) == 2 else pad                 # a symmetric (p0, p1) pair serves both axes, whichever way mmcv reads it
    if len(pad) != 4 or any(not 0 <= int(p) <= 3 for p in pad) or down not in (1, 2):
        raise ValueError(f'{what}: need four paddings in 0 .. 3 and down in (1, 2), got {pad!r}, {down!r}')
    return tuple(int(p) for p in pad)


@_on_tensor_device
def fir4(x: torch.Tensor, pad=2, down: int = 1, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vqhip_fir4_fwd: the blur ``upfirdn2d(x, outer([1, 3, 3, 1]) / 64, padding)`` of a [B, C, H, W] map per channel with zero
    padding ``pad`` = p | (p0, p1) | (py0, py1, px0, px1), keeping every ``down``-th output (only those are computed).  With
    ``bias`` the input passes through bias-activation on the way in: ``blur(bias_act(x, bias))`` from one read of x.  One launch."""
    dtype, layout, B, C, P = _sg2_head('fir4', x, bias)
    if x.dim() != 4:
        raise ValueError(f'fir4: need a [B, C, H, W] map, got {tuple(x.shape)}')
    pad = _fir4_pad('fir4', pad, down)
    H, W = x.shape[2:]
    OH, OW = fir4_out_size(H, W, pad, down)
    if OH < 1 or OW < 1:
        raise ValueError(f'fir4: the padded {H} x {W} plane is smaller than the filter')
    b = None if bias is None else _fp32_vector(bias)
    out = _empty_like(x, (B, C, OH, OW))
    check(_lib.lib().vqhip_fir4_fwd(_ptr(x), dtype, layout, B, C, H, W, down, *pad, _ptr(b), _ptr(out), _stream()), 'vqhip_fir4_fwd')
    return out


@_on_tensor_device
def fir4_backward(g: torch.Tensor, size, pad=2, down: int = 1, x: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
    """vqhip_fir4_bwd: the exact adjoint of ``fir4`` for an input plane of ``size`` = (H, W): ``gx`` [B, C, H, W] in g's dtype and
    layout.  With ``x`` and ``bias`` (the saved input of the fused forward) returns ``(gx, gbias)``:
    ``gx = adjoint(g) * scale * (x + bias > 0 ? 1 : slope)`` and its per-channel sum, fp32 [C], in a fixed order."""
    if g.dim() != 4 or (x is None) != (bias is None):
        raise ValueError('fir4_backward: need a [B, C, OH, OW] gradient, and x and bias together or neither')
    _require_cuda(g, x)
    if x is not None:
        _refuse('fir4_backward', dense_refusal('x', x))
    g = dense(g) if x is None else _dense_like(g, x)                            # (in x's layout for the fused form)
    dtype, layout, B, C, _ = _sg2_head('fir4_backward', g)
    pad = _fir4_pad('fir4_backward', pad, down)
    H, W = (int(v) for v in size)
    if tuple(g.shape[2:]) != fir4_out_size(H, W, pad, down):
        raise ValueError(f'fir4_backward: g is {tuple(g.shape)}, the blur of a {H} x {W} plane gives {fir4_out_size(H, W, pad, down)}')
    gbias = ws = b = None
    if x is not None:
        _require_cuda(bias)
        if x.dtype != g.dtype or tuple(x.shape) != (B, C, H, W):
            raise ValueError(f'fir4_backward: x must be a dense {g.dtype} [{B}, {C}, {H}, {W}] map')
        layout = LAYOUTS[dense_layout(x)]
        b = _fp32_vector(bias)
        slabs = _lib.lib().vqhip_fir4_slabs(layout, B, C, H, W)
        ws = torch.empty(slabs * C, dtype=torch.float32, device=g.device)
        gbias = torch.empty(C, dtype=torch.float32, device=g.device)
    gx = _empty_like(g if x is None else x, (B, C, H, W))
    if gx.numel() >= (1 << 31):
        raise ValueError(f'fir4_backward: {gx.numel()} elements are outside 1 .. 2^31-1')
    check(_lib.lib().vqhip_fir4_bwd(_ptr(g), dtype, layout, B, C, H, W, down, *pad, _ptr(x), _ptr(b), _ptr(gx), _ptr(gbias), _ptr(ws),
                                    0 if ws is None else ws.numel() * 4, _stream()), 'vqhip_fir4_bwd')
    return gx if x is None else (gx, gbias)


# ---- GroupNorm (+ SiLU) of the VQGAN encoder and decoder (vq/algorithms/vqgan/autoencoder.py) ---------------------------------

GROUP_NORM_ACTS = {None: 0, 'silu': 1, 'leaky_relu': _lib.GN_ACT_LEAKY}      # 'leaky_relu': slope 0.2 (VQHIP_GN_LEAKY_SLOPE)


def group_norm_refusal(x: torch.Tensor, num_groups: int) -> str:
    """Why vqhip_group_norm_* would refuse this activation ('' if they would not): the clauses of their LIMITS that depend on the
    tensor's dtype, shape and strides.  ``num_groups=0`` is batch statistics (VQHIP_GN_BATCH at the ABI): one group per channel over
    all images."""
    why = float_dtype_refusal('the activation is', x) \
        or ('' if x.dim() >= 2 else f'the activation is {x.dim()}-D, not [B, C, ...]') \
        or ('' if x.numel() else f'empty activation {tuple(x.shape)}')
    if why or num_groups != 0:
        return why \
            or ('' if num_groups >= 1 and x.shape[1] % num_groups == 0 else f'C={x.shape[1]} is no multiple of num_groups={num_groups}') \
            or dense_refusal('the activation', x) \
            or ('' if x.numel() // (x.shape[0] * num_groups) < (1 << 31) else
                f'a group of {x.numel() // (x.shape[0] * num_groups)} values is outside 1 .. 2^31-1')
    n = x.numel() // x.shape[1]
    return dense_refusal('the activation', x) or ('' if 2 <= n < (1 << 31) else f'a channel of {n} values over the batch is outside 2 .. 2^31-1')


def _gn_head(what: str, x: torch.Tensor, num_groups: int, weight: torch.Tensor, bias: torch.Tensor, act):
    _require_cuda(x, weight, bias)
    why = group_norm_refusal(x, num_groups)
    if not why and act not in GROUP_NORM_ACTS:
        why = f'act={act!r} is none of None, \'silu\', \'leaky_relu\''
    if not why and act == 'leaky_relu' and num_groups != 0:
        why = 'act=\'leaky_relu\' is fused behind batch statistics (num_groups=0) only'
    if not why and (weight.numel() != x.shape[1] or bias.numel() != x.shape[1]):
        why = f'weight and bias have {weight.numel()} and {bias.numel()} elements, not C={x.shape[1]}'
    _refuse(what, why)
    B, C = x.shape[:2]
    P = x.numel() // (B * C)
    layout = LAYOUTS[dense_layout(x)]
    ws_bytes = _lib.lib().vqhip_group_norm_ws_bytes(layout, B, C, P, num_groups or _lib.GN_BATCH)
    if ws_bytes < 0:
        raise ValueError(f'{what}: {tuple(x.shape)} in {num_groups} groups is beyond the sizes of vqhip_group_norm_*')
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    return FLOAT_DTYPES[x.dtype], layout, B, C, P, ws


@_on_tensor_device
def group_norm(x: torch.Tensor, num_groups: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6, act=None):
    """vqhip_group_norm_fwd: ``(y, stats)`` for ``y = act(group_norm(x) * weight[c] + bias[c])`` of a [B, C, ...] activation read in
    place, in its dtype and memory format (NCHW or channels-last); ``act``: None or 'silu'.  ``stats`` [B, G, 2] fp32 holds each
    group's mean and 1 / sqrt(var + eps), what the backward reads.  One launch, two where a group is split over workgroups.
    ``num_groups=0``: batch statistics, ``stats`` [C, 2], ``act`` also 'leaky_relu' (slope 0.2); ``batch_norm`` returns the
    call's block of means and unbiased variances as well."""
    return _group_norm(x, num_groups, weight, bias, eps, act)[:2]


def _group_norm(x, num_groups, weight, bias, eps, act):
    dtype, layout, B, C, P, ws = _gn_head('group_norm', x, num_groups, weight, bias, act)
    w, b = _fp32_vector(weight), _fp32_vector(bias)
    y = torch.empty_like(x)
    stats = torch.empty((B, num_groups, 2) if num_groups else (C, 2), dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_group_norm_fwd(_ptr(x), dtype, layout, B, C, P, num_groups or _lib.GN_BATCH, _ptr(w), _ptr(b), float(eps), GROUP_NORM_ACTS[act],
                                          _ptr(y), _ptr(stats), _ptr(ws), ws.numel() * 4, _stream()), 'vqhip_group_norm_fwd')
    return y, stats, ws


@_on_tensor_device
def group_norm_backward(g: torch.Tensor, x: torch.Tensor, stats: torch.Tensor, num_groups: int, weight: torch.Tensor, bias: torch.Tensor,
                        act=None):
    """vqhip_group_norm_bwd: ``(gx, dgamma, dbeta)`` from the incoming gradient, the saved input and the forward's ``stats``; the
    affine value and the SiLU derivative are recomputed.  ``gx`` in x's dtype and layout, ``dgamma`` and ``dbeta`` fp32 [C] from a
    fixed-order two-stage sum."""
    dtype, layout, B, C, P, ws = _gn_head('group_norm_backward', x, num_groups, weight, bias, act)
    _require_cuda(g, stats)
    if g.shape != x.shape or g.dtype != x.dtype:
        raise ValueError(f'group_norm_backward: g is {g.dtype} {tuple(g.shape)}, x {x.dtype} {tuple(x.shape)}')
    if stats.dtype != torch.float32 or stats.numel() != (B * num_groups if num_groups else C) * 2 or not stats.is_contiguous():
        raise ValueError(f'group_norm_backward: stats must be the contiguous fp32 '
                         f'{[B, num_groups, 2] if num_groups else [C, 2]} of the forward')
    g = _dense_like(g, x)
    w, b = _fp32_vector(weight), _fp32_vector(bias)
    gx = torch.empty_like(x)
    dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_group_norm_bwd(_ptr(g), _ptr(x), dtype, layout, B, C, P, num_groups or _lib.GN_BATCH, _ptr(w), _ptr(b), _ptr(stats),
                                          GROUP_NORM_ACTS[act], _ptr(gx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel() * 4, _stream()),
          'vqhip_group_norm_bwd')
    return gx, dgamma, dbeta


@_on_tensor_device
def batch_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, act=None):
    """vqhip_group_norm_fwd with G = VQHIP_GN_BATCH: ``(y, stats, mean, unbiased_var)`` for ``y = act(batch_norm(x) * weight[c] +
    bias[c])`` with the statistics of this batch (training mode), of a [B, C, ...] activation read in place.  ``stats`` [C, 2] fp32
    (mean, 1 / sqrt(var + eps)) is what the backward reads; ``mean`` and ``unbiased_var`` [C] are views of the call's workspace,
    what the running statistics take.  One launch where a workgroup holds a channel, three otherwise."""
    y, stats, ws = _group_norm(x, 0, weight, bias, eps, act)
    C = x.shape[1]
    return y, stats, ws[:C], ws[C:2 * C]


def batch_norm_backward(g: torch.Tensor, x: torch.Tensor, stats: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, act=None):
    """vqhip_group_norm_bwd with G = VQHIP_GN_BATCH: ``(gx, dgamma, dbeta)``; the channel sums are the parameter gradients."""
    return group_norm_backward(g, x, stats, 0, weight, bias, act)


# ---- the row ops of VQKDEncoder / VQKDDecoder (vq/algorithms/vqkd/autoencoder.py): add + LayerNorm, bias + GELU / tanh -------------

ROW_ACTS = {'gelu': _lib.ROW_ACT_GELU, 'tanh': _lib.ROW_ACT_TANH}


def vit_rows_refusal(name: str, t: torch.Tensor) -> str:
    """Why vqhip_add_layer_norm_* / vqhip_row_bias_act_* would refuse ``t`` [..., D] ('' if they would not): the clauses of their
    LIMITS that depend on the tensor's dtype, shape and strides.  Rows must be dense: no copy is made here."""
    rows = row_view(t, name)
    if isinstance(rows, str):
        return rows
    rows, stride = rows
    R, D = rows.shape
    return ('' if R >= 1 and D >= 1 else f'{name} {tuple(t.shape)} is empty') \
        or ('' if stride == D else f'the rows of {name} are not dense (row stride {stride}, D={D})') \
        or ('' if D <= _lib.VIT_MAX_D else f'D={D} is beyond {_lib.VIT_MAX_D}') \
        or ('' if R <= _lib.VIT_MAX_R else f'R={R} rows are beyond 2^24') \
        or ('' if R * D < (1 << 31) else f'{R * D} elements are outside 1 .. 2^31-1')


def _vit_rows(what: str, name: str, t: torch.Tensor):
    _require_cuda(t)
    _refuse(what, vit_rows_refusal(name, t))
    return row_view(t, name)[0]


def ln_pair_refusal(x: torch.Tensor, y_dtype) -> str:
    """'' where (x's dtype, the dtype of res, y and g) is a row of the table of include/vqhip.h, else the sentence that says so."""
    ok = y_dtype in FLOAT_DTYPES and (y_dtype == x.dtype or x.dtype == torch.float32)
    return '' if ok else f'x is {x.dtype} and the other side {y_dtype}: need one float dtype, or float32 x with bfloat16 or float16'


def _add_norm(what: str, x, res, weight, bias, eps, out_dtype):
    """vqhip_add_layer_norm_fwd in either mode: ``bias`` None is the RMS mode (beta == NULL).  What both ops decide alike: the row
    view, the dtype table, res's shape and dtype, the parameter vectors."""
    xr = _vit_rows(what, 'x', x)
    out_dtype = out_dtype or (x.dtype if res is None else res.dtype)
    why = ln_pair_refusal(x, out_dtype)
    rr = None
    if not why and res is not None:
        why = ('' if res.shape == x.shape and res.dtype == out_dtype else
               f'res is {res.dtype} {tuple(res.shape)}, not {out_dtype} {tuple(x.shape)}') or vit_rows_refusal('res', res)
        _require_cuda(res)
    R, D = xr.shape
    if not why and (weight.numel() != D or (bias is not None and bias.numel() != D)):
        why = f'weight and bias have {weight.numel()} and {D if bias is None else bias.numel()} elements, not D={D}'
    _refuse(what, why)
    _require_cuda(weight, bias)
    if res is not None:
        rr = row_view(res, 'res')[0]
    w, b = _fp32_vector(weight), None if bias is None else _fp32_vector(bias)
    s = x if res is None else torch.empty_like(xr).view(x.shape)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    stats = torch.empty(R, 2, dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_add_layer_norm_fwd(_ptr(xr), FLOAT_DTYPES[x.dtype], _ptr(rr), FLOAT_DTYPES[out_dtype], R, D, _ptr(w), _ptr(b),
                                              float(eps), None if res is None else _ptr(s), _ptr(y), FLOAT_DTYPES[out_dtype], _ptr(stats),
                                              _stream()), 'vqhip_add_layer_norm_fwd')
    return s, y, stats


@_on_tensor_device
def add_layer_norm(x: torch.Tensor, res: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6,
                   out_dtype=None):
    """vqhip_add_layer_norm_fwd: ``(s, y, stats)`` with ``s = x + res`` in x's dtype (``x`` itself where ``res`` is None),
    ``y = layer_norm(s) * weight + bias`` in ``out_dtype`` (default: res's dtype, else x's) and ``stats`` [R, 2] fp32 (each row's
    mean and 1 / sqrt(var + eps)).  Rows [..., D] read in place; fp32 x with a bf16 / fp16 res and y is the autocast case.  One launch."""
    if bias is None:
        raise ValueError('add_layer_norm: bias is required (add_rms_norm is the op without one)')
    return _add_norm('add_layer_norm', x, res, weight, bias, eps, out_dtype)


@_on_tensor_device
def add_rms_norm(x: torch.Tensor, res: Optional[torch.Tensor], weight: torch.Tensor, eps: float = 1e-5, out_dtype=None):
    """vqhip_add_layer_norm_fwd with beta == NULL: ``(s, y, stats)`` with ``s = x + res`` in x's dtype (``x`` itself where ``res``
    is None), ``y = s / sqrt(mean(s^2) + eps) * weight`` in ``out_dtype``, computed in fp32 and rounded once, and ``stats`` [R, 2]
    fp32 (0 and each row's 1 / sqrt(mean(s^2) + eps)).  Everything else as ``add_layer_norm``.  One launch."""
    return _add_norm('add_rms_norm', x, res, weight, None, eps, out_dtype)


def _add_norm_backward(what: str, g, s, stats, weight, g_skip, rms: bool):
    """vqhip_add_layer_norm_bwd in either mode: ``rms`` passes dbeta == NULL and returns None for it."""
    sr = _vit_rows(what, 's', s)
    R, D = sr.shape
    why = ln_pair_refusal(s, g.dtype) or ('' if g.shape == s.shape else f'g is {tuple(g.shape)}, s {tuple(s.shape)}') \
        or vit_rows_refusal('g', g)
    if not why and g_skip is not None:
        why = ('' if g_skip.shape == s.shape and g_skip.dtype == s.dtype else
               f'g_skip is {g_skip.dtype} {tuple(g_skip.shape)}, not {s.dtype} {tuple(s.shape)}') or vit_rows_refusal('g_skip', g_skip)
    if not why and (stats.dtype != torch.float32 or stats.numel() != 2 * R or not stats.is_contiguous()):
        why = f'stats must be the contiguous fp32 [{R}, 2] of the forward'
    if not why and weight.numel() != D:
        why = f'weight has {weight.numel()} elements, not D={D}'
    _refuse(what, why)
    _require_cuda(g, g_skip, stats, weight)
    w = _fp32_vector(weight)
    gr = row_view(g, 'g')[0]
    kr = None if g_skip is None else row_view(g_skip, 'g_skip')[0]
    gx = torch.empty_like(sr).view(s.shape)
    slabs = _lib.lib().vqhip_add_layer_norm_slabs(R, D)
    ws = torch.empty(2 * slabs * D, dtype=torch.float32, device=s.device)
    dgamma = torch.empty(D, dtype=torch.float32, device=s.device)
    dbeta = None if rms else torch.empty(D, dtype=torch.float32, device=s.device)
    check(_lib.lib().vqhip_add_layer_norm_bwd(_ptr(gr), FLOAT_DTYPES[g.dtype], _ptr(sr), FLOAT_DTYPES[s.dtype], _ptr(kr), R, D, _ptr(w),
                                              _ptr(stats), _ptr(gx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel() * 4, _stream()),
          'vqhip_add_layer_norm_bwd')
    return gx, dgamma, dbeta


@_on_tensor_device
def add_layer_norm_backward(g: torch.Tensor, s: torch.Tensor, stats: torch.Tensor, weight: torch.Tensor,
                            g_skip: Optional[torch.Tensor] = None):
    """vqhip_add_layer_norm_bwd: ``(gx, dgamma, dbeta)`` from the gradient ``g`` arriving at y, the saved sum ``s`` and the
    forward's ``stats``; ``g_skip``, the gradient arriving at s itself, is added in the same pass.  ``gx`` in s's dtype (it is the
    gradient of x and, cast, of res), ``dgamma`` and ``dbeta`` fp32 [D] from a fixed-order two-stage sum."""
    return _add_norm_backward('add_layer_norm_backward', g, s, stats, weight, g_skip, False)


@_on_tensor_device
def add_rms_norm_backward(g: torch.Tensor, s: torch.Tensor, stats: torch.Tensor, weight: torch.Tensor,
                          g_skip: Optional[torch.Tensor] = None):
    """vqhip_add_layer_norm_bwd with dbeta == NULL: ``(gx, dgamma)`` of ``add_rms_norm`` from ITS ``stats`` (the pairing of the two
    modes is held here: the library sees one call at a time)."""
    return _add_norm_backward('add_rms_norm_backward', g, s, stats, weight, g_skip, True)[:2]


def _row_act_head(what: str, x: torch.Tensor, bias: torch.Tensor, act):
    xr = _vit_rows(what, 'x', x)
    why = ('' if act in ROW_ACTS else f'act={act!r} is neither \'gelu\' nor \'tanh\'') \
        or ('' if bias.numel() == xr.shape[1] else f'the bias has {bias.numel()} elements, not D={xr.shape[1]}')
    _refuse(what, why)
    _require_cuda(bias)
    return xr, _fp32_vector(bias)


@_on_tensor_device
def row_bias_act(x: torch.Tensor, bias: torch.Tensor, act='gelu') -> torch.Tensor:
    """vqhip_row_bias_act_fwd: ``act(x + bias)`` of rows [..., D] read in place, in x's dtype; ``act``: 'gelu' (the erf form) or
    'tanh'.  One launch."""
    xr, b = _row_act_head('row_bias_act', x, bias, act)
    y = torch.empty_like(xr).view(x.shape)
    check(_lib.lib().vqhip_row_bias_act_fwd(_ptr(xr), FLOAT_DTYPES[x.dtype], *xr.shape, _ptr(b), ROW_ACTS[act], _ptr(y), _stream()),
          'vqhip_row_bias_act_fwd')
    return y


@_on_tensor_device
def row_bias_act_backward(g: torch.Tensor, x: torch.Tensor, bias: torch.Tensor, act='gelu', need_dbias: bool = True):
    """vqhip_row_bias_act_bwd: ``(gx, dbias)`` from the incoming gradient and the SAVED INPUT ``x`` and ``bias`` (the derivative
    is recomputed; y is not kept).  ``gx`` in x's dtype, ``dbias`` fp32 [D] from a fixed-order two-stage sum (None without
    ``need_dbias``)."""
    xr, b = _row_act_head('row_bias_act_backward', x, bias, act)
    _refuse('row_bias_act_backward', ('' if g.shape == x.shape and g.dtype == x.dtype else
                                      f'g is {g.dtype} {tuple(g.shape)}, x {x.dtype} {tuple(x.shape)}') or vit_rows_refusal('g', g))
    _require_cuda(g)
    gr = row_view(g, 'g')[0]
    R, D = xr.shape
    gx = torch.empty_like(xr).view(x.shape)
    dbias = ws = None
    if need_dbias:
        slabs = _lib.lib().vqhip_row_bias_act_slabs(R, D)
        ws = torch.empty(slabs * D, dtype=torch.float32, device=x.device)
        dbias = torch.empty(D, dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_row_bias_act_bwd(_ptr(gr), _ptr(xr), FLOAT_DTYPES[x.dtype], R, D, _ptr(b), ROW_ACTS[act], _ptr(gx), _ptr(dbias),
                                            _ptr(ws), 0 if ws is None else ws.numel() * 4, _stream()), 'vqhip_row_bias_act_bwd')
    return gx, dbias


def swiglu_refusal(name: str, t: torch.Tensor) -> str:
    """Why the SwiGLU mode of vqhip_row_bias_act_* would refuse ``t`` [..., 2 F] = (gate | up) ('' if it would not): the clauses of
    ``vit_rows_refusal`` with D read as the output width F and the element count as R 2 F.  Rows must be dense: no copy is made here."""
    rows = row_view(t, name)
    if isinstance(rows, str):
        return rows
    rows, stride = rows
    R, W2 = rows.shape
    F = W2 // 2
    return ('' if R >= 1 and W2 >= 1 else f'{name} {tuple(t.shape)} is empty') \
        or ('' if W2 % 2 == 0 else f'{name} has {W2} columns: (gate | up) needs an even number') \
        or ('' if stride == W2 else f'the rows of {name} are not dense (row stride {stride}, 2 F={W2})') \
        or ('' if F <= _lib.VIT_MAX_D else f'F={F} is beyond {_lib.VIT_MAX_D}') \
        or ('' if R <= _lib.VIT_MAX_R else f'R={R} rows are beyond 2^24') \
        or ('' if R * W2 < (1 << 31) else f'{R * W2} elements are outside 1 .. 2^31-1')


def _swiglu_rows(what: str, x: torch.Tensor):
    _require_cuda(x)
    _refuse(what, swiglu_refusal('x', x))
    return row_view(x, 'x')[0]


@_on_tensor_device
def swiglu(x: torch.Tensor) -> torch.Tensor:
    """vqhip_row_bias_act_fwd with act = VQHIP_ROW_ACT_SWIGLU: ``silu(x[..., :F]) * x[..., F:]`` of rows [..., 2 F] read in place,
    [..., F] in x's dtype.  One launch."""
    xr = _swiglu_rows('swiglu', x)
    R, F = xr.shape[0], xr.shape[1] // 2
    y = torch.empty(x.shape[:-1] + (F,), dtype=x.dtype, device=x.device)
    check(_lib.lib().vqhip_row_bias_act_fwd(_ptr(xr), FLOAT_DTYPES[x.dtype], R, F, None, _lib.ROW_ACT_SWIGLU, _ptr(y), _stream()),
          'vqhip_row_bias_act_fwd')
    return y


@_on_tensor_device
def swiglu_backward(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """vqhip_row_bias_act_bwd with act = VQHIP_ROW_ACT_SWIGLU: ``gx`` [..., 2 F] in x's dtype, both halves in one launch, from the
    incoming gradient ``g`` [..., F] and the SAVED INPUT ``x`` (the sigmoid is recomputed; y is not kept)."""
    xr = _swiglu_rows('swiglu_backward', x)
    R, F = xr.shape[0], xr.shape[1] // 2
    _refuse('swiglu_backward', ('' if g.shape == x.shape[:-1] + (F,) and g.dtype == x.dtype else
                                f'g is {g.dtype} {tuple(g.shape)}, x {x.dtype} {tuple(x.shape)}') or vit_rows_refusal('g', g))
    _require_cuda(g)
    gr = row_view(g, 'g')[0]
    gx = torch.empty_like(xr).view(x.shape)
    check(_lib.lib().vqhip_row_bias_act_bwd(_ptr(gr), _ptr(xr), FLOAT_DTYPES[x.dtype], R, F, None, _lib.ROW_ACT_SWIGLU, _ptr(gx), None,
                                            None, 0, _stream()), 'vqhip_row_bias_act_bwd')
    return gx


# ---- static KV cache: rotary + append, and the one-token attention over the cache (LlamaTransformer, static_cache=True) --------

def attention_shape_refusal(Hq: int, Hkv: int, Dh: int) -> str:
    """Why vqhip_decode_attention / vqhip_rope_append would refuse these head counts and this head dimension ('' if not)."""
    return ('' if Dh % 8 == 0 and 16 <= Dh <= _lib.ATTN_MAX_HEAD_DIM else
            f'a head dimension of {Dh} is not a multiple of 8 in 16 .. {_lib.ATTN_MAX_HEAD_DIM}') \
        or ('' if Hkv >= 1 and Hq >= 1 and Hq % Hkv == 0 else f'{Hq} query heads are not a multiple of {Hkv} key-value heads') \
        or ('' if Hq // Hkv <= _lib.ATTN_MAX_GROUP else f'{Hq // Hkv} query heads per key-value head are beyond {_lib.ATTN_MAX_GROUP}')


def attention_refusal(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, seen: int, L: int = 1, tables: bool = False) -> str:
    """Why vqhip_decode_attention (``L`` = 1) / vqhip_rope_append would refuse these tensors ('' if they would not): the clauses of
    their LIMITS that depend on dtypes, shapes, strides and alignment.  q [B L, Hq Dh], k and v [B L, Hkv Dh] are read in place
    through their row strides (three views into one packed row pass), cos and sin are [L, Dh] (or anything that flattens to it),
    the caches [B, Hkv, cap, Dh].  ``tables``: vqhip_decode_attention_at - cos and sin are the [cap, Dh] tables and there is no
    ``seen`` to refuse (the kernel reads the position)."""
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        return f'the caches must both be [B, Hkv, cap, Dh], got {tuple(k_cache.shape)} and {tuple(v_cache.shape)}'
    B, Hkv, cap, Dh = k_cache.shape
    why = float_dtype_refusal('q is', q)
    for name, t in (('k', k), ('v', v), ('k_cache', k_cache), ('v_cache', v_cache)):
        why = why or ('' if t.dtype == q.dtype else f'{name} is {t.dtype}, q {q.dtype}')
    for name, t in (('q', q), ('k', k), ('v', v)):
        why = why or ('' if t.dim() == 2 and t.shape[0] == B * L and (t.stride(1) == 1 or t.shape[1] == 1) and
                      (t.stride(0) >= t.shape[1] or t.shape[0] == 1) else
                      f'{name} {tuple(t.shape)} with strides {t.stride()} is not {B * L} rows of contiguous heads')
    if why:
        return why
    Hq = q.shape[1] // max(Dh, 1)
    return ('' if q.shape[1] == Hq * Dh and k.shape[1] == Hkv * Dh and v.shape[1] == Hkv * Dh else
            f'rows of {q.shape[1]}, {k.shape[1]} and {v.shape[1]} values are not heads of {Dh} for {Hkv} key-value heads') \
        or attention_shape_refusal(Hq, Hkv, Dh) \
        or ('' if 1 <= cap <= _lib.ATTN_MAX_LEN else f'a capacity of {cap} is outside 1 .. {_lib.ATTN_MAX_LEN}') \
        or ('' if tables or (seen >= 0 and L >= 1 and seen + L <= cap) else f'{L} tokens behind {seen} do not fit a capacity of {cap}') \
        or ('' if all(t.dtype == torch.float32 and t.numel() == (cap if tables else L) * Dh and t.is_contiguous() for t in (cos, sin)) else
            f'cos and sin must be contiguous float32 with {cap if tables else L} x {Dh} elements, got {cos.dtype} {tuple(cos.shape)} and '
            f'{sin.dtype} {tuple(sin.shape)}') \
        or ('' if k_cache.is_contiguous() and v_cache.is_contiguous() else 'the caches are not contiguous') \
        or ('' if k_cache.data_ptr() % 16 == 0 and v_cache.data_ptr() % 16 == 0 else 'the caches are not 16-byte aligned')


def position_refusal(pos: torch.Tensor) -> str:
    """Why ``pos`` is not the device position of vqhip_decode_attention_at / vqhip_decode_advance ('' if it is): one int32."""
    return '' if pos.dtype == torch.int32 and pos.numel() == 1 else f'pos must hold one int32, got {pos.dtype} {tuple(pos.shape)}'


def _attention_args(what: str, q, k, v, cos, sin, k_cache, v_cache, seen, L: int):
    """``seen``: the host count, or the int32 device tensor of the position (cos and sin are then the [cap, Dh] tables)."""
    at = torch.is_tensor(seen)
    _require_cuda(q, k, v, cos, sin, k_cache, v_cache, seen if at else None)
    _refuse(what, (position_refusal(seen) if at else '') or attention_refusal(q, k, v, cos, sin, k_cache, v_cache, 0 if at else seen, L, at))
    B, Hkv, cap, Dh = k_cache.shape

    def stride(t):
        return max(t.stride(0), t.shape[1])
    return (_ptr(q), stride(q), _ptr(k), stride(k), _ptr(v), stride(v), FLOAT_DTYPES[q.dtype], _ptr(cos), _ptr(sin), _ptr(k_cache),
            _ptr(v_cache), _ptr(seen) if at else int(seen), cap), (B, q.shape[1] // Dh, Hkv, Dh)


@_on_tensor_device
def decode_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, seen: int, scale: Optional[float] = None) -> torch.Tensor:
    """vqhip_decode_attention: one new token per batch row.  Rotates q [B, Hq Dh] and k [B, Hkv Dh] by ``cos`` / ``sin`` (fp32 [Dh]),
    stores the rounded k' and v at position ``seen`` of the caches [B, Hkv, cap, Dh] (in place) and returns the attention of q'
    over positions 0 .. seen as rows [B, Hq Dh] in q's dtype - what ``o_proj`` reads.  ``scale`` defaults to Dh ** -0.5.  One launch."""
    head, (B, Hq, Hkv, Dh) = _attention_args('decode_attention', q, k, v, cos, sin, k_cache, v_cache, seen, 1)
    out = torch.empty(B, Hq * Dh, dtype=q.dtype, device=q.device)
    check(_lib.lib().vqhip_decode_attention(*head, float(Dh ** -0.5 if scale is None else scale), B, Hq, Hkv, Dh, _ptr(out), _stream()),
          'vqhip_decode_attention')
    return out


@_on_tensor_device
def decode_attention_at(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos_table: torch.Tensor, sin_table: torch.Tensor,
                        k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, scale: Optional[float] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vqhip_decode_attention_at: ``decode_attention`` with the position read from ``pos`` (one int32 on the device) and the rotary
    rows from ``cos_table`` / ``sin_table`` (fp32 [cap, Dh]), bit for bit - a launch that a captured graph can replay for every
    generated token.  A position outside 0 .. cap - 1 writes nothing: ``out`` (a dense [B, Hq Dh] tensor to write into; a new one if
    None) and the caches are left as they are.  One launch."""
    head, (B, Hq, Hkv, Dh) = _attention_args('decode_attention_at', q, k, v, cos_table, sin_table, k_cache, v_cache, pos, 1)
    if out is None:
        out = torch.empty(B, Hq * Dh, dtype=q.dtype, device=q.device)
    elif out.shape != (B, Hq * Dh) or out.dtype != q.dtype or out.device != q.device or not out.is_contiguous():
        raise ValueError(f'decode_attention_at: out must be contiguous {q.dtype} {(B, Hq * Dh)} on {q.device}, got {out.dtype} {tuple(out.shape)}')
    check(_lib.lib().vqhip_decode_attention_at(*head, float(Dh ** -0.5 if scale is None else scale), B, Hq, Hkv, Dh, _ptr(out), _stream()),
          'vqhip_decode_attention_at')
    return out


@_on_tensor_device
def decode_advance(token: torch.Tensor, next_token: torch.Tensor, sequence: torch.Tensor, pos: torch.Tensor) -> None:
    """vqhip_decode_advance: the end of a replayed step.  With s = ``pos`` (one int32 on the device) and s + 1 < length:
    ``sequence[:, s + 1] = token`` as it is, ``next_token = max(token, 0)`` and ``pos = s + 1``; otherwise nothing.  ``token`` and
    ``next_token`` hold R int64 each, ``sequence`` is int64 [R, length]; all are written and read in place.  One launch."""
    _require_cuda(token, next_token, sequence, pos)
    R = token.numel()
    _refuse('decode_advance', position_refusal(pos)
            or ('' if sequence.dim() == 2 and sequence.shape[0] == R and next_token.numel() == R else
                f'token {tuple(token.shape)}, next {tuple(next_token.shape)} and sequence {tuple(sequence.shape)} are not R, R and [R, length]')
            or ('' if all(t.dtype == torch.int64 and t.is_contiguous() for t in (token, next_token, sequence)) else
                'token, next and sequence must be contiguous int64')
            or ('' if all(t.device == pos.device for t in (token, next_token, sequence)) else 'the tensors are on several devices'))
    check(_lib.lib().vqhip_decode_advance(_ptr(token), _ptr(next_token), _ptr(sequence), R, sequence.shape[1], _ptr(pos), _stream()),
          'vqhip_decode_advance')


@_on_tensor_device
def rope_append(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, seen: int) -> torch.Tensor:
    """vqhip_rope_append: L >= 1 new tokens per batch row, rows [B L, H Dh] (row b L + t), ``cos`` / ``sin`` fp32 [L, Dh].  Stores the
    rounded k' and v at positions seen .. seen + L - 1 of the caches (in place) and returns q' [B, Hq, L, Dh] in q's dtype, the
    layout a causal sdpa reads.  One launch."""
    L = max(cos.numel() // max(k_cache.shape[-1], 1), 1) if k_cache.dim() == 4 else 1
    head, (B, Hq, Hkv, Dh) = _attention_args('rope_append', q, k, v, cos, sin, k_cache, v_cache, seen, L)
    q_out = torch.empty(B, Hq, L, Dh, dtype=q.dtype, device=q.device)
    check(_lib.lib().vqhip_rope_append(*head, B, L, Hq, Hkv, Dh, _ptr(q_out), _stream()), 'vqhip_rope_append')
    return q_out


# ---- fused reconstruction metrics (validation: vq/runners/metrics/loss.py over vq/tasks/image_reconstruction/losses.py) -----

IMAGE_METRIC_COLUMNS = ('l1', 'mse', 'psnr', 'ssim')
SSIM_C1, SSIM_C2 = (0.01 * 1) ** 2, (0.03 * 1) ** 2           # scikit-image's (K1 * data_range) ** 2, (K2 * data_range) ** 2


def image_metrics_refusal(pred: torch.Tensor, image: torch.Tensor, ssim: bool = True) -> str:
    """Why vqhip_image_metrics would refuse this pair ('' if it would not): the clauses of its LIMITS that depend on the tensors."""
    if pred.dim() != 4 or pred.shape != image.shape:
        return f'pred and image must both be [B, C, H, W], got {tuple(pred.shape)} and {tuple(image.shape)}'
    for name, t in (('pred', pred), ('image', image)):
        if t.dtype not in IMAGE_DTYPES:
            return f'{name} is {t.dtype}, not float32, bfloat16, float16 or uint8'
    if pred.numel() == 0:
        return f'empty images {tuple(pred.shape)}'
    why = dense_refusal('pred', pred) or dense_refusal('image', image)
    if why:
        return why
    B, C, H, W = pred.shape
    if ssim and (H < 7 or W < 7):
        return f'SSIM needs H >= 7 and W >= 7 (a 7 x 7 window), got {H} x {W}'
    if ssim and C * (H - 6) * (W - 6) > _lib.IMAGE_SSIM_MAX_WINDOWS:
        return f'C (H - 6) (W - 6) = {C * (H - 6) * (W - 6)} windows are beyond the size cap of 2^22 of the fixed-point SSIM sum'
    return ''


@_on_tensor_device
def image_metrics(pred: torch.Tensor, image: torch.Tensor, *, ssim: bool = True) -> dict:
    """vqhip_image_metrics of include/vqhip.h: ``pred`` and ``image`` [B, C, H, W] - fp32 / bf16 / fp16 in the model's range
    [-1, 1], or uint8 already decoded; NCHW-contiguous or channels-last, each tensor on its own - to one row per image:
    fp32 ``l1``, ``mse``, ``psnr``, ``ssim`` [B] (columns of ``values32``), float64 ``values64`` [B, 4], int64 ``abs_sum`` and
    ``sq_sum`` [B].  Two launches, no copy of an image, no synchronisation.  ``ssim=False``: the ssim column is NaN and any
    H, W >= 1 is taken.  ValueError for what the library refuses."""
    _refuse('image_metrics', image_metrics_refusal(pred, image, ssim))
    _require_cuda(pred, image)
    B, C, H, W = pred.shape
    L, dev = _lib.lib(), pred.device
    ws_bytes = L.vqhip_image_metrics_workspace_bytes(B, C, H, W)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    values64 = torch.empty(B, 4, dtype=torch.float64, device=dev)
    values32 = torch.empty(B, 4, dtype=torch.float32, device=dev)
    sums = torch.empty(B, 2, dtype=torch.int64, device=dev)
    rc = L.vqhip_image_metrics(_ptr(pred), IMAGE_DTYPES[pred.dtype], IMAGE_LAYOUTS[dense_layout(pred)], _ptr(image),
                               IMAGE_DTYPES[image.dtype], IMAGE_LAYOUTS[dense_layout(image)], B, C, H, W, 1 if ssim else 0, SSIM_C1, SSIM_C2, _ptr(ws), ws_bytes,
                               _ptr(values64), _ptr(values32), _ptr(sums), _stream())
    if rc == -22:                                                              # VQHIP_EINVAL
        raise ValueError(f'image_metrics: {L.vqhip_last_error().decode()}')
    check(rc, 'vqhip_image_metrics')
    out = {name: values32[:, k] for k, name in enumerate(IMAGE_METRIC_COLUMNS)}
    out.update(values64=values64, values32=values32, abs_sum=sums[:, 0], sq_sum=sums[:, 1])
    return out


# ---- pooled code features (the linear probe, vq/tasks/image_classification/models.py:101-109) ----------------------------

def _pool_tokens(quant: torch.Tensor, what: str):
    """(dense tokens, token dtype code, B, HW) of ``quant`` [B, *]: positions are everything after the first dimension."""
    if quant.dim() < 2:
        raise ValueError(f'{what}: expected tokens [B, *] with at least two dimensions, got {tuple(quant.shape)}')
    if quant.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'{what}: tokens must be int32 or int64, got {quant.dtype}')
    B = quant.shape[0]
    quant = quant.reshape(B, -1).contiguous()
    return quant, (_lib.DTYPE_I32 if quant.dtype == torch.int32 else _lib.DTYPE_I64), B, quant.shape[1]


@_on_tensor_device
def decode_pool(e: torch.Tensor, quant: torch.Tensor) -> torch.Tensor:
    """features fp32 [B, D] = mean over the positions of e[quant] for tokens ``quant`` [B, *] (int32 / int64), one launch, in the
    fixed summation order of include/vqhip.h; the decoded rows are never written.  A token outside [0, K) makes its image's
    row NaN."""
    _require_cuda(e, quant)
    e = _codebook(e)
    quant, qdt, B, HW = _pool_tokens(quant, 'decode_pool')
    K, D = e.shape
    out = torch.empty(B, D, dtype=torch.float32, device=quant.device)
    check(_lib.lib().vqhip_decode_pool(_ptr(e), K, D, _ptr(quant), qdt, B, HW, _ptr(out), _stream()), 'vqhip_decode_pool')
    return out


@_on_tensor_device
def decode_pool_bwd(g: torch.Tensor, quant: torch.Tensor, K: int) -> torch.Tensor:
    """grad_e fp32 [K, D] of ``decode_pool`` from g = dL/dfeatures [B, D]: grad_e[quant[b, p]] += g[b] / HW (float atomics);
    tokens outside [0, K) contribute nothing."""
    _require_cuda(g, quant)
    quant, qdt, B, HW = _pool_tokens(quant, 'decode_pool_bwd')
    g = g.float().contiguous()
    if g.dim() != 2 or g.shape[0] != B:
        raise ValueError(f'decode_pool_bwd: expected g [{B}, D], got {tuple(g.shape)}')
    D = g.shape[1]
    grad_e = torch.zeros(K, D, dtype=torch.float32, device=g.device)
    check(_lib.lib().vqhip_decode_pool_bwd(_ptr(g), _ptr(quant), qdt, B, HW, K, D, _ptr(grad_e), _stream()), 'vqhip_decode_pool_bwd')
    return grad_e


@_on_tensor_device
def fsq_decode_pool(quant: torch.Tensor, q: _lib.FsqConstants) -> torch.Tensor:
    """features fp32 [B, C] = mean over the positions of ``fsq_decode``'s values for tokens ``quant`` [B, *] (int32 / int64), one
    launch, same summation order as ``decode_pool``; any token decodes (negative and >= K ones as ``fsq_decode`` gives them)."""
    _require_cuda(quant)
    quant, qdt, B, HW = _pool_tokens(quant, 'fsq_decode_pool')
    out = torch.empty(B, q.C, dtype=torch.float32, device=quant.device)
    check(_lib.lib().vqhip_fsq_decode_pool(ctypes.byref(q), _ptr(quant), qdt, B, HW, _ptr(out), _stream()), 'vqhip_fsq_decode_pool')
    return out


ORDERED_MAX_K = 32768     # the ordered (deterministic) route keeps one code histogram per 1024-token chunk in LDS


def use_ordered(K: int, D: int, ordered: Optional[bool] = None, N: Optional[int] = None, backward: bool = False) -> bool:
    """Policy of the codebook-side sums (k-means centroid sums, codebook gradient).  The ordered route — tokens sorted
    by code, sums in a fixed order, bit-reproducible — is taken when asked for explicitly, under
    ``torch.use_deterministic_algorithms(True)``, and by default where it is also the faster one on MI355X (measured,
    tools/bench_ordered.py): centroid sums from N >= 32768; the fused backward (``backward=True``) from N >= 131072, or
    from N >= 32768 on contended small codebooks (K <= 4096).
    Otherwise fp32 atomics.  It needs K <= 32768 and D % 4 == 0.  ``VQHIP_ORDERED=0/1`` overrides the default."""
    ok = K <= ORDERED_MAX_K and D % 4 == 0
    if ordered is None:
        if torch.are_deterministic_algorithms_enabled():
            if not ok:
                raise RuntimeError(f'vector_quantization_amd: no deterministic codebook-side sum for K={K}, D={D} '
                                   f'(needs K <= {ORDERED_MAX_K} and D % 4 == 0)')
            return True
        env = os.environ.get('VQHIP_ORDERED')
        if env is not None:
            return env != '0' and ok
        if not ok or N is None:
            return False
        if backward:
            return N >= 131072 or (K <= 4096 and N >= 32768)
        return N >= 32768
    if ordered and not ok:
        raise ValueError(f'ordered sums need K <= {ORDERED_MAX_K} and D % 4 == 0 (got K={K}, D={D})')
    return bool(ordered)


@_on_tensor_device
def token_order(idx: torch.Tensor, K: int):
    """Stable counting sort of the token ids by code: (counts int32[K], offsets int32[K+1], order int32[N])."""
    _require_cuda(idx)
    idx = idx.reshape(-1).contiguous()
    assert idx.dtype == torch.int64
    N = idx.numel()
    L = _lib.lib()
    counts = torch.empty(K, dtype=torch.int32, device=idx.device)
    offsets = torch.empty(K + 1, dtype=torch.int32, device=idx.device)
    order = torch.empty(max(N, 1), dtype=torch.int32, device=idx.device)
    ws = _bytes(L.vqhip_order_workspace_bytes(N, K), idx.device)
    check(L.vqhip_token_order(_ptr(idx), N, K, _ptr(counts), _ptr(offsets), _ptr(order), _ptr(ws), ws.numel(), _stream()),
          'vqhip_token_order')
    return counts, offsets, order[:N]


@_on_tensor_device
def segsum_rows(src: torch.Tensor, idx: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor, K: int) -> torch.Tensor:
    """out[k] = sum of src[order[p]] for p in [offsets[k], offsets[k+1]) in the fixed blocked order of the ordered route
    (fp32; see include/vqhip.h)."""
    _require_cuda(src, idx, offsets, order)
    src = src.float().contiguous()
    N, D = src.shape
    L = _lib.lib()
    out = torch.empty(K, D, dtype=torch.float32, device=src.device)
    ws = _bytes(L.vqhip_segsum_workspace_bytes(N, D), src.device)
    check(L.vqhip_segsum_rows(_ptr(src), _ptr(idx), _ptr(order), _ptr(offsets), N, K, D, _ptr(out), _ptr(ws), ws.numel(),
                              _stream()), 'vqhip_segsum_rows')
    return out


@_on_tensor_device
def scatter_add_rows(src: torch.Tensor, idx: torch.Tensor, K: int, out: Optional[torch.Tensor] = None,
                     ordered: Optional[bool] = None) -> torch.Tensor:
    """out[idx[n]] += src[n] (centroid sums / dense embedding backward).  Ordered route (see ``use_ordered``) when no
    accumulator is passed in; fp32 atomics otherwise."""
    _require_cuda(src, idx)
    src = src.float().contiguous()
    idx = idx.reshape(-1).contiguous()
    if out is None and use_ordered(K, src.shape[1], ordered, src.shape[0]):
        _, offsets, order = token_order(idx, K)
        return segsum_rows(src, idx, offsets, order, K)
    if out is None:
        out = torch.zeros(K, src.shape[1], dtype=torch.float32, device=src.device)
    check(_lib.lib().vqhip_scatter_add_rows(_ptr(src), _ptr(idx), src.shape[0], K, src.shape[1], _ptr(out), _stream()),
          'vqhip_scatter_add_rows')
    return out


@_on_tensor_device
def gather_rows(x: torch.Tensor, row_idx: torch.Tensor) -> torch.Tensor:
    _require_cuda(x, row_idx)
    x, dt = _latents(x)
    row_idx = row_idx.reshape(-1).contiguous()
    out = torch.empty(row_idx.numel(), x.shape[1], dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_gather_rows(_ptr(x), dt, _ptr(row_idx), row_idx.numel(), x.shape[1], _ptr(out), _stream()),
          'vqhip_gather_rows')
    return out


@_on_tensor_device
def vqkd_update_(w: torch.Tensor, hist64: torch.Tensor, sums: torch.Tensor, decay: float, mode: str = 'full') -> torch.Tensor:
    """In-place VQ-KD codebook update on a contiguous fp32 [K, D] tensor (mode 'centroid': k-means centroids only)."""
    _require_cuda(w, hist64, sums)
    assert w.dtype == torch.float32 and w.is_contiguous() and hist64.dtype == torch.int64
    K, D = w.shape
    hist64, sums = hist64.contiguous(), sums.contiguous()      # named: they must outlive the enqueue
    check(_lib.lib().vqhip_vqkd_update(_ptr(w), _ptr(hist64), _ptr(sums), K, D, decay,
                                       1 if mode == 'centroid' else 0, _stream()), 'vqhip_vqkd_update')
    return w


@_on_tensor_device
def cvq_update_(w: torch.Tensor, p: torch.Tensor, hist64: Optional[torch.Tensor], numel, anchors: Optional[torch.Tensor],
                ema_decay: float, eps: float, stage: int = 3) -> None:
    """In-place CVQ-VAE update; stage 1 = probability only, 2 = codebook only (from the current p), 3 = both.
    ``numel`` is an int or a device int64 scalar tensor."""
    _require_cuda(w, p)
    assert w.dtype == torch.float32 and w.is_contiguous() and p.dtype == torch.float32 and p.is_contiguous()
    K, D = w.shape
    numel_dev = numel if isinstance(numel, torch.Tensor) else None
    if numel_dev is not None:
        numel_dev = numel_dev.to(torch.int64).reshape(1)
        assert numel_dev.is_cuda
    hist64 = None if hist64 is None else hist64.contiguous()
    anchors = None if anchors is None else anchors.contiguous()
    check(_lib.lib().vqhip_cvq_update(_ptr(w), _ptr(p), _ptr(hist64), 0 if (numel_dev is not None or numel is None)
                                      else int(numel), _ptr(numel_dev), _ptr(anchors), K, D, ema_decay, eps, stage,
                                      _stream()), 'vqhip_cvq_update')


@_on_tensor_device
def cvq_step(w_in: torch.Tensor, w_out: torch.Tensor, p_in: torch.Tensor, p_out: torch.Tensor, hist32: torch.Tensor,
             numel: int, x: torch.Tensor, col_idx: torch.Tensor, ema_decay: float, eps: float) -> None:
    """The one-rank CVQ-VAE update (probability EMA, decay, NearestAnchor gather, blend) in one launch; ``w_out`` /
    ``p_out`` may be ``w_in`` / ``p_in`` themselves."""
    _require_cuda(w_in, w_out, p_in, p_out, hist32, x, col_idx)
    x, dt = _latents(x)
    K, D = w_in.shape
    for t in (w_in, w_out):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (K, D)
    for t in (p_in, p_out):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == K
    assert hist32.dtype == torch.int32 and hist32.is_contiguous() and hist32.numel() == K
    col_idx = col_idx.to(torch.int64).contiguous()
    assert col_idx.numel() == K and x.shape[1] == D
    check(_lib.lib().vqhip_cvq_step(_ptr(w_in), _ptr(w_out), _ptr(p_in), _ptr(p_out), _ptr(hist32), int(numel), _ptr(x), dt,
                                    _ptr(col_idx), K, D, ema_decay, eps, _stream()), 'vqhip_cvq_step')


@_on_tensor_device
def cvq_decay(p: torch.Tensor, K: int, ema_decay: float, eps: float) -> torch.Tensor:
    """decay_k = 1 - exp(-p_k*K*10/(1-ema_decay) - eps) with the update kernel's own expression (fp32 [K])."""
    _require_cuda(p)
    assert p.dtype == torch.float32 and p.is_contiguous()
    out = torch.empty(K, dtype=torch.float32, device=p.device)
    check(_lib.lib().vqhip_cvq_decay(_ptr(p), K, ema_decay, eps, _ptr(out), _stream()), 'vqhip_cvq_decay')
    return out


@_on_tensor_device
def cvq_update_rows_(w: torch.Tensor, p: torch.Tensor, rows: torch.Tensor, anchors_sub: torch.Tensor, ema_decay: float,
                     eps: float) -> None:
    """In place: w[rows[i]] = w[rows[i]]*decay + anchors_sub[i]*(1-decay) — stage 2 of the CVQ-VAE update for the
    listed codes only (the others have decay == 1 and would keep their weight anyway)."""
    _require_cuda(w, p, rows, anchors_sub)
    assert w.dtype == torch.float32 and w.is_contiguous() and p.dtype == torch.float32 and p.is_contiguous()
    rows = rows.to(torch.int64).contiguous()
    anchors_sub = anchors_sub.float().contiguous()
    K, D = w.shape
    assert anchors_sub.shape == (rows.numel(), D)
    check(_lib.lib().vqhip_cvq_update_rows(_ptr(w), _ptr(p), _ptr(rows), _ptr(anchors_sub), rows.numel(), K, D, ema_decay,
                                           eps, _stream()), 'vqhip_cvq_update_rows')


# ---- CVQ-VAE with anchors for the codes that can need one, and the packed exchange (include/vqhip.h) ----------------

@_on_tensor_device
def cvq_rows(p: torch.Tensor, K: int, ema_decay: float, eps: float, out=None):
    """(rows int32[K], slot int32[K], count int32[1]) — the codes whose decay can come out below 1 in the step that starts
    from the probabilities ``p`` (ascending; slot[k] = position in rows or -1).  ``out``: reuse those three tensors."""
    _require_cuda(p)
    assert p.dtype == torch.float32 and p.is_contiguous() and p.numel() == K
    if out is None:
        rows = torch.empty(K, dtype=torch.int32, device=p.device)
        slot = torch.empty(K, dtype=torch.int32, device=p.device)
        count = torch.empty(1, dtype=torch.int32, device=p.device)
    else:
        rows, slot, count = out
    check(_lib.lib().vqhip_cvq_rows(_ptr(p), K, ema_decay, eps, _ptr(rows), _ptr(slot), _ptr(count), _stream()), 'vqhip_cvq_rows')
    return rows, slot, count


@_on_tensor_device
def col_argmin_rows(x: torch.Tensor, e: torch.Tensor, rows: torch.Tensor, count: torch.Tensor, cap: int, metric='L2') -> torch.Tensor:
    """NearestAnchor indices of the listed codes only: out[i] = nearest latent of code rows[i] for i < count (int64 [cap];
    entries past the count are unspecified).  ``cap`` >= the count sizes the launches."""
    _require_cuda(x, e, rows, count)
    x, dt = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    assert rows.dtype == torch.int32 and count.dtype == torch.int32 and 0 <= cap <= K
    L = _lib.lib()
    out = torch.empty(max(cap, 1), dtype=torch.int64, device=x.device)
    if cap > 0:
        ws = _bytes(L.vqhip_col_rows_workspace_bytes(N, cap, D), x.device)
        check(L.vqhip_col_argmin_rows(_ptr(x), dt, _ptr(e), _ptr(rows), _ptr(count), cap, N, K, D, METRICS[metric], _ptr(out),
                                      _ptr(ws), ws.numel(), _stream()), 'vqhip_col_argmin_rows')
    return out[:cap]


def pack_floats(K: int, M: int, D: int) -> int:
    return int(_lib.lib().vqhip_pack_floats(K, M, D))


@_on_tensor_device
def pack_counts(hist: torch.Tensor, numel: int, packed: torch.Tensor) -> torch.Tensor:
    """Header of the packed exchange buffer from an int32 / int64 histogram and this rank's token count."""
    _require_cuda(hist, packed)
    K = hist.numel()
    assert hist.dtype in (torch.int32, torch.int64) and hist.is_contiguous()
    assert packed.dtype == torch.float32 and packed.is_contiguous() and packed.numel() >= 2 * K + 4
    check(_lib.lib().vqhip_pack_counts(_ptr(hist), 1 if hist.dtype == torch.int64 else 0, int(numel), K, _ptr(packed), _stream()),
          'vqhip_pack_counts')
    return packed


@_on_tensor_device
def unpack_counts(packed: torch.Tensor, K: int) -> torch.Tensor:
    """int64 [K + 1] = code counts ‖ token count of an (all-reduced) packed buffer."""
    _require_cuda(packed)
    assert packed.dtype == torch.float32 and packed.is_contiguous()
    out = torch.empty(K + 1, dtype=torch.int64, device=packed.device)
    check(_lib.lib().vqhip_unpack_counts(_ptr(packed), K, _ptr(out), _stream()), 'vqhip_unpack_counts')
    return out


@_on_tensor_device
def cvq_pack(hist32: torch.Tensor, numel: int, x: torch.Tensor, col_idx: torch.Tensor, count: torch.Tensor, cap: int, K: int) -> torch.Tensor:
    """This rank's packed buffer for the CVQ-VAE exchange: fp32 [2K + 4 + cap*D]."""
    _require_cuda(hist32, x)
    x, dt = _latents(x)
    D = x.shape[1]
    assert hist32.dtype == torch.int32 and hist32.is_contiguous() and hist32.numel() == K
    packed = torch.empty(pack_floats(K, cap, D), dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_cvq_pack(_ptr(hist32), int(numel), _ptr(x), dt, _ptr(col_idx) if cap else None, _ptr(count) if cap else None,
                                    cap, K, D, _ptr(packed), _stream()), 'vqhip_cvq_pack')
    return packed


@_on_tensor_device
def cvq_apply(w_in: torch.Tensor, w_out: torch.Tensor, p_in: torch.Tensor, p_out: torch.Tensor, slot: torch.Tensor,
              ema_decay: float, eps: float, hist32: Optional[torch.Tensor] = None, numel: int = 0,
              x: Optional[torch.Tensor] = None, col_idx: Optional[torch.Tensor] = None,
              packed: Optional[torch.Tensor] = None, world: int = 1, cap: Optional[int] = None) -> None:
    """The CVQ-VAE update with anchors for the listed codes (``slot``): from the all-reduced ``packed`` buffer of ``world``
    ranks, or (one rank) from ``hist32`` / ``numel`` / ``x`` / ``col_idx``.  ``w_out`` / ``p_out`` may alias the inputs.
    ``cap``: the capacity the column pass / the pack were sized for (default: what the buffers handed in hold)."""
    _require_cuda(w_in, w_out, p_in, p_out, slot)
    K, D = w_in.shape
    for t in (w_in, w_out):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (K, D)
    for t in (p_in, p_out):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == K
    assert slot.dtype == torch.int32 and slot.numel() == K
    dt = _lib.DTYPE_F32
    if packed is None:
        assert hist32 is not None and hist32.dtype == torch.int32 and hist32.is_contiguous() and numel > 0
        if x is not None:
            x, dt = _latents(x)
            assert x.shape[1] == D
    else:
        assert packed.dtype == torch.float32 and packed.is_contiguous()
    if cap is None:
        cap = (packed.numel() - (2 * K + 4)) // D if packed is not None else (col_idx.numel() if col_idx is not None else 0)
    cap = max(0, min(int(cap), K))
    check(_lib.lib().vqhip_cvq_apply(_ptr(w_in), _ptr(w_out), _ptr(p_in), _ptr(p_out), _ptr(hist32), int(numel), _ptr(x), dt,
                                     _ptr(col_idx), _ptr(packed), int(world), _ptr(slot), cap, K, D, ema_decay, eps, _stream()),
          'vqhip_cvq_apply')


SYNC_MAX_ROWS = 1 << 24


@_on_tensor_device
def cvq_col_keys(x: torch.Tensor, e: torch.Tensor, rows: torch.Tensor, count: torch.Tensor, cap: int, col_idx: torch.Tensor,
                 metric, rank: int) -> torch.Tensor:
    """NearestAnchor(sync=True) across ranks (include/vqhip.h: vqhip_cvq_col_keys): int64 [cap] keys of this rank's local column
    winners — (distance, rank, row) in torch.argmin's order, MIN-all-reducible as signed integers.  ``x`` / ``e`` are the operands
    ``col_argmin_rows`` was given."""
    _require_cuda(x, e, rows, count, col_idx)
    x, dt = _latents(x)
    e = _codebook(e)
    N, D = x.shape
    K = e.shape[0]
    keys = torch.empty(max(cap, 1), dtype=torch.int64, device=x.device)
    if cap > 0:
        check(_lib.lib().vqhip_cvq_col_keys(_ptr(x), dt, _ptr(e), _ptr(rows), _ptr(count), cap, _ptr(col_idx), N, K, D, METRICS[metric],
                                            int(rank), _ptr(keys), _stream()), 'vqhip_cvq_col_keys')
    return keys[:cap]


@_on_tensor_device
def cvq_pack_sync(hist32: torch.Tensor, numel: int, x: torch.Tensor, keys: torch.Tensor, count: torch.Tensor, cap: int, K: int,
                  rank: int) -> torch.Tensor:
    """``cvq_pack`` behind the MIN all-reduce of the keys: payload row i = x[row] on the rank the reduced key names, -0.0 elsewhere."""
    _require_cuda(hist32, x)
    x, dt = _latents(x)
    D = x.shape[1]
    assert hist32.dtype == torch.int32 and hist32.is_contiguous() and hist32.numel() == K
    packed = torch.empty(pack_floats(K, cap, D), dtype=torch.float32, device=x.device)
    check(_lib.lib().vqhip_cvq_pack_sync(_ptr(hist32), int(numel), _ptr(x), dt, _ptr(keys) if cap else None, _ptr(count) if cap else None,
                                         cap, int(rank), K, D, _ptr(packed), _stream()), 'vqhip_cvq_pack_sync')
    return packed


def _any(t: torch.Tensor):
    """Flat contiguous fp32/bf16 view + dtype code for the elementwise kernels."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    t = t.contiguous()
    return t, (_lib.DTYPE_F32 if t.dtype == torch.float32 else _lib.DTYPE_BF16)


@_on_tensor_device
def sse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """sum((a-b)^2) as a float64[1] device tensor."""
    _require_cuda(a, b)
    a, da = _any(a)
    b, db = _any(b)
    assert a.numel() == b.numel()
    out = torch.zeros(1, dtype=torch.float64, device=a.device)
    check(_lib.lib().vqhip_diff(_ptr(a), da, _ptr(b), db, a.numel(), 1.0, None, None, _ptr(out), _stream()),
          'vqhip_diff')
    return out


@_on_tensor_device
def diff_scale(a: torch.Tensor, b: torch.Tensor, scale: float, scale_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(a - b) * scale [* scale_dev] as fp32 (the MSE backward; scale_dev = upstream scalar gradient on the device)."""
    _require_cuda(a, b)
    shape = a.shape
    a, da = _any(a)
    b, db = _any(b)
    out = torch.empty(a.numel(), dtype=torch.float32, device=a.device)
    if scale_dev is not None:
        scale_dev = scale_dev.detach().float().reshape(1).contiguous()
    check(_lib.lib().vqhip_diff(_ptr(a), da, _ptr(b), db, a.numel(), float(scale), _ptr(scale_dev), _ptr(out), None,
                                _stream()), 'vqhip_diff')
    return out.view(shape)


@_on_tensor_device
def ste(x: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """x + (z - x) as fp32."""
    _require_cuda(x, z)
    shape = z.shape
    x, dx = _any(x)
    z = z.float().contiguous()
    out = torch.empty(z.numel(), dtype=torch.float32, device=z.device)
    check(_lib.lib().vqhip_ste(_ptr(x), dx, _ptr(z), z.numel(), _ptr(out), _stream()), 'vqhip_ste')
    return out.view(shape)


@_on_tensor_device
def normalize_rows_bwd(v: torch.Tensor, g: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    _require_cuda(v, g)
    v, dt = _latents(v)
    g = g.float().contiguous()
    out = torch.empty(v.shape, dtype=torch.float32, device=v.device)
    check(_lib.lib().vqhip_normalize_rows_bwd(_ptr(v), dt, _ptr(g), v.shape[0], v.shape[1], eps, _ptr(out), _stream()),
          'vqhip_normalize_rows_bwd')
    return out


@_on_tensor_device
def vq_backward(x: torch.Tensor, e: torch.Tensor, idx: torch.Tensor, g_zste: Optional[torch.Tensor],
                g_cb: Optional[torch.Tensor], g_cm: Optional[torch.Tensor], need_x: bool, need_w: bool,
                ordered: Optional[bool] = None, g_comb: Optional[torch.Tensor] = None, beta: float = 0.0):
    """Fused backward of the quantizer forward; returns (grad_x fp32 or None, grad_w fp32 [K, D] or None).  The
    codebook gradient is summed code by code in token order (``use_ordered``) or with fp32 atomics."""
    _require_cuda(x, e, idx)
    x, dt = _latents(x)
    e = _codebook(e)
    idx = idx.reshape(-1).contiguous()
    N, D = x.shape
    K = e.shape[0]
    if not need_x and not need_w:
        return None, None
    L = _lib.lib()
    gx = torch.empty(N, D, dtype=torch.float32, device=x.device) if need_x else None
    if g_zste is not None:
        g_zste = g_zste.float().contiguous()
    scal = [None if g is None else g.detach().float().reshape(1).contiguous() for g in (g_cb, g_cm, g_comb)]
    ordered_w = need_w and use_ordered(K, D, ordered, N, backward=True)
    if ordered_w and scal[2] is not None:        # the ordered kernel takes one scalar: fold the combined gradient in here
        scal[0] = scal[2] if scal[0] is None else scal[0] + scal[2]
    gw = None
    if need_w:
        gw = torch.empty(e.shape, dtype=torch.float32, device=x.device) if ordered_w else \
            torch.zeros(e.shape, dtype=torch.float32, device=x.device)
    if need_x or (need_w and not ordered_w):
        check(L.vqhip_vq_backward_ex(_ptr(x), dt, _ptr(e), _ptr(idx), N, D, _ptr(g_zste), _ptr(scal[0]), _ptr(scal[1]),
                                     _ptr(scal[2]), float(beta), _ptr(gx), None if ordered_w else _ptr(gw), _stream()),
              'vqhip_vq_backward_ex')
    if ordered_w:
        _, offsets, order = token_order(idx, K)
        ws = _bytes(L.vqhip_segsum_workspace_bytes(N, D), x.device)
        check(L.vqhip_vq_backward_w_ordered(_ptr(x), dt, _ptr(e), _ptr(idx), _ptr(order), _ptr(offsets), N, K, D,
                                            _ptr(scal[0]), _ptr(gw), _ptr(ws), ws.numel(), _stream()), 'vqhip_vq_backward_w_ordered')
    return gx, gw


def backward_map_supported(D: int, hw: int) -> bool:
    """Shapes ``vq_backward_map`` takes (whole 1 KiB channel rows per wave-instruction): HW % 256 == 0, D % 32 == 0."""
    return hw % 256 == 0 and D % 32 == 0


@_on_tensor_device
def vq_backward_map(x_rows: torch.Tensor, e: torch.Tensor, idx: torch.Tensor, shape, g_map: Optional[torch.Tensor],
                    g_cm: Optional[torch.Tensor], g_comb: Optional[torch.Tensor], beta: float, out_dtype: torch.dtype) -> torch.Tensor:
    """Gradient of the latents of a quantizer call on the NCHW map [B, D, H, W], written as that map in ``out_dtype`` (fp32 or
    bf16) from the upstream gradient ``g_map`` of the straight-through output given as the map too (include/vqhip.h:
    vqhip_vq_backward_map — no transposes, no cast)."""
    _require_cuda(x_rows, e, idx)
    b, d, h, w = shape
    x_rows, dt = _latents(x_rows)
    e = _codebook(e)
    idx = idx.reshape(-1).contiguous()
    assert tuple(x_rows.shape) == (b * h * w, d) and out_dtype in (torch.float32, torch.bfloat16)
    if g_map is not None:
        g_map = g_map.float().contiguous()
        assert tuple(g_map.shape) == (b, d, h, w)
    scal = [None if g is None else g.detach().float().reshape(1).contiguous() for g in (g_cm, g_comb)]
    out = torch.empty(b, d, h, w, dtype=out_dtype, device=x_rows.device)
    check(_lib.lib().vqhip_vq_backward_map(_ptr(x_rows), dt, _ptr(e), _ptr(idx), b, h * w, d, _ptr(g_map), _ptr(scal[0]), _ptr(scal[1]),
                                           float(beta), _ptr(out), _lib.DTYPE_F32 if out_dtype == torch.float32 else _lib.DTYPE_BF16,
                                           _stream()), 'vqhip_vq_backward_map')
    return out


@_on_tensor_device
def transpose_last2(t: torch.Tensor) -> torch.Tensor:
    """[B, R, C] -> [B, C, R] for fp32 / bf16 / fp16 tensors (the BCHW <-> (BHW)C rearrangement)."""
    _require_cuda(t)
    assert t.dim() == 3 and t.element_size() in (2, 4)
    t = t.contiguous()
    B, R, C = t.shape
    out = torch.empty(B, C, R, dtype=t.dtype, device=t.device)
    check(_lib.lib().vqhip_transpose(_ptr(t), _ptr(out), t.element_size(), B, R, C, _stream()), 'vqhip_transpose')
    return out


@_on_tensor_device
def codebook_metrics(counts: torch.Tensor) -> torch.Tensor:
    """float64[2] device tensor: (usage = nonzero/K, entropy in nats) of an int64 count vector."""
    _require_cuda(counts)
    counts = counts.to(torch.int64).contiguous()
    out = torch.empty(2, dtype=torch.float64, device=counts.device)
    check(_lib.lib().vqhip_codebook_metrics(_ptr(counts), counts.numel(), _ptr(out), _stream()), 'vqhip_codebook_metrics')
    return out


@_on_tensor_device
def debug_proposal_scores(x: torch.Tensor, cb: PreparedCodebook):
    """(scores[N, K], margin[N], scale) of the fp16 proposal pass — verification aid for the error-bound tests."""
    _require_cuda(x)
    x, dt = _latents(x)
    N, D = x.shape
    L = _lib.lib()
    scores = torch.empty(N, cb.K, dtype=torch.float32, device=x.device)
    margin = torch.empty(N, dtype=torch.float32, device=x.device)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = _bytes(L.vqhip_workspace_bytes(N, cb.K, D), x.device)
    check(L.vqhip_debug_proposal_scores(_ptr(x), dt, _ptr(cb.image), N, cb.K, D, cb.metric, _ptr(scores), _ptr(margin),
                                        _ptr(scale), _ptr(ws), ws.numel(), _stream()), 'vqhip_debug_proposal_scores')
    return scores, margin, scale
