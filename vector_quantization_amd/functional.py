"""Autograd-aware building blocks of the quantizer path.  Forward and backward arithmetic runs in libvqhip;
torch.autograd.Function is only the glue that hooks the HIP kernels into PyTorch's graph."""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops


def _as2d(t: torch.Tensor) -> torch.Tensor:
    return t if t.dim() == 2 else t.reshape(-1, t.shape[-1])


class _Embedding(Function):
    """z = W[idx] (nn.Embedding, vq/algorithms/vq/quantizers.py:107); backward = dense scatter-add into W."""

    @staticmethod
    def forward(ctx, weight: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        flat = idx.reshape(-1)
        ctx.save_for_backward(flat)
        ctx.shape = weight.shape
        z = ops.gather_rows(weight, flat)
        return z.view(*idx.shape, weight.shape[1])

    @staticmethod
    def backward(ctx, g):
        (flat,) = ctx.saved_tensors
        K, D = ctx.shape
        gw = ops.scatter_add_rows(_as2d(g), flat, K) if ctx.needs_input_grad[0] else None
        return gw, None


def embedding(weight: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return _Embedding.apply(weight, idx)


class _DecodePool(Function):
    """features[b] = mean_p W[quant[b, p]] (``decode`` + einops.reduce 'b h w c -> b c' mean of the linear probe,
    vq/tasks/image_classification/models.py:105-109) in one launch; backward = atomics into W (tokens get no gradient)."""

    @staticmethod
    def forward(ctx, weight: torch.Tensor, quant: torch.Tensor) -> torch.Tensor:
        ctx.save_for_backward(quant)
        ctx.K = weight.shape[0]
        ctx.wdtype = weight.dtype
        return ops.decode_pool(weight, quant)

    @staticmethod
    def backward(ctx, g):
        (quant,) = ctx.saved_tensors
        gw = ops.decode_pool_bwd(g, quant, ctx.K).to(ctx.wdtype) if ctx.needs_input_grad[0] else None
        return gw, None


def decode_pool(weight: torch.Tensor, quant: torch.Tensor) -> torch.Tensor:
    """fp32 [B, D] mean-pooled code embeddings of tokens ``quant`` [B, *]; the gradient goes to ``weight`` only."""
    return _DecodePool.apply(weight, quant)


class _MSE(Function):
    """mean((a-b)^2) (todd MSELoss, mean reduction; vq/algorithms/vq/losses.py:50,62)."""

    @staticmethod
    def forward(ctx, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        ctx.save_for_backward(a, b)
        sse = ops.sse(a, b)
        return (sse / a.numel()).float().reshape(())

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = ops.diff_scale(a, b, 2.0 / a.numel(), g).to(a.dtype)
        if ctx.needs_input_grad[1]:
            gb = ops.diff_scale(b, a, 2.0 / a.numel(), g).to(b.dtype)
        return ga, gb


def mse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _MSE.apply(a, b)


class _Normalize(Function):
    """F.normalize(v, dim=1, eps=1e-12) in the oracle's summation order."""

    @staticmethod
    def forward(ctx, v: torch.Tensor, eps: float) -> torch.Tensor:
        ctx.save_for_backward(v)
        ctx.eps = eps
        return ops.normalize_rows(_as2d(v), eps).view(v.shape)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        gv = ops.normalize_rows_bwd(_as2d(v), _as2d(g), ctx.eps).view(v.shape).to(v.dtype)
        return gv, None


def normalize(v: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    return _Normalize.apply(v, eps)


class _STE(Function):
    """x + (z - x).detach() (vq/tasks/image_tokenization/models/quantizers/utils/ste.py:9-10)."""

    @staticmethod
    def forward(ctx, z: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        ctx.xdtype = x.dtype
        return ops.ste(x, z)

    @staticmethod
    def backward(ctx, g):
        return None, g.to(ctx.xdtype)


def ste(z: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return _STE.apply(z, x)


class _FSQ(Function):
    """FiniteScalarQuantizer's encode (vq/algorithms/fsq/quantizers.py:110-125): x -> (z, quant) with z = ste(round(t), t) / h
    and t = (tanh(x + shift) * M - odd) / 2, one launch; the backward (one launch) recomputes tanh from x.  ``x`` is [N, C]
    rows or the NCHW-contiguous map [B, C, H, W]; z has x's layout (fp32), quant is int32 [N] (not differentiable)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, q, hist: Optional[torch.Tensor] = None):
        quant, z, _ = ops.fsq_encode(x, q, hist=hist)
        ctx.save_for_backward(x)
        ctx.q = q
        ctx.mark_non_differentiable(quant)
        return z, quant

    @staticmethod
    def backward(ctx, g, g_quant):
        (x,) = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        return ops.fsq_backward(x, g, ctx.q), None, None


def fsq(x: torch.Tensor, q, hist: Optional[torch.Tensor] = None):
    """(z fp32 with gradient to x, quant int32 [N]) of FiniteScalarQuantizer's encode; ``q`` = ops.fsq_constants(levels, eps)."""
    return _FSQ.apply(x, q, hist)


class _FusedMapDecodeLoss(Function):
    """``fused_decode_loss`` for a quantizer call on the NCHW feature map (tokenization.quantize): the straight-through
    output is written directly as the map [B, D, H, W], the loss values are those of the token form.  ``x_rows`` are the
    token-major rows the map encode produced (``ops.encode_map``); gradients flow to ``x_map`` and the codebook."""

    @staticmethod
    def forward(ctx, x_map: torch.Tensor, x_rows: torch.Tensor, weight: torch.Tensor, idx: torch.Tensor, beta: float = 0.0):
        ctx.set_materialize_grads(False)
        ctx.beta = float(beta)
        b, d, h, w = x_map.shape
        ctx.map_shape, ctx.map_dtype = (b, d, h, w), x_map.dtype
        z_map, mse = ops.gather_ste_map(x_rows, weight, idx, b, h, w, beta=beta)
        ctx.save_for_backward(x_rows, weight, idx)
        return z_map, mse[0], mse[1], mse[2]

    @staticmethod
    def backward(ctx, g_map, g_cb, g_cm, g_comb):
        x_rows, weight, idx = ctx.saved_tensors
        b, d, h, w = ctx.map_shape
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if ops.backward_map_supported(d, h * w) and ctx.map_dtype in (torch.float32, torch.bfloat16):
            # both rearrangements folded into the kernel: the upstream gradient is read as the map, the latents' gradient written
            # as the map in the map's dtype (vqhip_vq_backward_map); the codebook gradient from the token-major rows as before
            gx = ops.vq_backward_map(x_rows, weight, idx, (b, d, h, w), g_map, g_cm, g_comb, ctx.beta, ctx.map_dtype) if need_x else None
            gw = ops.vq_backward(x_rows, weight, idx, None, g_cb, g_cm, False, True, g_comb=g_comb, beta=ctx.beta)[1] if need_w else None
            return gx, None, gw, None, None
        g_tok = None
        if g_map is not None:                                    # 'b c h w -> (b h w) c' of the incoming gradient
            g_tok = ops.transpose_last2(g_map.float().contiguous().reshape(b, d, h * w)).reshape(b * h * w, d)
        gx, gw = ops.vq_backward(x_rows, weight, idx, g_tok, g_cb, g_cm, need_x, need_w, g_comb=g_comb, beta=ctx.beta)
        if gx is not None:
            gx = ops.transpose_last2(gx.reshape(b, h * w, d)).reshape(b, d, h, w).to(ctx.map_dtype)
        return gx, None, gw, None, None


def fused_map_decode_loss(x_map: torch.Tensor, x_rows: torch.Tensor, weight: torch.Tensor, idx: torch.Tensor, beta: float = 0.0):
    """Returns (z_map [B, D, H, W], m_cb, m_cm, m_cb + beta*m_cm)."""
    return _FusedMapDecodeLoss.apply(x_map, x_rows, weight, idx, beta)


class _Computed:
    """Tensors a one-call training forward (train_step.py) has already produced, handed to the autograd wrappers below
    without becoming graph inputs."""

    def __init__(self, **tensors) -> None:
        self.__dict__.update(tensors)


class _VqkdStep(Function):
    """Autograd node of the VQ-KD one-call forward: outputs xn = F.normalize(x) (what memo['x'] holds), the straight-through
    output xn + sg(z - xn) and the commitment loss mean((F.normalize(sg z) - F.normalize(xn))^2) (CommitmentLoss with
    mse norm=True); backward is ONE kernel (vqhip_vqkd_backward).  The codebook receives no gradient: the commitment term
    detaches z and the straight-through output detaches (z - xn)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, done: _Computed):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, done.xn, weight, done.idx)
        xn = done.xn.view(x.shape)
        if not ctx.needs_input_grad[0]:
            ctx.mark_non_differentiable(xn)
        return xn, done.z_ste.view(x.shape), done.mse[0]

    @staticmethod
    def backward(ctx, g_xn, g_zste, g_loss):
        from . import train_step
        x, xn, weight, idx = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = g_zste
        if g_xn is not None:                                    # a consumer of memo['x'] other than the straight-through output
            g = g_xn if g is None else g + g_xn
        gx = train_step.vqkd_backward(_as2d(x), xn, weight, idx, None if g is None else _as2d(g), g_loss)
        return gx.view(x.shape).to(x.dtype), None, None


def vqkd_step(x: torch.Tensor, weight: torch.Tensor, done: _Computed):
    """(xn, z_ste, commitment loss) tied into the autograd graph."""
    return _VqkdStep.apply(x, weight, done)


class _VqStep(Function):
    """The one autograd node of the decode / straight-through / MSE-loss tail:
        z = W[idx];  z_ste = r + sg(z - r);  m_cb = mse(z, sg r);  m_cm = mse(sg z, r)   (same value, two graph nodes)
        combined = m_cb + beta * m_cm   (VQGANLoss, losses.py:119-127 — finished inside the kernel)
    on rows r = x, or r = xn = F.normalize(x) when ``done.xn`` is given (NormalizeCallback; xn is then the first output: what
    memo['x'] holds).  The forward values come from ``done`` — a one-call forward (vqhip_vq_forward, vqhip_cvq_forward) or
    ``fused_decode_loss`` has produced them — and the node only ties them into the graph.  Backward is one fused kernel
    (vqhip_vq_backward_ex): m_cb's gradient flows to W, m_cm's and z_ste's to the rows, the combined value's to both; gradients of
    unused outputs are not materialised; then F.normalize's backward when the rows were normalised."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, done: _Computed, beta: float):
        ctx.set_materialize_grads(False)
        ctx.beta = float(beta)
        ctx.normalized = done.xn is not None
        mse = done.mse
        if ctx.normalized:
            ctx.save_for_backward(x, done.xn, weight, done.idx)
            xn = done.xn.view(x.shape)
            if not ctx.needs_input_grad[0]:                      # F.normalize(x) of latents without a graph has none either
                ctx.mark_non_differentiable(xn)
            return xn, done.z_ste.view(x.shape), mse[0], mse[1], mse[2]
        ctx.save_for_backward(x, weight, done.idx)
        return None, done.z_ste.view(x.shape), mse[0], mse[1], mse[2]

    @staticmethod
    def backward(ctx, g_xn, g_zste, g_cb, g_cm, g_comb):
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if ctx.normalized:
            x, xn, weight, idx = ctx.saved_tensors
            rows = xn
        else:
            x, weight, idx = ctx.saved_tensors
            rows = _as2d(x)
        gr, gw = ops.vq_backward(rows, weight, idx, None if g_zste is None else _as2d(g_zste), g_cb, g_cm, need_x, need_w,
                                 g_comb=g_comb, beta=ctx.beta)
        gx = None
        if need_x:
            if ctx.normalized:
                if g_xn is not None:                             # a consumer of memo['x'] other than the decode / loss tail
                    gr = _as2d(g_xn).float() if gr is None else gr + _as2d(g_xn)
                gx = ops.normalize_rows_bwd(_as2d(x), gr, 1e-12).view(x.shape).to(x.dtype)
            elif gr is not None:
                gx = gr.view(x.shape).to(x.dtype)
        return gx, gw, None, None


def vq_step(x: torch.Tensor, weight: torch.Tensor, done: _Computed, beta: float = 0.0):
    """(xn or None, z_ste, m_cb, m_cm, m_cb + beta*m_cm) of a one-call forward, tied into the autograd graph."""
    return _VqStep.apply(x, weight, done, beta)


def fused_decode_loss(x: torch.Tensor, weight: torch.Tensor, idx: torch.Tensor, beta: float = 0.0):
    """Returns (z_ste, m_cb, m_cm, m_cb + beta*m_cm): the straight-through output, the codebook / commitment MSE values and
    their VQGAN combination, from one gather kernel, tied into the graph by ``vq_step``."""
    xd = x.detach()
    if x.numel() == 0:
        _, z_ste, sse = ops.gather_ste_loss(xd, weight.detach(), idx, need_z=False, need_ste=True, need_sse=True)
        m = (sse / x.numel()).float().reshape(())                      # nan, as mse_loss of an empty tensor
        mse = (m, m.clone(), m + beta * m)
    else:
        _, z_ste, mse = ops.gather_ste_mse(xd, weight.detach(), idx, beta=beta)   # means and their combination finished inside the kernel
    return vq_step(x, weight, _Computed(xn=None, z_ste=z_ste, mse=mse, idx=idx), beta)[1:]


class _TokenCE(Function):
    """The fused token cross-entropy (vqhip_token_ce_fwd / _bwd of include/vqhip.h).  Saves ``lse`` and the logits AS GIVEN (a
    view stays a view: no copy); the backward is one launch that writes every element of the gradient."""

    @staticmethod
    def forward(ctx, logits, targets, weight, start, end, label_smoothing, ignore_index, shift, reduction):
        kw = dict(label_smoothing=label_smoothing, ignore_index=ignore_index, weight=weight, shift=shift)
        f = ops.token_ce_forward(logits, targets, start, end, **kw)
        ctx.save_for_backward(logits, targets, weight, f['lse'], f['out'])
        ctx.args, ctx.kw, ctx.reduction = (start, end), kw, reduction
        out = f['out']
        if reduction == 'mean':
            value = out[3]
        elif reduction == 'sum':
            value = out[0]
        else:
            rows = f['loss'] if weight is None else f['loss'] * weight.reshape(-1).to(torch.float32)
            value = rows.view(logits.shape[:-1])
        stats = (f['lse'], f['loss'], f['hit'], out)
        ctx.mark_non_differentiable(*stats)
        return (value.clone(),) + stats                                        # (its own storage: the statistics are outputs too)

    @staticmethod
    def backward(ctx, g, *unused):
        logits, targets, weight, lse, out = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 9
        grad = ops.token_ce_backward(logits, targets, lse, g, *ctx.args, **dict(ctx.kw, weight=weight),
                                     weight_sum=out[1:2] if ctx.reduction == 'mean' else None)
        return (grad,) + (None,) * 8


def token_cross_entropy(logits: torch.Tensor, targets: torch.Tensor, start: int = 0, end: Optional[int] = None, *,
                        label_smoothing: float = 0.0, ignore_index: int = -100, weight: Optional[torch.Tensor] = None,
                        shift: bool = False, reduction: str = 'mean', want_stats: bool = False):
    """The cross-entropy of stage-2 training in fp32 from logits of any of the three dtypes, read in place:
    ``logits`` [..., V_total] (the view rules of ``ops.sample_tokens``), ``targets`` int32 / int64 of shape ``logits.shape[:-1]``
    holding vocabulary indices in [start, end) or ``ignore_index``; ``weight`` one value per row (MAGE's mask); ``shift``: row
    (b, l) is held to ``targets[b, l + 1]`` and the last position of every sequence is ignored (HF's ``labels=tokens``).
    ``reduction``: 'mean' (sum w loss / sum w over the rows that are not ignored, divided on the device), 'sum', or 'none' (w_r
    loss_r, shaped ``logits.shape[:-1]``).  Returns the fp32 loss; with ``want_stats`` also a dict of ``lse``, per-row ``loss``
    (unweighted), ``hit``, and the device scalars ``weight_sum`` and ``hits``."""
    if reduction not in ops.TOKEN_CE_REDUCTIONS:
        raise ValueError(f'token_cross_entropy: reduction must be one of {ops.TOKEN_CE_REDUCTIONS}, got {reduction!r}')
    end = logits.shape[-1] if end is None else end
    value, lse, loss, hit, out = _TokenCE.apply(logits, targets, weight, int(start), int(end), float(label_smoothing),
                                                int(ignore_index), bool(shift), reduction)
    if not want_stats:
        return value
    shape = logits.shape[:-1]
    return value, dict(lse=lse.view(shape), loss=loss.view(shape), hit=hit.view(shape), weight_sum=out[1], hits=out[2])


class _CosineEmbed(Function):
    """The fused CosineEmbeddingLoss (vqhip_cosine_embed_fwd / _bwd of include/vqhip.h).  Saves ``stats`` and both tensors AS
    GIVEN (a view stays a view, a bf16 activation stays bf16: no copy); the backward is one launch that writes every element of
    the gradient.  The target gets no gradient (the teacher is frozen)."""

    @staticmethod
    def forward(ctx, pred, target, layout, reduction):
        f = ops.cosine_embedding_forward(pred, target, layout=layout)
        ctx.save_for_backward(pred, target, f['stats'])
        ctx.layout, ctx.reduction = layout, reduction
        if reduction == 'mean':
            return f['out'][1].clone()
        if reduction == 'sum':
            return f['out'][0].clone()
        return f['loss'].view(pred.shape[:-1] if layout != 'map' else pred.shape[:1] + pred.shape[2:])

    @staticmethod
    def backward(ctx, g):
        pred, target, stats = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        grad = ops.cosine_embedding_backward(pred, target, stats, g, layout=ctx.layout, mean=ctx.reduction == 'mean')
        return grad, None, None, None


def cosine_embedding_loss(pred: torch.Tensor, target: torch.Tensor, reduction: str = 'mean', *, layout: Optional[str] = None):
    """``F.cosine_embedding_loss(pred, target, ones)`` in fp32 from operands of any of the three dtypes, read in place:
    ``pred`` and ``target`` [..., C] ('rows', the default), or ``pred`` the NCHW-contiguous map [B, C, *positions] against
    ``target`` [B, *positions, C] ('map').  ``reduction``: 'mean' (divided on the device), 'sum', or 'none' (shaped
    ``pred.shape[:-1]``; map: [B, *positions]).  The gradient goes to ``pred`` only, in its dtype and layout."""
    if reduction not in ops.COSINE_REDUCTIONS:
        raise ValueError(f'cosine_embedding_loss: reduction must be one of {ops.COSINE_REDUCTIONS}, got {reduction!r}')
    return _CosineEmbed.apply(pred, target.detach(), layout, reduction)



class _LpipsDistance(Function):
    """The fused LPIPS tail over the list of feature pairs (vqhip_lpips_fwd / _bwd of include/vqhip.h).  Saves the features AS GIVEN
    (a bf16 activation stays bf16, channels-last stays channels-last: no copy), the weights and four floats per pixel; the backward
    is one launch per layer that writes every element of that layer's gradient.  The targets and the weights get no gradient.  The
    backward keeps nothing and changes nothing it saved: run twice on one graph it gives the same bits."""

    @staticmethod
    def forward(ctx, seed, p, n, *tensors):
        preds, targets, weights = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        value, stats = None, []
        for layer, (f, g, w) in enumerate(zip(preds, targets, weights)):
            out = ops.lpips_layer_forward(f, g, w, seed=seed, p=p, layer=layer, value=value)
            value = out['value']
            stats.append(out['stats'])
        ctx.save_for_backward(*tensors, *stats, *(() if seed is None else (seed,)))
        ctx.n, ctx.p, ctx.seeded = n, p, seed is not None
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        n = ctx.n
        saved = ctx.saved_tensors
        preds, targets, weights, stats = saved[:n], saved[n:2 * n], saved[2 * n:3 * n], saved[3 * n:4 * n]
        seed = saved[4 * n] if ctx.seeded else None
        g = g.contiguous()
        grads = [ops.lpips_layer_backward(preds[i], targets[i], weights[i], stats[i], g, seed=seed, p=ctx.p, layer=i)
                 if ctx.needs_input_grad[3 + i] else None for i in range(n)]
        return (None, None, None, *grads, *([None] * (2 * n)))


def lpips_distance(pred_features, target_features, weights, seed: Optional[torch.Tensor] = None, p: float = 0.5) -> torch.Tensor:
    """sum over the layers of mean_p sum_c m w_c (normalize(pred)_c - normalize(target)_c)^2, ``[B]`` fp32: the reference's
    ``losses_`` before its reshape, from lists of feature maps [B, C_l, H_l, W_l] of any of the three dtypes, read in place, each
    pair NCHW-contiguous or channels-last; ``weights``: one fp32 tensor of C_l elements per layer (the 1 x 1 convolutions').
    ``seed``: two 32-bit words on the device switch dropout with probability ``p`` on (another stream than torch's, the same
    distribution).  The gradient goes to the pred features only, in their dtype and layout."""
    n = len(pred_features)
    if n == 0 or len(target_features) != n or len(weights) != n:
        raise ValueError(f'lpips_distance: need as many targets and weights as pred features, got {n}, {len(target_features)}, {len(weights)}')
    return _LpipsDistance.apply(seed, float(p), n, *pred_features, *(t.detach() for t in target_features), *(w.detach() for w in weights))


# ---- StyleGAN2 discriminator ops: every backward is linear in the incoming gradient and is itself a Function, so a graph built
#      with create_graph=True (R1GradientPenalty) differentiates through it: the second derivative with respect to x is zero ----

class _BiasActBackward(Function):
    """(gx, gbias) = vqhip_bias_act_bwd(g; y).  Its derivative with respect to g is the same call on ggx + ggbias[c]."""

    @staticmethod
    def forward(ctx, g, y, need_gbias):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y)
        gx, gbias = ops.bias_act_backward(g, y, need_gbias)
        if gbias is None:
            gbias = g.new_zeros(0)
            ctx.mark_non_differentiable(gbias)
        return gx, gbias

    @staticmethod
    def backward(ctx, ggx, ggbias):
        y, = ctx.saved_tensors
        if ggbias is not None and ggbias.numel():
            shape = (1, -1) + (1,) * (y.dim() - 2)
            term = ggbias.to(y.dtype).view(shape).expand_as(y)
            ggx = term if ggx is None else ggx + term
        if ggx is None:
            return None, None, None
        return _BiasActBackward.apply(ggx, y, False)[0], None, None


class _BiasAct(Function):
    """vqhip_bias_act_fwd; saves the OUTPUT only (its sign selects the branch of the backward)."""

    @staticmethod
    def forward(ctx, x, bias):
        y = ops.bias_act(x, bias)
        ctx.save_for_backward(y)
        ctx.bias_dtype = bias.dtype
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        gx, gbias = _BiasActBackward.apply(g, y, ctx.needs_input_grad[1])
        return gx, (gbias.to(ctx.bias_dtype) if ctx.needs_input_grad[1] else None)


def bias_act(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``leaky_relu(x + bias[c], 0.2) * 2**0.5`` (mmcv's FusedBiasLeakyReLU) of a [B, C] or [B, C, H, W] activation in its dtype and
    memory format, with gradients to both; twice differentiable (the double backward is ``gg * scale * mask``)."""
    return _BiasAct.apply(x, bias)


class _Fir4Backward(Function):
    """The adjoint of the blur; its derivative is the blur."""

    @staticmethod
    def forward(ctx, g, size, pad, down):
        ctx.pad, ctx.down = pad, down
        return ops.fir4_backward(g, size, pad, down)

    @staticmethod
    def backward(ctx, gg):
        return _Fir4.apply(ops.dense(gg), ctx.pad, ctx.down), None, None, None


class _Fir4(Function):
    @staticmethod
    def forward(ctx, x, pad, down):
        ctx.pad, ctx.down, ctx.size = pad, down, tuple(x.shape[2:])
        return ops.fir4(x, pad, down)

    @staticmethod
    def backward(ctx, g):
        return _Fir4Backward.apply(g, ctx.size, ctx.pad, ctx.down), None, None


def blur(x: torch.Tensor, pad=2, down: int = 1) -> torch.Tensor:
    """``upfirdn2d(x, outer([1, 3, 3, 1]) / 64, padding=pad)`` keeping every ``down``-th output, with the exact adjoint as its
    gradient; differentiable any number of times (the blur is linear)."""
    return _Fir4.apply(x, pad, down)


class _BiasActBlurBackward(Function):
    """(gx, gbias) = vqhip_fir4_bwd(g; x, bias), linear in g.  Its derivative with respect to g is blur((ggx + ggbias[c]) * factor),
    formed from three launches of the unfused kernels (a path only a create_graph=True penalty takes)."""

    @staticmethod
    def forward(ctx, g, x, bias, pad, down):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, bias)
        ctx.pad, ctx.down = pad, down
        return ops.fir4_backward(g, x.shape[2:], pad, down, x=x, bias=bias)

    @staticmethod
    def backward(ctx, ggx, ggbias):
        x, bias = ctx.saved_tensors
        if ggbias is not None:
            term = ggbias.to(x.dtype).view(1, -1, 1, 1).expand_as(x)
            ggx = term if ggx is None else ggx + term
        if ggx is None:
            return None, None, None, None, None
        y = ops.bias_act(x, bias)                            # the sign of the activation, recomputed: nothing else was kept
        masked = _BiasActBackward.apply(ggx, y, False)[0]
        return _Fir4.apply(masked, ctx.pad, ctx.down), None, None, None, None


class _BiasActBlur(Function):
    """vqhip_fir4_fwd with a bias: blur(act(x + bias)) from one read of the convolution's output, which is what it saves."""

    @staticmethod
    def forward(ctx, x, bias, pad, down):
        ctx.save_for_backward(x, bias)
        ctx.pad, ctx.down = pad, down
        return ops.fir4(x, pad, down, bias=bias)

    @staticmethod
    def backward(ctx, g):
        x, bias = ctx.saved_tensors
        gx, gbias = _BiasActBlurBackward.apply(g, x, bias, ctx.pad, ctx.down)
        return gx, (gbias.to(bias.dtype) if ctx.needs_input_grad[1] else None), None, None


def bias_act_blur(x: torch.Tensor, bias: torch.Tensor, pad=2, down: int = 1) -> torch.Tensor:
    """``blur(bias_act(x, bias), pad, down)`` in one launch: one read of ``x``, one write of the blurred map; the backward writes
    ``gx`` and ``gbias`` in one call from the saved ``x``.  Twice differentiable."""
    return _BiasActBlur.apply(x, bias, pad, down)


# ---- GroupNorm (+ SiLU) of the VQGAN encoder and decoder: one read and one write forward; the backward recomputes the affine
#      value and the SiLU derivative from x and the saved [B, G, 2] statistics, so nothing activation-sized is kept besides x ----

class _GroupNorm(Function):
    """vqhip_group_norm_fwd / _bwd.  Nothing in a generator step differentiates it twice: the backward is once differentiable."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, act):
        y, stats = ops.group_norm(x, num_groups, weight, bias, eps, act)
        ctx.save_for_backward(x, weight, bias, stats)
        ctx.num_groups, ctx.act = num_groups, act
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight, bias, stats = ctx.saved_tensors
        gx, dgamma, dbeta = ops.group_norm_backward(g, x, stats, ctx.num_groups, weight, bias, ctx.act)
        return (gx if ctx.needs_input_grad[0] else None, dgamma.to(weight.dtype).view_as(weight) if ctx.needs_input_grad[1] else None,
                dbeta.to(bias.dtype).view_as(bias) if ctx.needs_input_grad[2] else None, None, None, None)


def group_norm_torch(x: torch.Tensor, num_groups: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6, act=None) -> torch.Tensor:
    """The same definition with ``F.group_norm`` and ``F.silu``: CPU tensors, float64, layouts that are not dense."""
    y = torch.nn.functional.group_norm(x, num_groups, weight, bias, eps)
    return torch.nn.functional.silu(y) if act == 'silu' else y


def group_norm(x: torch.Tensor, num_groups: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6, act=None) -> torch.Tensor:
    """``act(group_norm(x, num_groups, weight, bias, eps))`` with ``act`` None or 'silu', of a [B, C, ...] activation in its dtype
    and memory format: one launch reads x and writes y (two where a group is split over workgroups), fp32 arithmetic whatever the
    dtype, gradients to x, weight and bias.  A CPU tensor, float64 or a layout that is neither NCHW-contiguous nor channels-last
    dense computes the same definition in torch."""
    if act not in (None, 'silu'):                                               # ('leaky_relu' is fused behind batch statistics only)
        raise ValueError(f'group_norm: act={act!r} is neither None nor \'silu\'')
    if not x.is_cuda or ops.group_norm_refusal(x, num_groups):
        return group_norm_torch(x, num_groups, weight, bias, eps, act)
    return _GroupNorm.apply(x, weight, bias, int(num_groups), float(eps), act)


# ---- BatchNorm2d (+ LeakyReLU) of PatchGANDiscriminator in training mode: two reads and one write forward; the backward recomputes
#      the affine value and the branch from x and the saved [C, 2] statistics, so nothing activation-sized is kept besides x ----

class _BatchNorm(Function):
    """vqhip_group_norm_fwd / _bwd with batch statistics.  Outputs (y, mean, unbiased_var); the last two are the call's block, not
    differentiable.  Nothing in a discriminator step differentiates it twice (R1GradientPenalty runs in eval mode, on the torch
    route): the backward is once differentiable."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, act):
        y, stats, mean, var = ops.batch_norm(x, weight, bias, eps, act)
        ctx.save_for_backward(x, weight, bias, stats)
        ctx.act = act
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gmean, _gvar):
        x, weight, bias, stats = ctx.saved_tensors
        gx, dgamma, dbeta = ops.batch_norm_backward(g, x, stats, weight, bias, ctx.act)
        return (gx if ctx.needs_input_grad[0] else None, dgamma.to(weight.dtype).view_as(weight) if ctx.needs_input_grad[1] else None,
                dbeta.to(bias.dtype).view_as(bias) if ctx.needs_input_grad[2] else None, None, None)


def batch_norm_torch(x: torch.Tensor, running_mean, running_var, weight, bias, training: bool = True, momentum=0.1, eps: float = 1e-5,
                     act=None) -> torch.Tensor:
    """The same definition with ``F.batch_norm`` and ``F.leaky_relu(., 0.2)``: eval mode, CPU tensors, float64, layouts that are not
    dense, a module without running statistics or affine parameters.  Twice differentiable."""
    y = torch.nn.functional.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps)
    return torch.nn.functional.leaky_relu(y, 0.2) if act == 'leaky_relu' else y


def batch_norm_refusal(x: torch.Tensor, running_mean, running_var, weight, bias, training: bool, momentum) -> str:
    """Why one batch-norm site goes to torch ('' if it does not): the clauses of ``routes.patchgan_why`` that belong to a site."""
    if not training:
        return 'eval mode: the running statistics normalise, there is no kernel for that'
    if momentum is None:
        return 'momentum=None: the cumulative average needs the counter on the host'
    if running_mean is None or running_var is None:
        return 'track_running_stats=False'
    if weight is None or bias is None:
        return 'affine=False'
    return ('' if x.is_cuda else f'the activation is on device {x.device}, not on a GPU') or ops.group_norm_refusal(x, 0)


def batch_norm(x: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               training: bool = True, momentum=0.1, eps: float = 1e-5, act=None, num_batches_tracked=None) -> torch.Tensor:
    """``act(batch_norm(x))`` with ``act`` None or 'leaky_relu' (slope 0.2), of a [B, C, ...] activation in its dtype and memory
    format, as ``nn.BatchNorm2d`` computes it: in training mode from the statistics of this batch, fp32 arithmetic whatever the
    dtype, gradients to x, weight and bias (once differentiable); ``running_mean`` / ``running_var`` move by ``momentum`` towards the
    batch's mean and unbiased variance in one ``torch._foreach_lerp_`` and ``num_batches_tracked`` (if given) grows by one - no
    host synchronisation, so the step can be captured in a graph.  Whatever ``batch_norm_refusal`` names computes the same
    definition in torch."""
    if act not in (None, 'leaky_relu'):
        raise ValueError(f'batch_norm: act={act!r} is neither None nor \'leaky_relu\'')
    if batch_norm_refusal(x, running_mean, running_var, weight, bias, training, momentum):
        if training and num_batches_tracked is not None:
            num_batches_tracked.add_(1)
        if momentum is None:                                                    # the cumulative average of nn.BatchNorm2d
            if training and num_batches_tracked is None:
                raise ValueError('batch_norm: momentum=None needs num_batches_tracked')
            momentum = 1.0 / float(num_batches_tracked) if training else 0.0
        return batch_norm_torch(x, running_mean, running_var, weight, bias, training, momentum, eps, act)
    y, mean, var = _BatchNorm.apply(x, weight, bias, float(eps), act)
    with torch.no_grad():
        torch._foreach_lerp_([running_mean, running_var], [mean.to(running_mean.dtype), var.to(running_var.dtype)], float(momentum))
        if num_batches_tracked is not None:
            num_batches_tracked.add_(1)
    return y


# ---- the row ops of VQKDEncoder / VQKDDecoder: the residual add folded into the LayerNorm that follows it, and bias + GELU / tanh.
#      The norm keeps the sum s and two floats per row; the activation keeps its input: both backwards recompute the rest ----

class _AddLayerNorm(Function):
    """vqhip_add_layer_norm_fwd / _bwd.  Outputs (s, y) with a branch to add, (y,) without; the gradient arriving at s is the
    kernel's g_skip.  ``bias`` None is the RMS mode, forward and backward."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps, out_dtype):
        if bias is None:
            s, y, stats = ops.add_rms_norm(x, res, weight, eps, out_dtype)
        else:
            s, y, stats = ops.add_layer_norm(x, res, weight, bias, eps, out_dtype)
        ctx.save_for_backward(s, weight, stats)
        ctx.set_materialize_grads(False)
        ctx.res_dtype = None if res is None else res.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return (y,) if res is None else (s, y)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        s, weight, stats = ctx.saved_tensors
        g_s, g_y = (None, grads[0]) if ctx.res_dtype is None else grads
        if g_y is None:                                                         # y took no part in the loss: the add alone
            gx, dgamma, dbeta = g_s, None, None
        else:
            skip = None if g_s is None else g_s.to(s.dtype).contiguous()
            if ctx.bias_dtype is None:
                gx, dgamma = ops.add_rms_norm_backward(g_y.contiguous(), s, stats, weight, skip)
                dbeta = None
            else:
                gx, dgamma, dbeta = ops.add_layer_norm_backward(g_y.contiguous(), s, stats, weight, skip)
        need = ctx.needs_input_grad
        return (gx if need[0] else None,
                gx.to(ctx.res_dtype) if need[1] and gx is not None and ctx.res_dtype is not None else None,
                dgamma.to(weight.dtype).view_as(weight) if need[2] and dgamma is not None else None,
                dbeta.to(ctx.bias_dtype).view_as(weight) if need[3] and dbeta is not None else None, None, None)


def add_layer_norm_torch(x: torch.Tensor, res: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6,
                         out_dtype=None):
    """The same definition in the reference's lines, ``x = x + branch`` and ``norm(x)``: CPU tensors, float64, ``fused=False``."""
    s = x if res is None else x + res
    y = torch.nn.functional.layer_norm(s, (s.shape[-1],), weight, bias, eps)
    return s, (y if out_dtype is None else y.to(out_dtype))


def _vit_refusal(x: torch.Tensor) -> str:
    """Why the row kernels would not read ``x`` (made contiguous) in place: device, dtype, shape."""
    return ('' if x.is_cuda else f'the rows are on device {x.device}, not on a GPU') or ops.float_dtype_refusal('the rows are', x) \
        or ops.vit_rows_refusal('x', x.contiguous())


def _add_norm(what: str, x, res, weight, bias, eps, out_dtype, strict: bool):
    """What ``add_layer_norm`` and ``add_rms_norm`` (``bias`` None) decide alike: the refusal, ``strict``, the torch route."""
    y_dtype = out_dtype or (x.dtype if res is None else res.dtype)
    why = _vit_refusal(x) or ops.ln_pair_refusal(x, y_dtype) \
        or ('' if res is None or (res.dtype == y_dtype and res.shape == x.shape) else
            f'res is {res.dtype} {tuple(res.shape)}, not {y_dtype} {tuple(x.shape)}')
    if why:
        if strict:
            raise ValueError(f'{what}: {why}')
        if bias is None:
            return add_rms_norm_torch(x, res, weight, eps, out_dtype)
        return add_layer_norm_torch(x, res, weight, bias, eps, out_dtype)
    x, res = x.contiguous(), None if res is None else res.contiguous()
    out = _AddLayerNorm.apply(x, res, weight, bias, float(eps), y_dtype)
    return (x, out[0]) if res is None else out


def add_layer_norm(x: torch.Tensor, res: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6,
                   out_dtype=None, *, strict: bool = False):
    """``(s, y)`` with ``s = x + res`` (``x`` itself where ``res`` is None) in x's dtype and ``y = layer_norm(s, weight, bias, eps)``
    in ``out_dtype`` (default: res's dtype, else x's): one launch reads x and res and writes s and y, fp32 arithmetic whatever the
    dtypes, gradients to x, res, weight and bias.  fp32 x with a bf16 / fp16 res and y is the autocast case.  A CPU tensor, float64
    or a dtype combination the kernels do not read computes the same definition in torch - or, with ``strict`` (a module that
    has reported the fused route), raises with the reason."""
    return _add_norm('add_layer_norm', x, res, weight, bias, eps, out_dtype, strict)


def add_rms_norm_torch(x: torch.Tensor, res: Optional[torch.Tensor], weight: torch.Tensor, eps: float = 1e-5, out_dtype=None):
    """The same definition in torch, ``x = x + branch`` and the lines of transformers' ``LlamaRMSNorm`` with its one difference
    removed: the normalised rows stay fp32 through the product with ``weight`` and are rounded once (for an fp32 or float64
    stream, which is what the reference trains with, the two coincide).  CPU tensors, float64, ``fused=False``."""
    s = x if res is None else x + res
    h = s if s.dtype == torch.float64 else s.to(torch.float32)
    y = (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)) * weight.to(h.dtype)
    return s, y.to(out_dtype or s.dtype)


def add_rms_norm(x: torch.Tensor, res: Optional[torch.Tensor], weight: torch.Tensor, eps: float = 1e-5, out_dtype=None, *,
                 strict: bool = False):
    """``(s, y)`` with ``s = x + res`` (``x`` itself where ``res`` is None) in x's dtype and ``y = s / sqrt(mean(s^2) + eps) * weight``
    in ``out_dtype`` (default: res's dtype, else x's): the RMS mode of ``add_layer_norm``, one launch, fp32 arithmetic rounded once,
    gradients to x, res and weight.  The routes, the autocast rows and ``strict`` are ``add_layer_norm``'s."""
    return _add_norm('add_rms_norm', x, res, weight, None, eps, out_dtype, strict)


ROW_ACTS_TORCH = {'gelu': torch.nn.functional.gelu, 'tanh': torch.tanh}


class _RowBiasAct(Function):
    """vqhip_row_bias_act_fwd / _bwd; saves the INPUT and the bias (the backward recomputes the derivative)."""

    @staticmethod
    def forward(ctx, x, bias, act):
        ctx.save_for_backward(x, bias)
        ctx.act = act
        return ops.row_bias_act(x, bias, act)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, bias = ctx.saved_tensors
        gx, dbias = ops.row_bias_act_backward(g.contiguous(), x, bias, ctx.act, ctx.needs_input_grad[1])
        return gx if ctx.needs_input_grad[0] else None, None if dbias is None else dbias.to(bias.dtype).view_as(bias), None


def row_bias_act_torch(x: torch.Tensor, bias: torch.Tensor, act='gelu') -> torch.Tensor:
    """The same definition in torch: the bias a ``Linear`` would have added, in x's dtype, then ``F.gelu`` / ``torch.tanh``."""
    return ROW_ACTS_TORCH[act](x + bias.to(x.dtype))


def row_bias_act(x: torch.Tensor, bias: torch.Tensor, act='gelu', *, strict: bool = False) -> torch.Tensor:
    """``act(x + bias)`` of rows [..., D] with ``act`` 'gelu' (the erf form, ``nn.GELU()``) or 'tanh', in x's dtype: one launch, and a
    backward that writes ``gx`` and the bias gradient in one pass from the saved ``x``.  A CPU tensor, float64 or rows the kernels
    do not read compute the same definition in torch - or, with ``strict``, raise with the reason."""
    if act not in ROW_ACTS_TORCH:
        raise ValueError(f'row_bias_act: act={act!r} is neither \'gelu\' nor \'tanh\'')
    why = _vit_refusal(x)
    if why:
        if strict:
            raise ValueError(f'row_bias_act: {why}')
        return row_bias_act_torch(x, bias, act)
    return _RowBiasAct.apply(x.contiguous(), bias, act)


class _SwiGLU(Function):
    """vqhip_row_bias_act_fwd / _bwd with act = VQHIP_ROW_ACT_SWIGLU; saves the INPUT (the backward recomputes the sigmoid)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.swiglu(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return ops.swiglu_backward(g.contiguous(), x)


def swiglu_torch(gate_up: torch.Tensor) -> torch.Tensor:
    """The same definition in torch: ``act_fn(gate_proj(x)) * up_proj(x)`` of transformers' ``LlamaMLP`` on the two halves."""
    gate, up = gate_up.chunk(2, dim=-1)
    return torch.nn.functional.silu(gate) * up


def swiglu(gate_up: torch.Tensor, *, strict: bool = False) -> torch.Tensor:
    """``silu(gate) * up`` of rows [..., 2 F] = (gate | up), [..., F] in the rows' dtype: one launch, fp32 arithmetic rounded once (no
    bf16 intermediate), and a backward that writes both halves of the gradient in one launch from the saved input.  A CPU tensor,
    float64 or rows the kernels do not read compute the same definition in torch - or, with ``strict``, raise with the reason."""
    why = ('' if gate_up.is_cuda else f'the rows are on device {gate_up.device}, not on a GPU') \
        or ops.float_dtype_refusal('the rows are', gate_up) or ops.swiglu_refusal('x', gate_up.contiguous())
    if why:
        if strict:
            raise ValueError(f'swiglu: {why}')
        return swiglu_torch(gate_up)
    return _SwiGLU.apply(gate_up.contiguous())


# ---- the attention step of cached generation behind a kv_cache.StaticKVCache: rotary + append, and one token's attention over
#      the cache.  Inference ops: no autograd ----

def _rope_torch(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """transformers' ``apply_rotary_pos_emb`` on one tensor: ``x * cos + rotate_half(x) * sin``."""
    half = x.shape[-1] // 2
    return x * cos + torch.cat((-x[..., half:], x[..., :half]), -1) * sin


def _attn_compute_dtype(q: torch.Tensor):
    return torch.float64 if q.dtype == torch.float64 else torch.float32


def rope_append_torch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache, layer: int):
    """The same definition in torch, any device and dtype (float64 computes in float64, everything else in fp32): see ``rope_append``."""
    kc, vc, seen = cache.layer(layer)
    B, Hkv, _, Dh = kc.shape
    L = q.shape[0] // B
    cache.require_room(L)
    ct = _attn_compute_dtype(q)
    cos, sin = cos.reshape(1, L, 1, Dh).to(ct), sin.reshape(1, L, 1, Dh).to(ct)
    q_rot = _rope_torch(q.reshape(B, L, -1, Dh).to(ct), cos, sin)
    k_rot = _rope_torch(k.reshape(B, L, Hkv, Dh).to(ct), cos, sin)
    kc[:, :, seen:seen + L] = k_rot.transpose(1, 2).to(kc.dtype)
    vc[:, :, seen:seen + L] = v.reshape(B, L, Hkv, Dh).transpose(1, 2).to(vc.dtype)
    return q_rot.transpose(1, 2).to(q.dtype).contiguous()


def decode_attention_torch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache, layer: int, *,
                           scale: Optional[float] = None) -> torch.Tensor:
    """The same definition in torch, any device and dtype (float64 computes in float64, everything else in fp32): see
    ``decode_attention``.  The step's own key enters the scores as stored, after its rounding to the cache's dtype."""
    kc, vc, seen = cache.layer(layer)
    cache.require_room(1)
    return _decode_attention_at(q, k, v, cos, sin, kc, vc, seen, scale)


def _decode_attention_at(q, k, v, cos, sin, kc, vc, seen: int, scale: Optional[float]) -> torch.Tensor:
    """``decode_attention_torch`` at position ``seen`` of the caches ``kc``, ``vc``, with that position's ``cos``, ``sin``."""
    B, Hkv, _, Dh = kc.shape
    ct = _attn_compute_dtype(q)
    cos, sin = cos.reshape(1, 1, Dh).to(ct), sin.reshape(1, 1, Dh).to(ct)
    q_rot = _rope_torch(q.reshape(B, -1, Dh).to(ct), cos, sin)                  # stays in the compute dtype
    Hq = q_rot.shape[1]
    kc[:, :, seen] = _rope_torch(k.reshape(B, Hkv, Dh).to(ct), cos, sin).to(kc.dtype)
    vc[:, :, seen] = v.reshape(B, Hkv, Dh).to(vc.dtype)
    keys = kc[:, :, :seen + 1].to(ct).repeat_interleave(Hq // Hkv, dim=1)       # query head h reads kv head h // (Hq // Hkv)
    values = vc[:, :, :seen + 1].to(ct).repeat_interleave(Hq // Hkv, dim=1)
    s = torch.einsum('bhd,bhnd->bhn', q_rot, keys) * (Dh ** -0.5 if scale is None else scale)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    out = torch.einsum('bhn,bhnd->bhd', p, values) / p.sum(-1, keepdim=True)
    return out.reshape(B, Hq * Dh).to(q.dtype)


def decode_attention_at_torch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos_table: torch.Tensor, sin_table: torch.Tensor, cache,
                              layer: int, *, scale: Optional[float] = None) -> torch.Tensor:
    """``decode_attention_at`` in torch: ``decode_attention_torch`` at the position ``cache.position`` holds, read with ``.item()`` -
    a host synchronisation, so this serves CPU and float64 tensors (the tests, the ``torch_ops`` walk), never a capture.  A
    position outside the cache writes nothing and returns zeros."""
    kc, vc, _ = cache.layer(layer)
    s = int(cache.position.item())
    if not 0 <= s < kc.shape[2]:
        return q.new_zeros(kc.shape[0], q.shape[1])
    return _decode_attention_at(q, k, v, cos_table[s], sin_table[s], kc, vc, s, scale)


def decode_advance_torch(token: torch.Tensor, next_token: torch.Tensor, sequence: torch.Tensor, pos: torch.Tensor) -> None:
    """``decode_advance`` in torch (``pos`` read with ``.item()``): see there."""
    s = int(pos.item())
    if 0 <= s and s + 1 < sequence.shape[1]:
        sequence[:, s + 1] = token.reshape(-1)
        next_token.copy_(token.clamp(min=0).reshape(next_token.shape))
        pos.fill_(s + 1)


def _attention_refusal(what: str, q, k, v, cos, sin, cache, layer: int, L: int, tables: bool = False) -> str:
    """Why the kernels would not take this step ('' if they would); inputs that require grad raise here: these ops have no backward."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        raise ValueError(f'{what}: q, k or v requires grad and grad mode is on: an inference op without a backward')
    kc, vc, seen = cache.layer(layer)
    return ('' if q.is_cuda else f'q is on device {q.device}, not on a GPU') or ops.float_dtype_refusal('q is', q) \
        or ('' if kc.device == q.device else f'the cache is on device {kc.device}, q on {q.device}') \
        or ops.attention_refusal(q, k, v, cos, sin, kc, vc, seen, L, tables)


def _fp32_table(t: torch.Tensor, L: int) -> torch.Tensor:
    """cos or sin as the kernels read it: contiguous fp32 [L, Dh] (no copy where ``LlamaRotaryEmbedding`` returned fp32)."""
    return t.reshape(L, -1).to(torch.float32).contiguous()


def decode_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache, layer: int, *,
                     scale: Optional[float] = None, strict: bool = False) -> torch.Tensor:
    """One generated token's attention step behind ``cache`` (a ``StaticKVCache``), layer ``layer``, in one launch: rotates ``q``
    [B, Hq Dh] and ``k`` [B, Hkv Dh] by ``cos`` / ``sin`` [Dh] (``rotate_half`` convention, fp32), stores the rounded k' and ``v`` at
    the cache's position ``seen`` in place, and returns softmax(scale q' K^T) V over positions 0 .. seen with grouped-query heads as
    rows [B, Hq Dh] in q's dtype - what ``o_proj`` reads.  q, k and v may be views into one packed GEMM output.  The caller
    advances the cache once per model step.  CPU tensors, float64 and shapes the kernel does not take compute the same definition
    in torch - or, with ``strict``, raise with the reason.  No autograd."""
    cos32, sin32 = _fp32_table(cos, 1), _fp32_table(sin, 1)
    why = _attention_refusal('decode_attention', q, k, v, cos32, sin32, cache, layer, 1)
    if why:
        if strict:
            raise ValueError(f'decode_attention: {why}')
        return decode_attention_torch(q, k, v, cos, sin, cache, layer, scale=scale)
    kc, vc, seen = cache.layer(layer)
    return ops.decode_attention(q, k, v, cos32, sin32, kc, vc, seen, scale)


def decode_attention_at(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos_table: torch.Tensor, sin_table: torch.Tensor, cache,
                        layer: int, *, scale: Optional[float] = None, strict: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``decode_attention`` with the position read on the device: ``cache.position`` (one int32, counted by ``decode_advance``) in
    place of the host count, and row ``position`` of ``cos_table`` / ``sin_table`` (contiguous fp32 [capacity, Dh]:
    ``LlamaRotaryEmbedding`` over ``arange(capacity)``, before its cast) in place of one position's cos and sin.  Bit for bit what
    ``decode_attention`` gives at ``seen == position``, in one launch that a captured graph can replay for every generated
    token.  A position outside the cache writes nothing - neither the caches nor ``out`` (optional: a dense [B, Hq Dh] tensor to
    write into).  The host count is not read and not advanced.  Routes and ``strict`` as ``decode_attention``."""
    why = _attention_refusal('decode_attention_at', q, k, v, cos_table, sin_table, cache, layer, 1, tables=True)
    if why:
        if strict:
            raise ValueError(f'decode_attention_at: {why}')
        got = decode_attention_at_torch(q, k, v, cos_table, sin_table, cache, layer, scale=scale)
        return got if out is None else out.copy_(got)
    kc, vc, _ = cache.layer(layer)
    return ops.decode_attention_at(q, k, v, cos_table, sin_table, kc, vc, cache.position, scale, out)


def decode_advance(token: torch.Tensor, next_token: torch.Tensor, sequence: torch.Tensor, pos: torch.Tensor, *, strict: bool = False) -> None:
    """The end of a replayed generation step, in one launch: with s = ``pos`` (one int32 on the device) and s + 1 < length, writes
    the sampled ``token`` (R int64) into column s + 1 of ``sequence`` (int64 [R, length]) as it is - the sampler's -1 for a bad row
    stays visible -, into ``next_token`` (R int64, the next step's input) with negatives clamped to 0, and counts ``pos`` to s + 1.
    At the last column, or with a position outside the sequence, nothing is written.  CPU tensors compute the same in torch - or,
    with ``strict``, raise."""
    why = '' if all(t.is_cuda for t in (token, next_token, sequence, pos)) else 'a tensor is not on a GPU'
    if why:
        if strict:
            raise ValueError(f'decode_advance: {why}')
        return decode_advance_torch(token, next_token, sequence, pos)
    return ops.decode_advance(token, next_token, sequence, pos)


def rope_append(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache, layer: int, *,
                strict: bool = False) -> torch.Tensor:
    """The prefill form of ``decode_attention``'s storage step, for L >= 1 new tokens per batch row in one launch: rows [B L, H Dh]
    (row b L + t), ``cos`` / ``sin`` [L, Dh].  Stores the rounded k' and ``v`` at positions seen .. seen + L - 1 of the cache in place
    and returns q' [B, Hq, L, Dh] in q's dtype for a causal sdpa over the cache's first positions.  Routes and ``strict`` as
    ``decode_attention``."""
    L = max(q.shape[0] // max(cache.batch, 1), 1)
    cos32, sin32 = _fp32_table(cos, L), _fp32_table(sin, L)
    why = _attention_refusal('rope_append', q, k, v, cos32, sin32, cache, layer, L)
    if why:
        if strict:
            raise ValueError(f'rope_append: {why}')
        return rope_append_torch(q, k, v, cos, sin, cache, layer)
    kc, vc, seen = cache.layer(layer)
    return ops.rope_append(q, k, v, cos32, sin32, kc, vc, seen)
