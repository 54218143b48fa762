"""Which route a quantizer step takes: the one place that decides, and says why.

A decision returns ``Route(name, why)``.  ``why`` is empty when the fastest route of that decision is taken; otherwise it names
the first clause that refused it.  Every clause is written once, as a function that returns '' or the reason.  A decision has
a configuration part, which reads only the module (usable on a module built on the CPU), and an input part (tensor device,
shape, dtype, alignment, the probability buffer, the world size, train / eval).  Both are evaluated on every call.

    step          one_call_plain | one_call_cvq | one_call_vqkd | fused_tail | hooks
    cvq_update    sparse | dense_one_launch | reference
    map_entry     map | tokens
    decode_entry  map | tokens
    pooled_entry  pooled | rows
    sampler_why   fused | torch
    token_ce_why  fused | torch
    image_metrics_why  fused | torch
    cosine_embedding_why  fused | torch
    lpips_why             fused | torch
    stylegan2_why         fused | torch
    patchgan_why          fused | torch
    group_norm_why        fused | torch
    vit_why               fused | torch
    multinomial_anchor_why  fused | matrix
    llama_why             fused | torch
    llama_decode_why      decode | walk | torch
    llama_graph_why       graph | decode (| what llama_decode_why refuses)
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import exchange, ops
from ..utils import autocast_dtype, exchanging, get_world_size
# (the three modules, not names out of them: each of them imports this module the same way, so neither side of the cycle reads an
#  attribute of the other before a call, and any of the four may be imported first)
from . import callbacks as _cb, scalar_quantizer as _sq, vector_quantizer as _vq
from .anchors import MultinomialAnchor, NearestAnchor
from .distances import CosineDistance, L2Distance, LazyDistance
from .losses import CodebookLoss, CommitmentLoss, VQGANLoss
from .memo import get_memo
from .quantizer_api import BaseQuantizer


class Route(NamedTuple):
    name: str
    why: str = ''


DECODE_LOSS_HOOKS = ('before_decode', 'after_decode', 'before_loss', 'after_loss')


# ---- the clauses: '' or the reason ---------------------------------------------------------------------------------------

def token_rows(x: torch.Tensor) -> str:
    """[N, D] rows on a device, with a row count the kernels index in 32 bits."""
    if x.dim() != 2:
        return f'the latents are {x.dim()}-D, not [N, D] token rows'
    if not x.is_cuda:
        return f'the latents are on device {x.device}, not on a GPU'
    if not 0 < x.shape[0] < (1 << 31):
        return f'N={x.shape[0]} is outside 1 .. 2^31-1'
    return ''


def dense_codebook(w: torch.Tensor) -> str:
    if not w.is_cuda:
        return f'the codebook is on device {w.device}, not on a GPU'
    if w.dtype != torch.float32:
        return f'the codebook is {w.dtype}, not float32'
    return '' if w.is_contiguous() else 'the codebook is not contiguous'


def nchw_map(x: torch.Tensor, D: int, aligned: bool) -> str:
    """A map [B, D, H, W] the kernels read as it is (``aligned``: the encode reads it in 16-byte pieces; FSQ's does not)."""
    if x.dim() != 4:
        return f'the map is {x.dim()}-D, not [B, C, H, W]'
    if not x.is_cuda:
        return f'the map is on device {x.device}, not on a GPU'
    if not x.is_contiguous():
        return 'the map is not NCHW-contiguous'
    if x.dtype not in (torch.float32, torch.bfloat16):
        return f'the map is {x.dtype}, not float32 or bfloat16'
    if x.shape[1] != D:
        return f'C={x.shape[1]} is not embedding_dim={D}'
    return 'the map is not 16-byte aligned' if aligned and x.data_ptr() % 16 else ''


def no_module_hooks(q, forward_hooks: bool = True) -> str:
    """A route that is called directly, not through nn.Module.__call__, or that folds the first hook-by-hook step away, would
    bypass a registered hook (the one-shot lazy-init pre-hook of LazyInitWeightsMixin, or anything a user attached)."""
    if len(q._forward_pre_hooks) > 0:
        return 'forward pre-hook registered (lazy init pending)'
    return 'forward hook registered' if forward_hooks and len(q._forward_hooks) > 0 else ''


def own(obj, base: type, *names: str) -> str:
    """``type(obj)`` has not overridden ``base``'s methods ``names``."""
    for name in names:
        if getattr(type(obj), name) is not getattr(base, name):
            return f'{type(obj).__name__} overrides {name}'
    return ''


def leaves(callbacks, *hooks: str) -> str:
    """No callback of the ComposedCallback ``callbacks`` customises one of ``hooks``."""
    for cb in callbacks.callbacks:
        why = own(cb, _cb.BaseCallback, *hooks)
        if why:
            return why
    return ''


def proposal_image(D: int) -> str:
    return '' if ops.coarse_supported(D) else f'D={D} has no proposal image'


def fused_distance(q, *kinds: type) -> str:
    return '' if type(q.distance) in kinds else f'{type(q.distance).__name__} has no fused encode for this step'


def is_token_major(x: torch.Tensor) -> bool:
    """True when a [B,C,H,W] tensor is stored channels-last, i.e. its memory already is the [(B H W), C] token matrix."""
    return x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous()


def fused(q) -> str:
    return '' if q._fused else 'fused=False'


def with_ema(cb) -> str:
    return '' if cb.with_ema else 'ema=None'


def nearest_anchor(cb) -> str:
    return '' if type(cb._anchor) is NearestAnchor else f'the anchor is {type(cb._anchor).__name__}, not NearestAnchor'


def fp32_device_probabilities(p: torch.Tensor) -> str:
    return '' if p.is_cuda and p.dtype == torch.float32 else f'the probabilities are {p.dtype} on device {p.device}, not float32 on a GPU'


def no_cache(q) -> str:
    return 'cache_codebook=True' if q._cache_codebook else ''


def training(q) -> str:
    return '' if q.training else 'eval mode: there is no codebook update to fold in'


def packed_world() -> str:
    world = get_world_size()
    return f'world size {world} is beyond the packed exchange ({exchange.MAX_WORLD})' if world > exchange.MAX_WORLD else ''


def probability(cb) -> str:
    """The fp32 device probabilities of a CVQVAECallback (registered by init_weights in train mode, or loaded)."""
    if '_probability' not in cb.quantizer._buffers:
        return 'no probability buffer yet (init_weights in train mode registers it)'
    return fp32_device_probabilities(cb.probability)


# ---- decode + loss as one kernel ------------------------------------------------------------------------------------------

def tail(q) -> str:
    """'' when nothing customises decode or loss: VectorQuantizer — gather, STE and the plain MSE losses are one kernel with one
    backward; FiniteScalarQuantizer — no loss at all, so forward_map returns the encode's z map."""
    if isinstance(q, _sq.FiniteScalarQuantizer):
        return (leaves(q._callbacks, *DECODE_LOSS_HOOKS) or ('a loss is configured' if len(q._losses) > 0 else '')
                or own(q, _sq.FiniteScalarQuantizer, '_decode', 'decode') or own(q, BaseQuantizer, '_loss', 'loss', 'forward'))
    why = fused(q) or leaves(q._callbacks, *DECODE_LOSS_HOOKS) \
        or own(q, _vq.VectorQuantizer, '_decode') or own(q, BaseQuantizer, '_loss')
    if why:
        return why
    for name, loss in q._losses.items():
        if not (isinstance(loss, (VQGANLoss, CodebookLoss, CommitmentLoss)) and loss.plain):
            return f'loss {name!r} is not a plain MSE loss'
    return ''


# ---- step ------------------------------------------------------------------------------------------------------------------

def _sparse_flow_config(cb) -> str:
    if cb._sparse_anchors is False:
        return 'sparse_anchors=False'
    return nearest_anchor(cb) or proposal_image(cb.quantizer.embedding_dim)


def _sparse_flow_input(cb, tokens: int) -> str:
    if cb._sync_exchange() and tokens > ops.SYNC_MAX_ROWS:               # a key holds the row in 24 bits (include/vqhip.h)
        return f'N={tokens} is beyond the synchronised anchor exchange ({ops.SYNC_MAX_ROWS})'
    return packed_world() or probability(cb)


def _cvq_forward_config(cb) -> str:
    q = cb.quantizer
    return with_ema(cb) or fused_distance(q, L2Distance, CosineDistance) or no_cache(q) or _sparse_flow_config(cb)


def _cvq_forward_input(cb, x: torch.Tensor) -> str:
    why = training(cb.quantizer) or _sparse_flow_input(cb, x.shape[0])
    if why:
        return why
    p = cb.probability
    if not p.is_contiguous():
        return 'the probabilities are not contiguous'
    if p.device != x.device:
        return f'the probabilities are on device {p.device}, the latents on {x.device}'
    return dense_codebook(cb.quantizer.embedding.weight)


def _vqkd_forward_config(cb) -> str:
    q = cb.quantizer
    return with_ema(cb) or fused_distance(q, CosineDistance) or proposal_image(q.embedding_dim) or no_cache(q) \
        or no_module_hooks(q, forward_hooks=False)


def _vqkd_forward_input(cb, x: torch.Tensor) -> str:
    return training(cb.quantizer) or packed_world() or dense_codebook(cb.quantizer.embedding.weight)


def callback_forward_why(cb, x: torch.Tensor) -> str:
    """The callback's own part of one_call_cvq / one_call_vqkd (``cb.fused_forward_ok``): '' when it can enqueue this step by one call."""
    if isinstance(cb, _cb.CVQVAECallback):
        return token_rows(x) or _cvq_forward_config(cb) or _cvq_forward_input(cb, x)
    return token_rows(x) or _vqkd_forward_config(cb) or _vqkd_forward_input(cb, x)


def _one_call_config(q) -> tuple[str, str, str]:
    """(the one-call route this configuration is made for, why it does not take it, the route of a step that does not)."""
    tail_why = tail(q)
    fallback = 'hooks' if tail_why else 'fused_tail'
    cbs = q._callbacks.callbacks
    why = ('' if q.one_call_steps else 'one_call_steps=False') or fused(q) \
        or (f'{len(cbs)} callbacks' if len(cbs) > 1 else '') \
        or own(q, _vq.VectorQuantizer, '_encode', '_decode') or own(q, BaseQuantizer, '_loss', 'encode')
    if why:
        return '', why, fallback
    kind = type(cbs[0]) if cbs else None
    if kind is None or kind is _cb.NormalizeCallback:
        # no update callback (VQGAN: configs/vqgan/model.py:19-23), or NormalizeCallback alone (LlamaGen: configs/llamagen/
        # vqgan.py:18-20), train and eval alike: vqhip_vq_forward
        return 'one_call_plain', tail_why or no_cache(q) or fused_distance(q, L2Distance, CosineDistance), fallback
    if kind is _cb.CVQVAECallback:               # the sparse-anchor flow as one call: vqhip_cvq_forward
        return 'one_call_cvq', tail_why or _cvq_forward_config(cbs[0]), fallback
    if kind is _cb.VQKDCallback:                 # VQKDCallback + CommitmentLoss(norm=True) (configs/vqkd/model.py:20-26): vqhip_vqkd_forward
        losses = list(q._losses.values())
        ok = (len(losses) == 1 and type(losses[0]) is CommitmentLoss and losses[0]._mse.norm
              and losses[0]._mse._weight._value == 1.0 and losses[0]._weight._value == 1.0)
        return 'one_call_vqkd', ('' if ok else 'the loss is not one CommitmentLoss(norm=True) of weight 1') or _vqkd_forward_config(cbs[0]), fallback
    return '', f'{kind.__name__} has no one-call forward', fallback


def step_config(q) -> Route:
    """The configuration part of ``step``: the route of a training step on device rows."""
    if not isinstance(q, _vq.VectorQuantizer):        # (hook by hook is all there is: its fastest route)
        return Route('hooks')
    name, why, fallback = _one_call_config(q)
    return Route(fallback, why) if why else Route(name)


def step(q, x: torch.Tensor) -> Route:
    """How ``forward`` runs: one library call (train_step.py), encode hook by hook + the fused decode/loss tail, or hook by hook."""
    if not isinstance(q, _vq.VectorQuantizer):
        return step_config(q)
    name, why, fallback = _one_call_config(q)
    why = token_rows(x) or why
    if not why:
        if name == 'one_call_plain':
            why = dense_codebook(q.embedding.weight)
        else:
            why = (_cvq_forward_input if name == 'one_call_cvq' else _vqkd_forward_input)(q._callbacks.callbacks[0], x)
        if not why:
            return Route(name)
    return Route(fallback if x.dim() == 2 else 'hooks', why)


# ---- the CVQ-VAE update of a hook-by-hook step -------------------------------------------------------------------------------

def _dense_update_config(cb) -> str:
    return nearest_anchor(cb) or ('the anchor is synchronised' if cb._anchor._sync else '')


def cvq_update_config(cb) -> Route:
    why = _sparse_flow_config(cb)
    if not why:
        return Route('sparse')
    dense = _dense_update_config(cb)
    return Route('reference', why if dense == why else f'{why}; {dense}') if dense else Route('dense_one_launch', why)


def cvq_update(cb, d, hist32) -> Route:
    """CVQVAECallback.after_encode: anchors for the listed codes only (`_sparse_step`), the dense update in one launch
    (vqhip_cvq_step, one rank), or the reference's staged data flow."""
    epilogue = ('' if isinstance(d, LazyDistance) else 'memo distance is a matrix, not the lazy handle of the fused encode') \
        or ('' if hist32 is not None else 'the encode left no histogram')
    why = epilogue or _sparse_flow_config(cb) or _sparse_flow_input(cb, d.shape[0])
    if not why:
        return Route('sparse')
    dense = ('an exchange between ranks is active' if exchanging() else '') or _dense_update_config(cb) or epilogue
    dense = dense or fp32_device_probabilities(cb.probability)
    return Route('reference', why if dense == why else f'{why}; {dense}') if dense else Route('dense_one_launch', why)


# ---- the NCHW map entry points (tokenization.quantize / encode_to_quant / decode_from_quant) -----------------------------------

def map_config(q, decode: bool) -> str:
    """'' when nothing in the module needs the token matrix before the encode, no hook would be bypassed (the map entry points
    are not called through nn.Module.__call__) and, for ``decode``, the tail is the fused one."""
    if isinstance(q, _vq.VectorQuantizer):
        # (NormalizeCallback rewrites the latents before the encode: the normalised rows are a new token-major tensor anyway)
        why = no_cache(q) or own(q, _vq.VectorQuantizer, '_encode') \
            or ('' if hasattr(q._distance, 'encode_map') else f'{type(q._distance).__name__} has no encode_map') \
            or no_module_hooks(q) or leaves(q._callbacks, 'before_encode') or proposal_image(q.embedding_dim)
    elif isinstance(q, _sq.FiniteScalarQuantizer):
        why = own(q, _sq.FiniteScalarQuantizer, '_encode') or no_module_hooks(q) or leaves(q._callbacks, 'before_encode', 'after_encode')
    else:
        return f'{type(q).__name__} has no map entry points'
    return why or (tail(q) if decode else '')


def map_why(q, x: torch.Tensor, decode: bool = False) -> str:
    """'' when ``encode_map`` (``decode``: ``forward_map``) can take the NCHW map ``x`` as it is."""
    if not isinstance(q, (_vq.VectorQuantizer, _sq.FiniteScalarQuantizer)):
        return map_config(q, decode)
    return nchw_map(x, q.embedding_dim, aligned=isinstance(q, _vq.VectorQuantizer)) or map_config(q, decode)


def map_entry(q, x: torch.Tensor, decode: bool) -> Route:
    """tokenization.quantize (``decode``) / encode_to_quant: the map goes to the quantizer as it is, or through the token matrix."""
    why = ('the map is channels-last: its memory already is the token matrix' if is_token_major(x) else '') or map_why(q, x, decode)
    return Route('tokens', why) if why else Route('map')


def decode_config(q) -> str:
    if isinstance(q, _vq.VectorQuantizer):
        return fused(q) or own(q, _vq.VectorQuantizer, '_decode') or leaves(q._callbacks, *DECODE_LOSS_HOOKS)
    if isinstance(q, _sq.FiniteScalarQuantizer):
        return tail(q)
    return f'{type(q).__name__} has no decode_map'


def decode_entry(q, quant: torch.Tensor, memo: dict, token_major: bool) -> Route:
    """tokenization.decode_from_quant: tokens [B, H, W] decoded straight into the NCHW map, or rows first."""
    why = ('' if quant.is_cuda else f'the tokens are on device {quant.device}, not on a GPU') or decode_config(q) \
        or ('token_major=True asks for the channels-last view of the rows' if token_major else '')
    if not why and isinstance(q, _vq.VectorQuantizer):
        why = 'autograd is on: decode_map gives no gradient' if torch.is_grad_enabled() else ''
    elif not why:
        why = "memo['encode']['z'] is there to be handed on" if 'z' in get_memo(get_memo(memo, 'quantizer'), 'encode') else ''
    return Route('tokens', why) if why else Route('map')


# ---- pooled code features (tokenization.pool_from_quant / pooled_features) ------------------------------------------------------

def pooled_config(q) -> str:
    """'' when ``decode`` is the plain one — the codebook gather (FiniteScalarQuantizer: the digits of the token) with no callback
    before or after it — so that its mean over the positions can be taken inside the decode kernel."""
    if isinstance(q, _vq.VectorQuantizer):
        return own(q, _vq.VectorQuantizer, '_decode') or own(q, BaseQuantizer, 'decode') or leaves(q._callbacks, 'before_decode', 'after_decode')
    if isinstance(q, _sq.FiniteScalarQuantizer):
        return own(q, _sq.FiniteScalarQuantizer, '_decode', 'decode') or leaves(q._callbacks, 'before_decode', 'after_decode')
    return f'{type(q).__name__} has no decode_pooled'


def pooled_entry(q, quant: torch.Tensor) -> Route:
    """tokenization.pool_from_quant: tokens [B, *] -> features [B, D] in one launch (``decode_pooled``), or ``decode`` to rows and
    their mean over the positions."""
    why = pooled_config(q) or ('' if quant.is_cuda else f'the tokens are on device {quant.device}, not on a GPU') \
        or ('' if quant.dim() >= 2 else f'the tokens are {quant.dim()}-D, not [B, *]') \
        or ('' if quant.dtype in (torch.int32, torch.int64) else f'the tokens are {quant.dtype}, not int32 or int64') \
        or ('' if 0 < quant.numel() < (1 << 31) else f'{quant.numel()} tokens are outside 1 .. 2^31-1')
    return Route('rows', why) if why else Route('pooled')


# ---- the sampler of stage-2 generation (vector_quantization_amd/samplers.py) ---------------------------------------------

def plain_sampler(s) -> str:
    """``s`` draws as BaseSampler or TopKTopPSampler do: one of the two classes, or a subclass that keeps their ``sample``."""
    from .. import samplers as S
    if isinstance(s, S.CFGSampler):
        return f'{type(s).__name__} is not one of the two plain samplers'
    for base in (S.TopKTopPSampler, S.BaseSampler):
        if isinstance(s, base):
            return own(s, base, 'sample', 'fused_arguments')
    return f'{type(s).__name__} is not one of the two plain samplers'


def sampler_config(s) -> str:
    """The configuration part: what the fused launch computes is what ``s.sample`` would."""
    from .. import samplers as S
    if isinstance(s, S.CFGSampler):
        why = own(s, S.CFGSampler, 'sample', 'fused_arguments')
        inner = plain_sampler(s._sampler)
        return why or (f'the CFG inner sampler: {inner}' if inner else '')
    return plain_sampler(s)


def sampler_arguments(s) -> str:
    """The temperature the launch divides by is finite and > 0 (anything else: the reference's own arithmetic decides)."""
    t = s.fused_arguments()['temperature']
    try:
        ok = 0.0 < float(t) < float('inf')
    except (TypeError, ValueError):
        ok = False
    return '' if ok else f'temperature={t!r} is not a finite number > 0'


def device_logits(logits: torch.Tensor) -> str:
    """The logits are on a device, in a float dtype, with a last dimension of unit stride."""
    return ('' if logits.is_cuda else f'the logits are on device {logits.device}, not on a GPU') \
        or ('' if logits.dim() >= 1 and (logits.stride(-1) == 1 or logits.shape[-1] == 1) else 'the last dimension of the logits does not have stride 1') \
        or ops.float_dtype_refusal('the logits are', logits)


def sampler_rows(logits: torch.Tensor, start: int, end: int) -> str:
    """[start, end) lies inside the last dimension, and [..., V_total] is rows of ONE stride that do not overlap, read as a view
    (``ops.row_view``; behind ``device_logits`` its reason is one of those two)."""
    if not 0 <= start < end <= logits.shape[-1]:
        return f'[{start}, {end}) is not a non-empty slice of the last dimension ({logits.shape[-1]})'
    if end - start > ops.SAMPLE_MAX_V:
        return f'V={end - start} is beyond 2^20'
    view = ops.row_view(logits, 'the logits')
    return view if isinstance(view, str) else ''


def sampler_why(sampler, logits: torch.Tensor, start: int = 0, end=None) -> Route:
    """A sampler step: ONE launch of ``ops.sample_tokens`` on the logits as they are (``fused``), or the reference's composition
    with torch ops (``torch``), with the first clause that refused the launch."""
    end = logits.shape[-1] if end is None else end
    why = device_logits(logits) or sampler_config(sampler) or sampler_arguments(sampler) or sampler_rows(logits, start, end)
    return Route('torch', why) if why else Route('fused')


# ---- the token cross-entropy of stage-2 training (vector_quantization_amd/sequence_losses.py) -----------------------------

def token_ce_targets(logits: torch.Tensor, targets: torch.Tensor, shift: bool) -> str:
    """One int32 / int64 target per row, next to the logits; fewer than 2^31 rows."""
    if targets.dtype not in ops.TOKEN_DTYPES:
        return f'the targets are {targets.dtype}, not int32 or int64'
    if targets.shape != logits.shape[:-1]:
        return f'the targets are {tuple(targets.shape)}, not {tuple(logits.shape[:-1])} (one per row of the logits)'
    if targets.device != logits.device:
        return f'the targets are on device {targets.device}, the logits on {logits.device}'
    if shift and logits.dim() < 2:
        return 'shift needs logits [..., L, V_total]'
    return '' if 0 < targets.numel() < (1 << 31) else f'{targets.numel()} rows are outside 1 .. 2^31-1'


def token_ce_why(logits: torch.Tensor, targets: torch.Tensor, start: int = 0, end=None, *, label_smoothing: float = 0.0,
                 weight=None, shift: bool = False) -> Route:
    """A stage-2 loss: the fused launches of ``ops.token_cross_entropy`` on the logits as they are (``fused``), or the reference's
    composition with log_softmax / gather (``torch``), with the first clause that refused the launches."""
    end = logits.shape[-1] if end is None else end
    why = device_logits(logits) or sampler_rows(logits, start, end) or token_ce_targets(logits, targets, shift) \
        or ('' if 0.0 <= label_smoothing < 1.0 else f'label_smoothing={label_smoothing!r} is outside [0, 1)') \
        or ('' if weight is None or weight.numel() == targets.numel() else f'the weights are {tuple(weight.shape)}, not one per row')
    return Route('torch', why) if why else Route('fused')


# ---- the reconstruction metrics of a validation pass (vector_quantization_amd/image_losses.py, runners.ImageLossMetric) -------

def image_metrics_why(pred: torch.Tensor, image: torch.Tensor, *, ssim: bool = True, loss=None) -> Route:
    """L1 / MSE / PSNR / SSIM of a pair of image batches: the two launches of ``ops.image_metrics`` on the tensors as they are
    (``fused``), or the reference's composition with torch ops (``torch``), with the first clause that refused the launches:
    a CPU tensor, float64 (or any dtype the kernel does not decode), a layout that is neither NCHW-contiguous nor channels-last,
    the size cap of the fixed-point SSIM sum, a ``loss`` that is none of the four plain classes, or one whose class overrides
    their ``forward``."""
    from .. import image_losses
    why = ''
    if loss is not None and not image_losses.column_of(loss):
        why = f'{type(loss).__name__} is none of L1Loss, MSELoss, PSNRLoss and SSIMLoss'
    elif loss is not None and not image_losses.is_plain(loss):
        why = f'{type(loss).__name__} overrides forward of the plain loss classes'
    for name, t in (('pred', pred), ('image', image)):
        why = why or ('' if t.is_cuda else f'{name} is on device {t.device}, not on a GPU')
    why = why or ops.image_metrics_refusal(pred, image, ssim)
    return Route('torch', why) if why else Route('fused')


# ---- the distillation loss of VQ-KD (vector_quantization_amd/distill_losses.py) -------------------------------------------------

def cosine_embedding_why(pred: torch.Tensor, target: torch.Tensor, *, layout=None, loss=None) -> Route:
    """CosineEmbeddingLoss between the student's features and the teacher's: the launches of ``ops.cosine_embedding_loss`` on the
    tensors as they are (``fused``), or the reference's composition around ``F.cosine_embedding_loss`` (``torch``), with the
    first clause that refused the launches: a CPU tensor, float64 (or any dtype the kernels do not read), a target that requires
    grad (the kernels form no gradient for it), strides that are neither rows with unit column stride nor an NCHW-contiguous
    map, or a ``loss`` whose class overrides ``forward`` / ``forward_torch`` of ``CosineEmbeddingLoss``."""
    from .. import distill_losses
    why = ''
    if loss is not None:
        why = own(loss, distill_losses.CosineEmbeddingLoss, 'forward', 'forward_torch')
    for name, t in (('pred', pred), ('target', target)):
        why = why or ('' if t.is_cuda else f'{name} is on device {t.device}, not on a GPU')
    why = why or ('the target requires grad: the fused backward forms no gradient for it' if target.requires_grad else '') \
        or ops.cosine_embedding_refusal(pred, target, layout)
    return Route('torch', why) if why else Route('fused')


# ---- the perceptual loss of a VQGAN step (vector_quantization_amd/perceptual_losses.py) ------------------------------------------

def lpips_why(loss, pred_features, target_features) -> Route:
    """The tail of LPIPSLoss behind the VGG16 taps: the launches of ``ops.lpips_distance`` on the feature maps as they are
    (``fused``), or the reference's normalize / mse / dropout / 1 x 1 convolution / mean (``torch``), with the first clause that
    refused the launches: a ``loss`` whose class overrides ``forward``, ``forward_torch``, ``distance_torch`` or
    ``extract_features`` of ``LPIPSLoss``, a CPU tensor, a target that requires grad (the kernels form no gradient for it),
    float64 (or any dtype the kernels do not read), or strides that are neither NCHW-contiguous nor channels-last dense in both
    maps of a layer."""
    from .. import perceptual_losses
    why = ''
    if loss is not None:
        why = own(loss, perceptual_losses.LPIPSLoss, 'forward', 'forward_torch', 'distance_torch', 'extract_features')
        if not why and len(pred_features) != len(loss._convs):
            why = f'{len(pred_features)} feature maps for {len(loss._convs)} convolutions'
    if not why and (len(pred_features) == 0 or len(pred_features) != len(target_features)):
        why = f'{len(pred_features)} pred and {len(target_features)} target feature maps'
    for layer, (f, g) in enumerate(zip(pred_features, target_features)):
        for name, t in (('pred', f), ('target', g)):
            why = why or ('' if t.is_cuda else f'layer {layer}: {name} is on device {t.device}, not on a GPU')
        why = why or ('' if not g.requires_grad else f'layer {layer}: the target requires grad: the fused backward forms no gradient for it')
        if not why:
            refusal = ops.lpips_refusal(f, g, None if loss is None else loss._convs[layer].weight)
            why = f'layer {layer}: {refusal}' if refusal else ''
    return Route('torch', why) if why else Route('fused')


# ---- the StyleGAN2 discriminator of a VQGAN step (vector_quantization_amd/discriminators.py) ------------------------------------

def stylegan2_why(module, x: torch.Tensor) -> Route:
    """The bias-activations and blurs of ``StyleGAN2Discriminator`` (or of one of its layers): the HIP kernels of
    ``functional.bias_act`` / ``blur`` / ``bias_act_blur`` on the activations as they are (``fused``), or the same definitions in
    plain torch (``torch``), with the first clause that refused the kernels: ``fused=False`` on the module, a class that overrides
    ``forward``, a Blur for a kernel size other than 3 or 1 (its paddings are not known here), a CPU tensor, float64 (or any dtype
    the kernels do not read), strides that are neither NCHW-contiguous nor channels-last dense.  No shape is sent to ``torch``
    for speed: profiles/stylegan2.txt has the measurements."""
    from .. import discriminators
    why = ''
    if module is not None:
        why = '' if getattr(module, 'fused', True) else 'fused=False'
        if not why and isinstance(module, discriminators.StyleGAN2Discriminator):
            why = own(module, discriminators.StyleGAN2Discriminator, 'forward')
        for m in ([] if why else module.modules()):
            if isinstance(m, discriminators.Blur) and m._kernel_size not in (1, 3):
                why = f'a Blur for kernel_size={m._kernel_size}: the paddings are known for 3 and 1 only'
                break
    why = why or ('' if x.is_cuda else f'the input is on device {x.device}, not on a GPU')
    why = why or ops.stylegan2_refusal(x)
    return Route('torch', why) if why else Route('fused')


def patchgan_why(module, x: torch.Tensor) -> Route:
    """The ``BatchNorm2d -> LeakyReLU(0.2)`` sites of ``PatchGANDiscriminator``: the HIP kernels of ``functional.batch_norm`` on the
    activations as they are (``fused``), or the modules themselves (``torch``), with the first clause that refused the kernels.
    For the discriminator, on its input: ``fused=False`` on the module, a class that overrides ``forward``, a CPU tensor, float64
    (or any dtype the kernels do not read), strides that are neither NCHW-contiguous nor channels-last dense.  For one
    ``BatchNorm2d`` of it, on its own activation: eval mode (what ``R1GradientPenalty`` sets, whose ``create_graph=True`` so keeps
    working through torch), ``momentum=None`` (the cumulative average needs the counter on the host),
    ``track_running_stats=False``, ``affine=False``, one value per channel, and the tensor clauses again.  No shape is sent to
    ``torch`` for speed: profiles/batch_norm.txt has the measurements."""
    from .. import discriminators, functional
    if isinstance(module, torch.nn.modules.batchnorm._BatchNorm):
        why = functional.batch_norm_refusal(x, module.running_mean, module.running_var, module.weight, module.bias, module.training,
                                            module.momentum)
        return Route('torch', why) if why else Route('fused')
    why = ''
    if module is not None:
        why = '' if getattr(module, 'fused', True) else 'fused=False'
        if not why and isinstance(module, discriminators.PatchGANDiscriminator):
            why = own(module, discriminators.PatchGANDiscriminator, 'forward')
    why = why or ('' if x.is_cuda else f'the input is on device {x.device}, not on a GPU') \
        or ops.float_dtype_refusal('the input is', x) or ops.dense_refusal('the input', x)
    return Route('torch', why) if why else Route('fused')


# ---- the GroupNorm (+ SiLU) sites of VQGANEncoder / VQGANDecoder (vector_quantization_amd/autoencoders.py) --------------------------

def group_norm_why(module, x: torch.Tensor, num_groups: int = 32) -> Route:
    """The ``GroupNorm -> SiLU`` sites of ``VQGANEncoder`` / ``VQGANDecoder`` (or of one of their blocks): the HIP kernels of
    ``functional.group_norm`` on the activations as they are (``fused``), or ``F.group_norm`` and ``F.silu`` (``torch``), with the
    first clause that refused the kernels: ``fused=False`` on the module, a class that overrides ``forward``, a CPU tensor, float64
    (or any dtype the kernels do not read), strides that are neither NCHW-contiguous nor channels-last dense.  The decision is
    taken on the module's input; every site repeats the tensor clauses on its own activation (``functional.group_norm``)."""
    from .. import autoencoders
    why = ''
    if module is not None:
        why = '' if getattr(module, 'fused', True) else 'fused=False'
        if not why and isinstance(module, autoencoders.VQGANMixin):
            why = own(module, autoencoders.VQGANMixin, 'forward')
    why = why or ('' if x.is_cuda else f'the input is on device {x.device}, not on a GPU') \
        or ops.float_dtype_refusal('the input is', x) or ops.dense_refusal('the input', x)
    return Route('torch', why) if why else Route('fused')


# ---- the row ops of VQKDEncoder / VQKDDecoder (vector_quantization_amd/vqkd_autoencoders.py) -----------------------------------

def vit_why(module, x: torch.Tensor) -> Route:
    """The residual adds, LayerNorms and bias-activations of ``VQKDEncoder`` / ``VQKDDecoder`` (or of one of their blocks): the HIP
    kernels of ``functional.add_layer_norm`` / ``row_bias_act`` with ``F.scaled_dot_product_attention`` as the attention core
    (``fused``), or the reference's lines in torch (``torch``), with the first clause that refused the kernels: ``fused=False`` on
    the module, a class that overrides ``_forward_fused``, rows (the embedding or the MLP's hidden width, fixed at construction) wider than the
    kernels read, a CPU tensor, float64 input or parameters (or any dtype the kernels do not read).  The decision is taken on the
    module's input; a site whose own activation the kernels refuse after that raises with the reason: nothing falls back to torch
    behind a ``last_route`` that says ``fused``.  No shape is sent to ``torch`` for speed: profiles/vqkd_autoencoder.txt has the measurements."""
    from .. import vqkd_autoencoders
    why = ''
    if module is not None:
        why = '' if getattr(module, 'fused', True) else 'fused=False'
        if not why and isinstance(module, vqkd_autoencoders.VQKDMixin):
            why = own(module, vqkd_autoencoders.VQKDMixin, '_forward_fused')
        width = getattr(module, 'widest_row', 0)
        why = why or ('' if width <= ops._lib.VIT_MAX_D else f'rows of {width} values are beyond {ops._lib.VIT_MAX_D}')
    why = why or ('' if x.is_cuda else f'the input is on device {x.device}, not on a GPU') or ops.float_dtype_refusal('the input is', x)
    if not why and getattr(module, 'pos_embed', None) is not None:
        why = ops.float_dtype_refusal('the parameters are', module.pos_embed)
    return Route('torch', why) if why else Route('fused')


# ---- the row ops of LlamaTransformer (vector_quantization_amd/transformers.py) ----------------------------------------------------

def llama_why(module, tokens: torch.Tensor, kv_cache=None, attention_mask=None) -> Route:
    """The residual adds, RMSNorms and the gated activation of ``LlamaTransformer``: the walk over transformers' submodules on the HIP
    kernels of ``functional.add_rms_norm`` / ``swiglu`` (``fused``), or the reference's call of ``LlamaForCausalLM`` itself
    (``torch``), with the first clause that refused the walk: ``fused=False`` on the module, a class that overrides ``_walk``, an
    ``attention_mask`` (the walk passes none: the attention core is causal by itself), ``mlp_bias`` or ``attention_bias`` set (the
    gated kernel takes no bias; the walk is held to the shipped configuration), a ``hidden_act`` other than ``silu``, tied
    embeddings, an attention implementation other than ``sdpa`` (only there is ``attention_mask=None`` causal), several tokens behind
    a cache that is not empty (transformers builds a mask for them), a hidden or intermediate size beyond the kernels' rows, CPU
    tokens, float64 (or any dtype the kernels do not read) parameters.  A site whose own activation the kernels refuse after that
    raises with the reason: nothing falls back to torch behind a ``last_route`` that says ``fused``.  No shape is sent to
    ``torch`` for speed: profiles/llama_transformer.txt has the measurements."""
    from .. import transformers as vq_transformers
    why = '' if getattr(module, 'fused', True) else 'fused=False'
    why = why or own(module, vq_transformers.LlamaTransformer, '_walk')
    why = why or ('' if attention_mask is None else 'an attention_mask is given: the walk passes none')
    lm = module._transformer
    config = lm.config
    if not why:
        why = ('mlp_bias=True: the gated kernel takes no bias' if getattr(config, 'mlp_bias', False) else '') \
            or ('attention_bias=True' if getattr(config, 'attention_bias', False) else '') \
            or ('' if config.hidden_act == 'silu' else f'hidden_act={config.hidden_act!r} is not \'silu\'') \
            or ('the embeddings are tied' if getattr(config, 'tie_word_embeddings', False)
                or lm.lm_head.weight is lm.model.embed_tokens.weight else '') \
            or ('' if config._attn_implementation == 'sdpa' else
                f'attention implementation {config._attn_implementation!r}: only sdpa is causal without a mask')
    if not why and kv_cache is not None and tokens.dim() == 2 and tokens.shape[1] > 1 and kv_cache.get_seq_length() > 0:
        why = f'{tokens.shape[1]} tokens behind a cache of {kv_cache.get_seq_length()}: transformers builds a mask for them'
    width = max(config.hidden_size, config.intermediate_size)
    why = why or ('' if width <= ops._lib.VIT_MAX_D else f'rows of {width} values are beyond {ops._lib.VIT_MAX_D}')
    why = why or ('' if tokens.is_cuda else f'the tokens are on device {tokens.device}, not on a GPU') \
        or ops.float_dtype_refusal('the parameters are', lm.model.embed_tokens.weight)
    return Route('torch', why) if why else Route('fused')


def llama_decode_why(module, tokens: torch.Tensor, kv_cache=None) -> Route:
    """Cached generation of ``LlamaTransformer`` behind a ``StaticKVCache``: the walk that calls the attention's own submodules -
    one packed q/k/v GEMM, ``functional.decode_attention`` (one token) or ``rope_append`` + a causal sdpa (a prompt), ``o_proj`` -
    (``decode``); or, with the first clause that refused it, the fused walk behind a ``DynamicCache`` (``walk``) where only the
    attention step is refused, and transformers' own forward (``torch``) where ``llama_why`` refuses the walk itself.  The
    clauses of ``walk``: a class that overrides ``_walk_static``, a ``rope_type`` other than ``default`` or an
    ``attention_scaling`` other than 1 (the kernels rotate by cos and sin as they are), a sliding window, a head dimension or
    a group of query heads beyond the kernels' limits, a capacity beyond theirs, a cache (``kv_cache``, where one is given) of
    another shape, on another device or of another dtype than the projections produce (the autocast dtype under autocast, else
    the parameters').  Nothing falls back behind a route that says ``decode``: a step the kernels refuse after that raises."""
    from .. import transformers as vq_transformers
    base = llama_why(module, tokens, kv_cache)
    if base.name != 'fused':
        return base
    lm = module._transformer
    config, rotary = lm.config, lm.model.rotary_emb
    Hq, Hkv = config.num_attention_heads, config.num_key_value_heads
    Dh = getattr(config, 'head_dim', None) or config.hidden_size // Hq
    rope_type = getattr(rotary, 'rope_type', 'default')
    scaling = getattr(rotary, 'attention_scaling', 1.0)
    sliding = getattr(config, 'sliding_window', None) or 'sliding_attention' in (getattr(config, 'layer_types', None) or ())
    why = own(module, vq_transformers.LlamaTransformer, '_walk_static') \
        or ('' if rope_type == 'default' else f'rope_type={rope_type!r} is not \'default\'') \
        or ('' if scaling == 1 else f'attention_scaling={scaling} is not 1') \
        or ('a sliding window is configured' if sliding else '') \
        or ops.attention_shape_refusal(Hq, Hkv, Dh)
    if not why and kv_cache is not None:
        dtype = autocast_dtype(tokens) or lm.model.embed_tokens.weight.dtype
        shape = (config.num_hidden_layers, tokens.shape[0], Hkv, Dh)
        have = (getattr(kv_cache, 'layers', None), getattr(kv_cache, 'batch', None), getattr(kv_cache, 'kv_heads', None),
                getattr(kv_cache, 'head_dim', None))
        why = ('' if have == shape else f'the cache holds (layers, batch, kv heads, head dim) = {have}, the step needs {shape}') \
            or ('' if kv_cache.capacity <= ops._lib.ATTN_MAX_LEN else f'a capacity of {kv_cache.capacity} is beyond {ops._lib.ATTN_MAX_LEN}') \
            or ('' if kv_cache.device == tokens.device else f'the cache is on device {kv_cache.device}, the tokens on {tokens.device}') \
            or ('' if kv_cache.dtype == dtype else f'the cache is {kv_cache.dtype}, the projections produce {dtype}')
    return Route('walk', why) if why else Route('decode')


def llama_graph_why(module, tokens: torch.Tensor, length: int) -> Route:
    """``LlamaTransformer.generate`` behind a ``StaticKVCache``: the single-token steps replayed from ONE captured HIP graph
    (``decode_graph.DecodeGraph``: ``functional.decode_attention_at`` reads the position from device memory) (``graph``); or, with
    the first clause that refused it, today's eager decode loop (``decode``).  Where ``llama_decode_why`` refuses the decode route
    itself, its route comes back as it is.  The clauses of ``decode``: ``graph=False`` or ``static_cache=False`` on the module, a
    class that overrides ``_walk_static``, ``sample`` or ``_generate`` (the captured step stands in for the first, calls the second and
    is driven by the third), a sampler whose configuration or arguments ``sampler_why`` sends to its torch route (that one
    synchronises), fewer than two steps behind the prompt's own draw (the first runs eagerly as the capture's warm-up: there
    would be nothing to replay), a stream that is already capturing.  No shape is sent to either route for speed:
    profiles/llama_decode_graph.txt has the measurements."""
    from .. import transformers as vq_transformers
    base = llama_decode_why(module, tokens, None)
    if base.name != 'decode':
        return base
    steps = length - tokens.shape[1] - 1
    sampler = sampler_config(module.sampler) or sampler_arguments(module.sampler)
    why = ('' if getattr(module, 'graph', False) else 'graph=False') \
        or ('' if getattr(module, 'static_cache', False) else 'static_cache=False') \
        or own(module, vq_transformers.LlamaTransformer, '_walk_static', 'sample', '_generate') \
        or (f'the sampler takes its torch route: {sampler}' if sampler else '') \
        or ('' if steps >= 2 else f'{max(steps, 0)} steps behind the prompt\'s own draw: nothing to replay') \
        or ('the stream is already capturing' if torch.is_tensor(tokens) and tokens.is_cuda and torch.cuda.is_current_stream_capturing() else '')
    return Route('decode', why) if why else Route('graph')


# ---- MultinomialAnchor of a CVQ-VAE update (vector_quantization_amd/quantizers/anchors.py) ----------------------------------------

def multinomial_anchor_why(anchor, d, x: torch.Tensor) -> Route:
    """One latent per code drawn down the columns of the distances: ``LazyDistance.multinomial`` on bounded row blocks, the
    [N, K] matrix never formed (``fused``), or the reference's ``d.t().softmax(1).multinomial(1)`` on the materialised matrix
    (``matrix``), with the first clause that refused the fused route: ``fused=False``, a subclass that overrides ``_anchors`` or
    ``probabilities``, CPU tensors, a plain tensor or an already materialised handle (the caller paid for the matrix), a metric
    whose matrix is not the fp32 definition (the bf16-autocast cosine: the reference's matrix is bf16 there), float64 latents,
    or more rows than the fixed-point column sums hold.  No size threshold ships: where the whole matrix fits one tile - the only
    place one could apply - the fused route was measured faster than the matrix route (profiles/col_multinomial.txt, DESIGN.md
    §8); beyond one tile it trades time (three evaluations of the distances) for memory that does not grow with N * K."""
    why = ('' if anchor._fused is None else 'fused=False') or own(anchor, MultinomialAnchor, '_anchors', 'probabilities') \
        or ('' if x.is_cuda else f'the latents are on device {x.device}, not on a GPU') \
        or ('' if isinstance(d, LazyDistance) else 'memo distance is a matrix, not the lazy handle of the fused encode: it is paid for')
    if why:
        return Route('matrix', why)
    why = ('the handle is already materialised: the matrix is paid for' if d._value is not None else '') \
        or ('' if d.is_cuda else f'the distances are on device {d.device}, not on a GPU') \
        or ('' if d.metric in d._distance.FUSED_ENTROPY_METRICS else
            f'metric {d.metric!r}: the reference\'s matrix is not the fp32 definition there'
            if d.metric == 'CosineBF16' else f'{type(d._distance).__name__} has no fused column draw for metric {d.metric!r}') \
        or ('' if x.dtype != torch.float64 and d.operands[0].dtype != torch.float64 else 'the latents are float64') \
        or ('' if 0 < d.shape[0] <= ops.COL_MULTINOMIAL_MAX_N else f'N={d.shape[0]} is outside 1 .. 2^20') \
        or ('' if d.dim() == 2 and x.dim() == 2 and x.shape[0] == d.shape[0] else 'the latents are not the [N, D] rows of the distances')
    return Route('matrix', why) if why else Route('fused')
