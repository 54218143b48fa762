"""VectorQuantizer / VQGANQuantizer / VQKDQuantizer — mirror of vq/algorithms/vq/quantizers.py:19-117,
vq/algorithms/vqgan/quantizer.py:11-21 and vq/algorithms/vqkd/quantizers/base.py:11-15."""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch import nn

from .. import functional as VF
from .. import ops, train_step
from ..config import Config, Item, RegistryMeta
from ..registries import InitRegistry, ModelRegistry, VQITQuantizerDistanceRegistry, VQITQuantizerRegistry
from .memo import Memo, get_memo
from . import routes
from .quantizer_api import BaseQuantizer
from .distances import BaseDistance, LazyDistance
from .losses import CodebookLoss, VQGANLoss


@VQITQuantizerRegistry.register_()
class VectorQuantizer(BaseQuantizer):
    # False (or VQHIP_ONE_CALL=0 in the environment): the callback-driven training forwards run hook by hook, one library call
    # per piece, instead of as ONE call (train_step.py) — the same values either way (tests/test_gpu_one_call.py)
    one_call_steps = os.environ.get('VQHIP_ONE_CALL', '1') != '0'

    def __init__(self, *args, embedding: nn.Embedding, distance: BaseDistance, fused: bool = True,
                 cache_codebook: bool = False, **kwargs) -> None:
        """``fused`` / ``cache_codebook`` are extensions (defaults keep the reference semantics):
        fused          — decode + STE + plain MSE losses in one kernel when no callback customises decode/loss;
        cache_codebook — reuse the prepared codebook image while ``weight`` is bit-for-bit unchanged
                         (opt-in for frozen-codebook tokenisation; callers that mutate the weight must call
                         ``invalidate_codebook()``)."""
        super().__init__(*args, **kwargs)
        self._embedding = embedding
        self._distance = distance
        self._fused = fused
        self._cache_codebook = cache_codebook
        self._prepared: Optional[ops.PreparedCodebook] = None
        self._prepared_key = None
        self.last_route: Optional[routes.Route] = None      # what the last forward / map entry decided (diagnostics: routes.py)

    @classmethod
    def embedding_build_pre_hook(cls, config: Config, registry: RegistryMeta, item: Item) -> Config:
        config.embedding = ModelRegistry.build_or_return(config.embedding)
        return config

    @classmethod
    def distance_build_pre_hook(cls, config: Config, registry: RegistryMeta, item: Item) -> Config:
        config.distance = VQITQuantizerDistanceRegistry.build_or_return(config.distance)
        return config

    @classmethod
    def build_pre_hook(cls, config: Config, registry: RegistryMeta, item: Item) -> Config:
        config = super().build_pre_hook(config, registry, item)
        config = cls.embedding_build_pre_hook(config, registry, item)
        config = cls.distance_build_pre_hook(config, registry, item)
        return config

    @property
    def embedding(self) -> nn.Embedding:
        return self._embedding

    @property
    def distance(self) -> BaseDistance:
        return self._distance

    @property
    def embedding_dim(self) -> int:
        return self._embedding.embedding_dim

    @property
    def codebook_size(self) -> int:
        return self._embedding.num_embeddings

    @property
    def embeddings(self) -> torch.Tensor:
        return self._embedding.weight.detach().clone()

    def _init_weights(self, config: Config) -> bool:
        config = Config(config)
        if 'type' not in config:            # nothing configured: keep nn.Embedding's own initialisation
            return False
        func = InitRegistry.resolve(config.pop('type'))(**config)
        with torch.no_grad():
            func(self._embedding.weight)
        self.invalidate_codebook()
        return False

    # ---- encode: fused distance + argmin -------------------------------------------------------------------------
    def invalidate_codebook(self) -> None:
        self._prepared = None
        self._prepared_key = None

    def _prepare(self, w: torch.Tensor) -> ops.PreparedCodebook:
        if not self._cache_codebook:
            return self._distance.prepare(w)
        key = (w.data_ptr(), w._version, tuple(w.shape), w.device, self._distance.metric)
        if self._prepared is None or self._prepared_key != key:
            self._prepared = self._distance.prepare(w)
            self._prepared_key = key
        return self._prepared

    def _encode(self, x: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        """quantizers.py:92-100.  The reference clones the weight, materialises d[N, K] and takes argmin; here the
        weight is read in place, memo['distance'] is lazy, and the code-hit histogram falls out of the epilogue."""
        w = self._embedding.weight.detach()
        shape = x.shape[:-1]
        x2 = x.detach().reshape(-1, x.shape[-1])
        # the code-hit histogram is a by-product of the re-rank epilogue; only the training callbacks consume it
        hist = None
        want_hist = self.training and len(self._callbacks.callbacks) > 0
        stash = {}
        if self._cache_codebook:
            if want_hist:
                hist = torch.zeros(self.codebook_size, dtype=torch.int32, device=x.device)
            quant = self._distance.argmin(x2, w, hist=hist, prepared=self._prepare(w), stash=stash)
        else:                                   # the codebook may have changed since the last call: image made in the same call
            if want_hist:                       # zeroed by the call's first launch: no separate fill kernel
                hist = torch.empty(self.codebook_size, dtype=torch.int32, device=x.device)
            quant = self._distance.encode(x2, w, hist=hist, stash=stash, zero_hist=True)
        # memo['distance'] stays symbolic.  With autograd on, its operands keep their graph (EntropyLoss differentiates
        # through the matrix: losses.py:130-153); the codebook operand is an alias of the CURRENT weight storage, so the
        # values are those of encode time even after a callback rebinds weight.data (the reference clones them: :97).
        if torch.is_grad_enabled() and (x.requires_grad or self._embedding.weight.requires_grad):
            weight = self._embedding.weight
            memo['distance'] = LazyDistance(self._distance, x.reshape(-1, x.shape[-1]), weight.view_as(weight),
                                            xq=stash.get('xq'), eq=stash.get('eq'), metric=stash.get('metric'))
        else:
            memo['distance'] = LazyDistance(self._distance, x2, w, xq=stash.get('xq'), eq=stash.get('eq'),
                                            metric=stash.get('metric'))
        if hist is not None:
            memo['hist'] = hist
        return quant.reshape(shape), memo

    def _decode(self, quant: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        z = VF.embedding(self._embedding.weight, quant)
        return z, memo

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _fusable(self) -> bool:
        return not routes.tail(self)

    def _vqgan_beta(self) -> float:
        """beta of the (first) VQGANLoss: the combination m_cb + beta * m_cm that the fused kernels finish themselves."""
        return next((loss.beta for loss in self._losses.values() if isinstance(loss, VQGANLoss)), 0.0)

    def _loss_values(self, memo: Memo, m_cb, m_cm, m_vqgan, beta: float, like: torch.Tensor) -> torch.Tensor:
        """memo['loss'][name] of every configured (plain MSE) loss from the three values the fused kernel finished (``m_vqgan``
        with ``beta``), and their fp32 sum (base.py:151-171)."""
        losses = {}
        for name, loss in self._losses.items():
            if isinstance(loss, VQGANLoss):
                # codebook + beta * commitment: finished inside the gather kernel for the (one) VQGANLoss of the shipped
                # configs; a second VQGANLoss with another beta takes the two-term form
                losses[name] = m_vqgan if loss.beta == beta else torch.add(m_cb, m_cm, alpha=loss.beta)
            elif isinstance(loss, CodebookLoss):
                losses[name] = m_cb
            else:
                losses[name] = m_cm
        loss_memo = get_memo(memo, 'loss')
        loss_memo.update(losses)
        memo['loss'] = loss_memo
        values = list(losses.values())
        if len(values) == 1:                  # 0 + v == v: skip the zero-fill and the add of the general form below
            return values[0]
        return sum(values, like.new_zeros([], dtype=torch.float32))

    # routes.step's one-call names -> the method that enqueues that forward by ONE library call (train_step.py)
    _ONE_CALL = {'one_call_plain': '_forward_plain', 'one_call_cvq': '_forward_cvq', 'one_call_vqkd': '_forward_vqkd'}

    def _one_call_step(self, x: torch.Tensor):
        """The one-call training forward this step takes (bound), or None: it runs hook by hook (routes.step)."""
        name = self._ONE_CALL.get(routes.step(self, x).name)
        return getattr(self, name) if name else None

    def _encode_memo(self, memo: Memo, out: dict, x_op: torch.Tensor, e_op: torch.Tensor) -> None:
        """memo['encode'] of a one-call step (``out``: what train_step returned): the symbolic distance between ``x_op`` and
        ``e_op`` (the operands with their graph, where there is one), evaluated on the exact operands the library's encode
        used, and the code-hit histogram."""
        enc = get_memo(memo, 'encode')
        prepared = out['prepared']
        if out['xq'] is not None:                                # cosine: the normalised rows / the image's exact rows
            xq, eq = out['xq'], prepared.exact_rows()
        else:
            xq, eq = (out['xn'] if out.get('xn') is not None else out['x']), prepared.weight
        enc['distance'] = LazyDistance(self._distance, x_op, e_op, xq=xq, eq=eq, metric=ops.metric_name(prepared.metric))
        if out['hist'] is not None:
            enc['hist'] = out['hist']
        memo['encode'] = enc

    def _forward_cvq(self, x: torch.Tensor, memo: Memo):
        beta = self._vqgan_beta()
        quant, z_ste, m_cb, m_cm, m_vqgan = self._callbacks.callbacks[0].fused_forward(x, memo, beta)
        memo.update(x=x, quant=quant)
        memo['decode'] = get_memo(memo, 'decode')
        return z_ste, self._loss_values(memo, m_cb, m_cm, m_vqgan, beta, x), memo

    def _forward_plain(self, x: torch.Tensor, memo: Memo):
        """encode (+ NormalizeCallback.before_encode) + decode + MSE losses + STE from one library call (train_step.vq_forward)."""
        cbs = self._callbacks.callbacks
        weight = self._embedding.weight
        normalize = len(cbs) == 1
        w_in = weight.detach()
        w_out = None
        if normalize:
            w_out = w_in if cbs[0]._writes_in_place(weight) else torch.empty_like(w_in)
        beta = self._vqgan_beta()
        out = train_step.vq_forward(x.detach(), w_in, w_out, self._distance.metric_for(weight.shape[1]), beta, normalize=normalize,
                                    want_hist=self.training and len(cbs) > 0)
        if normalize:
            cbs[0]._publish_weight(weight, w_out)
        done = VF._Computed(xn=out['xn'], z_ste=out['z_ste'], mse=out['mse'], idx=out['idx'])
        xn, z_ste, m_cb, m_cm, m_vqgan = VF.vq_step(x, weight, done, beta)
        rows = xn if normalize else x
        grad = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)
        self._encode_memo(memo, out, rows if grad else (out['xn'] if normalize else out['x']),
                          weight.view_as(weight) if (grad and weight.requires_grad) else out['prepared'].weight)
        memo.update(x=rows, quant=out['idx'])
        memo['decode'] = get_memo(memo, 'decode')
        return z_ste, self._loss_values(memo, m_cb, m_cm, m_vqgan, beta, x), memo

    def _forward_vqkd(self, x: torch.Tensor, memo: Memo):
        cb = self._callbacks.callbacks[0]
        xn, quant, z_ste, value = cb.fused_forward(x, memo)
        memo.update(x=xn, quant=quant)
        memo['decode'] = get_memo(memo, 'decode')
        loss_memo = get_memo(memo, 'loss')
        loss_memo.update({next(iter(self._losses.keys())): value})
        memo['loss'] = loss_memo
        return z_ste, value, memo

    def forward(self, x: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, torch.Tensor, Memo]:
        """quantizers.py:110-117 (BaseQuantizer.forward, then ste(z, memo['x'])).  When nothing customises
        decode/loss the gather, the STE expression and the MSE sums are one kernel with one fused backward; the two
        callback-driven training configs (CVQ-VAE, VQ-KD) are one library call for the whole forward."""
        self.last_route = route = routes.step(self, x)
        if route.name in self._ONE_CALL:
            return getattr(self, self._ONE_CALL[route.name])(x, memo)
        if route.name == 'hooks':
            z, loss, memo = super().forward(x, memo)
            z = VF.ste(z, memo['x'])
            return z, loss, memo
        x, quant, memo = self.encode(x, memo)
        memo.update(x=x, quant=quant)
        beta = self._vqgan_beta()
        z_ste, m_cb, m_cm, m_vqgan = VF.fused_decode_loss(x, self._embedding.weight, quant, beta)
        memo['decode'] = get_memo(memo, 'decode')
        return z_ste, self._loss_values(memo, m_cb, m_cm, m_vqgan, beta, x), memo

    # ---- the same three entry points on the NCHW feature map (models/base.py:116-146) --------------------
    def map_fusable(self, x: torch.Tensor) -> bool:
        """True when ``encode_map`` takes the NCHW map ``x`` as it is (routes.map_why; ``forward_map`` also needs ``_fusable``)."""
        return not routes.map_why(self, x)

    def encode_map(self, x_map: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, torch.Tensor, Memo]:
        """``encode`` for latents given as the feature map [B, D, H, W]: (x_rows [B*H*W, D], quant [B*H*W], memo).  The
        'b c h w -> (b h w) c' of models/base.py:124,140 happens inside the encode's first kernel; ``x_rows`` — the token
        matrix the callbacks and the rest of the step see — is its by-product (detached)."""
        self.last_route = routes.Route('map')
        enc = get_memo(memo, 'encode')
        w = self._embedding.weight.detach()
        hist = None
        if self.training and len(self._callbacks.callbacks) > 0:
            hist = torch.empty(self.codebook_size, dtype=torch.int32, device=x_map.device)
        stash = {}
        quant, x_rows = self._distance.encode_map(x_map, w, hist=hist, stash=stash, zero_hist=True)
        enc['distance'] = LazyDistance(self._distance, x_rows, w, xq=stash.get('xq'), eq=stash.get('eq'), metric=stash.get('metric'))
        if hist is not None:
            enc['hist'] = hist
        memo['encode'] = enc
        return x_rows, self._callbacks.after_encode(x_rows, quant, memo), memo

    def forward_map(self, x_map: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, torch.Tensor, Memo]:
        """``forward`` on the feature map: (z_map [B, D, H, W] NCHW-contiguous, loss, memo) — BaseModel.quantize
        (models/base.py:116-128) without either rearrangement kernel.  Gradients flow to ``x_map`` and the codebook."""
        why = routes.map_why(self, x_map, decode=True)
        assert not why, why
        x_rows, quant, memo = self.encode_map(x_map, memo)
        memo.update(x=x_rows, quant=quant)
        beta = self._vqgan_beta()
        z_map, m_cb, m_cm, m_vqgan = VF.fused_map_decode_loss(x_map, x_rows, self._embedding.weight, quant, beta)
        memo['decode'] = get_memo(memo, 'decode')
        loss = self._loss_values(memo, m_cb, m_cm, m_vqgan, beta, x_map)
        return z_map, loss, memo

    def decode_map(self, quant: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        """``decode`` of an image-shaped index tensor [B, H, W] straight into the map [B, D, H, W] (decode_from_quant,
        image_reconstruction/models.py:97-106); no gradient (the reference decodes tokens under no_grad there)."""
        b, h, w = quant.shape
        z_map, _ = ops.gather_ste_map(None, self._embedding.weight.detach(), quant.reshape(-1), b, h, w)
        return z_map, memo

    def decode_pooled(self, quant: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        """``decode`` of tokens [B, *] followed by the mean over the positions (the linear probe's features,
        image_classification/models.py:105-109) as ONE launch: (features [B, D] fp32, memo); the [B, *, D] rows are never written.
        The summation order is fixed (include/vqhip.h), a token outside the codebook makes its image's row NaN instead of the
        reference's device assert, and the gradient goes to the codebook.  Needs the plain decode on device tokens
        (routes.pooled_entry; tokenization.pool_from_quant takes ``decode`` + mean otherwise)."""
        route = routes.pooled_entry(self, quant)
        assert route.name == 'pooled', route.why
        self.last_route = route
        memo['decode'] = get_memo(memo, 'decode')
        return VF.decode_pool(self._embedding.weight, quant), memo


@VQITQuantizerRegistry.register_()
class VQGANQuantizer(VectorQuantizer):

    def _init_weights(self, config: Config) -> bool:
        if Config(config) == Config(type='vqgan'):
            config = Config(type='uniform_', a=-1.0 / self.codebook_size, b=1.0 / self.codebook_size)
        return super()._init_weights(config)


@VQITQuantizerRegistry.register_()
class VQKDQuantizer(VectorQuantizer):

    def _init_weights(self, config: Config) -> bool:
        return False
