"""The stage-2 generator of the reference's LlamaGen configs under its names, registry and constructor arguments:
``BaseTransformer`` (vq/tasks/sequence_modeling/models/transformers.py with the KV-cache loop of vq/algorithms/ar/transformers/base.py),
``HFTransformer`` (hf.py) and ``LlamaTransformer`` (llama.py), selected by configs/ar/transformers/llama.py.  The network is
transformers' ``LlamaForCausalLM``, built from the config's dict unchanged and kept in ``_transformer``, so the state-dict keys are
the reference's and its checkpoints load with ``strict=True``.

The GEMMs, the rotary embedding and the attention core stay with the framework.  Everything between them is row-wise:

- route ``fused``: a walk over the submodules of ``LlamaForCausalLM`` that this file owns - nothing of transformers is edited and no
  module's ``forward`` is replaced.  There is ONE walk, ``LlamaTransformer._layers``, and every route below is a thin caller that
  gives it an attention step and a weight set (``llama_weights.LlamaWeights``).  The state carried from layer to layer is
  ``(x, pending)``, the residual stream and the branch not yet added to it.  Every ``LlamaRMSNorm`` is one
  ``functional.add_rms_norm`` call that adds the pending branch, leaves the sum and writes the normalised rows in the dtype the
  next ``linear`` reads (the autocast dtype under autocast, while the stream stays fp32); ``gate_proj`` and ``up_proj`` are ONE
  GEMM against their concatenated weights and ``functional.swiglu`` reads its two halves.  The attention step of this route
  (``_walk``) calls ``self_attn`` as it is with ``attention_mask=None`` and the cache (its sdpa path is causal by itself there),
  and its weight set holds nothing: the ``cat`` of gate and up is part of the autograd graph.  ``forward`` puts
  ``CausalTokenLoss`` on the logits in place of the ``labels=`` path (so ``memo['accuracy']`` exists on this route only: the torch
  route's memo carries ``logits`` alone, as the reference's);
- route ``torch``: the reference's two lines, ``self._transformer(tokens, labels=tokens)`` and
  ``self._transformer(tokens, past_key_values=kv_cache)`` - what serves CPU and float64 tensors, ``fused=False`` and every
  configuration ``routes.llama_why`` names.

``routes.llama_why`` decides per call; the decision is kept in ``last_route``.

``LlamaTransformer(..., static_cache=True)`` (off by default) generates behind a ``StaticKVCache`` instead of transformers'
``DynamicCache``: K and V are allocated once for the requested length and ``_walk_static`` is the same walk with the second
attention step, ``_attend_static``, which calls the attention's own submodules - one GEMM against the packed q/k/v weights, three
views into its rows, ``functional.decode_attention`` (one launch: rotary, append, grouped-query attention over the cache, rows as
``o_proj`` reads them) or, for a prompt, ``functional.rope_append`` and a causal sdpa, then ``o_proj``.  The weight set is packed once
per ``generate`` call, q/k/v and gate/up in the autocast dtype under autocast, kept in ``_packed`` while ``BaseTransformer``'s loop
runs (``_packing``) and dropped when it ends.  ``routes.llama_decode_why`` decides; a step on this route leaves ``Route('decode')``
in ``last_route``.

``LlamaTransformer(..., static_cache=True, graph=True)`` (off by default) runs the prompt and the first draw as above and then
hands over to a ``decode_graph.DecodeGraph``: the single-token step - the same walk and ``_attend_static`` again, around the third
attention core, ``functional.decode_attention_at``, which reads the position from device memory; then ``lm_head``, the sampler
and ``functional.decode_advance`` - captured once as a HIP graph and replayed for every further token, against a weight set that
the graph owns and refreshes in place.  ``routes.llama_graph_why`` decides (``graph_route`` keeps the decision); such a call leaves ``Route('graph')``
in ``last_route``, and the graph is kept on the module for the next call with the same key.
"""
from __future__ import annotations

import contextlib
import functools
from abc import ABC, abstractmethod
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import functional
from . import samplers  # noqa: F401  (registers the samplers a config names)
from .config import BuildPreHookMixin, Config
from .kv_cache import StaticKVCache
from .llama_weights import LlamaWeights
from .quantizers.memo import get_memo
from .registries import VQSMSamplerRegistry, VQSMTransformerRegistry
from .sequence_losses import CausalTokenLoss
from .utils import autocast_dtype

__all__ = ['BaseTransformer', 'HFTransformer', 'LlamaTransformer', 'StaticKVCache']


class BaseTransformer(BuildPreHookMixin, nn.Module, ABC):
    """``vocabulary_size`` and ``sampler`` (built through ``VQSMSamplerRegistry``), ``sample``, ``generate`` under ``no_grad`` and
    the KV-cache loop: the prompt goes through ``_inference`` once, every later step passes the one new token and the cache."""

    def __init__(self, *args, vocabulary_size: int, sampler, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._vocabulary_size = vocabulary_size
        self._sampler = sampler

    @property
    def vocabulary_size(self) -> int:
        return self._vocabulary_size

    @property
    def sampler(self):
        return self._sampler

    @classmethod
    def sampler_build_pre_hook(cls, config: Config, registry, item) -> Config:
        config.sampler = VQSMSamplerRegistry.build_or_return(config.sampler)
        return config

    @classmethod
    def build_pre_hook(cls, config: Config, registry, item) -> Config:
        config = super().build_pre_hook(config, registry, item)
        config = cls.sampler_build_pre_hook(config, registry, item)
        return config

    def sample(self, logits: torch.Tensor, codebook, memo):
        tokens, memo['sampler'] = self._sampler(logits, codebook.start, codebook.end, get_memo(memo, 'sampler'))
        return tokens, memo

    @abstractmethod
    def _inference(self, tokens: torch.Tensor, kv_cache, memo):
        pass

    @torch.no_grad()
    def inference(self, tokens: torch.Tensor, kv_cache, memo):
        return self._inference(tokens, kv_cache, memo)

    def _generate(self, tokens: torch.Tensor, length: int, codebook, memo, kv_cache=None):
        """The one loop; ``kv_cache`` is a cache the caller made for it (None: the first ``_inference`` makes one)."""
        assert tokens.shape[1] < length
        token = tokens
        while tokens.shape[1] < length:
            logits, kv_cache, memo = self.inference(token, kv_cache, memo)
            token, memo = self.sample(logits[:, [-1]], codebook, memo)
            tokens = torch.cat((tokens, token), 1)
        assert tokens.shape[1] == length
        return tokens, memo

    @torch.no_grad()
    def generate(self, tokens: torch.Tensor, length: int, codebook, memo):
        return self._generate(tokens, length, codebook, memo)

    @abstractmethod
    def forward(self, data, memo):
        pass


class HFTransformer(BaseTransformer):
    """A ``PreTrainedModel`` of transformers behind the interface above, resized to the vocabulary."""

    last_route = None

    def __init__(self, *args, transformer, fused: bool = True, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        transformer.resize_token_embeddings(self._vocabulary_size)
        self._transformer = transformer
        self.fused = fused

    @classmethod
    @abstractmethod
    def transformer_build_pre_hook(cls, config: Config, registry, item) -> Config:
        pass

    @classmethod
    def build_pre_hook(cls, config: Config, registry, item) -> Config:
        config = super().build_pre_hook(config, registry, item)
        config = cls.transformer_build_pre_hook(config, registry, item)
        return config

    def init_weights(self, config=None) -> bool:
        return False

    @staticmethod
    def _tokens(data) -> torch.Tensor:
        return data if torch.is_tensor(data) else data.tokens

    def _inference(self, tokens: torch.Tensor, kv_cache, memo):
        output = self._transformer(tokens, past_key_values=kv_cache)
        return output['logits'], output['past_key_values'], memo

    def forward(self, data, memo):
        tokens = self._tokens(data)
        output = self._transformer(tokens, labels=tokens)
        memo['logits'] = output['logits']
        return output['loss'], memo


@VQSMTransformerRegistry.register_()
class LlamaTransformer(HFTransformer):
    """``LlamaForCausalLM(LlamaConfig(**transformer))``.  ``fused=False`` pins the torch route; ``static_cache=True`` lets
    ``generate`` run behind a ``StaticKVCache`` where ``routes.llama_decode_why`` allows it (``decode_route`` keeps that decision);
    ``graph=True`` on top of it replays the single-token steps from one HIP graph where ``routes.llama_graph_why`` allows it
    (``graph_route`` keeps that decision; setting ``graph = False`` drops the captured graph)."""

    decode_route = None
    graph_route = None

    def __init__(self, *args, static_cache: bool = False, graph: bool = False, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._loss = CausalTokenLoss()
        self.static_cache = static_cache
        self._packed = None
        self._decode_graph = None
        self._graph = bool(graph)

    @property
    def graph(self) -> bool:
        return self._graph

    @graph.setter
    def graph(self, on: bool) -> None:
        self._graph = bool(on)
        if not on:
            self._decode_graph = None

    @classmethod
    def transformer_build_pre_hook(cls, config: Config, registry, item) -> Config:
        from transformers import LlamaConfig, LlamaForCausalLM
        if isinstance(config.transformer, dict):
            config.transformer = LlamaForCausalLM(LlamaConfig(**config.transformer))
        return config

    def init_weights(self, config=None) -> bool:

        def initializer(module: nn.Module) -> None:
            if isinstance(module, nn.Linear):
                module.weight.data.normal_(mean=0.0, std=0.02)
                if module.bias is not None:
                    module.bias.data.zero_()
            elif isinstance(module, nn.Embedding):
                module.weight.data.normal_(mean=0.0, std=0.02)

        super().init_weights(config)
        self._transformer.apply(initializer)
        nn.init.constant_(self._transformer.lm_head.weight, 0.0)
        return False

    # ---- the one walk --------------------------------------------------------------------------------------------------------
    @staticmethod
    def _op(name: str, torch_ops: bool):
        """``functional.<name>`` as the walk calls it: the kernel, which raises where it refuses (``strict=True``), or its
        ``_torch`` restatement - any device, float64 included.  The only place that choice is made."""
        return getattr(functional, name + '_torch') if torch_ops else functools.partial(getattr(functional, name), strict=True)

    @classmethod
    def _norm(cls, norm: nn.Module, x: torch.Tensor, pending: Optional[torch.Tensor], *, torch_ops: bool = False):
        """One norm site: ``(x + pending, rms_norm(x + pending))`` with the parameters of the ``LlamaRMSNorm`` child."""
        out_dtype = autocast_dtype(x)
        if pending is not None and pending.dtype != (out_dtype or x.dtype):
            pending = pending.to(out_dtype or x.dtype)
        return cls._op('add_rms_norm', torch_ops)(x, pending, norm.weight, norm.variance_epsilon, out_dtype)

    def _layers(self, x: torch.Tensor, weights: LlamaWeights, attend, *, torch_ops: bool = False) -> torch.Tensor:
        """The decoder layers and the final norm over the embedded rows ``x`` [B, L, D]: the rows ``lm_head`` reads.  Per layer
        add-and-norm, ``attend(i, layer, y)`` - the route's attention step: the normalised rows to the branch the next norm adds -
        add-and-norm, the packed gate/up GEMM, SwiGLU and ``down_proj``, every matrix from ``weights``."""
        swiglu = self._op('swiglu', torch_ops)
        pending = None
        for i, layer in enumerate(weights.layers):
            x, y = self._norm(layer.input_layernorm, x, pending, torch_ops=torch_ops)
            x, y = self._norm(layer.post_attention_layernorm, x, attend(i, layer, y), torch_ops=torch_ops)
            pending = F.linear(swiglu(F.linear(y, weights('gate_up', i))), weights('down', i))
        return self._norm(self._transformer.model.norm, x, pending, torch_ops=torch_ops)[1]

    def _walk(self, tokens: torch.Tensor, kv_cache=None, *, torch_ops: bool = False) -> torch.Tensor:
        """Logits [B, L, V] of ``tokens`` [B, L] behind ``kv_cache`` (updated in place): the walk with transformers' own
        ``self_attn`` as the attention step.  ``torch_ops`` puts the ``_torch`` restatements in place of the two kernels: the same
        walk on any device, what the CPU tests hold against HF's forward."""
        model = self._transformer.model
        x = model.embed_tokens(tokens)
        seen = kv_cache.get_seq_length() if kv_cache is not None else 0
        position_ids = (torch.arange(x.shape[1], device=x.device) + seen).unsqueeze(0)
        position_embeddings = model.rotary_emb(x, position_ids=position_ids)

        def attend(i, layer, y):
            return layer.self_attn(hidden_states=y, position_embeddings=position_embeddings, attention_mask=None,
                                   past_key_values=kv_cache)[0]
        weights = LlamaWeights(self)                                             # nothing held: ``cat(gate, up)`` inside autograd
        return F.linear(self._layers(x, weights, attend, torch_ops=torch_ops), weights('lm_head'))

    # ---- the decode route: the walk behind a StaticKVCache -----------------------------------------------------------------------
    def _attend_static(self, weights: LlamaWeights, kv_cache: StaticKVCache, core):
        """The attention step behind a ``StaticKVCache``: one GEMM against the packed q/k/v weights, ``core(i, scale, q, k, v)`` on
        three views into its rows - what the decode and the graph route differ in: it rotates, appends to layer ``i`` of the cache
        and attends, returning the rows ``o_proj`` reads - and ``o_proj``."""
        nq = self._transformer.config.num_attention_heads * kv_cache.head_dim
        nk = kv_cache.kv_heads * kv_cache.head_dim

        def attend(i, layer, y):
            rows = F.linear(y, weights('qkv', i)).view(-1, nq + 2 * nk)
            o = core(i, layer.self_attn.scaling, rows[:, :nq], rows[:, nq:nq + nk], rows[:, nq + nk:])
            return F.linear(o.view(*y.shape[:2], nq), weights('o', i))
        return attend

    def _walk_static(self, tokens: torch.Tensor, kv_cache: StaticKVCache, *, torch_ops: bool = False) -> torch.Tensor:
        """Logits [B, L, V] of ``tokens`` [B, L] behind the ``StaticKVCache`` (written in place, advanced once): the walk with
        ``_attend_static`` around ``decode_attention`` at the host's position (one token) or ``rope_append`` and a causal sdpa (a
        prompt).  One token: eight launches per layer - norm, qkv GEMM, attention, ``o_proj``, norm, gate-up GEMM, SwiGLU,
        ``down_proj``.  ``torch_ops`` puts the ``_torch`` restatements in place of the kernels: any device, float64 included."""
        model = self._transformer.model
        B, L = tokens.shape
        kv_cache.require_room(L)                                                 # before anything is launched
        seen = kv_cache.get_seq_length()
        x = model.embed_tokens(tokens)
        position_ids = (torch.arange(L, device=x.device) + seen).unsqueeze(0)
        cos, sin = model.rotary_emb(x, position_ids=position_ids)
        cos, sin = cos[0], sin[0]                                                # [L, Dh]
        weights = self._packed if self._packed is not None else LlamaWeights(self, autocast_dtype(x)).pack()
        decode, append = self._op('decode_attention', torch_ops), self._op('rope_append', torch_ops)
        gqa = model.config.num_attention_heads != kv_cache.kv_heads

        def core(i, scale, q, k, v):
            if L == 1:
                return decode(q, k, v, cos, sin, kv_cache, i, scale=scale)
            q_rot = append(q, k, v, cos, sin, kv_cache, i)
            kc, vc, _ = kv_cache.layer(i)
            return F.scaled_dot_product_attention(q_rot, kc[:, :, :seen + L], vc[:, :, :seen + L], is_causal=True, scale=scale,
                                                  enable_gqa=gqa).transpose(1, 2).reshape(B, L, -1)
        y = self._layers(x, weights, self._attend_static(weights, kv_cache, core), torch_ops=torch_ops)
        kv_cache.advance(L)
        return F.linear(y, weights('lm_head'))

    @contextlib.contextmanager
    def _packing(self, weights: LlamaWeights):
        """``weights`` as what ``_walk_static`` reads for the steps of one ``generate`` call, in place of packing per call."""
        self._packed = weights
        try:
            yield
        finally:
            self._packed = None

    def _generate_graph(self, tokens: torch.Tensor, length: int, codebook, memo):
        """``generate`` on the graph route: the prompt and the first draw on the eager decode route, every further token from the
        ``DecodeGraph`` (kept for the next call while its key stays).  Returns a clone of the graph's sequence buffer;
        ``memo['sampler']`` is what the captured sampler call left - its tensors live in the graph's memory and show the LAST
        replay, also after a later call has replayed again.  A draw of -1 (a row without a finite logit) does not reach an
        embedding: it is clamped on the device, found by one check behind the loop and raised as ``ValueError``."""
        from .decode_graph import DecodeGraph
        from .quantizers import routes
        autocast = autocast_dtype(tokens)
        dtype = autocast or self._transformer.model.embed_tokens.weight.dtype
        u = get_memo(memo, 'sampler').get('u')
        key = DecodeGraph.key_of(self, tokens, length, codebook, dtype, autocast, u is not None)
        if self._decode_graph is None or self._decode_graph.key != key:
            self._decode_graph = None                                            # (its memory goes before the next one's comes)
            self._decode_graph = DecodeGraph(self, tokens.shape[0], length, codebook, device=tokens.device, cache_dtype=dtype,
                                             autocast=autocast, with_u=u is not None, key=key)
        graph = self._decode_graph
        graph.begin(tokens, u)
        with self._packing(graph.weights):
            logits, _, memo = self.inference(tokens, graph.cache, memo)
            token, memo = self.sample(logits[:, [-1]], codebook, memo)
        sequence = graph.run(token).clone()
        self.last_route = routes.Route('graph')
        bad = sequence < 0
        if bool(bad.any()):
            column = int(bad.any(0).nonzero()[0])
            raise ValueError(f'LlamaTransformer.generate: the sampler drew no token for row {int(bad[:, column].nonzero()[0])} at column '
                             f'{column} (its logits hold NaN, +inf or nothing finite)')
        memo['sampler'] = dict(graph.memo.get('sampler', {}), **({} if u is None else {'u': u}))
        return sequence, memo

    def _generate(self, tokens: torch.Tensor, length: int, codebook, memo):
        """Decides the route, makes its cache and weight set, and runs ``BaseTransformer``'s loop (or ``_generate_graph``)."""
        from .quantizers import routes
        assert tokens.shape[1] < length
        if self._graph:
            self.graph_route = routes.llama_graph_why(self, tokens, length)
            if self.graph_route.name == 'graph':
                return self._generate_graph(tokens, length, codebook, memo)
        if self.static_cache:
            self.decode_route = routes.llama_decode_why(self, tokens, None)
        if not self.static_cache or self.decode_route.name != 'decode':          # the loop behind a DynamicCache; ``decode_route`` says why
            return super()._generate(tokens, length, codebook, memo)
        autocast = autocast_dtype(tokens)
        kv_cache = StaticKVCache.for_model(self._transformer.config, tokens.shape[0], length,
                                           autocast or self._transformer.model.embed_tokens.weight.dtype, tokens.device)
        with self._packing(LlamaWeights(self, autocast).pack()):
            return super()._generate(tokens, length, codebook, memo, kv_cache)

    def _route(self, tokens: torch.Tensor, kv_cache=None, attention_mask=None) -> bool:
        from .quantizers import routes
        self.last_route = route = routes.llama_why(self, tokens, kv_cache, attention_mask)
        return route.name == 'fused'

    def _inference(self, tokens: torch.Tensor, kv_cache, memo, attention_mask=None):
        if isinstance(kv_cache, StaticKVCache):
            from .quantizers import routes
            route = routes.llama_decode_why(self, tokens, kv_cache) if attention_mask is None else \
                routes.Route('torch', 'an attention_mask is given: the walk passes none')
            self.last_route = self.decode_route = route
            if route.name != 'decode':                                           # no other route reads a StaticKVCache
                raise ValueError(f'LlamaTransformer: a StaticKVCache was given, but the decode route is refused: {route.why}')
            return self._walk_static(tokens, kv_cache), kv_cache, memo
        if self._route(tokens, kv_cache, attention_mask):
            if kv_cache is None:
                from transformers import DynamicCache
                kv_cache = DynamicCache(config=self._transformer.config)
            return self._walk(tokens, kv_cache), kv_cache, memo
        output = self._transformer(tokens, past_key_values=kv_cache, attention_mask=attention_mask)
        return output['logits'], output['past_key_values'], memo

    def forward(self, data, memo, attention_mask=None):
        tokens = self._tokens(data)
        if self._route(tokens, None, attention_mask):
            logits = self._walk(tokens)
            memo['logits'] = logits
            return self._loss(logits, tokens, memo)
        output = self._transformer(tokens, labels=tokens, attention_mask=attention_mask)
        memo['logits'] = output['logits']
        return output['loss'], memo
