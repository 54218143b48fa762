"""``DecodeGraph``: the single-token step of ``LlamaTransformer.generate`` captured once as a HIP graph and replayed per token.

Behind a ``StaticKVCache`` a generated token costs about ten launches per layer, and the host issues them more slowly than the GPU
runs them (profiles/llama_decode.txt).  Every piece of such a step has a fixed shape and fixed addresses - the cache is allocated
once, the attention launch has a grid of ``B * Hkv`` workgroups whatever the length, the sampler is one launch - except the
position, which ``functional.decode_attention`` takes as a host integer.  ``functional.decode_attention_at`` reads it from device
memory (``StaticKVCache.position``) and ``functional.decode_advance`` counts it there, so one captured step serves every token.

A ``DecodeGraph`` owns everything a replay reads or writes by pointer: the ``[R, 1]`` input token, the ``[R, length]`` sequence, the
cache and its position, the ``[capacity, Dh]`` fp32 rotary tables (one ``rotary_emb`` call over ``arange(capacity)``, before its
cast), the weight set (``llama_weights.LlamaWeights`` in its allocated form: the packed q/k/v and gate/up weights, and under
autocast ``o_proj``, ``down_proj`` and ``lm_head`` in the autocast dtype too, so no replay repeats their cast), a ``[Ro]`` uniform
buffer where the caller gave ``memo['sampler']['u']``, a ``[R, V]`` buffer with the last step's logits, and the
``torch.cuda.CUDAGraph``.  ``step`` is not a walk of its own: it is ``LlamaTransformer._layers``, the one walk of every route, with
the attention step of the decode route (``_attend_static``) around ``decode_attention_at`` in place of ``decode_attention``,
followed by ``lm_head``, the sampler and ``decode_advance``, all on one stream: the captured graph is a single chain.

The first step behind the prompt runs eagerly through ``step`` on a side stream - the warm-up torch asks for in front of a capture,
and a real step: it advances the position.  The capture itself executes nothing; the remaining steps are ``graph.replay()``, with
one host ``advance(1)`` of the cache per replay, so the host count and the device position agree by construction.

``LlamaTransformer(..., static_cache=True, graph=True)`` keeps one ``DecodeGraph`` and reuses it while ``key_of`` gives the same
key; every ``generate`` call refreshes the weight set in place (weights trained in place between two calls are seen) and resets
the cache, the position and the sequence.
"""
from __future__ import annotations

import gc
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from .kv_cache import StaticKVCache
from .llama_weights import LlamaWeights, layers

__all__ = ['DecodeGraph']


class DecodeGraph:
    """The replayed decode step of ``module`` (a ``LlamaTransformer``) for ``R`` sequences of ``length`` tokens.

    ``begin(prompt, u)`` readies the buffers for one ``generate`` call, the caller runs the prompt through the eager decode route
    behind ``cache`` with ``weights`` as the module's weight set, and ``run(token)`` takes over from the first sampled token.
    ``autocast`` is the autocast dtype (None: off), ``with_u`` whether the sampler draws from the ``u`` buffer (else from torch's
    generator, inside the capture: every replay draws new uniforms)."""

    def __init__(self, module, R: int, length: int, codebook, *, device, cache_dtype, autocast=None, with_u: bool = False, key=None) -> None:
        lm = module._transformer
        model, config = lm.model, lm.config
        self.module, self.R, self.length, self.autocast, self.key = module, R, length, autocast, key
        self.codebook = SimpleNamespace(start=codebook.start, end=codebook.end)
        self.cache = StaticKVCache.for_model(config, R, length, cache_dtype, device)
        self.token = torch.zeros(R, 1, dtype=torch.int64, device=device)
        self.sequence = torch.zeros(R, length, dtype=torch.int64, device=device)
        self.cos = torch.empty(length, self.cache.head_dim, dtype=torch.float32, device=device)
        self.sin = torch.empty_like(self.cos)
        weight = model.embed_tokens.weight
        Ro = R // 2 if module.sampler.fused_arguments()['cfg_alpha'] is not None else R
        self.u = torch.zeros(Ro, dtype=torch.float32, device=device) if with_u else None
        self.memo = {'sampler': {'u': self.u}} if with_u else {}
        self.logits = torch.zeros(R, lm.lm_head.weight.shape[0], dtype=autocast or weight.dtype, device=device)
        # under autocast a linear would cast its fp32 weight in every replay: there the set holds the single projections as well
        self.weights = LlamaWeights(module, autocast).allocate(device)
        self.graph = None
        self.captures = 0

    def __deepcopy__(self, memo):
        return None                                                              # a copy of the module captures its own

    @staticmethod
    def key_of(module, tokens: torch.Tensor, length: int, codebook, cache_dtype, autocast, with_u: bool) -> tuple:
        """What a captured step depends on beyond the values it reads by pointer."""
        lm = module._transformer
        model = lm.model
        in_place = [model.embed_tokens.weight, model.norm.weight]
        for layer in layers(module):
            in_place +=[layer.input_layernorm.weight, layer.post_attention_layernorm.weight]
            if autocast is None:
                in_place += [layer.self_attn.o_proj.weight, layer.mlp.down_proj.weight]
        if autocast is None:
            in_place.append(lm.lm_head.weight)
        return (tokens.shape[0], length, cache_dtype, autocast, tuple(sorted(module.sampler.fused_arguments().items())), with_u,
                codebook.start, codebook.end, tokens.device, tuple(p.data_ptr() for p in in_place))

    # ---- one generate call -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> None:
        """The packed (and cast) copies and the rotary tables from the module's parameters as they are now, in place."""
        self.weights.refresh()
        positions = torch.arange(self.length, device=self.cos.device).unsqueeze(0)
        cos, sin = self.module._transformer.model.rotary_emb(self.cos, position_ids=positions)    # (an fp32 ``x``: the values before the cast)
        self.cos.copy_(cos[0])
        self.sin.copy_(sin[0])

    @torch.no_grad()
    def begin(self, prompt: torch.Tensor, u=None) -> None:
        """Readies the buffers for a ``generate`` call from ``prompt`` [R, P]; ``u``: the caller's ``memo['sampler']['u']``."""
        self.refresh()
        self.cache.reset()
        self.sequence.zero_()
        self.sequence[:, :prompt.shape[1]] = prompt
        if self.u is not None:
            self.u.copy_(u.reshape(-1))

    def step(self, torch_ops: bool = False) -> None:
        """One token: the module's walk with ``_attend_static`` around ``decode_attention_at`` - the cache's device position -
        then ``lm_head``, the sampler and ``decode_advance``.  Reads ``token``; leaves ``logits``, the next ``token``, one more
        column of ``sequence`` and the position counted.  ``torch_ops`` puts the ``_torch`` restatements in place of the kernels
        (they read the position on the host: any device, float64 included, never a capture)."""
        module, cache, weights, R = self.module, self.cache, self.weights, self.R
        attend_at = module._op('decode_attention_at', torch_ops)

        def core(i, scale, q, k, v):
            return attend_at(q, k, v, self.cos, self.sin, cache, i, scale=scale)
        x = module._transformer.model.embed_tokens(self.token)
        y = module._layers(x, weights, module._attend_static(weights, cache, core), torch_ops=torch_ops)
        logits = F.linear(y, weights('lm_head'))
        self.logits.copy_(logits[:, 0])
        token, self.memo = module.sample(logits, self.codebook, self.memo)
        module._op('decode_advance', torch_ops)(token.reshape(R), self.token.view(R), self.sequence, cache.position)

    def capture(self) -> None:
        """Captures ``step`` on the current device; nothing is executed.  The caller has run ``step`` eagerly on a side stream."""
        # No cyclic garbage collection while the stream captures: a graph that has become garbage would be destroyed wherever the
        # collector happens to run, and destroying one during another's capture ends the process (graphs.GraphedQuantizer).
        gc.collect()
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.step()
        finally:
            if gc_was_enabled:
                gc.enable()
        self.graph = graph
        self.captures += 1

    @torch.no_grad()
    def run(self, token: torch.Tensor) -> torch.Tensor:
        """Takes over behind the prompt: ``token`` [R, 1] is the first sampled token (column P, the cache holds P positions).
        Fills the sequence to ``length`` - the first step eagerly and then the capture where there is no graph yet, a replay per
        remaining token - and returns the sequence buffer."""
        cache = self.cache
        P = cache.get_seq_length()
        self.sequence[:, P] = token.reshape(-1)
        self.token.copy_(token.clamp(min=0).reshape(self.R, 1))
        cache.sync_position()
        steps = self.length - P - 1
        done = 0
        if self.graph is None:
            current = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(current)
            with torch.cuda.stream(side):
                self.step()
            current.wait_stream(side)
            cache.advance(1)
            done = 1
            route = self.module.sampler.last_route
            if route is None or route.name != 'fused':                           # nothing falls back inside a graph
                raise ValueError(f'DecodeGraph: the sampler left the fused route: {route}')
            self.capture()
        for _ in range(done, steps):
            self.graph.replay()
            cache.advance(1)
        return self.sequence
