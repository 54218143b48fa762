"""The stage-2 generator of the reference's LlamaGen configs under its names, registry and constructor arguments:
``BaseTransformer`` (vq/tasks/sequence_modeling/models/transformers.py with the KV-cache loop of vq/algorithms/ar/transformers/base.py),
``HFTransformer`` (hf.py) and ``LlamaTransformer`` (llama.py), selected by configs/ar/transformers/llama.py.  The network is
transformers' ``LlamaForCausalLM``, built from the config's dict unchanged and kept in ``_transformer``, so the state-dict keys are
the reference's and its checkpoints load with ``strict=True``.

The GEMMs, the rotary embedding and the attention core stay with the framework.  Everything between them is row-wise:

- route ``fused``: a walk over the submodules of ``LlamaForCausalLM`` that this file owns - nothing of transformers is edited and no
  module's ``forward`` is replaced.  The state carried from layer to layer is ``(x, pending)``, the residual stream and the branch not
  yet added to it.  Every ``LlamaRMSNorm`` is one ``functional.add_rms_norm`` call that adds the pending branch, leaves the sum and
  writes the normalised rows in the dtype the next ``linear`` reads (the autocast dtype under autocast, while the stream stays
  fp32); ``gate_proj`` and ``up_proj`` are ONE GEMM against their concatenated weights and ``functional.swiglu`` reads its two
  halves; ``self_attn`` is called as it is with ``attention_mask=None`` and the cache (its sdpa path is causal by itself there);
  ``forward`` puts ``CausalTokenLoss`` on the logits in place of the ``labels=`` path (so ``memo['accuracy']`` exists on this
  route only: the torch route's memo carries ``logits`` alone, as the reference's);
- route ``torch``: the reference's two lines, ``self._transformer(tokens, labels=tokens)`` and
  ``self._transformer(tokens, past_key_values=kv_cache)`` - what serves CPU and float64 tensors, ``fused=False`` and every
  configuration ``routes.llama_why`` names.

``routes.llama_why`` decides per call; the decision is kept in ``last_route``.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import functional
from . import samplers  # noqa: F401  (registers the samplers a config names)
from .config import BuildPreHookMixin, Config
from .quantizers.memo import get_memo
from .registries import VQSMSamplerRegistry, VQSMTransformerRegistry
from .sequence_losses import CausalTokenLoss
from .vqkd_autoencoders import _autocast_dtype

__all__ = ['BaseTransformer', 'HFTransformer', 'LlamaTransformer']


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

    def _generate(self, tokens: torch.Tensor, length: int, codebook, memo):
        assert tokens.shape[1] < length
        token = tokens
        kv_cache = None
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
    """``LlamaForCausalLM(LlamaConfig(**transformer))``.  ``fused=False`` pins the torch route."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._loss = CausalTokenLoss()

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

    # ---- the fused route -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _norm(norm: nn.Module, x: torch.Tensor, pending: Optional[torch.Tensor], *, torch_ops: bool = False):
        """One norm site: ``(x + pending, rms_norm(x + pending))`` with the parameters of the ``LlamaRMSNorm`` child."""
        out_dtype = _autocast_dtype(x)
        if pending is not None and pending.dtype != (out_dtype or x.dtype):
            pending = pending.to(out_dtype or x.dtype)
        if torch_ops:
            return functional.add_rms_norm_torch(x, pending, norm.weight, norm.variance_epsilon, out_dtype)
        return functional.add_rms_norm(x, pending, norm.weight, norm.variance_epsilon, out_dtype, strict=True)

    def _walk(self, tokens: torch.Tensor, kv_cache=None, *, torch_ops: bool = False) -> torch.Tensor:
        """Logits [B, L, V] of ``tokens`` [B, L] behind ``kv_cache`` (updated in place).  ``torch_ops`` puts the ``_torch``
        restatements in place of the two kernels: the same walk on any device, what the CPU tests hold against HF's forward."""
        lm = self._transformer
        model = lm.model
        x = model.embed_tokens(tokens)
        seen = kv_cache.get_seq_length() if kv_cache is not None else 0
        position_ids = (torch.arange(x.shape[1], device=x.device) + seen).unsqueeze(0)
        position_embeddings = model.rotary_emb(x, position_ids=position_ids)
        swiglu = functional.swiglu_torch if torch_ops else (lambda t: functional.swiglu(t, strict=True))
        pending = None
        for layer in model.layers[:model.config.num_hidden_layers]:
            x, y = self._norm(layer.input_layernorm, x, pending, torch_ops=torch_ops)
            attn, _ = layer.self_attn(hidden_states=y, position_embeddings=position_embeddings, attention_mask=None,
                                      past_key_values=kv_cache)
            x, y = self._norm(layer.post_attention_layernorm, x, attn, torch_ops=torch_ops)
            mlp = layer.mlp
            gate_up = F.linear(y, torch.cat((mlp.gate_proj.weight, mlp.up_proj.weight)))
            pending = mlp.down_proj(swiglu(gate_up))
        _, y = self._norm(model.norm, x, pending, torch_ops=torch_ops)
        return lm.lm_head(y)

    def _route(self, tokens: torch.Tensor, kv_cache=None, attention_mask=None) -> bool:
        from .quantizers import routes
        self.last_route = route = routes.llama_why(self, tokens, kv_cache, attention_mask)
        return route.name == 'fused'

    def _inference(self, tokens: torch.Tensor, kv_cache, memo, attention_mask=None):
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
