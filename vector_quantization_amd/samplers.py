"""The samplers of stage-2 generation under the reference's names and constructor kwargs
(vq/tasks/sequence_modeling/models/samplers.py:20-120): ``BaseSampler``, ``TopKTopPSampler``, ``CFGSampler``, registered in
``VQSMSamplerRegistry``.  ``BaseTransformer.sample`` (transformers.py:58-70) calls ``sampler(logits, codebook.start, codebook.end,
memo)`` once per generated position and gets ``(tokens, memo)``.

``forward`` takes the fused route — ONE launch of ``ops.sample_tokens`` on the logits as they are (slice, CFG mix, temperature,
top-k, top-p, draw, + start, CFG duplication; include/vqhip.h) — wherever ``routes.sampler_why`` allows it, and the reference's
composition written with torch ops otherwise (CPU tensors among them); the decision is kept in ``last_route``.

Randomness: the fused draw consumes one uniform per output row.  They come from the device's default generator in blocks of
``UNIFORM_BLOCK`` steps (``torch.rand(256, Ro)``), kept in the module and refilled when used up or when the number of rows
changes, so a step is one launch and a seeded run repeats itself.  ``memo['u']`` (fp32 [Ro]), if present, is used instead.
Inside a graph capture (``torch.cuda.graph``) the block is left alone and ``torch.rand(Ro)`` is captured with the launch, so
every replay draws new uniforms; a static ``memo['u']`` the caller refills between replays works as in eager mode.
The torch route draws with ``multinomial`` like the reference, or by the same inverse CDF when ``memo['u']`` is given.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import ops
from .config import BuildPreHookMixin, Config
from .registries import VQSMSamplerRegistry

__all__ = ['BaseSampler', 'TopKTopPSampler', 'CFGSampler']

UNIFORM_BLOCK = 256


def top_k_top_p_filtering(logits: torch.Tensor, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """transformers 4.35.2's ``top_k_top_p_filtering`` (TopKLogitsWarper, then the ascending-sort TopPLogitsWarper with
    min_tokens_to_keep = 1) with torch ops; the function left that library in later versions."""
    if top_k > 0:
        k = min(top_k, logits.shape[-1])
        kth = torch.topk(logits, k)[0][..., -1, None]
        logits = logits.masked_fill(logits < kth, -float('inf'))
    if 0 <= top_p <= 1.0:
        sorted_logits, sorted_indices = torch.sort(logits, descending=False)
        cumulative = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cumulative <= (1 - top_p)
        remove[..., -1:] = False
        remove = remove.scatter(-1, sorted_indices, remove)
        logits = logits.masked_fill(remove, -float('inf'))
    return logits


def draw_by_inverse_cdf(probabilities: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """[R, 1] tokens: the first index whose running probability exceeds u * total, the last token of non-zero probability if
    rounding leaves none (the draw of include/vqhip.h)."""
    p = probabilities.float()
    c = p.cumsum(-1)
    j = (c <= u.to(c.device, torch.float32).reshape(-1, 1) * c[:, -1:]).sum(-1)
    V = p.shape[-1]
    last = V - 1 - (p.flip(-1) > 0).int().argmax(-1)
    return torch.minimum(j, last).reshape(-1, 1)


class _Sampler(nn.Module):
    """What the three classes share: the route, the uniforms, ``forward``."""

    last_route = None

    def _draw(self, logits: torch.Tensor, memo) -> torch.Tensor:
        u = memo.get('u') if hasattr(memo, 'get') else None
        if u is not None:
            return draw_by_inverse_cdf(logits.softmax(-1), u)
        return logits.softmax(-1).multinomial(1)

    def sample(self, logits: torch.Tensor, memo):
        return self._draw(logits, memo), memo

    # ---- the fused route ---------------------------------------------------------------------------------------------------
    def fused_arguments(self) -> dict:
        """temperature / top_k / top_p / cfg_alpha of ``ops.sample_tokens`` for this sampler."""
        return dict(temperature=1.0, top_k=0, top_p=2.0, cfg_alpha=None)

    def _uniforms(self, Ro: int, device, memo) -> torch.Tensor:
        u = memo.get('u') if hasattr(memo, 'get') else None
        if u is not None:
            return u.to(device, torch.float32).reshape(-1).contiguous()
        if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            # a row of the module's block would be baked into the graph and every replay would draw from the same uniforms:
            # draw inside the capture, where torch's generator hands each replay its own Philox offset
            return torch.rand(Ro, device=device, dtype=torch.float32)
        block = getattr(self, '_u_block', None)
        if block is None or block.shape[1] != Ro or block.device != device or self._u_next >= block.shape[0]:
            block = torch.rand(UNIFORM_BLOCK, Ro, device=device, dtype=torch.float32)
            self._u_block, self._u_next = block, 0
        u = block[self._u_next]
        self._u_next += 1
        return u

    @torch.no_grad()
    def forward(self, logits: torch.Tensor, start: int, end: int, memo):
        from .quantizers import routes
        self.last_route = route = routes.sampler_why(self, logits, start, end)
        if route.name == 'fused':
            args = self.fused_arguments()
            R = logits.numel() // logits.shape[-1]
            Ro = R // 2 if args['cfg_alpha'] is not None else R
            tokens = ops.sample_tokens(logits, start, end, u=self._uniforms(Ro, logits.device, memo), **args)
            return tokens, memo
        return self.forward_torch(logits, start, end, memo)

    @torch.no_grad()
    def forward_torch(self, logits: torch.Tensor, start: int, end: int, memo):
        """The reference's ``forward`` as it stands (samplers.py:31-45): slice, ``sample``, + start."""
        shape = logits.shape
        logits = logits.reshape(-1, shape[-1])
        logits = logits[:, start:end]
        tokens, memo = self.sample(logits, memo)
        tokens = tokens + start
        tokens = tokens.reshape(shape[:-1])
        return tokens, memo


@VQSMSamplerRegistry.register_()
class BaseSampler(_Sampler):
    pass


@VQSMSamplerRegistry.register_()
class TopKTopPSampler(BaseSampler):

    def __init__(self, *args, temperature: float = 1.0, top_k: int = 600, top_p: float = 0.92, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._temperature = temperature
        self._top_k = top_k
        self._top_p = top_p

    def fused_arguments(self) -> dict:
        return dict(temperature=self._temperature, top_k=self._top_k, top_p=self._top_p, cfg_alpha=None)

    def sample(self, logits: torch.Tensor, memo):
        logits = logits / self._temperature
        logits = top_k_top_p_filtering(logits, self._top_k, self._top_p)
        return super().sample(logits, memo)


@VQSMSamplerRegistry.register_()
class CFGSampler(BuildPreHookMixin, BaseSampler):

    def __init__(self, *args, sampler: BaseSampler, alpha: float, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._sampler = sampler
        self._alpha = alpha

    @classmethod
    def sampler_build_pre_hook(cls, config: Config, registry, item) -> Config:
        config.sampler = VQSMSamplerRegistry.build_or_return(config.sampler)
        return config

    @classmethod
    def build_pre_hook(cls, config: Config, registry, item) -> Config:
        config = super().build_pre_hook(config, registry, item)
        config = cls.sampler_build_pre_hook(config, registry, item)
        return config

    def fused_arguments(self) -> dict:
        return dict(self._sampler.fused_arguments(), cfg_alpha=self._alpha)

    def sample(self, logits: torch.Tensor, memo):
        assert logits.shape[0] % 2 == 0
        unconditional_logits, conditional_logits = logits.chunk(2)
        cfg_logits = ((1 - self._alpha) * unconditional_logits + self._alpha * conditional_logits)
        tokens, memo = self._sampler.sample(cfg_logits, memo)
        tokens = tokens.repeat(2, *([1] * (tokens.dim() - 1)))                    # einops.repeat 'b ... -> (two b) ...'
        return tokens, memo
