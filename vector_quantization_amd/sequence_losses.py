"""The losses a stage-2 transformer trains on, on the fused token cross-entropy (``ops.token_cross_entropy``: one read of the
logits in the forward, one read and one write in the backward; include/vqhip.h):

- ``CausalTokenLoss``: ``output['loss']`` of the HF causal LM called with ``labels=tokens`` (vq/algorithms/ar/transformers/hf.py:61-69)
  - the mean cross-entropy of position l against token l + 1 over the whole vocabulary, ``ignore_index = -100``, in fp32.
- ``LabelSmoothingCrossEntropy``: MAGE's criterion (vq/algorithms/nar/transformers/mage.py:107-123), a per-row loss.
- ``MaskedTokenLoss``: MAGE's ``forward_loss`` (mage.py:479-489), the criterion averaged with the mask as weights.

``forward`` takes the fused route wherever ``routes.token_ce_why`` allows it, and the reference's composition written with
``log_softmax`` / ``gather`` otherwise (CPU tensors and float64 logits among them); the decision is kept in ``last_route``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import ops

__all__ = ['CausalTokenLoss', 'LabelSmoothingCrossEntropy', 'MaskedTokenLoss']


def smoothed_nll(x: torch.Tensor, target: torch.Tensor, smoothing: float) -> torch.Tensor:
    """mage.py:117-123 as it stands: rows ``x`` [N, V], ``target`` [N] -> the per-row loss [N]."""
    logprobs = F.log_softmax(x, dim=-1)
    nll_loss = -logprobs.gather(dim=-1, index=target.long().unsqueeze(1)).squeeze(1)
    if smoothing == 0:
        return nll_loss
    smooth_loss = -logprobs.mean(dim=-1)
    return (1. - smoothing) * nll_loss + smoothing * smooth_loss


class _TokenLoss(nn.Module):
    last_route = None

    def _route(self, logits, targets, start=0, end=None, **kwargs):
        from .quantizers import routes
        self.last_route = route = routes.token_ce_why(logits, targets, start, end, **kwargs)
        return route.name == 'fused'


class CausalTokenLoss(_TokenLoss):
    """``forward(logits [B, L, Vt], tokens [B, L], memo) -> (loss, memo)``: HF's shifted mean cross-entropy of ``labels=tokens``,
    with neither tensor sliced on the fused route.  ``memo['accuracy']``: the share of the counted positions whose arg-max is the
    next token, a device scalar."""

    def __init__(self, ignore_index: int = -100, label_smoothing: float = 0.0) -> None:
        super().__init__()
        self._ignore_index = ignore_index
        self._label_smoothing = label_smoothing

    def forward(self, logits: torch.Tensor, tokens: torch.Tensor, memo):
        if self._route(logits, tokens, label_smoothing=self._label_smoothing, shift=True):
            loss, stats = ops.token_cross_entropy(logits, tokens, label_smoothing=self._label_smoothing,
                                                  ignore_index=self._ignore_index, shift=True, want_stats=True)
            memo['accuracy'] = stats['hits'] / stats['weight_sum']
            return loss, memo
        return self.forward_torch(logits, tokens, memo)

    def forward_torch(self, logits: torch.Tensor, tokens: torch.Tensor, memo):
        """transformers' causal-LM loss: upcast (16-bit logits to fp32), shift, flatten, ``cross_entropy``."""
        logits = logits.float() if logits.dtype in (torch.bfloat16, torch.float16) else logits
        shift_logits = logits[..., :-1, :].reshape(-1, logits.shape[-1])
        shift_labels = tokens[..., 1:].reshape(-1).long()
        loss = F.cross_entropy(shift_logits, shift_labels, ignore_index=self._ignore_index, label_smoothing=self._label_smoothing)
        counted = shift_labels != self._ignore_index
        memo['accuracy'] = ((shift_logits.argmax(-1) == shift_labels) & counted).sum() / counted.sum()
        return loss, memo


class LabelSmoothingCrossEntropy(_TokenLoss):
    """NLL loss with label smoothing (the reference's name and signature): ``forward(x [N, V], target [N]) -> loss [N]``."""

    def __init__(self, smoothing: float = 0.1) -> None:
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self._route(x, target, label_smoothing=self.smoothing):
            # (no target is ignored in the reference's criterion: an index no target can hold)
            return ops.token_cross_entropy(x, target, label_smoothing=self.smoothing, ignore_index=-(1 << 62), reduction='none')
        return smoothed_nll(x, target, self.smoothing)


class MaskedTokenLoss(_TokenLoss):
    """MAGE's ``forward_loss``: ``forward(gt_indices [B, S], logits [B, S + 1, Vt], mask [B, S + 1])`` -> the mean of the
    criterion on ``logits[:, 1:, :codebook_size]`` with ``mask[:, 1:]`` as weights.

    The ``[:, 1:]`` view of the logits does not flatten to rows of one stride for B > 1, so the fused route passes ALL
    B (S + 1) rows and gives position 0 of every sequence weight 0 and an ignored target: those rows contribute exactly nothing
    to either sum and get a zero gradient, and nothing is copied but the [B, S + 1] targets and weights."""

    IGNORED = -100

    def __init__(self, codebook_size: int, smoothing: float = 0.1) -> None:
        super().__init__()
        self.codebook_size = codebook_size
        self.criterion = LabelSmoothingCrossEntropy(smoothing)

    def forward(self, gt_indices: torch.Tensor, logits: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        smoothing = self.criterion.smoothing
        if not (gt_indices.dim() == 2 and logits.dim() == 3 and logits.shape[:2] == mask.shape == (gt_indices.shape[0], gt_indices.shape[1] + 1)):
            from .quantizers.routes import Route
            self.last_route = Route('torch', 'gt_indices, logits and mask are not [B, S], [B, S + 1, Vt] and [B, S + 1]')
            return self.forward_torch(gt_indices, logits, mask)
        targets = F.pad(gt_indices, (1, 0), value=self.IGNORED)                   # [B, S + 1]: position 0 is ignored
        if self._route(logits, targets, 0, self.codebook_size, label_smoothing=smoothing, weight=mask):
            weight = mask.to(torch.float32).clone()
            weight[:, 0] = 0
            return ops.token_cross_entropy(logits, targets, 0, self.codebook_size, label_smoothing=smoothing,
                                           ignore_index=self.IGNORED, weight=weight)
        return self.forward_torch(gt_indices, logits, mask)

    def forward_torch(self, gt_indices: torch.Tensor, logits: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """mage.py:479-489 as it stands."""
        bsz, seq_len = gt_indices.size()
        loss = smoothed_nll(logits[:, 1:, :self.codebook_size].reshape(bsz * seq_len, -1), gt_indices.reshape(bsz * seq_len),
                            self.criterion.smoothing)
        loss = loss.reshape(bsz, seq_len)
        return (loss * mask[:, 1:]).sum() / mask[:, 1:].sum()
