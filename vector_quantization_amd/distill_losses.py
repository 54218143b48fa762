"""The distillation loss of VQ-KD, with the reference's name, registry and ``forward(pred_image, image)`` signature
(vq/algorithms/utils/losses.py:13-65): ``CosineEmbeddingLoss``, wired as ``r_loss`` between the decoder's ``pred_features`` and
the frozen teacher's ``target_features`` (configs/vqkd/model.py:62-74), added to the quantizer's loss by ``VQKD.forward``
(vq/algorithms/vqkd/base.py:82-92) and reported as ``cosine_embedding_r_loss`` (configs/vqkd/runner.py:91-94).

``forward`` takes the fused route (``ops.cosine_embedding_loss``: two launches forward, one backward, both tensors read in place
in their own dtypes) wherever ``routes.cosine_embedding_why`` allows it, and the reference's composition around
``F.cosine_embedding_loss`` otherwise (CPU tensors, float64, a target that requires grad); the decision is kept in ``last_route``.
``forward_map`` takes the decoder's NCHW map as it is (``tokenization.distill_loss``).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from .config import BuildPreHookMixin, Config
from .image_losses import BaseReconstructLoss
from .registries import VQLossRegistry

__all__ = ['CosineEmbeddingLoss']


@VQLossRegistry.register_()
class CosineEmbeddingLoss(BaseReconstructLoss, BuildPreHookMixin):
    """``1 - cos(pred, target)`` per feature vector, then ``reduction`` ('none' | 'mean' | 'sum') and a constant ``weight`` as
    ``BaseReconstructLoss`` has them.  ``cosine_embedding``: the keyword arguments of the inner ``F.cosine_embedding_loss``
    (the reference builds todd's wrapper of it with ``reduction='none'``); only ``margin`` is meaningful and it does not enter
    the target +1 branch, the only one the reference reaches."""

    def __init__(self, *args, cosine_embedding=None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._cosine_embedding = dict(cosine_embedding or {})

    @classmethod
    def build_pre_hook(cls, config: Config, registry, item) -> Config:
        config = super().build_pre_hook(config, registry, item)
        config.cosine_embedding = dict(config.get_config('cosine_embedding'))
        return config

    def _route(self, pred, target, layout):
        from .quantizers import routes
        self.last_route = route = routes.cosine_embedding_why(pred, target, layout=layout, loss=self)
        return route.name == 'fused'

    def _weigh(self, loss: torch.Tensor) -> torch.Tensor:
        return loss if self._weight == 1.0 else loss * self._weight

    def forward(self, pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        assert pred_image.shape == image.shape
        if self._route(pred_image, image, 'rows'):
            return self._weigh(ops.cosine_embedding_loss(pred_image, image, self._reduction))
        return self._reduce(self.forward_torch(pred_image, image))

    def forward_map(self, pred_map: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        """``forward`` for ``pred_map`` [B, C, *positions] as the decoder leaves it, against ``image`` [B, *positions, C] (or
        [B, P, C]): what ``forward(rearrange(pred_map, 'b c h w -> b (h w) c'), image)`` gives, without the rearrangement on the
        fused route.  'none' is shaped [B, *positions]."""
        if self._route(pred_map, image, 'map'):
            return self._weigh(ops.cosine_embedding_loss(pred_map, image, self._reduction, layout='map'))
        rows = pred_map.movedim(1, -1)
        return self._reduce(self.forward_torch(rows, image.reshape(rows.shape)))

    def forward_torch(self, pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        """The reference's forward in front of its ``_reduce``: flatten, ones target, the inner loss, reshape."""
        shape = pred_image.shape
        pred_image = pred_image.flatten(0, -2)
        image = image.flatten(0, -2)
        target = pred_image.new_ones(pred_image.shape[0])
        loss = F.cosine_embedding_loss(pred_image, image, target, reduction='none', **self._cosine_embedding)
        return loss.reshape(shape[:-1])
