"""The adversarial losses of a VQGAN step, with the reference's names, registries and signatures (vq/algorithms/vqgan/losses/):
``VQGANGeneratorLoss`` and ``NonSaturatingLoss`` over ``logits_fake``, ``VQGANDiscriminatorLoss`` (hinge) over
``(logits_fake, logits_real)``, and ``R1GradientPenalty`` over ``(discriminator, image)``.  Plain torch on a handful of logits;
``reduction`` and ``weight`` as ``image_losses.BaseReconstructLoss`` has them.  ``R1GradientPenalty`` differentiates the
discriminator with ``create_graph=True``: on the fused route of ``StyleGAN2Discriminator`` that runs the kernels' backward as a
differentiable function (functional.py), so the penalty's own backward reaches every parameter."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .image_losses import BaseReconstructLoss
from .registries import VQDiscriminatorLossRegistry, VQGeneratorLossRegistry

__all__ = ['VQGANGeneratorLoss', 'NonSaturatingLoss', 'VQGANDiscriminatorLoss', 'R1GradientPenalty']


class _BaseGANLoss(BaseReconstructLoss):
    """``reduction`` and ``weight`` only: ``forward`` belongs to the subclass."""

    def forward(self, *args, **kwargs) -> torch.Tensor:
        raise NotImplementedError


@VQGeneratorLossRegistry.register_()
class VQGANGeneratorLoss(_BaseGANLoss):

    def forward(self, logits_fake: torch.Tensor) -> torch.Tensor:
        return self._reduce(-logits_fake)


@VQGeneratorLossRegistry.register_()
class NonSaturatingLoss(_BaseGANLoss):
    """BCE against ones; ``binary_cross_entropy_with_logits`` averages already, as in the reference."""

    def forward(self, logits_fake: torch.Tensor) -> torch.Tensor:
        return self._reduce(F.binary_cross_entropy_with_logits(logits_fake, torch.ones_like(logits_fake)))


@VQDiscriminatorLossRegistry.register_()
class VQGANDiscriminatorLoss(_BaseGANLoss):

    def forward(self, logits_fake: torch.Tensor, logits_real: torch.Tensor) -> torch.Tensor:
        return self._reduce((F.relu(1. + logits_fake) + F.relu(1. - logits_real)) / 2)


class R1GradientPenalty(_BaseGANLoss):
    """https://arxiv.org/abs/1801.04406: the squared norm per image of d logits_real / d image, with the discriminator in eval mode
    for that forward (every module's mode is restored).  Unregistered, as in the reference: a trainer builds it by hand."""

    def forward(self, discriminator, image: torch.Tensor) -> torch.Tensor:
        image = image.clone().requires_grad_()
        training = {module: module.training for module in discriminator.modules()}
        discriminator.eval()
        try:
            logits_real = discriminator(image)
        finally:
            for module, mode in training.items():
                module.training = mode
        gradients, = torch.autograd.grad(logits_real, image, torch.ones_like(logits_real), create_graph=True)
        return self._reduce(gradients.flatten(1).norm(2, dim=1).pow(2))
