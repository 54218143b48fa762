"""The pixel losses of image reconstruction, with the reference's names and ``forward(pred_image, image)`` signature
(vq/tasks/image_reconstruction/losses.py): ``L1Loss``, ``MSELoss``, ``PSNRLoss``, ``SSIMLoss``.  The reference uses them as
validation metrics (configs/vqgan/runner.py:93-116).  ``LPIPSLoss``, the fifth class of that file, lives in ``perceptual_losses.py``: it
is no column of ``ops.image_metrics`` (``column_of`` and ``is_plain`` do not claim it) and has a fused route of its own.

- Float images in [0, 1], as ``dataset.decode(v) / 255`` gives them: the reference's composition with torch ops - route
  ``torch``, which also serves CPU tensors and keeps autograd for L1, MSE and PSNR.  ``SSIMLoss`` on this route is the
  definition scikit-image's defaults give when called as the reference calls it (``channel_axis=0, data_range=1``), through
  ``F.avg_pool2d(., 7, 1)`` in float64 on the tensor's device: no scikit-image, no host copy.
- uint8 images (already decoded): the loss per IMAGE, ``[B]``, before the reduction - on a GPU from ``ops.image_metrics`` (route
  ``fused``: one launch pair gives all four), elsewhere from the same torch composition on ``image / 255`` averaged per image.

``runners.ImageLossMetric`` is where the fusion pays: it hands the raw model-range images to ``ops.image_metrics`` once per batch
for all four.  The decision is kept in ``last_route``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .config import BuildPreHookMixin
from .registries import VQIRLossRegistry

__all__ = ['BaseReconstructLoss', 'L1Loss', 'MSELoss', 'PSNRLoss', 'SSIMLoss', 'ssim_torch', 'column_of', 'is_plain']


def ssim_torch(pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
    """SSIM per image ``[B]`` of float images in [0, 1], float64: uniform 7 x 7 window, sample covariance (49 / 48),
    K1 = 0.01, K2 = 0.03, data_range 1, windows wholly inside the image (scikit-image crops the 3-pixel border its filter's
    boundary mode touches), mean over windows and channels."""
    if pred_image.dim() != 4 or pred_image.shape != image.shape or min(pred_image.shape[-2:]) < 7:
        raise ValueError(f'SSIM needs two [B, C, H, W] batches with H, W >= 7, got {tuple(pred_image.shape)} and {tuple(image.shape)}')
    x, y = pred_image.double(), image.double()
    cov_norm = 49 / 48

    def mean(t):
        return F.avg_pool2d(t, 7, 1)

    ux, uy = mean(x), mean(y)
    vx = cov_norm * (mean(x * x) - ux * ux)
    vy = cov_norm * (mean(y * y) - uy * uy)
    vxy = cov_norm * (mean(x * y) - ux * uy)
    c1, c2 = ops.SSIM_C1, ops.SSIM_C2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.mean(dim=(1, 2, 3))


class BaseReconstructLoss(nn.Module):
    """What the four classes use of todd's BaseLoss: ``reduction`` ('none' | 'mean' | 'sum') and a constant ``weight``."""

    COLUMN = ''                                  # the column of ops.image_metrics that is this loss per image
    last_route = None

    def __init__(self, *args, reduction: str = 'mean', weight: float = 1.0, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        assert reduction in ('none', 'mean', 'sum'), reduction
        self._reduction = reduction
        self._weight = weight

    def _reduce(self, loss: torch.Tensor) -> torch.Tensor:
        if self._reduction == 'mean':
            loss = loss.mean()
        elif self._reduction == 'sum':
            loss = loss.sum()
        return loss if self._weight == 1.0 else loss * self._weight

    def forward(self, pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        from .quantizers import routes
        if pred_image.dtype == torch.uint8 and image.dtype == torch.uint8:
            self.last_route = route = routes.image_metrics_why(pred_image, image, ssim=self.COLUMN == 'ssim')
            if route.name == 'fused':
                return self._reduce(ops.image_metrics(pred_image, image, ssim=self.COLUMN == 'ssim')[self.COLUMN])
            return self._reduce(self.per_image(pred_image.float() / 255, image.float() / 255))
        self.last_route = routes.Route('torch', 'float images in [0, 1]: the reference\'s composition')
        return self._reduce(self.forward_torch(pred_image, image))

    def forward_torch(self, pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        """The reference's forward in front of its ``_reduce``."""
        raise NotImplementedError

    def per_image(self, pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        """``[B]``: ``forward_torch`` averaged per image, what ImageLossMetric makes of it (vq/runners/metrics/loss.py:36)."""
        loss = self.forward_torch(pred_image, image)
        return loss.reshape(loss.shape[0], -1).mean(dim=1)


@VQIRLossRegistry.register_()
class L1Loss(BaseReconstructLoss, BuildPreHookMixin):
    COLUMN = 'l1'

    def forward_torch(self, pred_image, image):
        return F.l1_loss(pred_image, image, reduction='none')


@VQIRLossRegistry.register_()
class MSELoss(BaseReconstructLoss, BuildPreHookMixin):
    COLUMN = 'mse'

    def forward_torch(self, pred_image, image):
        return F.mse_loss(pred_image, image, reduction='none')


@VQIRLossRegistry.register_()
class SSIMLoss(BaseReconstructLoss):
    COLUMN = 'ssim'

    def forward_torch(self, pred_image, image):
        return ssim_torch(pred_image, image)                                    # float64; the reference casts to pred's dtype


@VQIRLossRegistry.register_()
class PSNRLoss(MSELoss):
    COLUMN = 'psnr'

    def forward_torch(self, pred_image, image):
        loss = F.mse_loss(pred_image, image, reduction='none')
        loss = loss.reshape(loss.shape[0], -1).mean(dim=1)
        return -10 * loss.log10()


_PLAIN = (PSNRLoss, MSELoss, L1Loss, SSIMLoss)                                  # PSNRLoss first: it is an MSELoss


def column_of(loss) -> str:
    """'l1' / 'mse' / 'psnr' / 'ssim' for an instance of one of the four classes (or a subclass), '' for anything else."""
    for klass in _PLAIN:
        if isinstance(loss, klass):
            return klass.COLUMN
    return ''


def is_plain(loss) -> bool:
    """One of the four classes with the ``forward`` and ``forward_torch`` it came with: its value per image is a column of
    ``ops.image_metrics``.  A subclass that overrides either computes something else and is run as written."""
    for klass in _PLAIN:
        if isinstance(loss, klass):
            return type(loss).forward is BaseReconstructLoss.forward and type(loss).forward_torch is klass.forward_torch
    return False
