"""The perceptual loss of image reconstruction, with the reference's name, registry, state-dict keys and
``forward(pred_image, image)`` signature (vq/tasks/image_reconstruction/losses.py:99-178): ``LPIPSLoss``, wired as ``lpips_r_loss``
into every VQGAN generator step (configs/vqgan/model.py:29) and reported as ``lpips_loss`` by the validator
(configs/vqgan/runner.py:83-92).

The VGG16 feature stack runs in torch (its convolutions are the framework's); it is built here in plain torch with torchvision's
module indices and key names, so a reference checkpoint loads, and it stops after module 29 - the reference runs the rest of the
network and throws the result away.  Everything behind the five taps - the channel normalisation of both feature maps, the
squared difference, dropout, the 1 x 1 convolution and the spatial mean - takes the fused route (``ops.lpips_distance``: two
launches per layer forward, one backward, the features read in place in their own dtype and layout) wherever
``routes.lpips_why`` allows it, and the reference's lines (``distance_torch``) otherwise; the decision is kept in ``last_route``.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .config import Config
from .image_losses import BaseReconstructLoss
from .registries import VQIRLossRegistry

__all__ = ['LPIPSLoss', 'vgg16_features']

VGG16_LAYERS = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M')
TAPS = (3, 8, 15, 22, 29)                                   # the ReLUs whose outputs the reference hooks
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)


def vgg16_features() -> nn.Sequential:
    """torchvision's ``vgg16().features``: 13 convolutions, each followed by a ReLU, and 5 max-pools, 31 modules with the same
    indices (so the same state-dict keys)."""
    layers, channels = [], 3
    for v in VGG16_LAYERS:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(channels, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            channels = v
    return nn.Sequential(*layers)


class _VGG16(nn.Module):
    """The part of torchvision's VGG the loss uses, under its name ``features``."""

    def __init__(self) -> None:
        super().__init__()
        self.features = vgg16_features()


@VQIRLossRegistry.register_()
class LPIPSLoss(BaseReconstructLoss):
    """``sum_layers mean_hw conv1x1(dropout((normalize(vgg(pred)) - normalize(vgg(image)))^2))``, ``[B, 1, 1, 1]`` before the
    reduction, then ``reduction`` and ``weight`` as ``BaseReconstructLoss`` has them.  Every parameter is frozen.  Dropout
    (p = 0.5, the reference's ``nn.Dropout()``) is active exactly when ``self._dropout.training``."""

    _SKIPPED = ('_vgg.classifier.', '_vgg.avgpool')        # of a reference checkpoint: run there, never used

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.register_buffer('_mean', torch.tensor(MEAN).view(1, 3, 1, 1))
        self.register_buffer('_std', torch.tensor(STD).view(1, 3, 1, 1))
        self._vgg = _VGG16()
        self._dropout = nn.Dropout()
        self._convs = nn.ModuleList(nn.Conv2d(c, 1, 1, bias=False) for c in ops.LPIPS_CHANNELS)
        self.requires_grad_(False)
        self._register_load_state_dict_pre_hook(self._drop_skipped)

    @classmethod
    def _drop_skipped(cls, state_dict, prefix, *args) -> None:
        for key in [k for k in state_dict if k.startswith(tuple(prefix + s for s in cls._SKIPPED))]:
            del state_dict[key]

    def init_weights(self, config: Config) -> bool:
        """``_convs`` from ``config.pretrained`` (default: the reference's path) when that file exists; no recursion."""
        config = Config(config)
        path = config.get('pretrained', 'pretrained/lpips/vgg.pth.converted')
        if os.path.exists(path):
            self._convs.load_state_dict(torch.load(path, map_location='cpu'))
        return False

    def normalize(self, image: torch.Tensor) -> torch.Tensor:
        return (image - self._mean) / self._std

    def extract_features(self, image: torch.Tensor) -> list:
        """The outputs of modules 3, 8, 15, 22 and 29 for the normalised image, NOT normalised over the channels (the fused
        route does that itself; ``distance_torch`` does it as the reference's hook did)."""
        x, outs = self.normalize(image), []
        for i, module in enumerate(self._vgg.features):
            x = module(x)
            if i in TAPS:
                outs.append(x)
            if i == TAPS[-1]:
                break
        return outs

    def distance_torch(self, pred_features, features) -> torch.Tensor:
        """The reference's lines behind the feature extraction: ``losses_`` [B, 1, 1, 1]."""
        losses_ = pred_features[0].new_zeros([])
        for pred_feature, feature, conv in zip(pred_features, features, self._convs):
            pred_feature = F.normalize(pred_feature, p=2, dim=1, eps=1e-10)
            feature = F.normalize(feature, p=2, dim=1, eps=1e-10)
            loss = F.mse_loss(pred_feature, feature, reduction='none')
            loss = self._dropout(loss)
            loss = conv(loss)
            losses_ = losses_ + loss.mean(dim=(2, 3), keepdim=True)
        return losses_

    def forward_torch(self, pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        """The reference's forward in front of its ``_reduce``."""
        return self.distance_torch(self.extract_features(pred_image), self.extract_features(image))

    def _seed(self, device) -> torch.Tensor:
        """Two words from torch's generator of ``device``, left on the device: no host synchronisation, graph-capturable."""
        return torch.empty(2, dtype=torch.int32, device=device).random_()

    def forward(self, pred_image: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        from .quantizers import routes
        assert pred_image.shape == image.shape
        if pred_image.dim() == 4 and ops.dense_layout(pred_image) is not None and ops.dense_layout(image) != ops.dense_layout(pred_image):
            # three channels: a small copy that lets both feature stacks come out in one memory format
            nhwc = ops.dense_layout(pred_image) == 'rows'
            image = image.contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        pred_features = self.extract_features(pred_image)
        with torch.no_grad():
            features = self.extract_features(image)
        self.last_route = route = routes.lpips_why(self, pred_features, features)
        if route.name != 'fused':
            return self._reduce(self.distance_torch(pred_features, features))
        seed = self._seed(pred_image.device) if self._dropout.training else None
        value = ops.lpips_distance(pred_features, features, [conv.weight for conv in self._convs], seed, self._dropout.p)
        return self._reduce(value.view(-1, 1, 1, 1))
