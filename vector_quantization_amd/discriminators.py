"""The discriminators of the VQGAN configs, with the reference's names, registry, state-dict keys and ``forward(image)`` signature
(vq/algorithms/vqgan/discriminators/): ``PatchGANDiscriminator`` (configs/vqgan/model.py:26, plain torch modules) and
``StyleGAN2Discriminator`` (configs/vqgan/8192_stylegan2_imagenet_ddp.py, configs/llamagen/vqgan_stylegan2_imagenet_ddp.py).

The reference builds the StyleGAN2 discriminator on ``mmcv.ops.FusedBiasLeakyReLU`` and ``mmcv.ops.upfirdn2d``; mmcv is no
dependency here.  Both ops are restated (include/vqhip.h):

- route ``fused``: the HIP kernels of ``functional.bias_act``, ``functional.blur`` and ``functional.bias_act_blur``, the activations
  read in place in their dtype and memory format;
- route ``torch``: the same definitions in plain torch (``bias_act_torch``, ``blur_torch``), composed as the reference composes
  them - what serves CPU and float64 tensors and ``fused=False``.

The convolutions, the ``/ fan_in**0.5`` weight scale, ``Std`` and the ``/ 2**0.5`` of a Residual stay with torch on both routes.
``routes.stylegan2_why`` decides per call; the decision is kept in ``last_route``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from . import functional
from .config import Config
from .registries import VQDiscriminatorRegistry

__all__ = ['BaseDiscriminator', 'PatchGANDiscriminator', 'StyleGAN2Discriminator', 'bias_act_torch', 'blur_torch']

NEGATIVE_SLOPE, ACT_SCALE = 0.2, 2 ** 0.5


def bias_act_torch(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``leaky_relu(x + bias[c], 0.2) * 2**0.5`` for [B, C] or [B, C, H, W], in x's dtype."""
    shape = (1, -1) + (1,) * (x.dim() - 2)
    return F.leaky_relu(x + bias.to(x.dtype).view(shape), NEGATIVE_SLOPE) * ACT_SCALE


def blur_torch(x: torch.Tensor, kernel: torch.Tensor, pad, down: int = 1) -> torch.Tensor:
    """``upfirdn2d(x, kernel, padding=pad)`` per channel with zero padding, every ``down``-th output kept; ``pad`` = (p0, p1) for
    both axes.  The kernel is symmetric, so correlation and convolution agree."""
    C = x.shape[1]
    x = F.pad(x, (pad[0], pad[1], pad[0], pad[1]))
    weight = kernel.to(x.dtype).expand(C, 1, *kernel.shape)
    return F.conv2d(x, weight, groups=C)[:, :, ::down, ::down]


class BaseDiscriminator(nn.Module):
    last_route = None

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError


@VQDiscriminatorRegistry.register_()
class PatchGANDiscriminator(BaseDiscriminator):
    """The pix2pix patch discriminator: ``depth`` stride-2 convolutions, one stride-1, one to a single channel; batch norm on all but
    the first and the last.  Module indices under ``_discriminator`` as in the reference, so its checkpoints load.

    Route ``fused`` (``routes.patchgan_why``): every adjacent ``BatchNorm2d, LeakyReLU(0.2)`` pair in training mode is one
    ``functional.batch_norm(..., act='leaky_relu')`` - the HIP kernels of include/vqhip.h with batch statistics, the same
    parameters and buffers.  Route ``torch``, and any site the kernels refuse (eval mode, so ``R1GradientPenalty``): the modules
    as they are.  The convolutions and the first layer's LeakyReLU stay with torch on both routes."""

    def __init__(self, *args, in_channels: int = 3, width: int = 64, depth: int = 3, kernel_size: int = 4, padding: int = 1,
                 fused: bool = True, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.fused = fused
        mults = [1] + [min(2 ** n, 8) for n in range(1, depth + 1)]
        layers = [nn.Conv2d(in_channels, width, kernel_size, 2, padding), nn.LeakyReLU(0.2, True)]
        for n in range(1, depth + 1):
            stride = 2 if n < depth else 1
            layers += [nn.Conv2d(width * mults[n - 1], width * mults[n], kernel_size, stride, padding, bias=False),
                       nn.BatchNorm2d(width * mults[n]), nn.LeakyReLU(0.2, True)]
        layers.append(nn.Conv2d(width * mults[depth], 1, kernel_size, 1, padding))
        self._discriminator = nn.Sequential(*layers)

    def init_weights(self, config: Config) -> bool:
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight.data, 0.0, 0.02)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.normal_(m.weight.data, 1.0, 0.02)
                nn.init.constant_(m.bias.data, 0)
        return False

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        from .quantizers import routes
        self.last_route = route = routes.patchgan_why(self, image)
        if route.name != 'fused':
            return self._discriminator(image)
        layers, x, k, refused, taken = list(self._discriminator), image, 0, [], 0
        while k < len(layers):
            m, act = layers[k], layers[k + 1] if k + 1 < len(layers) else None
            if isinstance(m, nn.BatchNorm2d) and isinstance(act, nn.LeakyReLU):
                site = routes.patchgan_why(m, x)
                if site.name == 'fused' and act.negative_slope != NEGATIVE_SLOPE:
                    site = routes.Route('torch', f'negative_slope={act.negative_slope}, the kernels hold {NEGATIVE_SLOPE}')
                if site.name == 'fused':
                    x = functional.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps,
                                              'leaky_relu', m.num_batches_tracked)
                    k, taken = k + 2, taken + 1
                    continue
                refused.append(site.why)
            x = m(x)
            k += 1
        if not taken and refused:
            self.last_route = routes.Route('torch', refused[0])
        return x


class _Equalized(nn.Module):
    """Equalised learning rate: the parameter ``_original_weight`` ~ N(0, 1) is what the optimiser sees and the state dict holds;
    ``weight`` is a plain attribute, rewritten on every forward as ``_original_weight / fan_in**0.5``."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        original = self._parameters.pop('weight')
        self._original_weight = original
        self.weight = original.detach()

    @property
    def _fan_in(self) -> int:
        return math.prod(self._original_weight.shape[1:])

    def init_weights(self, config: Config) -> bool:
        nn.init.normal_(self._original_weight, 0., 1.)
        if self.bias is not None:
            nn.init.zeros_(self.bias)
        return False

    def _rescale(self) -> torch.Tensor:
        self.weight = self._original_weight / self._fan_in ** 0.5
        return self.weight


class FusedBiasLeakyReLU(nn.Module):
    """mmcv's module of that name: a zero-initialised ``bias`` [C], slope 0.2, scale 2**0.5."""

    def __init__(self, num_channels: int) -> None:
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(num_channels))

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        return functional.bias_act(x, self.bias) if fused else bias_act_torch(x, self.bias)


class Blur(nn.Module):
    """The [1, 3, 3, 1] blur in front of a downsampling convolution of ``kernel_size``, padded by
    ``(kernel_size // 2 + 1, (kernel_size + 1) // 2)``: (2, 2) for 3, (1, 1) for 1.  Both pairs are symmetric, so mmcv's old reading
    of a pair (before, after) and its new one (x, y) give the same four paddings; any other kernel size stays on the torch route
    (``routes.stylegan2_why``) rather than guess."""

    def __init__(self, *args, kernel_size: int, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        taps = torch.tensor([1., 3., 3., 1.])
        kernel = taps[None, :] * taps[:, None]
        self.register_buffer('_kernel', kernel / kernel.sum())
        self._kernel_size = kernel_size
        self._pad = (kernel_size // 2 + 1, (kernel_size + 1) // 2)

    @property
    def kernel(self) -> torch.Tensor:
        return self._kernel

    def forward(self, x: torch.Tensor, fused: bool = False, down: int = 1) -> torch.Tensor:
        return functional.blur(x, self._pad, down) if fused else blur_torch(x, self._kernel, self._pad, down)


class Linear(_Equalized, nn.Linear):

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        return F.linear(x, self._rescale(), self.bias)


class Conv2d(_Equalized, nn.Conv2d):
    """``downsample``: a Blur, then stride 2 without padding; otherwise stride 1 with ``kernel_size // 2``."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, *args, downsample: bool = False, **kwargs) -> None:
        stride, padding = (2, 0) if downsample else (1, kernel_size // 2)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, *args, **kwargs)
        self._downsample = downsample
        if downsample:
            self._blur = Blur(kernel_size=kernel_size)

    def _conv(self, x: torch.Tensor, stride=None) -> torch.Tensor:
        return F.conv2d(x, self._rescale(), self.bias, self.stride if stride is None else stride, self.padding)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        if not self._downsample:
            return self._conv(x)
        if fused and self.kernel_size == (1, 1):
            # blur, then a 1 x 1 convolution of stride 2, reads the blurred map at even positions only: the blur that keeps every
            # second output followed by the same convolution at stride 1 is the same sum, from a quarter of the blur outputs
            return self._conv(self._blur(x, True, down=2), stride=1)
        return self._conv(self._blur(x, fused))


class ActivateLinear(Linear):

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, bias=False, **kwargs)
        self._activate = FusedBiasLeakyReLU(self.out_features)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        return self._activate(super().forward(x), fused)


class ActivateConv2d(Conv2d):

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, bias=False, **kwargs)
        self._activate = FusedBiasLeakyReLU(self.out_channels)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        return self._activate(super().forward(x, fused), fused)


class Residual(nn.Module):
    """``(shortcut(x) + residual(x)) / 2**0.5``.  Route ``fused``: the residual branch runs conv3x3 -> ``bias_act_blur`` (pad 2: the
    first activation and the second convolution's blur in one launch, one read of the convolution's output and one write of the
    blurred map) -> conv3x3 stride 2 -> ``bias_act``; the shortcut runs ``blur`` (pad 1, down 2) -> conv1x1 stride 1, which is the
    reference's blur followed by its stride-2 1 x 1 convolution (that convolution reads the blurred map at even rows and columns
    only), with a quarter of the blur outputs computed."""

    def __init__(self, *args, in_channels: int, out_channels: int, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._residual = nn.Sequential(ActivateConv2d(in_channels, in_channels, 3),
                                       ActivateConv2d(in_channels, out_channels, 3, downsample=True))
        self._shortcut = Conv2d(in_channels, out_channels, 1, downsample=True, bias=False)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        first, second = self._residual
        if fused:
            r = functional.bias_act_blur(first._conv(x), first._activate.bias, second._blur._pad)
            r = second._activate(second._conv(r), True)
        else:
            r = second(first(x))
        return (self._shortcut(x, fused) + r) / 2 ** 0.5


class Std(nn.Module):
    """The minibatch standard deviation channel.  The batch is read as ``(bg b) c h w -> bg b c h w`` with bg = min(B, 4), as the
    reference writes it: sample n belongs to group n // (B / bg) and the deviation is taken ACROSS the groups, one value per
    position b inside a group, repeated ``(bg b)`` over the batch."""

    def __init__(self, *args, batch_groups: int = 4, eps: float = 1e-8, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._batch_groups = batch_groups
        self._eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        b, c, h, w = x.shape
        bg = min(b, self._batch_groups)
        y = x.reshape(bg, b // bg, c, h, w)
        y = (y.var(0, unbiased=False) + self._eps).sqrt()
        y = y.mean(dim=(1, 2, 3))
        y = y.repeat(bg).view(b, 1, 1, 1).expand(b, 1, h, w)
        return torch.cat([x, y], 1)


@VQDiscriminatorRegistry.register_()
class StyleGAN2Discriminator(BaseDiscriminator):
    """``forward(image [B, 3, S, S]) -> [B, 1]`` for S = ``image_size``, a power of two from 8 (B a multiple of min(B, 4), as
    ``Std`` needs).  ``fused=False`` pins the torch route."""

    CHANNELS = {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}

    def __init__(self, *args, image_size: int, fused: bool = True, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.fused = fused
        channels = [self.CHANNELS[2 ** i] for i in range(int(math.log2(image_size)), 1, -1)]
        self._layers = nn.Sequential(
            ActivateConv2d(3, channels[0], 1),
            *[Residual(in_channels=ic, out_channels=oc) for ic, oc in zip(channels[:-1], channels[1:])],
            Std(),
            ActivateConv2d(channels[-1] + 1, self.CHANNELS[4], 3),
        )
        self._projector = nn.Sequential(ActivateLinear(self.CHANNELS[4] * 4 * 4, self.CHANNELS[4]), Linear(self.CHANNELS[4], 1))

    def init_weights(self, config: Config) -> bool:
        """Every equalised layer: ``_original_weight`` ~ N(0, 1), its bias zero (the activations' biases are zero from construction).
        Stands in for the recursion the reference's framework runs over the children; returns False: nothing is left to recurse."""
        for m in self.modules():
            if isinstance(m, _Equalized):
                m.init_weights(config)
        return False

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        from .quantizers import routes
        self.last_route = route = routes.stylegan2_why(self, image)
        fused = route.name == 'fused'
        x = image
        for layer in self._layers:
            x = layer(x) if isinstance(layer, Std) else layer(x, fused)
        x = x.flatten(1)
        for layer in self._projector:
            x = layer(x, fused)
        return x
