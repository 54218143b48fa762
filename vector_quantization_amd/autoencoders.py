"""The two networks either side of the quantizer in the VQGAN configs, with the reference's names, registries, constructor
arguments, submodule names (so its checkpoints load with ``strict=True``) and ``forward(x, memo) -> (x, memo)`` signature
(vq/models/autoencoders.py, vq/algorithms/vqgan/autoencoder.py): ``VQGANEncoder`` and ``VQGANDecoder``, selected by
configs/vqgan/model.py, configs/decoder/vqgan.py and every configs/llamagen/vqgan*.py.

The convolutions and the single-head attention stay with the framework.  The step in front of every convolution,
``GroupNorm(32, C, 1e-6)`` followed by ``SiLU`` (25 sites in the default encoder, 35 in the default decoder), is one call:

- route ``fused``: ``functional.group_norm(..., act='silu')`` (``act=None`` for the norm of ``Attention``): the HIP kernels of
  include/vqhip.h read the activation in place in its dtype and memory format and write the activated result, fp32 arithmetic
  whatever the dtype;
- route ``torch``: ``F.group_norm`` and ``F.silu`` - what serves CPU and float64 tensors and ``fused=False``.

The norm's parameters stay an ``nn.GroupNorm`` child on both routes, so the state-dict keys do not depend on the route.
``routes.group_norm_why`` decides per call; the decision is kept in ``last_route``.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import functional
from .quantizers.memo import Memo
from .registries import VQDecoderRegistry, VQEncoderRegistry

__all__ = ['BaseEncoder', 'BaseDecoder', 'Attention', 'Residual', 'Layer', 'Downsample', 'Upsample', 'VQGANEncoder', 'VQGANDecoder']


class BaseEncoder(nn.Module, ABC):

    @property
    @abstractmethod
    def out_channels(self) -> int:
        pass

    @abstractmethod
    def forward(self, image: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        pass


class BaseDecoder(nn.Module, ABC):

    @property
    @abstractmethod
    def in_channels(self) -> int:
        pass

    @property
    @abstractmethod
    def last_parameter(self) -> nn.Parameter:
        pass

    @abstractmethod
    def forward(self, z: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        pass


def norm_act(norm: nn.GroupNorm, x: torch.Tensor, fused: bool, act: Optional[str] = 'silu') -> torch.Tensor:
    """One GroupNorm site with the parameters of the ``nn.GroupNorm`` child ``norm``, on the route the module took."""
    if fused:
        return functional.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps, act)
    return functional.group_norm_torch(x, norm.num_groups, norm.weight, norm.bias, norm.eps, act)


class Attention(nn.Module):
    """``x + attention(group_norm(x))`` over the H W positions, one head."""

    def __init__(self, *args, num_channels: int, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._num_channels = num_channels
        self._group_norm = nn.GroupNorm(32, self._num_channels, 1e-6)
        self._multihead_attention = nn.MultiheadAttention(self._num_channels, 1, batch_first=True)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        shortcut = x
        x = norm_act(self._group_norm, x, fused, None)
        x = x.flatten(2).transpose(1, 2)                                         # b c h w -> b (h w) c
        x, _ = self._multihead_attention(x, x, x, need_weights=False)
        x = x.transpose(1, 2).reshape(shortcut.shape)                            # b (h w) c -> b c h w
        return shortcut + x


class Residual(nn.Module):
    """``shortcut(x) + conv(act(norm(conv(act(norm(x))))))``; the two SiLU modules hold no state and run inside the norm's call."""

    def __init__(self, *args, in_channels: int, out_channels: int, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._in_channels = in_channels
        self._out_channels = out_channels
        self._residual = nn.Sequential(
            nn.GroupNorm(32, in_channels, 1e-6),
            nn.SiLU(),
            nn.Conv2d(in_channels, out_channels, 3, padding=1),
            nn.GroupNorm(32, out_channels, 1e-6),
            nn.SiLU(),
            nn.Conv2d(out_channels, out_channels, 3, padding=1),
        )
        self._shortcut = nn.Identity() if in_channels == out_channels else nn.Conv2d(in_channels, out_channels, 1)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        norm1, _, conv1, norm2, _, conv2 = self._residual
        r = conv1(norm_act(norm1, x, fused))
        r = conv2(norm_act(norm2, r, fused))
        return self._shortcut(x) + r


class Layer(nn.Module):

    def __init__(self, *args, in_channels: int, out_channels: int, depth: int, with_attentions: bool, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._in_channels = in_channels
        self._out_channels = out_channels
        self._depth = depth
        self._with_attentions = with_attentions
        self._residuals = nn.ModuleList(
            [Residual(in_channels=in_channels, out_channels=out_channels)]
            + [Residual(in_channels=out_channels, out_channels=out_channels) for _ in range(1, self._depth)],
        )
        if self._with_attentions:
            attentions = [Attention(num_channels=out_channels) for _ in range(self._depth)]
        else:
            attentions = [nn.Identity() for _ in range(self._depth)]
        self._attentions = nn.ModuleList(attentions)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        for residual, attention in zip(self._residuals, self._attentions):
            x = residual(x, fused)
            x = attention(x, fused) if isinstance(attention, Attention) else attention(x)
        return x


class Downsample(nn.Module):

    def __init__(self, *args, num_channels: int, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._num_channels = num_channels
        self._pad = nn.ZeroPad2d((0, 1, 0, 1))
        self._conv = nn.Conv2d(num_channels, num_channels, 3, 2)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._conv(self._pad(x))


class Upsample(nn.Module):
    """Nearest-neighbour doubling through float32 and back, as the reference writes it, then a 3 x 3 convolution."""

    def __init__(self, *args, num_channels: int, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._conv = nn.Conv2d(num_channels, num_channels, 3, padding=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        dtype = x.dtype
        x = F.interpolate(x.float(), scale_factor=2.0, mode='nearest')
        x = x.to(dtype)
        return self._conv(x)


class VQGANMixin(nn.Module):
    """``fused=False`` pins the torch route."""

    last_route = None

    def __init__(self, *args, in_channels: int, hidden_channels: int, out_channels: int, width: int, width_mults: tuple[int, ...],
                 depth_mult: int, attention_layer: Optional[int], refine_layer: Optional[int], resample_type: type,
                 fused: bool = True, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.fused = fused
        self._in_channels = in_channels
        self._hidden_channels = hidden_channels
        self._out_channels = out_channels
        self._width = width
        self._width_mults = width_mults
        self._depth_mult = depth_mult
        self._attention_layer = attention_layer
        self._refine_layer = refine_layer
        self._resample_type = resample_type

        self._in_conv = nn.Conv2d(in_channels, hidden_channels, 3, padding=1)

        widths = [width * wm for wm in self._width_mults]
        widths.insert(0, hidden_channels)

        if refine_layer is not None:
            refine_channels = widths[refine_layer]
            self._refine = nn.Sequential(
                Residual(in_channels=refine_channels, out_channels=refine_channels),
                Attention(num_channels=refine_channels),
                Residual(in_channels=refine_channels, out_channels=refine_channels),
            )

        with_attentions = [False] * len(self._width_mults)
        if attention_layer is not None:
            with_attentions[attention_layer] = True

        self._layers = nn.ModuleList([
            Layer(in_channels=ic, out_channels=oc, depth=self._depth_mult, with_attentions=wa)
            for ic, oc, wa in zip(widths[:-1], widths[1:], with_attentions)
        ])

        resamples = [resample_type(num_channels=c) for c in widths[1:-1]]
        resamples.append(nn.Identity())
        self._resamples = nn.Sequential(*resamples)

        self._projector = nn.Sequential(
            nn.GroupNorm(32, widths[-1], 1e-6),
            nn.SiLU(),
            nn.Conv2d(widths[-1], out_channels, 3, padding=1),
        )

    @property
    def num_layers(self) -> int:
        return len(self._width_mults)

    @property
    def in_channels(self) -> int:
        return self._in_channels

    @property
    def out_channels(self) -> int:
        return self._out_channels

    @property
    def last_parameter(self) -> nn.Parameter:
        conv = self._projector[-1]
        assert isinstance(conv, nn.Conv2d)
        return conv.weight

    def should_refine(self, layer: int) -> bool:
        return self._refine_layer is not None and layer == self._refine_layer

    def _run_refine(self, x: torch.Tensor, fused: bool) -> torch.Tensor:
        for block in self._refine:
            x = block(x, fused)
        return x

    def forward(self, x: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        from .quantizers import routes
        self.last_route = route = routes.group_norm_why(self, x)
        fused = route.name == 'fused'
        x = self._in_conv(x)
        for i, (layer, resample) in enumerate(zip(self._layers, self._resamples)):
            if self.should_refine(i):
                x = self._run_refine(x, fused)
            x = layer(x, fused)
            x = resample(x)
        if self.should_refine(self.num_layers):
            x = self._run_refine(x, fused)
        norm, _, conv = self._projector
        x = conv(norm_act(norm, x, fused))
        return x, memo


@VQEncoderRegistry.register_()
class VQGANEncoder(VQGANMixin, BaseEncoder):

    def __init__(self, *args, in_channels: int = 3, out_channels: int = 256, width: int = 128,
                 width_mults: tuple[int, ...] = (1, 1, 2, 2, 4), depth_mult: int = 2, **kwargs) -> None:
        kwargs.setdefault('attention_layer', len(width_mults) - 1)
        kwargs.setdefault('refine_layer', len(width_mults))
        kwargs.setdefault('resample_type', Downsample)
        super().__init__(*args, in_channels=in_channels, hidden_channels=width, out_channels=out_channels, width=width,
                         width_mults=width_mults, depth_mult=depth_mult, **kwargs)


@VQDecoderRegistry.register_()
class VQGANDecoder(VQGANMixin, BaseDecoder):

    def __init__(self, *args, in_channels: int = 256, out_channels: int = 3, width: int = 128,
                 width_mults: tuple[int, ...] = (4, 2, 2, 1, 1), depth_mult: int = 3, **kwargs) -> None:
        kwargs.setdefault('attention_layer', 0)
        kwargs.setdefault('refine_layer', 0)
        kwargs.setdefault('resample_type', Upsample)
        super().__init__(*args, in_channels=in_channels, hidden_channels=width * width_mults[0], out_channels=out_channels,
                         width=width, width_mults=width_mults, depth_mult=depth_mult, **kwargs)
