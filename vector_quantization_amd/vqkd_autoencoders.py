"""The two networks either side of the quantizer in the VQ-KD configs, with the reference's names, registries, constructor
arguments, submodule names (so its checkpoints load with ``strict=True``) and ``forward(x, memo) -> (x, memo)`` signature
(vq/algorithms/vqkd/autoencoder.py): ``VQKDEncoder`` and ``VQKDDecoder``, selected by configs/vqkd/model.py and
configs/decoder/vqkd.py.  Both are a plain pre-norm ViT: patch embedding, cls token, position embedding, ``depth`` blocks,
``fc_norm`` over the patch tokens and a ``Linear - Tanh - Linear`` task layer.

The GEMMs, the patch convolution and the attention core stay with the framework.  Everything between them is row-wise:

- route ``fused``: the state carried from block to block is ``(x, pending)``, the residual stream and the branch not yet added
  to it.  Every norm is one ``functional.add_layer_norm`` call that adds the pending branch, leaves the sum and writes the
  normalised rows in the dtype the next ``linear`` reads (the autocast dtype under autocast, while the stream stays fp32);
  ``fc1`` runs without its bias and ``functional.row_bias_act`` adds it inside the GELU, as the task layer's first ``Linear``
  does inside the tanh; the attention core is ``F.scaled_dot_product_attention``;
- route ``torch``: the reference's lines - what serves CPU and float64 tensors and ``fused=False``.

The norms stay ``nn.LayerNorm`` children on both routes, so the state-dict keys do not depend on the route.
``routes.vit_why`` decides per call; the decision is kept in ``last_route``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import functional
from .autoencoders import BaseDecoder, BaseEncoder
from .quantizers.memo import Memo
from .registries import VQDecoderRegistry, VQEncoderRegistry
from .utils import autocast_dtype

__all__ = ['Mlp', 'Attention', 'Block', 'PatchEmbed', 'VQKDEncoder', 'VQKDDecoder']


def _norm(norm: nn.LayerNorm, x: torch.Tensor, pending: Optional[torch.Tensor]):
    """One norm site of the fused route: ``(x + pending, norm(x + pending))`` with the parameters of the ``nn.LayerNorm`` child."""
    out_dtype = autocast_dtype(x)
    if pending is not None and pending.dtype != (out_dtype or x.dtype):
        pending = pending.to(out_dtype or x.dtype)
    return functional.add_layer_norm(x, pending, norm.weight, norm.bias, norm.eps, out_dtype, strict=True)


class Mlp(nn.Module):

    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        if fused:
            x = functional.row_bias_act(F.linear(x, self.fc1.weight), self.fc1.bias, 'gelu', strict=True)
        else:
            x = self.act(self.fc1(x))
        return self.fc2(x)


class Attention(nn.Module):

    def __init__(self, dim, num_heads=8):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        all_head_dim = head_dim * self.num_heads
        self.scale = head_dim**-0.5

        self.qkv = nn.Linear(dim, all_head_dim * 3, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(all_head_dim))
        self.v_bias = nn.Parameter(torch.zeros(all_head_dim))

        self.proj = nn.Linear(all_head_dim, dim)

    def forward(self, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
        b, n, _ = x.shape
        qkv_bias = torch.cat((self.q_bias, torch.zeros_like(self.v_bias, requires_grad=False), self.v_bias))
        qkv = F.linear(input=x, weight=self.qkv.weight, bias=qkv_bias)
        qkv = qkv.reshape(b, n, 3, self.num_heads, -1).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]                                         # (B, H, N, C)
        if fused:
            x = F.scaled_dot_product_attention(q, k, v, scale=self.scale)
        else:
            q = q * self.scale
            attn = q @ k.transpose(-2, -1)
            attn = attn.softmax(dim=-1)
            x = attn @ v
        x = x.transpose(1, 2).reshape(b, n, -1)
        return self.proj(x)


class Block(nn.Module):

    def __init__(self, dim, num_heads, norm_layer: Optional[dict] = None, mlp_ratio=4.):
        super().__init__()
        eps = dict(norm_layer or {}).get('eps', 1e-6)                            # the reference's dict(type='LN', eps=1e-06)
        self.norm1 = nn.LayerNorm(dim, eps)
        self.attn = Attention(dim, num_heads=num_heads)
        self.norm2 = nn.LayerNorm(dim, eps)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x + self.attn(self.norm1(x))
        x = x + self.mlp(self.norm2(x))
        return x

    def forward_fused(self, x: torch.Tensor, pending: Optional[torch.Tensor]):
        """``(x, pending)`` in, ``(x, pending)`` out: each norm adds the branch the previous step left."""
        x, y = _norm(self.norm1, x, pending)
        x, y = _norm(self.norm2, x, self.attn(y, True))
        return x, self.mlp(y, True)


class PatchEmbed(nn.Module):
    """Image to Patch Embedding."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        num_patches = (img_size // patch_size)**2
        self.patch_size = patch_size
        self.num_patches = num_patches

        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(x).flatten(2).transpose(1, 2)


class VQKDMixin(nn.Module):
    """``fused=False`` pins the torch route."""

    last_route = None

    def __init__(self, *args, img_size: int, patch_size: int, in_chans: int, out_chans: int, out_patch_size: int = 1,
                 embed_dim: int = 768, depth: int = 12, num_heads: int = 12, mlp_ratio: float = 4., fused: bool = True,
                 **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.fused = fused
        norm_layer = dict(type='LN', eps=1e-06)
        self.num_features = self.embed_dim = embed_dim
        self.patch_size = patch_size
        self.in_chans = in_chans
        self.out_chans = out_chans
        self.out_patch_size = out_patch_size

        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches

        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))

        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, norm_layer=norm_layer) for _ in range(depth)
        ])
        self.fc_norm = nn.LayerNorm(embed_dim, 1e-6)
        self.widest_row = max(embed_dim, int(embed_dim * mlp_ratio))          # what routes.vit_why holds against the kernels' rows

        self.task_layer = nn.Sequential(
            nn.Linear(embed_dim, embed_dim),
            nn.Tanh(),
            nn.Linear(embed_dim, out_chans * out_patch_size**2),
        )

    @staticmethod
    def _init_weights(m) -> None:
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
            return
        if isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.weight, 1.0)
            nn.init.constant_(m.bias, 0)
            return

    def init_weights(self, config=None) -> None:
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.blocks.apply(self._init_weights)
        self.fc_norm.apply(self._init_weights)
        for i, block in enumerate(self.blocks):
            divisor = (2 * (i + 1))**0.5
            block.attn.proj.weight.data.div_(divisor)
            block.mlp.fc2.weight.data.div_(divisor)
        self.task_layer.apply(self._init_weights)

    def interpolate_pos_encoding(self, x, w, h):
        npatch = x.shape[1] - 1
        n = self.pos_embed.shape[1] - 1
        if npatch == n and w == h:
            return self.pos_embed
        class_pos_embed = self.pos_embed[:, 0]
        patch_pos_embed = self.pos_embed[:, 1:]
        dim = x.shape[-1]
        w0 = w // self.patch_embed.patch_size
        h0 = h // self.patch_embed.patch_size
        # a small number is added to avoid a floating point error in the interpolation
        # (https://github.com/facebookresearch/dino/issues/8)
        w0, h0 = w0 + 0.1, h0 + 0.1
        patch_pos_embed = nn.functional.interpolate(
            patch_pos_embed.reshape(1, int(math.sqrt(n)), int(math.sqrt(n)), dim).permute(0, 3, 1, 2),
            scale_factor=(w0 / math.sqrt(n), h0 / math.sqrt(n)),
            mode='bicubic',
        )
        assert int(w0) == patch_pos_embed.shape[-2] and int(h0) == patch_pos_embed.shape[-1]
        patch_pos_embed = patch_pos_embed.permute(0, 2, 3, 1).reshape(1, -1, dim)
        return torch.cat((class_pos_embed.unsqueeze(0), patch_pos_embed), dim=1)

    def _embed(self, x: torch.Tensor) -> torch.Tensor:
        _, _, w, h = x.shape
        x = self.patch_embed(x)
        batch_size, _, _ = x.size()
        cls_tokens = self.cls_token.expand(batch_size, -1, -1)
        x = torch.cat((cls_tokens, x), dim=1)
        if self.pos_embed is not None:
            if x.shape[1] != self.pos_embed.shape[1]:
                x = x + self.interpolate_pos_encoding(x, w, h)
            else:
                x = x + self.pos_embed
        return x

    def _forward_fused(self, x: torch.Tensor) -> torch.Tensor:
        pending = None
        for blk in self.blocks:
            x, pending = blk.forward_fused(x, pending)
        # the last branch folds into fc_norm, which reads the patch tokens only: a dense copy of the two slices
        x = x[:, 1:, :].contiguous()
        pending = None if pending is None else pending[:, 1:, :].contiguous()
        _, x = _norm(self.fc_norm, x, pending)
        fc, _, head = self.task_layer
        x = functional.row_bias_act(F.linear(x, fc.weight), fc.bias, 'tanh', strict=True)
        return head(x)

    def forward(self, x: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        from .quantizers import routes
        self.last_route = route = routes.vit_why(self, x)
        x = self._embed(x)
        if route.name == 'fused':
            return self._forward_fused(x), memo
        for blk in self.blocks:
            x = blk(x)
        t = x[:, 1:, :]
        x = self.fc_norm(t)
        x = self.task_layer(x)
        return x, memo


@VQEncoderRegistry.register_()
class VQKDEncoder(VQKDMixin, BaseEncoder):
    """Vision Transformer from an image to one feature per patch, [B, out_chans, H / patch, W / patch]."""

    def __init__(self, *args, img_size: int = 224, patch_size: int = 16, in_chans: int = 3, out_chans: int = 32, **kwargs) -> None:
        super().__init__(*args, img_size=img_size, patch_size=patch_size, in_chans=in_chans, out_chans=out_chans, **kwargs)

    @property
    def out_channels(self) -> int:
        return self.out_chans

    def forward(self, x: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        b, _, w, h = x.shape
        x, memo = VQKDMixin.forward(self, x, memo)
        assert h % self.patch_size == 0 and w % self.patch_size == 0
        h_prime = h // self.patch_size
        w_prime = w // self.patch_size
        x = x.reshape(b, h_prime, w_prime, -1).permute(0, 3, 1, 2)               # b (h w) c -> b c h w
        x = x.contiguous()
        return x, memo


@VQDecoderRegistry.register_()
class VQKDDecoder(VQKDMixin, BaseDecoder):
    """Vision Transformer from the quantized map to ``out_chans`` values per ``out_patch_size`` x ``out_patch_size`` patch."""

    def __init__(self, *args, img_size: int = 14, patch_size: int = 1, in_chans: int = 32, out_chans: int = 512,
                 out_patch_size: int = 1, **kwargs) -> None:
        super().__init__(*args, img_size=img_size, patch_size=patch_size, in_chans=in_chans, out_chans=out_chans,
                         out_patch_size=out_patch_size, **kwargs)

    @property
    def in_channels(self) -> int:
        return self.in_chans

    @property
    def last_parameter(self) -> nn.Parameter:
        linear = self.task_layer[-1]
        assert isinstance(linear, nn.Linear)
        return linear.weight

    def forward(self, x: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        b, _, w, h = x.shape
        x, memo = VQKDMixin.forward(self, x, memo)
        p, c = self.out_patch_size, self.out_chans
        x = x.reshape(b, h, w, p, p, c).permute(0, 5, 1, 3, 2, 4).reshape(b, c, h * p, w * p)    # b (h w) (p q c) -> b c (h p) (w q)
        return x, memo
