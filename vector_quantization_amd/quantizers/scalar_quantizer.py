"""ScalarQuantizer / FiniteScalarQuantizer — mirror of vq/algorithms/sq/quantizers.py:1-12 and
vq/algorithms/fsq/quantizers.py:17-150.

FSQ is element-wise: per channel i with L_i levels, t = (tanh(x + atanh(odd / M)) * M - odd) / 2 with M = (L - 1) * (1 - eps),
the digit is round(t) + L // 2 and the token packs the digits in mixed radix (int32, as the reference's ``.to(torch.int)``).
Encode (tokens and z), its backward and the decode of tokens are one HIP launch each (``ops.fsq_encode`` / ``fsq_backward`` /
``fsq_decode``); the per-channel constants are evaluated once, at construction, by the reference's own torch expressions.
"""
from __future__ import annotations

from typing import Iterable

import torch
from torch import nn

from .. import functional as VF
from .. import ops
from ..registries import VQITQuantizerRegistry
from . import routes
from .memo import Memo, get_memo
from .quantizer_api import BaseQuantizer


@VQITQuantizerRegistry.register_()
class ScalarQuantizer(BaseQuantizer):
    pass


class BaseConverter(nn.Module):
    """Mixed-radix digits <-> tokens (fsq/quantizers.py:17-71).  Buffers: ``_cumprod`` int64 and ``_max_per_digit`` int32, both
    non-persistent (not in the state dict)."""

    def __init__(self, *args, max_per_digit: Iterable[int], **kwargs) -> None:
        super().__init__(*args, **kwargs)
        max_per_digit = tuple(max_per_digit)
        cumprod = torch.tensor((1, ) + max_per_digit[:-1]).cumprod(0)
        self.register_buffer('_cumprod', cumprod, persistent=False)
        self.register_buffer('_max_per_digit', torch.tensor(max_per_digit, dtype=torch.int), persistent=False)

    def __len__(self) -> int:
        return int(self.max_per_digit.prod().item())

    @property
    def num_digits(self) -> int:
        return self.max_per_digit.numel()

    @property
    def max_(self) -> torch.Tensor:
        return self.max_per_digit - 1

    @property
    def max_per_digit(self) -> torch.Tensor:
        return self.get_buffer('_max_per_digit')

    @property
    def cumprod(self) -> torch.Tensor:
        return self.get_buffer('_cumprod')


@VQITQuantizerRegistry.register_()
class FiniteScalarQuantizer(ScalarQuantizer):
    """fsq/quantizers.py:74-150.  ``quant`` is int32 (``to_decimal``'s ``.to(torch.int)``); ``memo['encode']['z']`` is the
    encode's z (fp32, with the gradient to x), which ``decode`` hands on as ``memo['decode']['z']`` and ``forward`` returns.
    Refused at construction (the reference computes NaN, divides by zero, or loses exactness): a level below 3, more than 16
    channels, a codebook larger than 2^24."""

    def __init__(self, *args, eps: float = 1e-3, num_scalars_per_channel: Iterable[int], **kwargs) -> None:
        super().__init__(*args, **kwargs)
        levels = ops.fsq_check_levels(num_scalars_per_channel)
        self._eps = eps
        self._base_converter = BaseConverter(max_per_digit=levels)
        self._consts = ops.fsq_constants(levels, eps)
        # the codebook exactly as the reference builds it (fsq/quantizers.py:94-97), once, on the host
        quant = torch.arange(self.codebook_size)
        digits = (quant[:, None] // self._base_converter.cumprod) % self._base_converter.max_per_digit
        self.register_buffer('_embeddings', digits / (self._base_converter.max_per_digit // 2) - 1)
        self.last_route = None                # what the last map entry decided (diagnostics: routes.py)

    @property
    def embedding_dim(self) -> int:
        return self._base_converter.num_digits

    @property
    def codebook_size(self) -> int:
        return len(self._base_converter)

    @property
    def embeddings(self) -> torch.Tensor:
        return self.get_buffer('_embeddings')

    @property
    def constants(self):
        """The vqhip_fsq_t the kernels receive (levels, atanh shift and scale M per channel)."""
        return self._consts

    def _encode(self, x: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        shape = x.shape
        z, quant = VF.fsq(x.reshape(-1, shape[-1]), self._consts)
        memo['z'] = z.view(shape)
        return quant.view(shape[:-1]), memo

    def _decode(self, quant: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        if 'z' in memo:
            z = memo['z']
        else:
            z = ops.fsq_decode(quant, self._consts)
        return z, memo

    def decode(self, quant: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        encode_memo = get_memo(memo, 'encode')
        decode_memo = get_memo(memo, 'decode')
        if 'z' in encode_memo:
            decode_memo['z'] = encode_memo['z']
        memo['decode'] = decode_memo
        return super().decode(quant, memo)

    # ---- the NCHW feature map without transposes (tokenization.quantize / encode_to_quant / decode_from_quant) ------------
    def map_fusable(self, x: torch.Tensor) -> bool:
        """True when ``encode_map`` takes the NCHW map ``x`` as it is (routes.map_why)."""
        return not routes.map_why(self, x)

    def _fusable(self) -> bool:
        """True when decode and loss are the plain ones (no loss configured, nothing overridden): forward_map may then return
        the z map straight from the encode."""
        return not routes.tail(self)

    def encode_map(self, x_map: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, torch.Tensor, Memo]:
        """``encode`` of the map [B, C, H, W]: (x_rows [B*H*W, C] in x's dtype, quant int32 [B*H*W], memo), one launch.
        memo['encode']['z'] is the token-major z [B*H*W, C] of the token route (no gradient: the tokens are the product here)."""
        self.last_route = routes.Route('map')
        enc = get_memo(memo, 'encode')
        quant, z, x_rows = ops.fsq_encode(x_map.detach(), self._consts, z_rows=True, want_rows=True)
        enc['z'] = z
        memo['encode'] = enc
        return x_rows, self._callbacks.after_encode(x_rows, quant, memo), memo

    def forward_map(self, x_map: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, torch.Tensor, Memo]:
        """``forward`` on the map: (z_map [B, C, H, W] fp32 NCHW-contiguous with the gradient to x_map, loss, memo) — one
        launch forward, one backward.  memo['encode']['z'] and memo['decode']['z'] are that z map, memo['x'] is the map."""
        why = routes.map_why(self, x_map, decode=True)
        assert not why, why
        self.last_route = routes.Route('map')
        enc = get_memo(memo, 'encode')
        z_map, quant = VF.fsq(x_map, self._consts)
        enc['z'] = z_map
        memo['encode'] = enc
        quant = self._callbacks.after_encode(x_map, quant, memo)
        memo.update(x=x_map, quant=quant)
        dec = get_memo(memo, 'decode')
        dec['z'] = z_map
        memo['decode'] = dec
        z_map = self._callbacks.after_decode(z_map, memo)
        loss, memo = self.loss(z_map, x_map, memo)
        return z_map, loss, memo

    def decode_map(self, quant: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        """``decode`` of an image-shaped token tensor [B, H, W] (int32 or int64) straight into the map [B, C, H, W]."""
        b, h, w = quant.shape
        return ops.fsq_decode(quant, self._consts, map_shape=(b, h, w)), memo

    def decode_pooled(self, quant: torch.Tensor, memo: Memo) -> tuple[torch.Tensor, Memo]:
        """``decode`` of tokens [B, *] (int32 or int64) followed by the mean over the positions, one launch: (features [B, C]
        fp32, memo).  Every value is the one ``ops.fsq_decode`` gives for the token, summed in the fixed order of include/vqhip.h.
        Needs the plain decode on device tokens (routes.pooled_entry)."""
        route = routes.pooled_entry(self, quant)
        assert route.name == 'pooled', route.why
        self.last_route = route
        memo['decode'] = get_memo(memo, 'decode')
        return ops.fsq_decode_pool(quant, self._consts), memo
