"""vector_quantization_amd — MI355X-native VQ codebook lookup (distance → argmin → gather/STE/loss →
codebook update) behind the quantizer API of magic-research/vector_quantization.

The arithmetic lives in libvqhip.so (hand-written HIP for gfx950, C ABI in include/vqhip.h);
this package is the thin Python host side: the reference's quantizer nn.Modules, registries and callbacks
re-expressed on top of that library.  There is no CPU fallback.
"""
from . import _lib  # noqa: F401
from .config import BuildPreHookMixin, Config, Registry, RegistryMeta
from .registries import (AnchorRegistry, InitRegistry, ModelRegistry, VQITQuantizerCallbackRegistry,
                         VQITQuantizerDistanceRegistry, VQITQuantizerLossRegistry, VQITQuantizerRegistry,
                         VQDiscriminatorLossRegistry, VQDiscriminatorRegistry, VQGeneratorLossRegistry,
                         VQDecoderRegistry, VQEncoderRegistry, VQSMSamplerRegistry, VQSMTransformerRegistry)
from .image_losses import L1Loss, MSELoss, PSNRLoss, SSIMLoss
from .distill_losses import CosineEmbeddingLoss
from .perceptual_losses import LPIPSLoss
from .discriminators import BaseDiscriminator, PatchGANDiscriminator, StyleGAN2Discriminator
from .autoencoders import BaseDecoder, BaseEncoder, VQGANDecoder, VQGANEncoder
from .vqkd_autoencoders import VQKDDecoder, VQKDEncoder
from .gan_losses import NonSaturatingLoss, R1GradientPenalty, VQGANDiscriminatorLoss, VQGANGeneratorLoss
from .sequence_losses import CausalTokenLoss, LabelSmoothingCrossEntropy, MaskedTokenLoss
from .transformers import BaseTransformer, HFTransformer, LlamaTransformer
from .kv_cache import StaticKVCache
from .utils import EMA, ema

__all__ = [
    'BuildPreHookMixin', 'Config', 'Registry', 'RegistryMeta', 'AnchorRegistry', 'InitRegistry', 'ModelRegistry',
    'VQITQuantizerCallbackRegistry', 'VQITQuantizerDistanceRegistry', 'VQITQuantizerLossRegistry',
    'VQITQuantizerRegistry', 'EMA', 'ema', 'build_quantizer', 'CausalTokenLoss', 'LabelSmoothingCrossEntropy',
    'MaskedTokenLoss', 'L1Loss', 'MSELoss', 'PSNRLoss', 'SSIMLoss', 'CosineEmbeddingLoss', 'LPIPSLoss',
    'BaseDiscriminator', 'PatchGANDiscriminator', 'StyleGAN2Discriminator', 'VQGANGeneratorLoss', 'NonSaturatingLoss',
    'VQGANDiscriminatorLoss', 'R1GradientPenalty', 'VQDiscriminatorRegistry', 'VQGeneratorLossRegistry', 'VQDiscriminatorLossRegistry',
    'BaseEncoder', 'BaseDecoder', 'VQGANEncoder', 'VQGANDecoder', 'VQKDEncoder', 'VQKDDecoder', 'VQEncoderRegistry', 'VQDecoderRegistry',
    'BaseTransformer', 'HFTransformer', 'LlamaTransformer', 'StaticKVCache', 'VQSMSamplerRegistry', 'VQSMTransformerRegistry',
]
__version__ = '0.1.0'


def build_quantizer(config, **kwargs):
    """VQITQuantizerRegistry.build(config) with this package's classes registered (the reference's
    ``custom_imports`` step, configs/vqgan/custom_imports.py:1-3)."""
    from . import quantizers  # noqa: F401  (registers the classes)
    return VQITQuantizerRegistry.build(config, **kwargs)
