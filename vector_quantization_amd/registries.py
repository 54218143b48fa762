"""Registry hierarchy of the quantizer path, same names as the reference
(vq/registries.py:18-35, vq/tasks/image_tokenization/registries.py:11-16, .../runners/registries.py:11-16,
vq/tasks/image_tokenization/models/registries.py, vq/models/registries.py:12-20, vq/tasks/image_reconstruction/registries.py:16,
vq/runners/registries.py:15, vq/algorithms/vqgan/registries.py:8, vq/algorithms/vqgan/losses/registries.py:9-14,
.../quantizers/registries.py:9-14, vq/algorithms/vq/distances.py:19-20, vq/algorithms/cvqvae/registries.py:8)."""
from .config import Registry


class ModelRegistry(Registry):
    """Stands in for todd.registries.ModelRegistry (resolves 'torch_nn_modules_sparse_Embedding')."""


class InitRegistry(Registry):
    """Stands in for todd.registries.InitRegistry: weight initialisers by name.  Any in-place initialiser of ``torch.nn.init``
    resolves by its own name — ``dict(type='trunc_normal_', std=0.02)``, ``dict(type='xavier_uniform_')`` ... — as a factory
    ``(**kwargs) -> (tensor -> tensor)``, what the generic branch of the reference hands to ``InitRegistry.build(config)``
    (vq/algorithms/vq/quantizers.py:87-90); explicitly registered names take precedence."""

    @classmethod
    def resolve(cls, type_):
        if isinstance(type_, str):
            key = type_.rsplit('.', 1)[-1]
            if cls._lookup(key) is None:
                from torch.nn import init
                fn = getattr(init, key, None)
                if callable(fn) and key.endswith('_') and not key.startswith('_'):
                    return lambda **kwargs: (lambda w: fn(w, **kwargs))
        return super().resolve(type_)


class VQRegistry(Registry):
    pass


class VQModelRegistry(VQRegistry, ModelRegistry):
    pass


class VQITQuantizerRegistry(VQModelRegistry):
    pass


class VQITConnectorRegistry(VQModelRegistry):
    pass


class VQITQuantizerDistanceRegistry(VQITQuantizerRegistry):
    pass


class VQITQuantizerCallbackRegistry(VQITQuantizerRegistry):
    pass


class VQITQuantizerLossRegistry(VQITQuantizerRegistry):
    pass


class VQLossRegistry(VQRegistry):
    pass


class VQIRLossRegistry(VQModelRegistry, VQLossRegistry):
    """The losses of image reconstruction (vq/tasks/image_reconstruction/losses.py): image_losses.py."""


class VQEncoderRegistry(VQModelRegistry):
    """The encoders of a tokenizer (vq/models/registries.py:12): autoencoders.py."""


class VQDecoderRegistry(VQModelRegistry):
    """The decoders of a tokenizer (vq/models/registries.py:16): autoencoders.py."""


class VQDiscriminatorRegistry(VQModelRegistry):
    """The discriminators of a VQGAN (vq/algorithms/vqgan/discriminators/): discriminators.py."""


class VQGeneratorLossRegistry(VQLossRegistry):
    """The adversarial losses of the generator step (vq/algorithms/vqgan/losses/generator.py): gan_losses.py."""


class VQDiscriminatorLossRegistry(VQLossRegistry):
    """The losses of the discriminator step (vq/algorithms/vqgan/losses/discriminator.py): gan_losses.py."""


class VQSMSamplerRegistry(VQModelRegistry):
    """The samplers of stage-2 generation (vq/tasks/sequence_modeling/models/registries.py:21-34).  As there, a ``cfg`` key in a
    sampler's config wraps the built sampler: ``dict(type='TopKTopPSampler', cfg=1.75)`` is ``CFGSampler(sampler=..., alpha=1.75)``
    (configs/ar/cfg.py)."""

    @classmethod
    def build(cls, config, **kwargs):
        config = dict(config)
        config.update(kwargs)
        cfg = config.pop('cfg', None)
        sampler = type(cls).build(cls, config)                                   # RegistryMeta.build: the plain lookup and pre-hook
        if cfg is not None:
            from .samplers import CFGSampler
            sampler = CFGSampler(sampler=sampler, alpha=cfg)
        return sampler


class VQSMTransformerRegistry(VQModelRegistry):
    """The transformers of stage 2 (vq/tasks/sequence_modeling/models/registries.py:17): transformers.py."""


class AnchorRegistry(Registry):
    pass


class RunnerRegistry(Registry):
    """Stands in for todd.registries.RunnerRegistry."""


class VQRunnerRegistry(VQRegistry, RunnerRegistry):
    pass


class VQITRunnerRegistry(VQRunnerRegistry):
    pass


class VQITCallbackRegistry(VQITRunnerRegistry):
    pass


class VQMetricRegistry(VQRegistry):
    """vq/runners/registries.py:15 (there also under todd's MetricRegistry)."""


class VQITMetricRegistry(VQITRunnerRegistry, VQMetricRegistry):
    pass
