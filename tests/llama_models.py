"""The tiny LlamaTransformer of the CPU and GPU tests (2 layers, hidden 64, 4 heads, intermediate 176, vocabulary 48, a randomised
lm_head - init_weights leaves it zero, which would make every logit 0) and its float64 model.

transformers' ``LlamaRMSNorm`` computes in fp32 whatever the input dtype, so ``model.double()`` alone still rounds every norm to
fp32 - an error of the size the tests measure.  ``exact64`` therefore also replaces each norm by ``RMSNorm64``: the same lines
without the cast."""
import copy

import torch
from torch import nn

from vector_quantization_amd.registries import VQSMTransformerRegistry

TINY = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=4, intermediate_size=176, rms_norm_eps=1e-5)
VOCABULARY = 48


def build_tiny(seed: int = 0, fused: bool = True, **extra):
    """The reference's config dict through the registry and ``init_weights``, then a randomised lm_head (logits of order 1)."""
    torch.manual_seed(seed)
    m = VQSMTransformerRegistry.build(dict(type='LlamaTransformer', transformer=dict(TINY, **extra), vocabulary_size=VOCABULARY,
                                           sampler=dict(type='BaseSampler'), fused=fused))
    m.init_weights(None)
    head = m._transformer.lm_head.weight
    with torch.no_grad():
        head.copy_(torch.randn(head.shape, generator=torch.Generator().manual_seed(seed + 1)) * head.shape[1] ** -0.5)
    return m.eval()


class RMSNorm64(nn.Module):
    """``LlamaRMSNorm.forward`` without ``hidden_states.to(torch.float32)``: float64 stays float64."""

    def __init__(self, norm) -> None:
        super().__init__()
        self.weight = norm.weight
        self.variance_epsilon = norm.variance_epsilon

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        variance = hidden_states.pow(2).mean(-1, keepdim=True)
        hidden_states = hidden_states * torch.rsqrt(variance + self.variance_epsilon)
        return self.weight * hidden_states


def exact64(m):
    """A float64 copy of ``m`` on the CPU whose norms compute in float64; the parameters keep their names and order."""
    m = copy.deepcopy(m).cpu().double()
    model = m._transformer.model
    for layer in model.layers:
        layer.input_layernorm = RMSNorm64(layer.input_layernorm)
        layer.post_attention_layernorm = RMSNorm64(layer.post_attention_layernorm)
    model.norm = RMSNorm64(model.norm)
    return m
