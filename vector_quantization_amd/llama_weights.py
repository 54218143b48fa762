"""``LlamaWeights``: the matrices the walk of ``LlamaTransformer`` multiplies by, under one owner - per layer the packed q/k/v rows,
the packed gate/up rows, ``o_proj`` and ``down_proj``, and the one ``lm_head``.  The order of the packed rows is written here and
nowhere else.  Every route of ``transformers.py`` and the captured step of ``decode_graph.py`` ask this object for a weight."""
from __future__ import annotations

import torch

# entry -> (the layer's submodule, its projections in the order of the entry's rows)
ENTRIES = {'qkv': ('self_attn', ('q_proj', 'k_proj', 'v_proj')), 'gate_up': ('mlp', ('gate_proj', 'up_proj')),
           'o': ('self_attn', ('o_proj',)), 'down': ('mlp', ('down_proj',))}


def layers(module):
    """The decoder layers the walk of ``module`` (a ``LlamaTransformer``) runs."""
    lm = module._transformer
    return lm.model.layers[:lm.config.num_hidden_layers]


class LlamaWeights:
    """``weights(name, i)`` is entry ``name`` (``qkv``, ``gate_up``, ``o``, ``down``) of layer ``i``, ``weights('lm_head')`` the head.

    An entry that is not held is built when it is asked for, from the parameters as they are then and inside autograd: the module's
    own parameter where it is one projection, ``torch.cat`` of its projections, cast to ``dtype`` unless that is None, where it is
    several.  That alone serves the fused route, whose gradients reach ``gate_proj`` and ``up_proj`` through the ``cat``.
    ``pack()`` builds every entry once and holds it (the eager decode route); ``allocate(device)`` holds memory of its own for every
    entry that is not a parameter read in place - the packed ones, and under a ``dtype`` the single ones as well - which
    ``refresh()`` fills in place, so the addresses a captured graph reads stay."""

    def __init__(self, module, dtype=None) -> None:
        self.module, self.dtype, self.layers, self.held = module, dtype, layers(module), {}

    def entries(self) -> list:
        """``(name, i)`` of every entry: layer by layer, ``lm_head`` last."""
        return [(name, i) for i in range(len(self.layers)) for name in ENTRIES] + [('lm_head', None)]

    def parts(self, name: str, i=None) -> tuple:
        """The parameters entry ``name`` of layer ``i`` is made of, in the order of its rows."""
        if name == 'lm_head':
            return (self.module._transformer.lm_head.weight,)
        owner, projections = ENTRIES[name]
        return tuple(getattr(getattr(self.layers[i], owner), p).weight for p in projections)

    def __call__(self, name: str, i=None) -> torch.Tensor:
        held = self.held.get((name, i))
        if held is not None:
            return held
        parts = self.parts(name, i)
        if len(parts) == 1:
            return parts[0]
        packed = torch.cat(parts)
        return packed if self.dtype is None else packed.to(self.dtype)

    def pack(self) -> 'LlamaWeights':
        for key in self.entries():
            self.held[key] = self(*key)
        return self

    def allocate(self, device) -> 'LlamaWeights':
        for key in self.entries():
            parts = self.parts(*key)
            if len(parts) > 1 or self.dtype is not None:
                self.held[key] = torch.empty(sum(p.shape[0] for p in parts), parts[0].shape[1], dtype=self.dtype or parts[0].dtype,
                                             device=device)
        return self

    @torch.no_grad()
    def refresh(self) -> None:
        """What ``allocate`` holds, from the module's parameters as they are now."""
        for key, buffer in self.held.items():
            at = 0
            for part in self.parts(*key):
                buffer[at:at + part.shape[0]].copy_(part)
                at += part.shape[0]
