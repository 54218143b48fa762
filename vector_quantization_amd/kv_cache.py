"""``StaticKVCache``: the keys and values of cached generation in memory allocated once.

transformers' ``DynamicCache`` grows by ``torch.cat``: every token re-allocates and copies the whole K and V of every layer.  Here a
layer's K and V are ``[B, Hkv, capacity, Dh]`` from the start; a step writes its position in place (``functional.decode_attention`` /
``functional.rope_append``) and the cache only counts.  The count is a host integer, and it is the authority: ``require_room`` and
``advance`` are host arithmetic.  A replayed decode step (``decode_graph.DecodeGraph``) cannot read a host integer, so a cache also
offers ``position``: one int32 on the device, created on first use and set from the host count, which
``functional.decode_attention_at`` reads and ``functional.decode_advance`` counts on the device.  The host counts one per replay
it issues, so the two agree by construction; nothing here reads the device back, and a cache that never asks for ``position`` has
none.
"""
from __future__ import annotations

import torch

__all__ = ['StaticKVCache']


class StaticKVCache:
    """K and V of ``layers`` attention layers, each ``[batch, kv_heads, capacity, head_dim]`` in ``dtype`` on ``device``.

    ``layer(i)`` gives ``(k, v, seen)``; every layer of a model step writes at ``seen`` and the step ends with ``advance(n)``."""

    def __init__(self, layers: int, batch: int, kv_heads: int, capacity: int, head_dim: int, dtype=torch.float32, device=None) -> None:
        if min(layers, batch, kv_heads, capacity, head_dim) < 1:
            raise ValueError(f'StaticKVCache: every extent must be >= 1, got layers={layers}, batch={batch}, kv_heads={kv_heads}, '
                             f'capacity={capacity}, head_dim={head_dim}')
        self._store = torch.zeros(layers, 2, batch, kv_heads, capacity, head_dim, dtype=dtype, device=device)
        self._seen = 0
        self._position = None

    @classmethod
    def for_model(cls, config, batch: int, capacity: int, dtype, device) -> 'StaticKVCache':
        """The cache of a ``LlamaConfig``-like ``config``."""
        head_dim = getattr(config, 'head_dim', None) or config.hidden_size // config.num_attention_heads
        return cls(config.num_hidden_layers, batch, config.num_key_value_heads, capacity, head_dim, dtype, device)

    layers = property(lambda self: self._store.shape[0])
    batch = property(lambda self: self._store.shape[2])
    kv_heads = property(lambda self: self._store.shape[3])
    capacity = property(lambda self: self._store.shape[4])
    head_dim = property(lambda self: self._store.shape[5])
    dtype = property(lambda self: self._store.dtype)
    device = property(lambda self: self._store.device)

    def get_seq_length(self, layer: int = 0) -> int:
        return self._seen

    def layer(self, i: int):
        """``(k, v, seen)`` of layer ``i``: the two ``[B, Hkv, capacity, Dh]`` views and the positions already stored."""
        return self._store[i, 0], self._store[i, 1], self._seen

    def require_room(self, n: int) -> None:
        """Raises where ``n`` more positions do not fit: before anything is launched."""
        if n < 1 or self._seen + n > self.capacity:
            raise ValueError(f'StaticKVCache: {n} tokens behind {self._seen} do not fit a capacity of {self.capacity}')

    def advance(self, n: int) -> int:
        """Counts ``n`` more positions as stored (once per model step, after its layers): host arithmetic only."""
        self.require_room(n)
        self._seen += n
        return self._seen

    @property
    def position(self) -> torch.Tensor:
        """The count as one int32 on the cache's device, for the steps that read it there.  Created on first use from the host
        count; after host-side steps (a prompt through ``rope_append``, ``reset``) ``sync_position`` sets it again."""
        if self._position is None:
            self._position = torch.full((1,), self._seen, dtype=torch.int32, device=self.device)
        return self._position

    def sync_position(self) -> torch.Tensor:
        """Sets the device position from the host count (one fill on the current stream) and returns it."""
        return self.position.fill_(self._seen)

    def reset(self) -> None:
        self._seen = 0
        if self._position is not None:
            self._position.zero_()
