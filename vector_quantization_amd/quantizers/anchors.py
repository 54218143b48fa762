"""CVQ-VAE anchor samplers — mirror of vq/algorithms/cvqvae/anchors.py:23-166."""
from __future__ import annotations

import random
from abc import ABC, abstractmethod
from typing import Mapping

import torch
import torch.distributed as dist
from torch import nn

from .. import ops
from ..config import Config
from ..registries import AnchorRegistry
from ..utils import Store, all_gather, all_reduce_sum, get_world_size, is_sync
from .memo import Memo
from .distances import LazyDistance, as_distance_tensor


class BaseAnchor(nn.Module, ABC):

    def __init__(self, *args, sync: bool = False, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._sync = sync

    @abstractmethod
    def _anchors(self, x, e, d, quant, p, memo: Memo) -> tuple[torch.Tensor, Memo]:
        pass

    def _gather(self, x, e, d, quant, p):
        """sync=True (anchors.py:50-57).  The reference all-gathers the [N, K] matrix; here only the latents travel
        and the matrix-dependent samplers rebuild what they need from the gathered rows."""
        x = torch.cat(all_gather(x))
        if Store.DRY_RUN:
            assert is_sync(e)
        quant = torch.cat(all_gather(quant))
        p = torch.stack(all_gather(p)).mean(0)
        if isinstance(d, LazyDistance):
            d = LazyDistance(d._distance, x, e)
        else:
            d = torch.cat(all_gather(d))
        return x, d, quant, p

    def forward(self, x, e, d, quant, p, memo: Memo | None = None) -> tuple[torch.Tensor, Memo]:
        if self._sync and get_world_size() > 1:
            x, d, quant, p = self._gather(x, e, d, quant, p)
        if memo is None:
            memo = Config()
        anchors, memo = self._anchors(x, e, d, quant, p, memo)
        if self._sync:
            if Store.DRY_RUN:
                assert is_sync(anchors)
        elif get_world_size() > 1:
            all_reduce_sum(anchors)
            anchors /= get_world_size()
        return anchors, memo


@AnchorRegistry.register_()
class NearestAnchor(BaseAnchor):
    """anchors[k] = x[argmin_n d[n, k]] — fused column argmin, the matrix is never formed."""

    def _anchors(self, x, e, d, quant, p, memo: Memo):
        indices = d.argmin(0)                   # LazyDistance.argmin(0) → vqhip_col_argmin; a tensor → torch
        anchors = ops.gather_rows(x, indices)
        return anchors, memo


@AnchorRegistry.register_()
class MultinomialAnchor(BaseAnchor):
    """One latent per code drawn from softmax over the code's column of distances (anchors.py:88-104; the reference softmaxes +d:
    farther latents are likelier, reproduced here).  No shipped config uses it.

    Fused route: while ``d`` is an unmaterialised ``LazyDistance`` of metric 'L2' or 'Cosine' on a GPU, ``u = torch.rand(K)`` is
    ONE draw from the device generator and the indices come from ``d.multinomial(u)`` — HIP kernels on one bounded [R, K]
    row-block tile (64 MiB by default), an inverse-CDF walk down each column on exact fixed-point masses (include/vqhip.h,
    vqhip_col_multinomial_*); the matrix, its transposed softmax and the [K, N] multinomial are never formed and the handle stays
    unmaterialised.  With ``sync=True`` on several ranks rank 0's ``u`` is broadcast, so every rank draws the same
    rows of the gathered latents by construction (the reference relies on equal seeds for its ``is_sync`` assert).
    Matrix route (the reference's composition, literally): ``probabilities(d).multinomial(1)`` on the materialised matrix.
    ``routes.multinomial_anchor_why`` decides and says why; ``last_route`` holds the decision of the last call.

    Stated differences of the fused route: (1) a seeded run picks DIFFERENT rows than the matrix route — it consumes K uniforms
    where ``multinomial`` consumes its own stream; the distribution is the same (to VQHIP_SAMPLE_DELTA(N) per cumulative share);
    (2) a code whose column holds a NaN or a +inf keeps its own ``e[k]`` as its anchor, so the update leaves it where it is —
    the reference's multinomial raises a device assert there.

    ``fused`` (extension; configs need not name it): None (default) — the fused route wherever it applies; False — always
    the matrix route."""

    def __init__(self, *args, fused: bool | None = None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        if fused not in (None, False):
            raise ValueError(f'MultinomialAnchor: fused must be None (auto) or False, got {fused!r}')
        self._fused = fused
        self.last_route = None

    @staticmethod
    def probabilities(d) -> torch.Tensor:
        return as_distance_tensor(d).detach().t().softmax(1)             # [K, N]

    def _uniforms(self, K: int, device) -> torch.Tensor:
        u = torch.rand(K, device=device)
        if self._sync and get_world_size() > 1:
            dist.broadcast(u, 0)
        return u

    def _anchors(self, x, e, d, quant, p, memo: Memo):
        from . import routes
        self.last_route = routes.multinomial_anchor_why(self, d, x)
        if self.last_route.name != 'fused':
            indices = self.probabilities(d).multinomial(1).reshape(-1)
            return ops.gather_rows(x, indices), memo
        indices = d.multinomial(self._uniforms(e.shape[0], x.device))
        anchors = ops.gather_rows(x, indices.clamp_min(0))
        return torch.where((indices < 0).unsqueeze(1), e.detach().to(anchors.dtype), anchors), memo


@AnchorRegistry.register_()
class CachedAnchor(BaseAnchor):
    """K anchors drawn without replacement from a pool of candidate rows: this step's latents, topped up — when the
    batch is smaller than the codebook — with the anchors of the previous step (the ``_cache`` buffer) and, if that is
    still not enough, with uniform noise (vq/algorithms/cvqvae/anchors.py:107-166; no shipped config uses it).
    The draw itself uses the host-side generators the reference uses (``random.sample`` when the pool is larger than
    the codebook, the CPU ``torch.randperm`` otherwise), so a seeded run selects the same rows as the reference on any
    device; only the noise rows come from the device generator."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.register_buffer('_cache', torch.empty(0))

    @property
    def cache(self) -> torch.Tensor:
        return self.get_buffer('_cache')

    def _load_from_state_dict(self, state_dict: Mapping[str, torch.Tensor], prefix: str, *args, **kwargs) -> None:
        saved = state_dict.get(prefix + '_cache')
        if saved is not None:
            self.cache.resize_(saved.shape)          # the buffer starts empty: give it the checkpoint's shape first
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _pool(self, x: torch.Tensor, K: int) -> torch.Tensor:
        pool = x.float()
        if pool.shape[0] < K and self.cache.numel() > 0:
            pool = torch.cat([pool, self.cache.to(pool.device)])
        return pool

    @staticmethod
    def _draw(rows: int, K: int) -> torch.Tensor:
        if rows > K:
            return torch.as_tensor(random.sample(range(rows), K))
        return torch.randperm(K)                      # indices >= rows select the noise rows appended below

    def _anchors(self, x, e, d, quant, p, memo: Memo):
        K = e.shape[0]
        pool = self._pool(x, K)
        picks = self._draw(pool.shape[0], K)
        short = K - pool.shape[0]
        if short > 0:
            pool = torch.cat([pool, torch.rand(short, pool.shape[1], device=pool.device)])
        return ops.gather_rows(pool, picks.to(pool.device)), memo

    def forward(self, *args, **kwargs):
        anchors, memo = super().forward(*args, **kwargs)
        self.register_buffer('_cache', anchors.detach())
        return anchors, memo
