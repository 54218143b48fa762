"""The runner-level callers of the path, same names and behaviour as the reference's

* ``Tokenizer``            vq/tasks/image_tokenization/runners/tokenizer.py:21-55 — the validator whose iteration is
                           ``model.encode_to_quant(image, memo)``;
* ``TokenizeCallback``     runners/callbacks.py:29-53 — ``tokens/{iter}_{rank}.pth`` = Tokens(id_, category, tokens[b, h, w]);
* ``LlamaGenTokenizeCallback``  tools/tokenize_llamagen.py:65-103 (there also called TokenizeCallback, registered with
                           ``force=True``) — ten-crop codes / labels as ``{i}.npy``;
* ``CodebookUsageMetric`` / ``CodebookPPLMetric``   runners/metrics.py:25-73 — bincount per iteration, one all-reduce at
                           summary time;
* ``ImageLossMetric``      vq/runners/metrics/loss.py:21-37 — L1 / MSE / PSNR / SSIM of ``pred_image`` against ``image``, all
                           four from one launch pair per batch (``vqhip_image_metrics``).

The reference builds these through todd's runner machinery (dataset / dataloader / strategy / logging builders, ETA,
checkpoints).  That machinery is control plane and out of scope; what is here is the protocol those four classes live in —
``bind(runner)``, ``before_run_iter`` / ``after_run_iter(batch, memo)``, ``forward(batch, memo)``, ``summary(memo)`` — and a
``Tokenizer.run`` loop that drives it over any iterable of batches.  The histogram and the two summaries run on the device
(``vqhip_hist``, ``vqhip_codebook_metrics``); the encoder in front of the quantizer is whatever callable the model holds.
"""
from __future__ import annotations

import pathlib
import re
import types
from typing import Any, Callable, Iterable, Mapping, Optional

import torch
import torch.distributed as dist
from torch import nn

from . import ops, tokenization
from . import image_losses
from .config import BuildPreHookMixin
from .registries import VQITCallbackRegistry, VQITMetricRegistry, VQITRunnerRegistry, VQLossRegistry, VQMetricRegistry
from .tokenization import Tokens
from .utils import get_rank, get_world_size

__all__ = ['Tokenizer', 'TokenizerModel', 'TokenizeCallback', 'LlamaGenTokenizeCallback', 'Tokens', 'CodebookMixin',
           'CodebookUsageMetric', 'CodebookPPLMetric', 'BaseCallback', 'BaseMetric', 'get_', 'ImageLossMetric', 'ImageRangeMixin']

_STEP = re.compile(r'''\[\s*(?:"([^"]*)"|'([^']*)'|(-?\d+))\s*\]|\.([A-Za-z_]\w*)''')


def get_(obj: Any, attr: str) -> Any:
    """todd's accessor strings as the configs write them — ``'["quantizer"]["quant"]'`` (configs/vqgan/runner.py:123),
    ``'["ir"]["encode_to_quant"]["quantizer"]["quant"]'`` (configs/ar/runner.py:116) — walked without ``eval``."""
    pos = 0
    for m in _STEP.finditer(attr):
        if m.start() != pos:
            break
        pos = m.end()
        dq, sq, num, name = m.groups()
        if name is not None:
            obj = getattr(obj, name)
        elif num is not None:
            obj = obj[int(num)]
        else:
            obj = obj[dq if dq is not None else sq]
    if pos != len(attr):
        raise ValueError(f'unsupported accessor {attr!r}')
    return obj


class _RunnerHolder:
    def __init__(self, *args, **kwargs) -> None:
        super().__init__()
        self._runner = None

    def bind(self, runner) -> None:
        self._runner = runner

    @property
    def runner(self):
        assert self._runner is not None, f'{type(self).__name__} is not bound to a runner'
        return self._runner


class BaseCallback(_RunnerHolder):
    def before_run_iter(self, batch: Mapping, memo: dict) -> None:
        pass

    def after_run_iter(self, batch: Mapping, memo: dict) -> None:
        pass


class BaseMetric(_RunnerHolder):
    def forward(self, batch: Mapping, memo: dict) -> dict:
        raise NotImplementedError

    def summary(self, memo: dict) -> float:
        raise NotImplementedError


# ---- token files ------------------------------------------------------------------------------------------------------

@VQITCallbackRegistry.register_()
class TokenizeCallback(BaseCallback):
    """runners/callbacks.py:29-53."""

    @property
    def token_dir(self) -> pathlib.Path:
        return pathlib.Path(self.runner.work_dir) / 'tokens'

    def bind(self, *args, **kwargs) -> None:
        super().bind(*args, **kwargs)
        self.token_dir.mkdir(parents=True, exist_ok=True)

    def after_run_iter(self, batch: Mapping, memo: dict) -> None:
        super().after_run_iter(batch, memo)
        quantizer_memo = memo['quantizer']
        tokenization.save_tokens(self.runner.work_dir, self.runner.iter_, batch['id_'], batch['category'],
                                 quantizer_memo['quant'], quantizer_memo['x_shape'])


@VQITCallbackRegistry.register_()
class LlamaGenTokenizeCallback(BaseCallback):
    """tools/tokenize_llamagen.py:65-103: batches are ONE image of ten crops (``[1, 10, C, H, W]``, squeezed before the
    iteration); ``llamagen_tokens/imagenet{S}_codes/{i}.npy`` int64 ``[1, 10, h*w]`` and ``…_labels/{i}.npy``,
    ``i = (iter - 1) * world_size + rank``."""

    @property
    def token_dir(self) -> pathlib.Path:
        return pathlib.Path(self.runner.work_dir) / 'llamagen_tokens'

    @property
    def code_dir(self) -> pathlib.Path:
        return self.token_dir / f'imagenet{self.runner.dataset.image_size}_codes'

    @property
    def label_dir(self) -> pathlib.Path:
        return self.token_dir / f'imagenet{self.runner.dataset.image_size}_labels'

    def bind(self, *args, **kwargs) -> None:
        super().bind(*args, **kwargs)
        self.code_dir.mkdir(parents=True, exist_ok=True)
        self.label_dir.mkdir(parents=True, exist_ok=True)

    def before_run_iter(self, batch, memo: dict) -> None:
        batch['original_image'] = batch['original_image'].squeeze(0)
        batch['image'] = batch['image'].squeeze(0)
        return super().before_run_iter(batch, memo)

    def after_run_iter(self, batch: Mapping, memo: dict) -> None:
        tokenization.save_llamagen(self.runner.work_dir, self.runner.dataset.image_size, self.runner.iter_,
                                   memo['quantizer']['quant'], batch['category'])


# ---- codebook metrics ---------------------------------------------------------------------------------------------------

class CodebookMixin(BaseMetric):
    """runners/metrics.py:25-56.  ``forward`` counts the tokens the accessor points at with one ``vqhip_hist`` launch
    (block-private LDS bins; int64 running totals like the reference's ``bincount``).  Device tokens only: like every
    other entry of this package there is no CPU path (``ops`` raises on a CPU tensor) — the reference's metric also runs
    on CPU tokens.  The summaries are evaluated in float64 on the device (``vqhip_codebook_metrics``) where the reference
    goes through fp32 ``Categorical.entropy``: equal to ~1e-6 relative, not bitwise (tests/test_runners.py)."""

    def __init__(self, *args, quant: str, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._quant = quant
        self._counts: Any = 0

    def bind(self, *args, **kwargs) -> None:
        super().bind(*args, **kwargs)
        self._codebook_size = self.runner.strategy.module.quantizer.codebook_size

    def forward(self, batch: Mapping, memo: dict) -> dict:
        quant: torch.Tensor = get_(memo, self._quant).flatten()
        counts = ops.hist(quant, self._codebook_size).to(torch.int64)
        self._counts = self._counts + counts
        return memo

    def _summary(self, memo: dict, counts: torch.Tensor) -> float:
        raise NotImplementedError

    def summary(self, memo: dict) -> float:
        if isinstance(self._counts, int):
            return 0.
        counts = self._counts.clone()
        if get_world_size() > 1:
            dist.all_reduce(counts)
        return self._summary(memo, counts)


@VQITMetricRegistry.register_()
class CodebookUsageMetric(CodebookMixin):
    """runners/metrics.py:59-63: codes used / K."""

    def _summary(self, memo: dict, counts: torch.Tensor) -> float:
        return float(ops.codebook_metrics(counts)[0].item())


@VQITMetricRegistry.register_()
class CodebookPPLMetric(CodebookMixin):
    """runners/metrics.py:66-73: entropy (nats) of the code histogram — the number docs/pretrained_models.md quotes as PPL."""

    def _summary(self, memo: dict, counts: torch.Tensor) -> float:
        return float(ops.codebook_metrics(counts)[1].item())


# ---- reconstruction metrics ---------------------------------------------------------------------------------------------------

class ImageRangeMixin:
    """The image range the model sees, [-1, 1], back to bytes: what ``vqhip_image_metrics`` does inside its launch, bit for bit.
    ``image_range_decode = True`` on a dataset (class or instance) declares its own ``decode`` to be this expression."""

    image_range_decode = True

    @staticmethod
    def decode(images: torch.Tensor) -> torch.Tensor:
        return ((images + 1) * 127.5).clamp(0, 255).to(torch.uint8)


def _tensor_key(*tensors: torch.Tensor) -> tuple:
    return tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype) for t in tensors)


@VQMetricRegistry.register_()
class ImageLossMetric(BuildPreHookMixin, BaseMetric):
    """vq/runners/metrics/loss.py:21-37: ``loss(dataset.decode(pred_image) / 255, dataset.decode(image) / 255)`` averaged per
    image, with ``pred_image`` / ``image`` accessor strings into the memo and ``loss`` a config of ``VQIRLossRegistry``.

    When the loss is one of the four plain classes of ``image_losses``, the RAW model-range images go to ``ops.image_metrics``,
    which decodes them as ``ImageRangeMixin.decode`` does, bit for bit, and yields all four values.  The result is kept in the
    iteration's memo under ``'image_metrics'``, keyed by the two tensors' ``data_ptr``, ``_version``, shape and dtype, so the
    four metric entries of the shipped configs cost ONE launch pair per batch.  Every entry holds the tensors it was made
    from, so an address in a key cannot be handed to another tensor while the memo lives.

    Which decode: without a runner, or with a dataset that has no ``decode``, the kernel's.  A dataset's ``decode`` stands for
    the kernel's only where that is DECLARED - ``image_range_decode = True`` on the dataset (``ImageRangeMixin`` has it) or as
    this metric's argument - because a function cannot be compared by what it computes: the reference's own dataset class
    (vq/datasets/base.py:70-73) is the same expression, but undeclared it is treated like any other and ASKED to decode.
    Then the dataset's uint8 result goes to the kernel (still fused, one decode of each image and one launch pair per batch
    for all four metrics: the decoded pair is kept in the memo, keyed by the raw tensors and the decode function), at the
    price of those two torch decodes.  A loss whose class overrides ``forward``, or is none of the four, runs as written on
    ``decode(v) / 255`` (route ``torch``, as for CPU tensors); ``last_route`` tells which.

    Per-image values are accumulated on the device in float64; ``summary()`` is their mean over everything THIS rank saw.
    todd's LossMetric, which owns the reference's accumulation and its cross-rank behaviour, is not in the reference tree and
    is not rebuilt: no collective is issued here."""

    last_route = None

    def __init__(self, *args, pred_image: str, image: str, loss, image_range_decode: Optional[bool] = None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._inputs = dict(pred_image=pred_image, image=image)
        self._loss = loss
        self._image_range_decode = image_range_decode
        self._sum: Any = 0.0
        self._count = 0
        self.last: Optional[torch.Tensor] = None                                  # the per-image values of the last batch

    @classmethod
    def build_pre_hook(cls, config, registry, item):
        config = super().build_pre_hook(config, registry, item)
        config.loss = VQLossRegistry.build_or_return(config.loss, reduction='none')
        return config

    def _decode(self):
        """(decode, own): the dataset's decode where the runner has one, and whether the kernel's decode stands for it."""
        dataset = getattr(self._runner, 'dataset', None) if self._runner is not None else None
        decode = getattr(dataset, 'decode', None)
        if decode is None:
            return ImageRangeMixin.decode, True
        declared = self._image_range_decode
        return decode, bool(getattr(dataset, 'image_range_decode', False) if declared is None else declared)

    @staticmethod
    def _decoded(memo: dict, decode, pred: torch.Tensor, image: torch.Tensor):
        """``decode`` of both images, once per (raw pair, decode function) and memo."""
        cache = memo.setdefault('image_metrics', {})
        fn = getattr(decode, '__func__', decode)                                  # (a bound method is a new object per access)
        key = ('decoded', fn, getattr(decode, '__self__', None)) + _tensor_key(pred, image)
        if key not in cache:
            cache[key] = dict(raw=(pred, image), decoded=(decode(pred), decode(image)))
        return cache[key]['decoded']

    def _forward(self, batch: Mapping, memo: dict):
        from .quantizers import routes
        pred, image = (get_(memo, v) for v in self._inputs.values())
        decode, own = self._decode()
        column = image_losses.column_of(self._loss)
        decoded = image_losses.is_plain(self._loss) and not own
        if decoded:                                                               # the dataset's own bytes go to the kernel
            pred, image = self._decoded(memo, decode, pred, image)
        # all four values from one call where SSIM fits; without it where only its clauses refuse and this metric is another
        ssim = True
        route = routes.image_metrics_why(pred, image, ssim=True, loss=self._loss)
        if route.name != 'fused' and column != 'ssim':
            without = routes.image_metrics_why(pred, image, ssim=False, loss=self._loss)
            if without.name == 'fused':
                ssim, route = False, without
        self.last_route = route
        if route.name != 'fused':
            if not decoded:
                pred, image = decode(pred), decode(image)
            loss = self._loss(pred / 255, image / 255)
            return loss.reshape(loss.shape[0], -1).mean(dim=1), memo
        cache = memo.setdefault('image_metrics', {})
        key = ('values', ssim) + _tensor_key(pred, image)
        if key not in cache:
            cache[key] = dict(inputs=(pred, image), **ops.image_metrics(pred, image, ssim=ssim))
        return cache[key][column], memo

    def forward(self, batch: Mapping, memo: dict) -> dict:
        loss, memo = self._forward(batch, memo)
        self.last = loss
        self._sum = self._sum + loss.detach().double().sum()
        self._count += loss.numel()
        return memo

    def summary(self, memo: dict) -> float:
        return float(self._sum / self._count) if self._count else 0.


# ---- the model the runner drives, and the runner ----------------------------------------------------------------------------

class TokenizerModel(nn.Module):
    """What ``Tokenizer._run_iter`` needs of the reference's BaseModel (models/base.py:29-146): ``encode_to_quant`` and the
    ``quantizer`` property.  ``encoder`` is any callable image -> latent map ``[b, c, h, w]`` (the reference's encoder +
    post_encode connector; identity when the batches already hold latents)."""

    def __init__(self, quantizer: nn.Module, encoder: Optional[Callable[[torch.Tensor], torch.Tensor]] = None) -> None:
        super().__init__()
        self._quantizer = quantizer
        self._encoder = encoder

    @property
    def quantizer(self) -> nn.Module:
        return self._quantizer

    def encode(self, image: torch.Tensor, memo: dict):
        return (image if self._encoder is None else self._encoder(image)), memo

    def encode_to_quant(self, image: torch.Tensor, memo: dict):
        x, memo = self.encode(image, memo)
        return tokenization.encode_to_quant(self._quantizer, x, memo)


@VQITRunnerRegistry.register_()
class Tokenizer:
    """runners/tokenizer.py:21-55.  ``run()`` is the validator loop reduced to what the four classes above observe:
    ``iter_`` counts from 1, callbacks see ``before_run_iter`` / ``after_run_iter``, metrics see ``forward`` per batch and
    ``summary`` once."""

    def __init__(self, *args, model: nn.Module, dataloader: Iterable[Mapping], work_dir, callbacks: Iterable[BaseCallback] = (),
                 metrics: Optional[Mapping[str, BaseMetric]] = None, dataset: Any = None, **kwargs) -> None:
        self.strategy = types.SimpleNamespace(module=model)
        self.dataloader = dataloader
        self.dataset = dataset if dataset is not None else getattr(dataloader, 'dataset', None)
        self.work_dir = pathlib.Path(work_dir)
        self.iter_ = 0
        self.callbacks = list(callbacks)
        self.metrics = dict(metrics or {})
        for holder in (*self.callbacks, *self.metrics.values()):
            holder.bind(self)

    def _run_iter(self, batch: Mapping, memo: dict, *args, **kwargs) -> dict:
        model = self.strategy.module
        original_image = batch['original_image']
        image = batch['image']
        if torch.cuda.is_available():
            original_image = original_image.cuda()
            image = image.cuda()
        memo.update(original_image=original_image, image=image)
        _, memo = model.encode_to_quant(image, memo)
        return memo

    @torch.no_grad()
    def run(self) -> dict:
        memo: dict = {}
        for batch in self.dataloader:
            self.iter_ += 1
            memo = {}
            for c in self.callbacks:
                c.before_run_iter(batch, memo)
            memo = self._run_iter(batch, memo)
            for m in self.metrics.values():
                memo = m.forward(batch, memo)
            for c in self.callbacks:
                c.after_run_iter(batch, memo)
        return {name: m.summary(memo) for name, m in self.metrics.items()}
