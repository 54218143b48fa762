"""One library call per training forward (include/vqhip.h: vqhip_cvq_forward, vqhip_vqkd_forward).

The reference's training step runs the quantizer forward as ~20 ATen calls; re-hosted call for call on libvqhip an eager
nn.Module step still makes ~10 host calls, and at the reference's per-rank batches (3 072 - 12 544 tokens) the HOST is the
bound (profiles/r05_train_shapes_before.txt: the host has issued a step exactly when the GPU has finished it).  Here the
whole forward of the two callback-driven training configs is enqueued by ONE call:

  CVQ-VAE (vq/algorithms/cvqvae/quantizer_callback.py:75-105): encode -> listed codes -> column argmin -> [pack ->
      all-reduce] -> apply -> prefetch of the next step's list -> decode / straight-through / loss
  VQ-KD   (vq/algorithms/vqkd/quantizers/callbacks.py:114-129): normalise codebook (twice) and latents -> encode ->
      histogram + centroid sums into the packed buffer -> [all-reduce] -> EMA update -> decode / STE / normalised MSE

Values are those of the chain of separate calls (the library makes the same launches in the same order).  This module owns
the persistent device buffers such a call needs (the list of codes, the pinned count word and its event, the arena) and the
argument blocks; the callbacks decide WHEN the fused form applies and keep the reference's memo side effects."""
from __future__ import annotations

import ctypes
import os
import time
from typing import Optional

import torch

from . import _lib, ops
from ._lib import STEP_AFTER_EXCHANGE, STEP_ALL, STEP_BEFORE_EXCHANGE, STEP_PACK_SYNC, check
from .ops import METRICS, _bytes, _codebook, _latents, _mse_scratch, _on_tensor_device, _stream


def _p(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


class _Arena:
    """Workspace + exchange buffer of one (shape, stream): allocated once, reused by every step on that stream (a fresh
    torch allocation per step costs host time, and the sizes never change in a training run).  Under HIP-graph capture
    nothing persistent is created: the buffers of a captured call come from the graph's pool."""

    def __init__(self) -> None:
        self._bufs: dict = {}

    def get(self, key, ws_bytes: int, packed_floats: int, device):
        if torch.cuda.is_current_stream_capturing():
            return _bytes(ws_bytes, device), (torch.empty(packed_floats, dtype=torch.float32, device=device) if packed_floats else None)
        skey = (key, ops._raw_stream(device.index) if ops._raw_stream is not None else 0)
        hit = self._bufs.get(skey)
        if hit is None or hit[0].numel() < ws_bytes or (packed_floats and (hit[1] is None or hit[1].numel() < packed_floats)):
            if len(self._bufs) > 8:            # shapes come and go (variable last batches): keep the set small
                self._bufs.clear()
            hit = (_bytes(ws_bytes, device), torch.empty(packed_floats, dtype=torch.float32, device=device) if packed_floats else None)
            self._bufs[skey] = hit
        return hit


class CvqStepState:
    """The listed-code state of a CVQVAECallback, shared by its three flows (hook by hook, eager one-call, chained graph
    replays): the device-side list of the codes that can need an anchor (vqhip_cvq_rows), its length in a pinned host word with
    the event behind which that word may be read, the early word and sequence counter of the graph chain, the key buffer of
    NearestAnchor(sync=True), the arena — and the ONE record of which probability tensor (object, version, storage) the list
    describes and who wrote it last:
      'host'    the host wrote or copied the count (`rebuild`, `prefetch`): the word is good behind `event`;
      'device'  a one-call step's list kernel stored it (`note_prefetched`): good behind `event` where pinned memory is coherent;
      a token   a chained graph replay (`claim_by_replay`): the count is in the early word, under the sequence number."""

    def __init__(self, K: int, device: torch.device, ema_decay: float, eps: float) -> None:
        self.K, self.device, self.ema_decay, self.eps = K, device, ema_decay, eps
        self.rows = torch.empty(K, dtype=torch.int32, device=device)
        self.slot = torch.empty(K, dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self.count_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event()
        with torch.cuda.device(device):
            self.event.record()                                   # created now: the library records / waits on its handle
        self.event_handle = int(getattr(self.event, 'cuda_event', 0) or 0)
        # early count (include/vqhip.h, vqhip_cvq_forward_t.early_word_host): {sequence number << 32 | count}, and the device counter
        self.early_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.seq_dev = torch.zeros(1, dtype=torch.int32, device=device)
        # a device store into pinned memory reaches the host behind an event only where pinned host memory is coherent
        # (hipHostMalloc's default).  HIP_HOST_COHERENT=0 switches that off process-wide: a one-call eager step then counts on
        # the spot (`rebuild`: one synchronisation per step) instead of trusting the word
        self.host_word_coherent = os.environ.get('HIP_HOST_COHERENT', '1') != '0'
        self.keys = None                                          # int64 [K]: NearestAnchor(sync=True)'s key exchange (lazily)
        self.arena = _Arena()
        self._list_of = self._writer = None
        self._seq = None                     # sequence number the last launched replay publishes (read back by `resync`)

    def _note(self, p: torch.Tensor, writer) -> None:
        self._list_of, self._writer = (p, p._version, p.data_ptr()), writer

    def _describes(self, p: torch.Tensor) -> bool:
        lo = self._list_of
        return lo is not None and lo[0] is p and lo[1] == p._version and lo[2] == p.data_ptr()

    def invalidate(self) -> None:
        self._list_of = self._writer = None

    def valid_for(self, p: torch.Tensor) -> bool:
        """True when rows / slot / count AND the pinned count word behind `event` describe exactly this ``p``."""
        return (self._writer == 'host' or (self._writer == 'device' and self.host_word_coherent)) and self._describes(p)

    def rebuild(self, p: torch.Tensor) -> int:
        """List the codes for ``p`` now and count them on the host (one synchronisation): a first step, a loaded checkpoint, a
        probability buffer replaced or modified from outside, another writer since."""
        ops.cvq_rows(p, self.K, self.ema_decay, self.eps, out=(self.rows, self.slot, self.count))
        n = int(self.count.item())
        self.count_host[0] = n
        self._note(p, 'host')
        return n

    def prefetch(self, p: torch.Tensor) -> None:
        """End of a hook-by-hook step: the NEXT step's list, its length on its way to the pinned word, the event behind it."""
        ops.cvq_rows(p, self.K, self.ema_decay, self.eps, out=(self.rows, self.slot, self.count))
        self.count_host.copy_(self.count, non_blocking=True)
        self.event.record()
        self._note(p, 'host')

    def note_prefetched(self, p: torch.Tensor) -> None:
        """A one-call eager step ended by listing the codes for ``p`` (the call's last but one launch stores the count)."""
        self._list_of, self._writer = (p, p._version, p.data_ptr()), 'device'

    def wait_count(self) -> int:
        """The prefetched length (`valid_for` holds): the one host wait of an eager step, on an event queued a step earlier."""
        self.event.synchronize()
        return int(self.count_host[0])

    # ---- the chain of graph replays (graphs.GraphedQuantizer): every replay ends by writing the next step's list and publishes
    # {its sequence number, that list's length} to the early word as soon as its histogram is final
    def published_count(self, token, p: torch.Tensor, timeout_s: float) -> Optional[int]:
        """Length of the list the replay is about to start from, or None when the chain is broken: the last writer was not a
        replay of ``token``'s owner (an eager step in between rewrites the list without touching the early word, and so does
        another GraphedQuantizer on the same module), ``p`` changed from outside, or the word never arrived (a failed replay, a
        non-coherent pinned pool) — `resync` then."""
        if self._writer != token or not self._describes(p):
            return None
        word = int(self.early_host[0])       # usually long since there: the rest of the previous replay is what the GPU runs now
        if (word >> 32) != self._seq:
            deadline = time.monotonic() + timeout_s
            while (word >> 32) != self._seq and time.monotonic() < deadline:
                word = int(self.early_host[0])
        return (word & 0xFFFFFFFF) if (word >> 32) == self._seq else None

    def resync(self, p: torch.Tensor) -> int:
        """`rebuild`, and the device's sequence number re-read."""
        n = self.rebuild(p)
        self._seq = int(self.seq_dev.item())
        return n

    def claim_by_replay(self, token, p: torch.Tensor) -> None:
        """A chained replay has been launched: it advances the device counter by one and leaves the list describing the ``p`` it
        writes in place (no version bump).  The host knows no count behind `event`: an eager step after it rebuilds."""
        self._seq += 1
        self._note(p, token)


def _begin(a, x: torch.Tensor, w_in: torch.Tensor, metric, *, hist: bool = True, xq: Optional[bool] = None, tail: bool = True):
    """What the three one-call forwards share: the common outputs (tokens, histogram, cosine rows, straight-through output, loss
    means, codebook image) allocated and the fields the three argument blocks have under the same name filled in (``xq`` None:
    cosine metrics only).  Returns (out dict, image, (N, K, D, x dtype code, metric code))."""
    x, dt = _latents(x)
    (N, D), K, dev, m = x.shape, w_in.shape[0], x.device, METRICS[metric]
    if xq is None:
        xq = m in (_lib.METRIC_COS, _lib.METRIC_COS_BF16)
    out = dict(x=x, idx=torch.empty(N, dtype=torch.int64, device=dev),
               hist=torch.empty(K, dtype=torch.int32, device=dev) if hist else None,
               xq=torch.empty(N, D, dtype=torch.float32, device=dev) if xq else None,
               z_ste=torch.empty(N, D, dtype=torch.float32, device=dev) if tail else None,
               mse=torch.empty(4, dtype=torch.float32, device=dev) if tail else None)
    image = _bytes(_lib.lib().vqhip_codebook_bytes(K, D), dev)
    a.struct_bytes = ctypes.sizeof(a)
    a.N, a.K, a.D, a.x_dtype, a.metric = N, K, D, dt, m
    a.x, a.w_in = x.data_ptr(), w_in.data_ptr()
    a.cb, a.cb_bytes = image.data_ptr(), image.numel()
    a.idx, a.hist, a.xq = out['idx'].data_ptr(), _p(out['hist']), _p(out['xq'])
    a.z_ste, a.mse = _p(out['z_ste']), _p(out['mse'])
    a.scratch16 = _mse_scratch(dev).data_ptr() if tail else None
    return out, image, (N, K, D, dt, m)


def _caller_exchanges(exchange: bool, comm, world: int, all_reduce) -> bool:
    """True when the step's exchange is a collective the CALLER issues between the library's phases: there is one to run and
    the library has no communicator to run it on."""
    return bool(exchange) and comm is None and not (world == 1 and all_reduce is None)


def _run(fn, name: str, a, between=()) -> None:
    """Enqueue the step: ONE call — or the step's phases around the collectives the caller issues itself (``between``: the
    packed SUM, behind the key-MIN step of NearestAnchor(sync=True) when there are two)."""
    stream, ref = _stream(), ctypes.byref(a)
    if not between:
        a.phases = STEP_ALL
        return check(fn(ref, stream), name)
    phases = (STEP_BEFORE_EXCHANGE, STEP_PACK_SYNC, STEP_AFTER_EXCHANGE) if len(between) == 2 else (STEP_BEFORE_EXCHANGE, STEP_AFTER_EXCHANGE)
    for phase, collective in zip(phases, between + (None,)):
        a.phases = phase
        check(fn(ref, stream), name)
        if collective is not None:
            collective()


@_on_tensor_device
def cvq_forward(x: torch.Tensor, w_in: torch.Tensor, p_in: torch.Tensor, w_out: torch.Tensor, p_out: torch.Tensor, metric,
                ema_decay: float, eps: float, beta: float, state: CvqStepState, *, cap: int, list_ready: bool, prefetch: bool,
                exchange: bool, world: int, comm: Optional[int], all_reduce=None, tail: bool = True, early_count: bool = False,
                anchor_sync: bool = False, rank: int = 0, all_reduce_min=None):
    """The CVQ-VAE training forward as one library call (two around a caller-issued collective when ``comm`` is None and the
    exchange has more than one rank: ``all_reduce(packed_view)`` is then called between the halves).

    cap >= 0: capacity of the listed-code launches; cap < 0: the library reads the prefetched count itself (the pinned word
    of ``state``, behind the event of its copy).  ``anchor_sync`` (with ``exchange``): NearestAnchor(sync=True) — the ranks agree
    on the global nearest latent per listed code through ``all_reduce_min(keys)`` before the packed SUM (three library calls
    around the two collectives, one with a communicator).  Returns a dict: idx, hist, xq (cosine), prepared (the codebook image),
    z_ste, mse (fp32[4]), cap_used, exchange_floats."""
    ops._require_cuda(x, w_in, p_in, w_out, p_out)
    L = _lib.lib()
    a = _lib.CvqForwardArgs()
    out, image, (N, K, D, dt, m) = _begin(a, x, w_in, metric, tail=tail)
    dev = out['x'].device
    capturing = torch.cuda.is_current_stream_capturing()
    cap_max = cap if cap >= 0 else K
    ws_bytes = L.vqhip_cvq_forward_ws_bytes(N, K, D, cap_max)
    ws, packed = state.arena.get((N, K, D, dt, cap_max), ws_bytes, ops.pack_floats(K, cap_max, D) if exchange else 0, dev)
    a.world = int(world)
    a.ema_decay, a.eps, a.beta = float(ema_decay), float(eps), float(beta)
    a.exchange, a.list_ready, a.prefetch = int(bool(exchange)), int(bool(list_ready)), int(bool(prefetch))
    a.cap = int(cap)
    a.p_in, a.w_out, a.p_out = p_in.data_ptr(), w_out.data_ptr(), p_out.data_ptr()
    a.rows, a.slot, a.count = state.rows.data_ptr(), state.slot.data_ptr(), state.count.data_ptr()
    # the pinned count word: written by the prefetch (a store of the list kernel itself, capturable), read by the call when cap < 0;
    # the event around it belongs to eager steps only (a captured step's replay is followed by the caller's own event)
    use_host_word = prefetch or cap < 0
    a.count_host = state.count_host.data_ptr() if use_host_word else None
    a.count_event = (state.event_handle or None) if (use_host_word and not capturing) else None
    a.comm = comm
    a.packed, a.packed_floats = _p(packed), (packed.numel() if packed is not None else 0)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    a.cap_used, a.exchange_floats = -1, 0
    a.early_word_host = state.early_host.data_ptr() if early_count else None
    a.early_seq_dev = state.seq_dev.data_ptr() if early_count else None
    sync = bool(anchor_sync and exchange)
    a.anchor_sync, a.rank = int(sync), int(rank)
    keys = None
    if sync:
        if capturing:
            keys = torch.empty(K, dtype=torch.int64, device=dev)
        else:
            if state.keys is None:
                state.keys = torch.empty(K, dtype=torch.int64, device=dev)
            keys = state.keys
    a.keys = _p(keys)
    if cap < 0 and not state.event_handle:           # no raw handle on this torch build: the wait happens here instead
        a.cap = state.wait_count()
    between = ()
    if _caller_exchanges(exchange, comm, world, all_reduce):
        between = (lambda: all_reduce(packed[:a.exchange_floats]),)
        if sync:
            between = (lambda: a.cap_used > 0 and all_reduce_min(keys[:a.cap_used]),) + between
    _run(L.vqhip_cvq_forward, 'vqhip_cvq_forward', a, between)
    if use_host_word and prefetch and not capturing and not state.event_handle:
        state.event.record()
    out.update(prepared=ops.PreparedCodebook(image, w_in, K, D, m), cap_used=int(a.cap_used), exchange_floats=int(a.exchange_floats))
    return out


class VqkdStepState:
    """Arena of a VQKDCallback's fused forward."""

    def __init__(self) -> None:
        self.arena = _Arena()


@_on_tensor_device
def vqkd_forward(x: torch.Tensor, w_in: torch.Tensor, w_mid: torch.Tensor, w_out: torch.Tensor, metric, ema_decay: float,
                 state: VqkdStepState, *, exchange: bool, world: int, comm: Optional[int], all_reduce=None,
                 ordered: bool = False, tail: bool = True):
    """The VQ-KD training forward as one library call (two around a caller-issued collective, as ``cvq_forward``).
    Returns a dict: xn (F.normalize(x)), xq (F.normalize(xn)), idx, hist, prepared, z_ste, mse (fp32[4], [0] = the
    commitment loss with norm=True)."""
    ops._require_cuda(x, w_in, w_mid, w_out)
    L = _lib.lib()
    a = _lib.VqkdForwardArgs()
    out, image, (N, K, D, dt, m) = _begin(a, x, w_in, metric, xq=True, tail=tail)
    dev = out['x'].device
    floats = ops.pack_floats(K, K, D)
    ws, packed = state.arena.get((N, K, D, dt), L.vqhip_vqkd_forward_ws_bytes(N, K, D), floats, dev)
    xn = torch.empty(N, D, dtype=torch.float32, device=dev)
    a.world = int(world)
    a.ema_decay = float(ema_decay)
    a.exchange, a.ordered, a.tail = int(bool(exchange)), int(bool(ordered)), int(bool(tail))
    a.w_mid, a.w_out = w_mid.data_ptr(), w_out.data_ptr()
    a.xn = xn.data_ptr()
    a.comm = comm
    a.packed, a.packed_floats = packed.data_ptr(), packed.numel()
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    _run(L.vqhip_vqkd_forward, 'vqhip_vqkd_forward', a,
         (lambda: all_reduce(packed[:floats]),) if _caller_exchanges(exchange, comm, world, all_reduce) else ())
    out.update(xn=xn, prepared=ops.PreparedCodebook(image, w_mid, K, D, m))
    return out


@_on_tensor_device
def vq_forward(x: torch.Tensor, w_in: torch.Tensor, w_out: Optional[torch.Tensor], metric, beta: float, *, normalize: bool,
               want_hist: bool, tail: bool = True):
    """The forward of a quantizer without an update callback — or with NormalizeCallback alone (``normalize``) — as one library
    call (include/vqhip.h: vqhip_vq_forward).  Returns a dict: xn (F.normalize(x), normalize only), idx, hist, xq (cosine),
    prepared, z_ste, mse, x (the latents as the library read them)."""
    ops._require_cuda(x, w_in)
    L = _lib.lib()
    a = _lib.VqForwardArgs()
    out, image, (N, K, D, dt, m) = _begin(a, x, w_in, metric, hist=want_hist, tail=tail)
    dev = out['x'].device
    ws = _bytes(L.vqhip_workspace_bytes(N, K, D), dev)
    xn = torch.empty(N, D, dtype=torch.float32, device=dev) if normalize else None
    a.normalize, a.beta = int(bool(normalize)), float(beta)
    a.w_out, a.xn = _p(w_out), _p(xn)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    check(L.vqhip_vq_forward(ctypes.byref(a), _stream()), 'vqhip_vq_forward')
    out.update(xn=xn, prepared=ops.PreparedCodebook(image, w_out if normalize else w_in, K, D, m))
    return out


@_on_tensor_device
def vqkd_backward(x: torch.Tensor, xn: torch.Tensor, w: torch.Tensor, idx: torch.Tensor, g_zste: Optional[torch.Tensor],
                  g_loss: Optional[torch.Tensor]) -> torch.Tensor:
    """grad_x of the VQ-KD tail (include/vqhip.h: vqhip_vqkd_backward) as fp32 [N, D]."""
    ops._require_cuda(x, xn, w, idx)
    x, dt = _latents(x)
    N, D = x.shape
    w = _codebook(w)
    gx = torch.empty(N, D, dtype=torch.float32, device=x.device)
    if g_zste is not None:
        g_zste = g_zste.float().contiguous()
    if g_loss is not None:
        g_loss = g_loss.detach().float().reshape(1).contiguous()
    check(_lib.lib().vqhip_vqkd_backward(x.data_ptr(), dt, xn.data_ptr(), w.data_ptr(), idx.data_ptr(), N, D, _p(g_zste), _p(g_loss),
                                         gx.data_ptr(), _stream()), 'vqhip_vqkd_backward')
    return gx
