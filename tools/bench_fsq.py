"""FiniteScalarQuantizer on one MI355X: the HIP path against the reference's ATen chain restated in torch, same GPU.

    python tools/bench_fsq.py                      # timing table (us per call, kernels per call)
    python tools/bench_fsq.py --profile-only       # the 524 288 x 6 bf16 calls only, for `rocprofv3 --kernel-trace --stats`
    python tools/bench_fsq.py --stats DIR          # kernel time and bytes/s of the fsq kernels from that run's *_kernel_stats.csv

Sizes: the FSQ configs' per-rank training batch (96 images over 8 ranks at 16x16 latents: 3 072 tokens, C = 5, levels
[8,8,5,5,5]) and a tokenization batch (524 288 tokens, C = 6, levels [8,8,8,5,5,5]); fp32 and bf16 latents.  Calls: the module
forward, forward + backward, and tokenization.encode_to_quant of the NCHW map.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vector_quantization_amd import build_quantizer, tokenization as T  # noqa: E402

SIZES = [('train', 3072, [8, 8, 5, 5, 5], (12, 16, 16)), ('tokenize', 524288, [8, 8, 8, 5, 5, 5], (2048, 16, 16))]
HBM_PEAK = 8.0e12          # bytes/s, spec


class AtenFSQ(torch.nn.Module):
    """vq/algorithms/fsq/quantizers.py:110-125 and base.py:175-182 as plain torch ops (the reference's launches)."""

    def __init__(self, levels, eps=1e-3):
        super().__init__()
        L = torch.tensor(levels, dtype=torch.int)
        self.register_buffer('M', (L - 1) * (1 - eps))
        self.register_buffer('odd', (L - 1) % 2)
        self.register_buffer('h', L // 2)
        self.register_buffer('cum', torch.tensor((1, ) + tuple(levels[:-1])).cumprod(0))

    def forward(self, x):
        z = torch.tanh(x + torch.atanh(self.odd / self.M)) * self.M - self.odd
        z = z / 2
        z = z + (z.round() - z).detach()
        out = z / self.h
        quant = ((z + self.h) * self.cum).sum(-1).to(torch.int)
        return out, quant


def _time(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _kernels(fn):
    """GPU kernels one call launches (torch.profiler device events); None where the profiler yields none."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    return n or None


def calls(levels, N, shape, dtype):
    q = build_quantizer(dict(type='FiniteScalarQuantizer', num_scalars_per_channel=levels)).cuda()
    ref = AtenFSQ(levels).cuda()
    C = len(levels)
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = (torch.randn(N, C, device='cuda', generator=gen) * 1.5).to(dtype).requires_grad_(True)
    g = torch.randn(N, C, device='cuda', generator=gen)
    b, h, w = shape
    x_map = (torch.randn(b, C, h, w, device='cuda', generator=gen) * 1.5).to(dtype)

    def hip_fwd():
        return q(x, {})[0]

    def hip_fwd_bwd():
        x.grad = None                                                # no accumulation kernel into an old gradient
        q(x, {})[0].backward(g)

    def hip_e2q():
        with torch.no_grad():
            T.encode_to_quant(q, x_map, {})

    def aten_fwd():
        return ref(x)[0]

    def aten_fwd_bwd():
        x.grad = None
        ref(x)[0].backward(g)

    def aten_e2q():
        with torch.no_grad():
            ref(x_map.permute(0, 2, 3, 1).reshape(-1, C))           # einops 'b c h w -> (b h w) c' + the encode (models/base.py:140-143)

    return [('forward', hip_fwd, aten_fwd), ('forward+backward', hip_fwd_bwd, aten_fwd_bwd), ('encode_to_quant', hip_e2q, aten_e2q)]


def table(iters):
    print(f'{"size":9s} {"dtype":5s} {"call":17s} {"hip us":>9s} {"aten us":>9s} {"speedup":>8s} {"hip k":>6s} {"aten k":>7s}')
    for name, N, levels, shape in SIZES:
        for dtype in (torch.float32, torch.bfloat16):
            for call, hip, aten in calls(levels, N, shape, dtype):
                th, ta = _time(hip, iters), _time(aten, iters)
                kh, ka = _kernels(hip), _kernels(aten)
                print(f'{name:9s} {str(dtype)[6:]:5s} {call:17s} {th:9.1f} {ta:9.1f} {ta / th:7.2f}x {str(kh):>6s} {str(ka):>7s}',
                      flush=True)


def profile_only(iters):
    name, N, levels, shape = SIZES[1]
    for call, hip, _ in calls(levels, N, shape, torch.bfloat16):
        for _ in range(iters):
            hip()
    torch.cuda.synchronize()


# bytes one launch moves at 524 288 x 6 bf16, by kernel (the encode of the token route, its backward, the map encode of
# encode_to_quant with its token rows and z rows)
N_BIG, C_BIG = 524288, 6
BYTES = {'fsq_encode_kernel<1, false>': N_BIG * (2 * C_BIG + 4 + 4 * C_BIG),
         'fsq_backward_kernel<1, false>': N_BIG * C_BIG * (2 + 4 + 2),
         'fsq_encode_kernel<1, true>': N_BIG * (2 * C_BIG + 2 * C_BIG + 4 + 4 * C_BIG)}


def stats(path):
    files = glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True)
    assert files, f'no *kernel_stats.csv under {path}'
    with open(files[0]) as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        name = r['Name']
        key = next((k for k in BYTES if k.replace(' ', '') in name.replace(' ', '')), None)
        avg_ns = float(r['AverageNs'])
        line = f'{name[:60]:60s} calls={r["Calls"]:>6s} avg={avg_ns / 1e3:8.2f} us'
        if key:
            bw = BYTES[key] / (avg_ns * 1e-9)
            line += f'  {BYTES[key] / 1e6:6.1f} MB  {bw / 1e12:5.2f} TB/s  ({BYTES[key] / HBM_PEAK * 1e6:.2f} us at HBM peak)'
        print(line)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--profile-only', action='store_true')
    ap.add_argument('--stats', default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    elif a.profile_only:
        profile_only(a.iters)
    else:
        table(a.iters)
