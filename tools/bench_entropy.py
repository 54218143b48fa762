"""Forward + backward of EntropyLoss, matrix route (fused=False: the [N, K] matrix with autograd on stock ops) against the fused
route (HIP kernels on one bounded row-block tile), in the same process.

    python tools/bench_entropy.py [--blocks 7] [--iters 5] [--out FILE]

Shapes: N = 12 544 x K = 16 384 x D = 256, L2 (the largest per-rank training batch of the shipped configs) and
N = 3 072 x K = 8 192 x D = 32, Cosine; bf16 latents, T = 0.5.  Per route: warm-up, then ``blocks`` blocks of ``iters``
steps timed with device events, the two routes alternating block by block; the figure is the median of the block means.
Peak memory beyond inputs and outputs is taken from a separate step.  One JSON line per shape.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vector_quantization_amd import quantizers as Q  # noqa: E402
from vector_quantization_amd.quantizers.distances import LazyDistance  # noqa: E402
from vector_quantization_amd.quantizers.losses import EntropyLoss  # noqa: E402

SHAPES = [(12544, 16384, 256, 'L2'), (3072, 8192, 32, 'Cosine')]


def step(x, w, dist, loss):
    x.grad = w.grad = None
    d = LazyDistance(dist, x, w)
    loss(None, x, dict(distance=d)).backward()


def block_ms(x, w, dist, loss, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step(x, w, dist, loss)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_mib(x, w, dist, loss):
    x.grad = w.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(x, w, dist, loss)
    torch.cuda.synchronize()
    out = x.grad.numel() * x.grad.element_size() + w.grad.numel() * w.grad.element_size()
    return (torch.cuda.max_memory_allocated() - base - out) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--routes', default='matrix,fused')
    args = ap.parse_args()
    routes = args.routes.split(',')
    lines = []
    for N, K, D, metric in SHAPES:
        g = torch.Generator().manual_seed(N + K)
        x = torch.randn(N, D, generator=g).bfloat16().cuda().requires_grad_(True)
        w = torch.randn(K, D, generator=g).cuda().requires_grad_(True)
        dist = Q.L2Distance() if metric == 'L2' else Q.CosineDistance(autocast=None)
        losses = {r: EntropyLoss(temperature=0.5, fused=(False if r == 'matrix' else None)) for r in routes}
        ms = {r: [] for r in routes}
        for r in routes:
            block_ms(x, w, dist, losses[r], 2)
        for _ in range(args.blocks):
            for r in routes:
                ms[r].append(block_ms(x, w, dist, losses[r], args.iters))
        rec = dict(N=N, K=K, D=D, metric=metric, dtype='bf16', blocks=args.blocks, iters=args.iters)
        for r in routes:
            rec[f'{r}_ms'] = round(statistics.median(ms[r]), 4)
            rec[f'{r}_ms_min_max'] = [round(min(ms[r]), 4), round(max(ms[r]), 4)]
            rec[f'{r}_peak_mib'] = round(peak_mib(x, w, dist, losses[r]), 1)
        if 'matrix' in ms and 'fused' in ms:
            rec['fused_over_matrix'] = round(rec['fused_ms'] / rec['matrix_ms'], 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
