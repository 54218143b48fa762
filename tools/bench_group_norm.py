"""The GroupNorm + SiLU site of VQGANEncoder / VQGANDecoder: ``functional.group_norm(act='silu')`` (one HIP launch forward, the
recomputing backward) against ``F.silu(F.group_norm(..))`` under bf16 autocast, cast back to bf16, and autograd, forward + backward, in the same process on the same GPU.

    python tools/bench_group_norm.py [--blocks 5] [--iters 20] [--out profiles/vqgan_autoencoder.txt]

Shapes: [8, 128, 256, 256] (the configs' largest map: 256 groups of 262144 values, split over 32 workgroups each) and
[8, 512, 16, 16] (one workgroup per group of 4096), bf16, NCHW and channels-last, G = 32, eps = 1e-6.  Warm-up, then ``blocks``
blocks of ``iters`` steps timed with device events, the routes alternating block by block; the figure is the median of the block
means in microseconds, host enqueue included, with the smallest and largest block.  ``gbs`` is the bytes the fused route must
move (x read twice forward where a group is split, once otherwise, y written; g and x read, twice where split, gx written) over
that time.  One JSON line per case; ``--out`` appends the lines to a file.  Whatever is measured is written down as it is."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((8, 128, 256, 256), (8, 512, 16, 16))


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fns, blocks, iters):
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(block_us(fn, iters))
    return {name: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for name, v in times.items()}


def main():
    from vector_quantization_amd import _lib, functional
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_group_norm.py needs an MI355X'
    lines = []
    for shape in SHAPES:
        for fmt, name in ((torch.contiguous_format, 'nchw'), (torch.channels_last, 'channels_last')):
            torch.manual_seed(0)
            x = torch.randn(shape, device='cuda').to(torch.bfloat16).contiguous(memory_format=fmt).requires_grad_()
            g = torch.randn(shape, device='cuda').to(torch.bfloat16).contiguous(memory_format=fmt)
            w = torch.randn(shape[1], device='cuda', requires_grad=True)
            b = torch.randn(shape[1], device='cuda', requires_grad=True)

            def run(fn):
                x.grad = w.grad = b.grad = None
                fn().backward(g)

            def torch_route():
                # as the modules run it under bf16 autocast: group_norm is fp32-listed, the next convolution casts the result back
                with torch.autocast('cuda', torch.bfloat16):
                    return F.silu(F.group_norm(x, 32, w, b, 1e-6)).to(torch.bfloat16)

            r = alternate({'fused': lambda: run(lambda: functional.group_norm(x, 32, w, b, 1e-6, 'silu')),
                           'torch': lambda: run(torch_route)}, args.blocks, args.iters)
            n = shape[1] // 32 * shape[2] * shape[3]
            passes = (3 if n <= _lib.GN_CHUNK else 4) + (3 if n <= _lib.GN_CHUNK else 5)    # tensor-sized reads and writes, forward + backward
            nbytes = passes * x.numel() * 2
            line = dict(case='group_norm_silu_fwd_bwd', shape=list(shape), dtype='bf16', layout=name, fused=r['fused'], torch=r['torch'],
                        torch_over_fused=round(r['torch']['median_us'] / r['fused']['median_us'], 2),
                        fused_gbs=round(nbytes / r['fused']['median_us'] / 1e3, 1), blocks=args.blocks, iters=args.iters)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
