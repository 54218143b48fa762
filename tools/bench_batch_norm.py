"""The BatchNorm2d + LeakyReLU(0.2) sites of PatchGANDiscriminator: ``functional.batch_norm(act='leaky_relu')`` (the HIP kernels with
batch statistics, the recomputing backward, the running-statistics update) against ``F.leaky_relu(F.batch_norm(..), 0.2)`` and
autograd - the modules' own route, ``fused=False`` - forward + backward, in the same process on the same GPU.

    python tools/bench_batch_norm.py [--blocks 5] [--iters 20] [--out profiles/batch_norm.txt]

Sites at 256 x 256 images: [B, 128, 64, 64], [B, 256, 32, 32], [B, 512, 31, 31]; B = 12 (configs/vqgan/interface.py: 96 images
in total over 8 ranks) and 8; bf16 (what the convolutions hand on under autocast) and fp32; NCHW and channels-last.  Then a whole
``PatchGANDiscriminator`` forward + backward on [B, 3, 256, 256] under bf16 autocast and in fp32, ``fused=True`` against
``fused=False``.  Warm-up, then ``blocks`` blocks of ``iters`` steps timed with device events, the routes alternating block by
block; the figure is the median of the block means in microseconds, host enqueue included, with the smallest and largest block.
``gbs`` is the bytes the fused route must move (x read twice and y written forward; g and x read twice and gx written backward:
eight tensor-sized passes, six where a workgroup holds a channel) over that time.  One JSON line per case; ``--out`` appends the
lines to a file.  Whatever is measured is written down as it is: no ratio is promised."""
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

SITES = ((128, 64, 64), (256, 32, 32), (512, 31, 31))
BATCHES = (12, 8)


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


def site(B, C, H, W, dtype, fmt, args):
    from vector_quantization_amd import functional
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, device='cuda').to(dtype).contiguous(memory_format=fmt).requires_grad_()
    g = torch.randn(B, C, H, W, device='cuda').to(dtype).contiguous(memory_format=fmt)
    w = torch.randn(C, device='cuda', requires_grad=True)
    b = torch.randn(C, device='cuda', requires_grad=True)
    rm, rv, count = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda'), torch.zeros((), dtype=torch.long, device='cuda')

    def run(fn):
        x.grad = w.grad = b.grad = None
        fn().backward(g)

    def torch_route():
        # as nn.BatchNorm2d and the in-place nn.LeakyReLU run it (batch_norm keeps the input's dtype under autocast)
        count.add_(1)
        return F.leaky_relu_(F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5), 0.2)

    r = alternate({'fused': lambda: run(lambda: functional.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5, 'leaky_relu', count)),
                   'torch': lambda: run(torch_route)}, args.blocks, args.iters)
    nbytes = 8 * x.numel() * x.element_size()
    return dict(case='batch_norm_leaky_relu_fwd_bwd', shape=[B, C, H, W], dtype=str(dtype).split('.')[-1],
                layout='nchw' if fmt == torch.contiguous_format else 'channels_last', fused=r['fused'], torch=r['torch'],
                torch_over_fused=round(r['torch']['median_us'] / r['fused']['median_us'], 2),
                fused_gbs=round(nbytes / r['fused']['median_us'] / 1e3, 1), blocks=args.blocks, iters=args.iters)


def module(B, autocast, fmt, args):
    from vector_quantization_amd.discriminators import PatchGANDiscriminator
    torch.manual_seed(0)
    fused = PatchGANDiscriminator().cuda()
    plain = PatchGANDiscriminator(fused=False).cuda()
    plain.load_state_dict(fused.state_dict())
    image = torch.randn(B, 3, 256, 256, device='cuda').contiguous(memory_format=fmt)

    def run(d):
        d.zero_grad(set_to_none=True)
        with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
            out = d(image)
        out.float().mean().backward()

    r = alternate({'fused': lambda: run(fused), 'torch': lambda: run(plain)}, args.blocks, args.iters)
    assert fused.last_route.name == 'fused' and plain.last_route.name == 'torch'
    return dict(case='patchgan_discriminator_fwd_bwd', shape=[B, 3, 256, 256], dtype='bf16_autocast' if autocast else 'float32',
                layout='nchw' if fmt == torch.contiguous_format else 'channels_last', fused=r['fused'], torch=r['torch'],
                torch_over_fused=round(r['torch']['median_us'] / r['fused']['median_us'], 2), blocks=args.blocks, iters=args.iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_batch_norm.py needs an MI355X'
    lines = []
    formats = (torch.contiguous_format, torch.channels_last)
    for B in BATCHES:
        for C, H, W in SITES:
            for dtype in (torch.bfloat16, torch.float32):
                for fmt in formats:
                    lines.append(site(B, C, H, W, dtype, fmt, args))
                    print(json.dumps(lines[-1]), flush=True)
    for B in BATCHES:
        for autocast in (True, False):
            for fmt in formats:
                lines.append(module(B, autocast, fmt, args))
                print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
