"""StyleGAN2Discriminator at image_size 256: the fused route (HIP bias-activation, blur and their fusion between the convolutions)
against the torch route (the reference's composition with the two ops written in plain torch - what runs on this hardware
without mmcv) with the same weights, in the same process on the same GPU.

    python tools/bench_stylegan2.py [--blocks 3] [--iters 3] [--out profiles/stylegan2.txt]

Without ``--case`` the tool is a driver: every measurement runs in a fresh child process under its own ``timeout``, one after the
other, and the driver stops at the first child that fails.  Cases: the module at per-rank batches 4, 8 and 16, fp32 and bf16
autocast, each in NCHW and channels-last - forward alone, and forward + backward of ``logits.sum()`` - and the two ops alone at every
Residual block's shape (B = 8, bf16, both layouts): ``bias_act_blur`` against ``blur_torch(bias_act_torch(.))`` and the shortcut's
``blur(down=2)`` against ``blur_torch`` (which the stride-2 convolution then subsamples), forward + backward.  Warm-up, then
``blocks`` blocks of ``iters`` steps timed with device events, the routes alternating block by block; the figure is the median of
the block means in microseconds, host enqueue included.  ``peak_mib`` is ``torch.cuda.max_memory_allocated`` of one forward +
backward above what was allocated before it.  One JSON line per case; ``--out`` appends the lines to a file.  Whatever is measured
is written down as it is, a shape where the fused route loses included.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCHES = (4, 8, 16)
CHILD_SECONDS = 240


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fns, blocks, iters):
    """{name: median of block means} for the named callables, warmed up, alternating block by block."""
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(block_us(fn, iters))
    return {name: round(statistics.median(v), 1) for name, v in times.items()}


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def module_case(B, dtype, blocks, iters):
    from vector_quantization_amd import StyleGAN2Discriminator
    torch.manual_seed(0)
    fused = StyleGAN2Discriminator(image_size=256).cuda()
    fused.init_weights({})
    plain = StyleGAN2Discriminator(image_size=256, fused=False).cuda()
    plain.load_state_dict(fused.state_dict(), strict=True)
    cast = torch.autocast('cuda', torch.bfloat16) if dtype == 'bf16' else contextlib.nullcontext()
    lines = []
    for layout, fmt in (('nchw', torch.contiguous_format), ('channels_last', torch.channels_last)):
        image = torch.randn(B, 3, 256, 256, device='cuda').contiguous(memory_format=fmt)

        def fwd(m):
            with torch.no_grad(), cast:
                m(image)

        def fwd_bwd(m):
            with cast:
                out = m(image)
            out.float().sum().backward()
            m.zero_grad(set_to_none=True)

        f = alternate({'fused': lambda: fwd(fused), 'torch': lambda: fwd(plain)}, blocks, iters)
        fb = alternate({'fused': lambda: fwd_bwd(fused), 'torch': lambda: fwd_bwd(plain)}, blocks, iters)
        assert fused.last_route.name == 'fused' and plain.last_route.name == 'torch'
        lines.append(dict(case='module', B=B, dtype=dtype, layout=layout, fwd_us=f, fwd_bwd_us=fb,
                          fwd_speedup=round(f['torch'] / f['fused'], 3), fwd_bwd_speedup=round(fb['torch'] / fb['fused'], 3),
                          peak_mib=dict(fused=peak_mib(lambda: fwd_bwd(fused)), torch=peak_mib(lambda: fwd_bwd(plain)))))
    return lines


def ops_case(blocks, iters, B=8):
    from vector_quantization_amd import StyleGAN2Discriminator, discriminators, functional
    kernel = discriminators.Blur(kernel_size=3).kernel.cuda()
    ch = StyleGAN2Discriminator.CHANNELS
    lines = []
    for size in (256, 128, 64, 32, 16, 8):
        C = ch[size]
        for layout, fmt in (('nchw', torch.contiguous_format), ('channels_last', torch.channels_last)):
            x = torch.randn(B, C, size, size, device='cuda', dtype=torch.bfloat16).contiguous(memory_format=fmt).requires_grad_()
            bias = torch.randn(C, device='cuda', requires_grad=True)

            def run(fn):
                fn().float().sum().backward()
                x.grad = bias.grad = None

            ab = alternate({'fused': lambda: run(lambda: functional.bias_act_blur(x, bias, 2)),
                            'torch': lambda: run(lambda: discriminators.blur_torch(discriminators.bias_act_torch(x, bias), kernel, (2, 2)))},
                           blocks, iters)
            sc = alternate({'fused': lambda: run(lambda: functional.blur(x, 1, 2)),
                            'torch': lambda: run(lambda: discriminators.blur_torch(x, kernel, (1, 1)))}, blocks, iters)
            lines.append(dict(case='ops', B=B, C=C, size=size, dtype='bf16', layout=layout, bias_act_blur_fwd_bwd_us=ab,
                              shortcut_blur_fwd_bwd_us=sc, bias_act_blur_speedup=round(ab['torch'] / ab['fused'], 3),
                              shortcut_blur_speedup=round(sc['torch'] / sc['fused'], 3)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', default=None, help='module:B:dtype or ops (set by the driver)')
    args = ap.parse_args()
    if args.case is None:
        cases = [f'module:{B}:{dtype}' for B in BATCHES for dtype in ('fp32', 'bf16')] + ['ops']
        for case in cases:
            cmd = ['timeout', '-k', '10', str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), '--case', case,
                   '--blocks', str(args.blocks), '--iters', str(args.iters)] + (['--out', args.out] if args.out else [])
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit(f'bench_stylegan2.py: case {case} ended with status {rc}; nothing further is started')
        return
    if not torch.cuda.is_available():
        raise SystemExit('bench_stylegan2.py times kernels: it needs an MI355X')
    if args.case == 'ops':
        lines = ops_case(args.blocks, args.iters)
    else:
        _, B, dtype = args.case.split(':')
        lines = module_case(int(B), dtype, args.blocks, args.iters)
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(text + '\n')


if __name__ == '__main__':
    main()
