"""The row ops of VQKDEncoder / VQKDDecoder: ``functional.add_layer_norm`` and ``functional.row_bias_act`` (one HIP launch forward,
the recomputing backwards) against the torch composition a block runs (``x + branch``, ``F.layer_norm``; ``fc1``'s bias add and
``F.gelu``), forward + backward, and one training step of the default ``VQKDEncoder`` on both routes and on the torch route with the fused route's
attention core (``torch_sdpa``), in the same process on the same GPU.

    python tools/bench_vit_ops.py [--batch 64] [--blocks 5] [--iters 20] [--skip-module] [--out profiles/vqkd_autoencoder.txt]

Shapes: [B * 197, 768] (the residual stream) and [B * 197, 3072] (the MLP hidden tensor) with B = ``--batch`` images of 224 x 224
(the VQ-KD per-rank batch is not pinned in this repository; 64 is the default here and is written into every line), fp32 and
bf16 autocast (fp32 stream, bf16 branch and output).  Warm-up, then ``blocks`` blocks of ``iters`` steps timed with device events,
the routes alternating block by block; the figure is the median of the block means in microseconds, host enqueue included, with
the smallest and largest block.  One JSON line per case; ``--out`` appends the lines to a file.  Whatever is measured is written
down as it is."""
from __future__ import annotations

import argparse
import functools
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def norm_case(functional, R, D, autocast, args):
    torch.manual_seed(0)
    low = torch.bfloat16 if autocast else torch.float32
    x = torch.randn(R, D, device='cuda', requires_grad=True)
    r = torch.randn(R, D, device='cuda').to(low).requires_grad_()
    w, b = torch.randn(D, device='cuda', requires_grad=True), torch.randn(D, device='cuda', requires_grad=True)
    g, gs = torch.randn(R, D, device='cuda').to(low), torch.randn(R, D, device='cuda')

    def run(fn):
        x.grad = r.grad = w.grad = b.grad = None
        s, y = fn()
        torch.autograd.backward((s, y), (gs, g))

    def torch_route():
        # as a block runs it: the add promotes to the stream's fp32, layer_norm is fp32-listed under autocast and the next linear casts
        with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
            s = x + r
            return s, F.layer_norm(s, (D,), w, b, 1e-6).to(low)

    res = alternate({'fused': lambda: run(lambda: functional.add_layer_norm(x, r, w, b, 1e-6, low)), 'torch': lambda: run(torch_route)},
                    args.blocks, args.iters)
    # forward reads x and res, writes s and y; backward reads g, s and g_skip, writes gx (and the cast of gx for res under autocast)
    nbytes = R * D * (4 + r.element_size() + 4 + r.element_size() + g.element_size() + 4 + 4 + 4)
    return dict(case='add_layer_norm_fwd_bwd', nbytes=nbytes, **res)


def act_case(functional, R, D, autocast, args):
    torch.manual_seed(0)
    low = torch.bfloat16 if autocast else torch.float32
    h = torch.randn(R, D, device='cuda').to(low).requires_grad_()
    b = torch.randn(D, device='cuda', requires_grad=True)
    g = torch.randn(R, D, device='cuda').to(low)

    def run(fn):
        h.grad = b.grad = None
        fn().backward(g)

    res = alternate({'fused': lambda: run(lambda: functional.row_bias_act(h, b, 'gelu')),
                     'torch': lambda: run(lambda: F.gelu(h + b.to(low)))}, args.blocks, args.iters)
    nbytes = R * D * h.element_size() * 5                                        # x read twice, y written; g read, gx written
    return dict(case='row_bias_gelu_fwd_bwd', nbytes=nbytes, **res)


def module_case(vqa, autocast, args):
    torch.manual_seed(0)
    # 'torch_sdpa': the torch route with only its attention core swapped for F.scaled_dot_product_attention, which the fused route
    # uses too - what separates the gain of the HIP row ops from the gain of not keeping the [B, heads, 197, 197] matrix
    nets = {name: vqa.VQKDEncoder(fused=name == 'fused').cuda() for name in ('fused', 'torch', 'torch_sdpa')}
    nets['fused'].init_weights()
    for name in ('torch', 'torch_sdpa'):
        nets[name].load_state_dict(nets['fused'].state_dict(), strict=True)
    for blk in nets['torch_sdpa'].blocks:
        blk.attn.forward = functools.partial(blk.attn.forward, fused=True)
    image = torch.randn(args.batch, 3, 224, 224, device='cuda')

    def step(net):
        net.zero_grad(set_to_none=True)
        with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
            z, _ = net(image, {})
        z.float().square().mean().backward()

    res = alternate({name: (lambda n=net: step(n)) for name, net in nets.items()}, args.blocks, max(2, args.iters // 4))
    assert nets['fused'].last_route.name == 'fused', nets['fused'].last_route
    peak = {}
    for name, net in nets.items():
        torch.cuda.reset_peak_memory_stats()
        step(net)
        torch.cuda.synchronize()
        peak[name + '_peak_mib'] = round(torch.cuda.max_memory_allocated() / 2 ** 20)
    return dict(case='vqkd_encoder_default_step', **res, **peak)


def main():
    import vector_quantization_amd as vqa
    from vector_quantization_amd import functional
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-module', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_vit_ops.py needs an MI355X'
    R = args.batch * 197
    lines = []

    def emit(line, shape, autocast):
        nbytes = line.pop('nbytes', None)
        line.update(shape=shape, B=args.batch, dtype='bf16_autocast' if autocast else 'fp32',
                    torch_over_fused=round(line['torch']['median_us'] / line['fused']['median_us'], 2), blocks=args.blocks, iters=args.iters)
        if 'torch_sdpa' in line:
            line['torch_sdpa_over_fused'] = round(line['torch_sdpa']['median_us'] / line['fused']['median_us'], 2)
        if nbytes:
            line['fused_gbs'] = round(nbytes / line['fused']['median_us'] / 1e3, 1)
        print(json.dumps(line), flush=True)
        lines.append(line)

    for autocast in (False, True):
        emit(norm_case(functional, R, 768, autocast, args), [R, 768], autocast)
        emit(act_case(functional, R, 3072, autocast, args), [R, 3072], autocast)
    if not args.skip_module:
        for autocast in (False, True):
            emit(module_case(vqa, autocast, args), [args.batch, 3, 224, 224], autocast)
    if args.out:
        with open(args.out, 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
