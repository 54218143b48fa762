"""One sampler step of stage-2 generation: the fused launch (ops.sample_tokens behind the sampler modules) against the 'torch'
route (the reference's composition with torch ops: slice, CFG mix, division, topk, sort, softmax, cumsum, scatter, softmax,
multinomial, add, repeat), in the same process on the same GPU.

    python tools/bench_sampler.py [--blocks 7] [--iters 200] [--out FILE]

Shapes (R, V_total, start, end): (32, 17385, 1001, 17385) and (128, 17385, 1001, 17385) bf16 under CFG (alpha 1.75) with top-k 600 /
top-p 0.92; (16, 16384, 0, 16384) fp32 plain BaseSampler; (32, 65001, 1001, 65001) bf16 under CFG with top-k 600 / top-p 0.92.
Per route: warm-up, then ``blocks`` blocks of ``iters`` steps timed with device events, the two routes alternating block by
block; the figure is the median of the block means (microseconds per step, host enqueue included: the step is launch-bound).
One JSON line per shape.
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

from vector_quantization_amd import samplers as S  # noqa: E402

# name, R, V_total, start, end, dtype, sampler factory
SHAPES = [
    ('cfg_topk_topp_r32', 32, 17385, 1001, 17385, torch.bfloat16, lambda: S.CFGSampler(sampler=S.TopKTopPSampler(), alpha=1.75)),
    ('cfg_topk_topp_r128', 128, 17385, 1001, 17385, torch.bfloat16, lambda: S.CFGSampler(sampler=S.TopKTopPSampler(), alpha=1.75)),
    ('base_fp32_r16', 16, 16384, 0, 16384, torch.float32, lambda: S.BaseSampler()),
    ('cfg_topk_topp_r32_v64000', 32, 65001, 1001, 65001, torch.bfloat16, lambda: S.CFGSampler(sampler=S.TopKTopPSampler(), alpha=1.75)),
]


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sampler.py times kernels: it needs an MI355X')
    lines = []
    for name, R, Vt, start, end, dtype, factory in SHAPES:
        logits = (torch.randn(R, Vt, generator=torch.Generator().manual_seed(R + Vt)) * 2).cuda().to(dtype)
        sampler = factory()
        routes = {'torch': lambda: sampler.forward_torch(logits, start, end, {}), 'fused': lambda: sampler(logits, start, end, {})}
        tokens, _ = sampler(logits, start, end, {})
        assert sampler.last_route.name == 'fused', sampler.last_route
        assert bool(((tokens >= start) & (tokens < end)).all())
        us = {r: [] for r in routes}
        for fn in routes.values():
            block_us(fn, 10)
        for _ in range(args.blocks):
            for r, fn in routes.items():
                us[r].append(block_us(fn, args.iters))
        rec = dict(shape=name, R=R, V_total=Vt, start=start, end=end, dtype=str(dtype).replace('torch.', ''), blocks=args.blocks,
                   iters=args.iters)
        for r in routes:
            rec[f'{r}_us'] = round(statistics.median(us[r]), 2)
            rec[f'{r}_us_min_max'] = [round(min(us[r]), 2), round(max(us[r]), 2)]
        rec['fused_over_torch'] = round(rec['fused_us'] / rec['torch_us'], 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
