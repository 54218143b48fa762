"""The stage-2 training loss: the fused route (ops.token_cross_entropy: two launches forward, one backward, the logits read in
place) against the torch composition it replaces (``logits.float()``, ``F.cross_entropy``, ``.backward()``), in the same process
on the same GPU.

    python tools/bench_token_ce.py [--blocks 7] [--iters 50] [--out FILE]

Shapes: 12 x 257 and 32 x 257 rows of V_total = 17 385 (the whole vocabulary, start = 0), bf16 and fp32; and the MAGE slice,
[0, 16 384) of the same rows with label smoothing 0.1.  Per route and shape: forward alone and forward + backward; warm-up, then
``blocks`` blocks of ``iters`` steps timed with device events, the routes alternating block by block; the figure is the median
of the block means (microseconds, host enqueue included).  Algorithmic bytes: the forward reads the slice once (R V s bytes),
the backward reads it once more and writes R V_total s bytes of gradient; the share is of the 8 TB/s HBM peak.
Also records the largest error of the fused kernel and of the torch fp32 composition against float64 over the test cases of
tests/token_ce_ref.py, next to the derived bound.  One JSON line per shape; ``--out`` also writes the lines to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from vector_quantization_amd import ops  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
VT = 17385
# name, B, L, dtype, end, label smoothing
SHAPES = [(f'{name}_b{B}_{str(dt).replace("torch.", "")}', B, 257, dt, end, eps)
          for name, end, eps in (('ar_vocab', VT, 0.0), ('mage_slice', 16384, 0.1))
          for B in (12, 32) for dt in (torch.bfloat16, torch.float32)]


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def error_record():
    """Largest |value - float64| of lse / loss over the cases of tests/token_ce_ref.py, as a share of the derived bound, for the
    fused kernel and for the torch fp32 composition on the GPU."""
    import numpy as np
    import token_ce_ref as ref
    worst = dict(fused_abs=0.0, fused_over_bound=0.0, torch_abs=0.0, torch_over_bound=0.0)
    for case in ref.cases():
        V, start, R, dtype, seed = case
        x, t = ref.make_case(*case)
        a = ref.slice64(x, start, V)
        for eps in (0.0, 0.1):
            e = ref.reference(a, ref.row_targets(t.numpy(), start, V), eps)
            b = np.array([ref.bound(V, am) for am in np.abs(a).max(-1)])
            f = ops.token_ce_forward(x.cuda(), t.cuda(), start, start + V, label_smoothing=eps)
            sl = x.cuda()[:, start:start + V].float()
            tt = torch.where(t == ref.IGNORE, t, t - start).cuda()
            tl = F.cross_entropy(sl, tt, ignore_index=ref.IGNORE, label_smoothing=eps, reduction='none')
            for name, got in (('fused', f['loss']), ('torch', tl)):
                err = np.abs(got.double().cpu().numpy() - e['loss'])
                worst[f'{name}_abs'] = max(worst[f'{name}_abs'], float(err.max()))
                worst[f'{name}_over_bound'] = max(worst[f'{name}_over_bound'], float((err / b).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_token_ce.py times kernels: it needs an MI355X')
    lines = []
    for name, B, L, dtype, end, eps in SHAPES:
        g = torch.Generator().manual_seed(B + end)
        logits = (torch.randn(B, L, VT, generator=g) * 2).to(dtype).cuda().requires_grad_()
        tokens = torch.randint(0, end, (B, L), generator=g).cuda()
        rows, flat = logits.view(-1, VT), tokens.view(-1)

        def fused_fwd():
            return ops.token_cross_entropy(logits, tokens, 0, end, label_smoothing=eps)

        def torch_fwd():
            return F.cross_entropy(rows[:, :end].float(), flat, label_smoothing=eps)

        def fwd_bwd(fwd):
            def run():
                logits.grad = None
                fwd().backward()
            return run

        a, b = float(fused_fwd()), float(torch_fwd())
        assert abs(a - b) <= 1e-3 * abs(b), (a, b)
        routes = {'torch_fwd': torch_fwd, 'fused_fwd': fused_fwd, 'torch_fwd_bwd': fwd_bwd(torch_fwd), 'fused_fwd_bwd': fwd_bwd(fused_fwd)}
        us = {r: [] for r in routes}
        for fn in routes.values():
            block_us(fn, 5)
        for _ in range(args.blocks):
            for r, fn in routes.items():
                us[r].append(block_us(fn, args.iters))
        R, s = B * L, logits.element_size()
        nbytes = {'fwd': R * end * s, 'fwd_bwd': 2 * R * end * s + R * VT * s}
        rec = dict(shape=name, R=R, V_total=VT, end=end, dtype=str(dtype).replace('torch.', ''), label_smoothing=eps,
                   blocks=args.blocks, iters=args.iters)
        for r in routes:
            rec[f'{r}_us'] = round(statistics.median(us[r]), 2)
            rec[f'{r}_us_min_max'] = [round(min(us[r]), 2), round(max(us[r]), 2)]
        for k in ('fwd', 'fwd_bwd'):
            rate = nbytes[k] / (rec[f'fused_{k}_us'] * 1e-6)
            rec[f'fused_{k}_bytes'] = nbytes[k]
            rec[f'fused_{k}_TB_per_s'] = round(rate / 1e12, 3)
            rec[f'fused_{k}_hbm_share'] = round(rate / HBM_BYTES_PER_S, 3)
            rec[f'fused_over_torch_{k}'] = round(rec[f'fused_{k}_us'] / rec[f'torch_{k}_us'], 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del logits, rows
    lines.append(json.dumps(dict(error_record=error_record())))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
