"""VQ-KD's distillation loss: the fused route (ops.cosine_embedding_loss: two launches forward, one backward, both tensors read in
place in their own dtypes) against the composition it replaces (``CosineEmbeddingLoss.forward_torch`` - the reference's forward
around ``F.cosine_embedding_loss`` - its mean, and ``.backward()``) under the same autocast state, in the same process on the same
GPU.

    python tools/bench_cosine_embed.py [--blocks 7] [--iters 50] [--out FILE]

Shapes: R = 64 x 196 and 32 x 196 rows (the per-rank batches of configs/vqkd), C = 512, 768, 1024; pred bf16 against an fp32
target (inside ``torch.autocast('cuda', bfloat16)``, where the composition runs in fp32 on a copy) and both fp32 (no autocast).
The rows layout at every shape, the map layout (pred NCHW-contiguous [B, C, 14, 14]; the composition takes the rearranged view)
at C = 768.  Per route and shape: forward alone and forward + backward; warm-up, then ``blocks`` blocks of ``iters`` steps timed
with device events, the routes alternating block by block; the figure is the median of the block means (microseconds, host
enqueue included).  Algorithmic bytes: the forward reads pred and target once, the backward reads both once more and writes the
gradient in pred's dtype; the share is of the 8 TB/s HBM peak.  Also records the largest error of the fused kernel and of the
torch fp32 composition against float64 over the rows grid of tests/cosine_embed_ref.py, as a share of the derived bound.
One JSON line per shape; ``--out`` also writes the lines to a file.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from vector_quantization_amd import CosineEmbeddingLoss, ops, tokenization  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
P = 196
# name, B, C, pred dtype, layout
SHAPES = [(f'{layout}_b{B}_c{C}_{str(dt).replace("torch.", "")}', B, C, dt, layout)
          for layout, cs in (('rows', (512, 768, 1024)), ('map', (768,)))
          for B in (64, 32) for C in cs for dt in (torch.bfloat16, torch.float32)]


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def error_record():
    """Largest |per-row loss - float64| over the rows grid of tests/cosine_embed_ref.py, as a share of the derived bound, for the
    fused kernel and for the torch fp32 composition on the GPU."""
    import numpy as np
    import torch.nn.functional as F
    import cosine_embed_ref as ref
    worst = dict(fused_abs=0.0, fused_over_bound=0.0, torch_abs=0.0, torch_over_bound=0.0)
    for case in ref.cases():
        C, R, pad, dtypes, seed = case
        if pad:
            continue
        pred, target = ref.make_case(*case)
        e = ref.expected(case)
        pd, td = pred.cuda(), target.cuda()
        f = ops.cosine_embedding_forward(pd, td)
        tl = F.cosine_embedding_loss(pd.float(), td.float(), torch.ones(R, device='cuda'), reduction='none')
        for name, got in (('fused', f['loss']), ('torch', tl)):
            err = np.abs(got.double().cpu().numpy() - e['loss'])
            worst[f'{name}_abs'] = max(worst[f'{name}_abs'], float(err.max()))
            worst[f'{name}_over_bound'] = max(worst[f'{name}_over_bound'], float(err.max() / ref.bound(C)))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cosine_embed.py times kernels: it needs an MI355X')
    module = CosineEmbeddingLoss()
    lines = []
    for name, B, C, dtype, layout in SHAPES:
        g = torch.Generator().manual_seed(B + C)
        target = torch.randn(B, P, C, generator=g).cuda()
        if layout == 'rows':
            pred = torch.randn(B, P, C, generator=g).to(dtype).cuda().requires_grad_()
            rows = pred
        else:
            pred = torch.randn(B, C, 14, 14, generator=g).to(dtype).cuda().requires_grad_()
            rows = pred.flatten(2).transpose(1, 2)                             # the distiller's Rearrange, as a view
        autocast = (lambda: torch.autocast('cuda', dtype=torch.bfloat16)) if dtype == torch.bfloat16 else contextlib.nullcontext

        def fused_fwd():
            with autocast():
                return module(pred, target) if layout == 'rows' else tokenization.distill_loss(module, pred, target)

        def torch_fwd():
            with autocast():
                return module.forward_torch(rows, target).mean()

        def fwd_bwd(fwd):
            def run():
                pred.grad = None
                fwd().backward()
            return run

        a, b = float(fused_fwd()), float(torch_fwd())
        assert module.last_route.name == 'fused', module.last_route
        assert abs(a - b) <= 1e-4, (a, b)
        routes = {'torch_fwd': torch_fwd, 'fused_fwd': fused_fwd, 'torch_fwd_bwd': fwd_bwd(torch_fwd), 'fused_fwd_bwd': fwd_bwd(fused_fwd)}
        us = {r: [] for r in routes}
        for fn in routes.values():
            block_us(fn, 5)
        for _ in range(args.blocks):
            for r, fn in routes.items():
                us[r].append(block_us(fn, args.iters))
        R, s = B * P, pred.element_size()
        nbytes = {'fwd': R * C * (s + 4), 'fwd_bwd': 2 * R * C * (s + 4) + R * C * s}
        rec = dict(shape=name, layout=layout, R=R, C=C, pred_dtype=str(dtype).replace('torch.', ''), target_dtype='float32',
                   autocast=dtype == torch.bfloat16, blocks=args.blocks, iters=args.iters)
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
        del pred, rows, target
    lines.append(json.dumps(dict(error_record=error_record())))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
