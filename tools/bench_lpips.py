"""The tail of LPIPSLoss behind the VGG16 taps: the fused route (ops.lpips_distance: two launches per layer forward, one backward,
the features read in place in their own dtype and layout) against the composition it replaces (``LPIPSLoss.distance_torch`` -
the reference's normalize / mse_loss / dropout / 1 x 1 convolution / mean - and autograd) under the same autocast state, in the
same process on the same GPU.

    python tools/bench_lpips.py [--blocks 5] [--iters 10] [--eval] [--out FILE]

Shapes: synthetic post-ReLU features at the five tap shapes of a 256 x 256 image - [B, 64, 256, 256], [B, 128, 128, 128],
[B, 256, 64, 64], [B, 512, 32, 32], [B, 512, 16, 16] - each alone and all five as one loss, at B = 12 (configs/vqgan: 96 images
over 8 ranks), bf16 (inside ``torch.autocast('cuda', bfloat16)``) and fp32, NCHW-contiguous and channels-last.  Dropout is on
(the training step; ``--eval`` turns it off, the validation pass).  Per route and shape: forward alone, and forward plus TWO
backwards - ``torch.autograd.grad(loss, features, retain_graph=True)`` and then ``loss.backward()``, what ``VQGAN._aglw`` makes of
a generator step; warm-up, then ``blocks`` blocks of ``iters`` steps timed with device events, the routes alternating block by
block; the figure is the median of the block means (microseconds, host enqueue included).  Peak allocated memory of one forward
plus two backwards above what the features themselves hold is recorded for both routes.  Algorithmic bytes of the fused route:
the forward reads both maps once from HBM (its second pass re-reads a tile the workgroup has just read), a backward reads both
once more and writes the gradient in pred's dtype; the share is of the 8 TB/s HBM peak.  One JSON line per shape; ``--out`` also
writes the lines to a file.  Whatever is measured is written down as it is, a shape where the fused route loses included.
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vector_quantization_amd import LPIPSLoss, ops  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
BATCH = 12
LAYERS = [(64, 256), (128, 128), (256, 64), (512, 32), (512, 16)]             # (C, H = W) of the five taps at 256 x 256


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def features(layers, dtype, fmt, B):
    preds, targets = [], []
    for i in layers:
        C, H = LAYERS[i]
        g = torch.Generator(device='cuda').manual_seed(C + H)
        f = torch.randn(B, C, H, H, generator=g, device='cuda').clamp_min_(0.0)
        t = (f + 0.5 * torch.randn(B, C, H, H, generator=g, device='cuda')).clamp_min_(0.0)
        preds.append(f.to(dtype).contiguous(memory_format=fmt).requires_grad_())
        targets.append(t.to(dtype).contiguous(memory_format=fmt))
    return preds, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--batch', type=int, default=BATCH)
    ap.add_argument('--eval', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_lpips.py times kernels: it needs an MI355X')
    torch.manual_seed(0)
    module = LPIPSLoss().cuda().train(not args.eval)
    B, lines = args.batch, []
    for layers in [(i,) for i in range(5)] + [tuple(range(5))]:
        for dtype in (torch.bfloat16, torch.float32):
            for layout, fmt in (('nchw', torch.contiguous_format), ('channels_last', torch.channels_last)):
                preds, targets = features(layers, dtype, fmt, B)
                weights = [module._convs[i].weight for i in layers]
                autocast = (lambda: torch.autocast('cuda', dtype=torch.bfloat16)) if dtype == torch.bfloat16 else contextlib.nullcontext
                # (zip stops at the shorter list: distance_torch pairs these layers with the first convolutions, so hand it its own)
                convs = module._convs
                module._convs = torch.nn.ModuleList(convs[i] for i in layers)

                def fused_fwd():
                    seed = module._seed('cuda') if module._dropout.training else None
                    return ops.lpips_distance(preds, targets, weights, seed, module._dropout.p).mean()

                def torch_fwd():
                    with autocast():
                        return module.distance_torch(preds, targets).float().mean()

                def fwd_2bwd(fwd):
                    def run():
                        for f in preds:
                            f.grad = None
                        loss = fwd()
                        torch.autograd.grad(loss, preds, retain_graph=True)
                        loss.backward()
                    return run

                module._dropout.eval()
                values = [float(fused_fwd()), float(torch_fwd())]              # without dropout the two routes compute one value
                module._dropout.train(not args.eval)
                routes = {'torch_fwd': torch_fwd, 'fused_fwd': fused_fwd, 'torch_fwd_2bwd': fwd_2bwd(torch_fwd),
                          'fused_fwd_2bwd': fwd_2bwd(fused_fwd)}
                us, peak = {r: [] for r in routes}, {}
                for r, fn in routes.items():
                    block_us(fn, 3)
                    for f in preds:
                        f.grad = None
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    fn()
                    torch.cuda.synchronize()
                    peak[r] = torch.cuda.max_memory_allocated() - base
                for _ in range(args.blocks):
                    for r, fn in routes.items():
                        us[r].append(block_us(fn, args.iters))
                module._convs = convs
                elems = sum(B * LAYERS[i][0] * LAYERS[i][1] ** 2 for i in layers)
                s = preds[0].element_size()
                nbytes = {'fwd': elems * 2 * s, 'fwd_2bwd': elems * 2 * s + 2 * elems * 3 * s}
                rec = dict(layers=list(layers), shapes=[[B, LAYERS[i][0], LAYERS[i][1], LAYERS[i][1]] for i in layers], layout=layout,
                           dtype=str(dtype).replace('torch.', ''), autocast=dtype == torch.bfloat16, dropout=not args.eval,
                           blocks=args.blocks, iters=args.iters, feature_bytes=elems * 2 * s,
                           value_without_dropout=dict(fused=values[0], torch=values[1]))
                for r in routes:
                    rec[f'{r}_us'] = round(statistics.median(us[r]), 2)
                    rec[f'{r}_us_min_max'] = [round(min(us[r]), 2), round(max(us[r]), 2)]
                    rec[f'{r}_peak_bytes'] = int(peak[r])
                for k in ('fwd', 'fwd_2bwd'):
                    rate = nbytes[k] / (rec[f'fused_{k}_us'] * 1e-6)
                    rec[f'fused_{k}_bytes'] = nbytes[k]
                    rec[f'fused_{k}_TB_per_s'] = round(rate / 1e12, 3)
                    rec[f'fused_{k}_hbm_share'] = round(rate / HBM_BYTES_PER_S, 3)
                    rec[f'fused_over_torch_{k}'] = round(rec[f'fused_{k}_us'] / rec[f'torch_{k}_us'], 4)
                    rec[f'fused_over_torch_{k}_peak'] = round(rec[f'fused_{k}_peak_bytes'] / max(rec[f'torch_{k}_peak_bytes'], 1), 4)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                del preds, targets
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
