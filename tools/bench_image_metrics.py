"""The reconstruction metrics of a validation pass: the fused route (ops.image_metrics: one launch pair for L1, MSE, PSNR and
SSIM) against the four-metric torch composition it replaces (``decode(v) / 255`` on both images for each of the four metrics,
then the loss classes' torch route; SSIM through ``F.avg_pool2d`` in float64 on the device), in the same process on the same GPU.

    python tools/bench_image_metrics.py [--blocks 7] [--iters 50] [--out FILE]

Shapes: 32 x 3 x 256 x 256 and 8 x 3 x 256 x 256, bf16 and fp32, NCHW and channels-last.  Per route and shape: warm-up, then
``blocks`` blocks of ``iters`` calls timed with device events, the routes alternating block by block; the figure is the median of
the block means (microseconds, host enqueue included).  Algorithmic bytes of the fused route: both images once.  Where
scikit-image imports, the reference's own SSIMLoss (host copy, one ``structural_similarity`` call per image) is timed too, by
the wall clock, and its values are compared.  One JSON line per shape; ``--out`` also writes the lines to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vector_quantization_amd import image_losses, ops, runners  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
SHAPES = [(B, dt, layout) for B in (32, 8) for dt in (torch.bfloat16, torch.float32) for layout in ('nchw', 'channels_last')]


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
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_metrics.py times kernels: it needs an MI355X')
    try:
        from skimage.metrics import structural_similarity
    except ImportError:
        structural_similarity = None
    decode = runners.ImageRangeMixin.decode
    losses = [klass(reduction='none') for klass in (image_losses.L1Loss, image_losses.MSELoss, image_losses.PSNRLoss, image_losses.SSIMLoss)]
    lines = []
    for B, dtype, layout in SHAPES:
        g = torch.Generator().manual_seed(B)
        image = torch.rand(B, 3, 256, 256, generator=g) * 2 - 1
        pred = (image + 0.1 * torch.randn(B, 3, 256, 256, generator=g)).to(dtype).cuda()
        image = image.to(dtype).cuda()
        if layout == 'channels_last':
            pred, image = (t.contiguous(memory_format=torch.channels_last) for t in (pred, image))

        def fused():
            return ops.image_metrics(pred, image)

        def composed():
            out = []
            for loss in losses:                                                 # as the validation loop: every metric decodes again
                v = loss(decode(pred) / 255, decode(image) / 255)
                out.append(v.reshape(B, -1).mean(1))
            return out

        f, c = fused()['values64'].cpu(), torch.stack([v.double() for v in composed()], 1).cpu()
        assert torch.allclose(f, c, rtol=1e-4, atol=1e-6), (f, c)
        routes = {'torch': composed, 'fused': fused}
        us = {r: [] for r in routes}
        for fn in routes.values():
            block_us(fn, 5)
        for _ in range(args.blocks):
            for r, fn in routes.items():
                us[r].append(block_us(fn, args.iters))
        nbytes = 2 * pred.numel() * pred.element_size()
        rec = dict(B=B, shape=[B, 3, 256, 256], dtype=str(dtype).replace('torch.', ''), layout=layout, blocks=args.blocks, iters=args.iters)
        for r in routes:
            rec[f'{r}_us'] = round(statistics.median(us[r]), 2)
            rec[f'{r}_us_min_max'] = [round(min(us[r]), 2), round(max(us[r]), 2)]
        rec['fused_over_torch'] = round(rec['fused_us'] / rec['torch_us'], 4)
        rec['fused_bytes'] = nbytes
        rec['fused_TB_per_s'] = round(nbytes / (rec['fused_us'] * 1e-6) / 1e12, 3)
        rec['fused_hbm_share'] = round(nbytes / (rec['fused_us'] * 1e-6) / HBM_BYTES_PER_S, 3)
        if structural_similarity is not None:
            t0 = time.perf_counter()
            x, y = (decode(pred) / 255).cpu().numpy(), (decode(image) / 255).cpu().numpy()
            ref = [structural_similarity(a, b, channel_axis=0, data_range=1) for a, b in zip(x, y)]
            rec['skimage_ssim_wall_us'] = round((time.perf_counter() - t0) * 1e6, 1)
            rec['skimage_ssim_max_abs_diff'] = float((torch.tensor(ref, dtype=torch.float64) - f[:, 3]).abs().max())
        else:
            rec['skimage'] = 'not importable'
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
