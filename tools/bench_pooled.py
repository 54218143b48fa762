"""The linear probe's features: tokenization.pool_from_quant (one launch, no decoded rows) against the composed route
(quantizer.decode, then the mean over the positions), in the same process.

    python tools/bench_pooled.py [--blocks 7] [--iters 200] [--out FILE]

Shapes (images x positions, codebook): VQGAN 256 x 16x16, K = 16 384, D = 256; VQ-KD 64 x 14x14, K = 8 192, D = 32; LlamaGen
256 x 16x16, K = 16 384, D = 8; FSQ 256 x 16x16, levels [8, 8, 8, 5, 5, 5].  int64 tokens (FSQ: int32, its encode's dtype), eval
mode, no autograd (the tokenizer is frozen under the probe).  Per route: warm-up, then ``blocks`` blocks of ``iters`` calls timed
with device events, the two routes alternating block by block; the figure is the median of the block means.  The bytes each
route needs are computed from the shape (gathered rows once, plus for the composed route the decoded matrix written and read
back).  One JSON line per shape.
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

from vector_quantization_amd import Config, build_quantizer, tokenization as T  # noqa: E402

EMB = 'torch_nn_modules_sparse_Embedding'
FSQ_LEVELS = [8, 8, 8, 5, 5, 5]
# name, images, (H, W), K, D
SHAPES = [('vqgan', 256, (16, 16), 16384, 256), ('vqkd', 64, (14, 14), 8192, 32), ('llamagen', 256, (16, 16), 16384, 8),
          ('fsq', 256, (16, 16), 64000, len(FSQ_LEVELS))]


def make(name, K, D):
    if name == 'fsq':
        cfg = dict(type='FiniteScalarQuantizer', num_scalars_per_channel=list(FSQ_LEVELS))
    else:
        cfg = dict(type='VQGANQuantizer', embedding=dict(type=EMB, num_embeddings=K, embedding_dim=D), distance=dict(type='L2Distance'),
                   losses=dict(vqgan_loss=dict(type='VQGANLoss')))
    q = build_quantizer(cfg)
    q.eval()
    q.init_weights(Config())
    q = q.cuda()
    if name != 'fsq':
        with torch.no_grad():
            q.embedding.weight.copy_(torch.randn(K, D, generator=torch.Generator().manual_seed(K + D)))
    return q


def fused(q, tokens):
    return T.pool_from_quant(q, tokens, {})[0]


def composed(q, tokens):
    z, _ = q.decode(tokens, {})
    return z.mean(dim=(1, 2))


def block_us(fn, q, tokens, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn(q, tokens)
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
        raise SystemExit('bench_pooled.py times kernels: it needs an MI355X')
    routes = {'composed': composed, 'fused': fused}
    lines = []
    with torch.no_grad():
        for name, B, (H, W), K, D in SHAPES:
            q = make(name, K, D)
            tokens = torch.randint(0, K, (B, H, W), generator=torch.Generator().manual_seed(B + K)).cuda()
            if name == 'fsq':
                tokens = tokens.int()
            out = {r: fn(q, tokens) for r, fn in routes.items()}
            assert q.last_route.name == 'pooled', q.last_route
            worst = float((out['fused'] - out['composed']).abs().max())
            us = {r: [] for r in routes}
            for r, fn in routes.items():
                block_us(fn, q, tokens, 5)
            for _ in range(args.blocks):
                for r, fn in routes.items():
                    us[r].append(block_us(fn, q, tokens, args.iters))
            rows = B * H * W * D * 4
            gathered = 0 if name == 'fsq' else rows
            rec = dict(shape=name, images=B, positions=H * W, K=K, D=D, token_dtype=str(tokens.dtype).replace('torch.', ''),
                       blocks=args.blocks, iters=args.iters,
                       fused_bytes=gathered + tokens.numel() * tokens.element_size() + B * D * 4,
                       composed_bytes=gathered + tokens.numel() * tokens.element_size() + 2 * rows + B * D * 4,
                       max_abs_difference=worst)
            for r in routes:
                rec[f'{r}_us'] = round(statistics.median(us[r]), 2)
                rec[f'{r}_us_min_max'] = [round(min(us[r]), 2), round(max(us[r]), 2)]
            rec['fused_over_composed'] = round(rec['fused_us'] / rec['composed_us'], 4)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
