"""MultinomialAnchor: the fused route (LazyDistance.multinomial - HIP kernels on one bounded row-block tile, the [N, K] matrix never
formed) against ``MultinomialAnchor(fused=False)`` - the matrix route: the HIP distance kernel materialises d, then
``d.t().softmax(1).multinomial(1)`` - in the same process on the same GPU.  A call is what CVQVAECallback makes once per training
step: a fresh lazy handle of the step's operands, the anchor module, K anchors out.

    python tools/bench_col_multinomial.py [--blocks 7] [--out FILE]

Shapes (N, K, D, metric): the CVQ-VAE training shape per rank under both metrics, a D = 32 codebook over 12 544 tokens, N = 65 536
(the matrix side is skipped if it does not fit), and two shapes whose whole matrix fits ONE tile (ops.ENTROPY_TILE_BYTES), where
the fused route evaluates the distances once - the only place a routing threshold could apply.  Per route and
shape: warm-up, then ``blocks`` blocks of steps timed with device events (as many steps as fill ~0.1 s), the routes alternating
block by block; the figure is the median of the block means in microseconds, host enqueue included, with the blocks' minimum
and maximum as the run-to-run spread.  Peak memory: ``torch.cuda.max_memory_allocated`` over a call, above what was allocated
before it.  Also records, at the training shape, the worst |share error| / delta of the fused indices under the acceptance rule
of tests/col_multinomial_ref.py.  One JSON line per shape; ``--out`` also writes the lines to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from vector_quantization_amd import ops  # noqa: E402
from vector_quantization_amd import quantizers as Q  # noqa: E402

SHAPES = [(3072, 16384, 256, 'Cosine'), (3072, 16384, 256, 'L2'), (12544, 8192, 32, 'Cosine'), (65536, 16384, 256, 'L2'),
          (1024, 16384, 256, 'Cosine'), (256, 1024, 32, 'L2')]


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def error_record(x, e, dist):
    import col_multinomial_ref as ref
    d = Q.LazyDistance(dist, x, e)
    u = torch.rand(e.shape[0], device='cuda')
    idx = d.multinomial(u)
    xq, eq = d.exact_operands()
    c = ref.check_pick(ops.distance(xq, eq, d.metric).cpu().numpy(), u.cpu().numpy(), idx.cpu().numpy(), ref.delta(x.shape[0]))
    return dict(worst_share_error_over_delta=round(c.worst, 4), columns_failing=int((~c.ok).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_col_multinomial.py times kernels: it needs an MI355X')
    lines = []
    for N, K, D, metric in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(N + K + D)
        x = torch.randn(N, D, device='cuda', generator=g)
        e = torch.randn(K, D, device='cuda', generator=g)
        p = torch.zeros(K, device='cuda')
        dist = Q.L2Distance() if metric == 'L2' else Q.CosineDistance(autocast=None)
        modules = {'fused': Q.MultinomialAnchor(), 'matrix': Q.MultinomialAnchor(fused=False)}

        def call(name):
            m = modules[name]
            return lambda: m(x, e, Q.LazyDistance(dist, x, e), None, p)[0]

        rec = dict(N=N, K=K, D=D, metric=metric, matrix_MiB=round(N * K * 4 / 2 ** 20, 1), one_tile=N * K * 4 <= ops.ENTROPY_TILE_BYTES,
                   block_rows=ops.entropy_block_rows(N, K), blocks=args.blocks)
        routes = {}
        for name in modules:
            try:
                rec[f'{name}_peak_MiB'] = round(peak_bytes(call(name)) / 2 ** 20, 1)
                routes[name] = call(name)
            except torch.OutOfMemoryError:
                rec[f'{name}_peak_MiB'] = None
                rec[f'{name}_skipped'] = 'does not fit'
                torch.cuda.empty_cache()
        assert modules['fused'].last_route.name == 'fused', modules['fused'].last_route
        us, iters = {r: [] for r in routes}, {}
        for r, fn in routes.items():
            block_us(fn, 2)
            iters[r] = max(2, min(200, int(1e5 / block_us(fn, 2))))
        for _ in range(args.blocks):
            for r, fn in routes.items():
                us[r].append(block_us(fn, iters[r]))
        for r in routes:
            rec[f'{r}_us'] = round(statistics.median(us[r]), 1)
            rec[f'{r}_us_min_max'] = [round(min(us[r]), 1), round(max(us[r]), 1)]
            rec[f'{r}_iters'] = iters[r]
        if len(routes) == 2:
            rec['fused_over_matrix'] = round(rec['fused_us'] / rec['matrix_us'], 4)
            # the matrix route is faster by more than the spread only if even its slowest block beats the fused route's fastest
            rec['matrix_faster_beyond_spread'] = max(us['matrix']) < min(us['fused'])
        if (N, K, D) == (3072, 16384, 256):
            rec.update(error_record(x, e, dist))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x, e, routes
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
