"""The D = 256 proposal kernels whose epilogue folds a token tile's eight scores through the max3 / med3 network
(csrc/vqhip_top2.h; DESIGN.md §4.1, "The epilogue as a network").

Three row counts reach the three forms that share the stream loop: N = 4 096 + 21 (token image, decision in the kernel),
16 384 + 512 + 37 (the token side made in the prologue, two workgroups per token block) and 66 085 (one workgroup streams both
codebook halves).  A stage holds 64 codes: K = 128 is one stage per half, 192 halves of one and two stages, 1024 halves of eight.

Data: the planted rows of oracle/synth.py, oracle/hostile.py's ulp_pairs, and a duplicates family built here — code rows copied
to k + 32 (the next code tile), k + 64 (the next stage) and k + K/2 (the other half of the codebook): equal scores that reach
the same lane under the same tag from different tiles; one latent in eight sits on such a code, so best and runner-up are the
same bits; and one all-zero row beside one all-zero code (scores of exactly zero under tag 0).

Per case: (1) the indices equal ops.argmin_exact (the all-fp32 route) on every row; (2) a second run is bit-identical; (3) the
return_stats path counters (second pass, multi-candidate, whole-codebook) equal PARENT_PATHS, recorded from a run of the
parent commit on the same seeded inputs: the records are bitwise the parent's, so every row takes the parent's route; (4) in
the families built for it (ulp_pairs, duplicates) at least one row leaves the single-candidate path — the runner-up the
network computes decides a route there.  (The planted rows all stay on the single-candidate path at these shapes, in the parent
too: they count for the indices and for the counters being zero.)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import hostile, synth

pytestmark = pytest.mark.gpu

D = 256
NS = [4096 + 21, 16384 + 512 + 37, 66085]
KS = [128, 192, 1024]
KINDS = ['planted', 'ulp_pairs', 'duplicates']
SEED = 20261022

# (kind, N, K, metric) -> [second pass, multi-candidate, whole-codebook] of the parent commit
# 9b679c6 "Split the quantizer core of libvqhip into one unit per concern"
PARENT_PATHS = {
    ('planted', 4117, 128, 'L2'): [0, 0, 0],
    ('planted', 4117, 128, 'Cosine'): [0, 0, 0],
    ('planted', 4117, 192, 'L2'): [0, 0, 0],
    ('planted', 4117, 192, 'Cosine'): [0, 0, 0],
    ('planted', 4117, 1024, 'L2'): [0, 0, 0],
    ('planted', 4117, 1024, 'Cosine'): [0, 0, 0],
    ('planted', 16933, 128, 'L2'): [0, 0, 0],
    ('planted', 16933, 128, 'Cosine'): [0, 0, 0],
    ('planted', 16933, 192, 'L2'): [0, 0, 0],
    ('planted', 16933, 192, 'Cosine'): [0, 0, 0],
    ('planted', 16933, 1024, 'L2'): [0, 0, 0],
    ('planted', 16933, 1024, 'Cosine'): [0, 0, 0],
    ('planted', 66085, 128, 'L2'): [0, 0, 0],
    ('planted', 66085, 128, 'Cosine'): [0, 0, 0],
    ('planted', 66085, 192, 'L2'): [0, 0, 0],
    ('planted', 66085, 192, 'Cosine'): [0, 0, 0],
    ('planted', 66085, 1024, 'L2'): [0, 0, 0],
    ('planted', 66085, 1024, 'Cosine'): [0, 0, 0],
    ('ulp_pairs', 4117, 128, 'L2'): [0, 4117, 0],
    ('ulp_pairs', 4117, 128, 'Cosine'): [0, 4117, 0],
    ('ulp_pairs', 4117, 192, 'L2'): [342, 3775, 0],
    ('ulp_pairs', 4117, 192, 'Cosine'): [342, 3775, 0],
    ('ulp_pairs', 4117, 1024, 'L2'): [0, 4117, 0],
    ('ulp_pairs', 4117, 1024, 'Cosine'): [0, 4117, 0],
    ('ulp_pairs', 16933, 128, 'L2'): [0, 16933, 0],
    ('ulp_pairs', 16933, 128, 'Cosine'): [0, 16933, 0],
    ('ulp_pairs', 16933, 192, 'L2'): [1363, 15570, 0],
    ('ulp_pairs', 16933, 192, 'Cosine'): [1363, 15570, 0],
    ('ulp_pairs', 16933, 1024, 'L2'): [0, 16933, 0],
    ('ulp_pairs', 16933, 1024, 'Cosine'): [0, 16933, 0],
    ('ulp_pairs', 66085, 128, 'L2'): [0, 66085, 0],
    ('ulp_pairs', 66085, 128, 'Cosine'): [0, 66085, 0],
    ('ulp_pairs', 66085, 192, 'L2'): [5375, 60710, 0],
    ('ulp_pairs', 66085, 192, 'Cosine'): [5375, 60710, 0],
    ('ulp_pairs', 66085, 1024, 'L2'): [0, 66085, 0],
    ('ulp_pairs', 66085, 1024, 'Cosine'): [0, 66085, 0],
    ('duplicates', 4117, 128, 'L2'): [628, 0, 0],
    ('duplicates', 4117, 128, 'Cosine'): [650, 5, 1],
    ('duplicates', 4117, 192, 'L2'): [595, 0, 0],
    ('duplicates', 4117, 192, 'Cosine'): [605, 9, 1],
    ('duplicates', 4117, 1024, 'L2'): [569, 0, 0],
    ('duplicates', 4117, 1024, 'Cosine'): [573, 2, 1],
    ('duplicates', 16933, 128, 'L2'): [2580, 0, 0],
    ('duplicates', 16933, 128, 'Cosine'): [2660, 19, 1],
    ('duplicates', 16933, 192, 'L2'): [2400, 0, 0],
    ('duplicates', 16933, 192, 'Cosine'): [2447, 24, 1],
    ('duplicates', 16933, 1024, 'L2'): [2329, 0, 0],
    ('duplicates', 16933, 1024, 'Cosine'): [2335, 17, 1],
    ('duplicates', 66085, 128, 'L2'): [10106, 0, 0],
    ('duplicates', 66085, 128, 'Cosine'): [10371, 74, 1],
    ('duplicates', 66085, 192, 'L2'): [9475, 0, 0],
    ('duplicates', 66085, 192, 'Cosine'): [9650, 84, 1],
    ('duplicates', 66085, 1024, 'L2'): [9179, 0, 0],
    ('duplicates', 66085, 1024, 'Cosine'): [9204, 80, 1],
}


def duplicates(seed, N, K):
    """planted rows on a codebook with exact copies (see the module text)"""
    x, w = synth.make_inputs('planted', seed, N, K, D)
    x, w = x.copy(), w.copy()
    bases = [k for k in range(0, K // 2, 8) if k % 128 < 32 and k + 64 < K]
    assert bases
    for k in bases:
        for off in (32, 64, K // 2):
            w[k + off] = w[k]
    r = synth.rng(seed + 1)
    rows = np.arange(3, N, 8)
    x[rows] = w[r.choice(np.asarray(bases), size=rows.size)]
    zero_code = 97                       # no base and no copy at any K of this file
    w[zero_code] = 0.0
    x[5] = 0.0
    return x, w


@functools.lru_cache(maxsize=None)
def _inputs(kind, N, K):
    if kind == 'planted':
        x, w = synth.make_inputs('planted', SEED, N, K, D)
    elif kind == 'duplicates':
        x, w = duplicates(SEED, N, K)
    else:
        x, w = hostile.make(kind, SEED, N, K, D)
    return synth.bf16_round(x), w


def run_case(ops, kind, N, K, metric):
    """indices, path counters, the all-fp32 route's indices, and the second run's pair"""
    x, w = _inputs(kind, N, K)
    xd = torch.from_numpy(x).cuda().to(torch.bfloat16)
    wd = torch.from_numpy(w).cuda()
    xq, wq = (ops.normalize_rows(xd).to(torch.bfloat16), ops.normalize_rows(wd)) if metric == 'Cosine' else (xd, wd)
    cb = ops.prepare_codebook(wd, metric)
    ref = ops.argmin_exact(xq, wq, metric)
    got, st = ops.argmin(xq, cb, return_stats=True)
    again, st_again = ops.argmin(xq, cb, return_stats=True)
    return got, st, ref, again, st_again


@pytest.fixture(scope='module')
def ops():
    from vector_quantization_amd import ops as _ops
    return _ops


@pytest.mark.parametrize('metric', ['L2', 'Cosine'])
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('kind', KINDS)
def test_network_epilogue_keeps_indices_and_routes(ops, kind, N, K, metric):
    got, st, ref, again, st_again = run_case(ops, kind, N, K, metric)
    paths = [int(v) for v in st[:3]]
    print(f'{kind}/N={N}/K={K}/{metric}: rescan={paths[0]} multi={paths[1]} exact={paths[2]} of {N}')
    assert torch.equal(got, ref), f'{int((got != ref).sum())} rows differ from the all-fp32 route'
    assert torch.equal(again, got) and torch.equal(st_again, st), 'a second run differs'
    assert paths == PARENT_PATHS[(kind, N, K, metric)], 'the rows do not take the parent commit\'s routes'
    if kind in ('duplicates', 'ulp_pairs'):
        assert sum(paths) >= 1, 'no row left the single-candidate path: the case does not reach the runner-up'
