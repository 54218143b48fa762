"""coarse_kernel<..., XD = 2>: one workgroup per token block streams both codebook halves and decides its own tokens
("One workgroup per token block").

The form is taken for bf16 rows at D = 256 where the default slice count is two and the workgroups, half as many and twice as
long, fill no more rounds of the chip than the two-workgroup form's (vq_one_workgroup in csrc/vqhip.hip): from 129 token blocks
of 512 on.  N = 65 536 + 512 + 37 is just past that gate (130 blocks) and no multiple of 512 or 16: the last block is ragged
and its last tile is partial.  A stage holds 64 codes, so K = 128 is one stage per half, 192 halves of one and two stages, 200
halves of two stages with the second one padded, 1024 halves of eight.

Per case: (1) the indices equal ops.argmin_exact (the all-fp32 route) on every row; (2) indices and the return_stats path
counters equal those of the two-workgroup form (tuning key 2 = 2, restored afterwards); (3) a second run is bit-identical.
Data: planted rows of oracle/synth.py, and oracle/hostile.py's ulp_pairs, whose pairs sit in different halves of the codebook:
multi-candidate rows whose candidates come from both records, and second-pass rows.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import hostile, synth

pytestmark = pytest.mark.gpu

N, D = 65536 + 512 + 37, 256
KS = [128, 192, 200, 1024]
SEED = 20261021


@pytest.fixture(scope='module')
def ops():
    from vector_quantization_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _inputs(kind, K):
    if kind == 'planted':
        x, w = synth.make_inputs('planted', SEED, N, K, D)
    else:
        x, w = hostile.make(kind, SEED, N, K, D)
    return synth.bf16_round(x), w


def _operands(ops, kind, K, metric):
    x, w = _inputs(kind, K)
    xd = torch.from_numpy(x).cuda().to(torch.bfloat16)
    wd = torch.from_numpy(w).cuda()
    if metric == 'Cosine':
        return ops.normalize_rows(xd).to(torch.bfloat16), wd, ops.normalize_rows(wd)
    return xd, wd, wd


@pytest.mark.parametrize('metric', ['L2', 'Cosine'])
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('kind', ['planted', 'ulp_pairs'])
def test_one_workgroup_form(ops, kind, K, metric):
    from vector_quantization_amd import _lib
    L = _lib.lib()
    xq, wd, wq = _operands(ops, kind, K, metric)
    cb = ops.prepare_codebook(wd, metric)
    ref = ops.argmin_exact(xq, wq, metric)
    got, st = ops.argmin(xq, cb, return_stats=True)
    print(f'{kind}/K={K}/{metric}: rescan={int(st[0])} multi={int(st[1])} exact={int(st[2])} of {N}')
    assert torch.equal(got, ref), f'{int((got != ref).sum())} rows differ from the all-fp32 route'
    again, st_again = ops.argmin(xq, cb, return_stats=True)
    assert torch.equal(again, got) and torch.equal(st_again, st), 'a second run differs'
    try:
        assert L.vqhip_set_tuning(2, 2) == 0
        two, st_two = ops.argmin(xq, cb, return_stats=True)
    finally:
        L.vqhip_set_tuning(2, 0)
    assert torch.equal(two, got), f'{int((two != got).sum())} rows differ from the two-workgroup form'
    assert torch.equal(st_two, st), f'path counters {st.tolist()} against the two-workgroup form\'s {st_two.tolist()}'
    if kind == 'ulp_pairs' and metric == 'L2':
        assert int(st[0]) + int(st[1]) >= 1, 'no row left the fast path: the case does not reach the records of both halves'


def test_one_workgroup_form_graph_capture_and_replay(ops):
    """Captured and replayed, then replayed on a new batch in the captured input buffer."""
    K = 200
    x, w = _inputs('planted', K)
    x2 = synth.bf16_round(synth.make_inputs('planted', SEED + 7, N, K, D)[0])
    xd = torch.from_numpy(x).cuda().to(torch.bfloat16)
    wd = torch.from_numpy(w).cuda()
    cb = ops.prepare_codebook(wd, 'L2')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.argmin(xd, cb)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        idx = ops.argmin(xd, cb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, ops.argmin_exact(xd, wd, 'L2'))
    xd.copy_(torch.from_numpy(x2).cuda().to(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, ops.argmin_exact(xd, wd, 'L2'))
