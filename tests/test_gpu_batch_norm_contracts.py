"""The alignment, stream and capture clauses of include/vqhip.h for the batch-statistics mode of vqhip_group_norm_*: entries like
those of tests/contract_cases.py (one small shape per launch form, three dtypes, both layouts, forward and backward), run through
the property functions of tests/test_gpu_op_contracts.py as they are - placement at element offsets 1 and 3, a side stream,
capture and replay, each to the same bits - and one capture of ``functional.batch_norm`` through autograd with the update of the
running statistics inside the graph."""
import pytest
import torch

from vector_quantization_amd import _lib, functional, ops

import contract_cases as table
import test_gpu_op_contracts as contracts

pytestmark = pytest.mark.gpu

# one launch in both layouts; split in channels-last only (16- and 8-byte pieces); split in both (single-element pieces, ragged)
SHAPES = ((3, 5, 7, 7), (2, 16, 15, 10), (5, 3, 293, 7))
EPS, ACT = 1e-5, 'leaky_relu'
F32, P, S = table.F32, table.P, table.S


def _case(shape, dtype, nhwc, backward):
    B, C = shape[:2]
    Px = shape[2] * shape[3]

    def make(seed):
        gen = table._gen(seed)
        a = dict(x=table._randn(gen, shape, dtype, nhwc), gamma=torch.randn(C, generator=gen).cuda(), beta=torch.randn(C, generator=gen).cuda())
        if backward:
            a['g'] = table._randn(gen, shape, dtype, nhwc)
        return a

    def ws_of(a):
        n = _lib.lib().vqhip_group_norm_ws_bytes(table._layout_code(a['x']), B, C, Px, _lib.GN_BATCH)
        return torch.empty(n // 4, dtype=F32, device='cuda'), n

    if not backward:
        def call(a):
            y, stats, mean, var = ops.batch_norm(a['x'], a['gamma'], a['beta'], EPS, ACT)
            return y, stats, torch.cat([mean, var])

        def outs(a):
            return [table.like(a['x']), table.flat((C, 2), F32)]

        def call_abi(a, o):
            x = a['x']
            ws, n = ws_of(a)
            _lib.check(_lib.lib().vqhip_group_norm_fwd(P(x), table.CODE[dtype], table._layout_code(x), B, C, Px, _lib.GN_BATCH, P(a['gamma']),
                                                       P(a['beta']), EPS, _lib.GN_ACT_LEAKY, P(o[0]), P(o[1]), P(ws), n, S()),
                       'vqhip_group_norm_fwd')
        abi, free = ('vqhip_group_norm_fwd',), ('x', 'gamma', 'beta')
    else:
        def call(a):
            _, stats, _, _ = ops.batch_norm(a['x'], a['gamma'], a['beta'], EPS, ACT)
            return ops.batch_norm_backward(a['g'], a['x'], table.saved(stats), a['gamma'], a['beta'], ACT)

        def outs(a):
            return [table.like(a['x']), table.flat((C,), F32), table.flat((C,), F32)]

        def call_abi(a, o):
            x = a['x']
            _, stats, _, _ = ops.batch_norm(x, a['gamma'], a['beta'], EPS, ACT)
            ws, n = ws_of(a)
            _lib.check(_lib.lib().vqhip_group_norm_bwd(P(a['g']), P(x), table.CODE[dtype], table._layout_code(x), B, C, Px, _lib.GN_BATCH,
                                                       P(a['gamma']), P(a['beta']), P(table.saved(stats)), _lib.GN_ACT_LEAKY, P(o[0]), P(o[1]),
                                                       P(o[2]), P(ws), n, S()), 'vqhip_group_norm_bwd')
        abi, free = ('vqhip_group_norm_fwd', 'vqhip_group_norm_bwd'), ('x', 'gamma', 'beta', 'g')
    return table.Case(id=f'batch_norm{"_backward" if backward else ""}-{"x".join(map(str, shape))}-{table._lay(nhwc)}-{table.NAME[dtype]}',
                      family='group_norm', abi=abi, clause=table.CLAUSE['group_norm'], make=make, call=call, free=free, outs=outs,
                      call_abi=call_abi)


CASES = [_case(shape, dtype, nhwc, backward) for shape in SHAPES for dtype in table.DTYPES for nhwc in (False, True)
         for backward in (False, True)]


class _PlacedForward:
    """The forward entry for the placement property: its third result, the block, is no placed output (it lies in ws)."""

    def __init__(self, case):
        self.case = case

    def __getattr__(self, name):
        return getattr(self.case, name)

    def call(self, a):
        return self.case.call(a)[:2]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_placement(case):
    contracts.test_placement(_PlacedForward(case) if len(case.abi) == 1 else case)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_side_stream(case):
    contracts.test_side_stream(case)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_capture_and_replay(case):
    contracts.test_capture_and_replay(case)


def test_functional_batch_norm_through_autograd_in_one_capture():
    """Forward, the running-statistics update and the backward in one graph: a replay on new contents gives the bits of the eager
    calls, and k replays advance the counter by k."""
    shape, C = (5, 3, 293, 7), 3
    gen = torch.Generator().manual_seed(21)
    make = lambda: dict(x=torch.randn(shape, generator=gen).cuda(), g=torch.randn(shape, generator=gen).cuda())
    w, b = torch.randn(C, generator=gen).cuda().requires_grad_(), torch.randn(C, generator=gen).cuda().requires_grad_()
    rm, rv, count = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda'), torch.zeros((), dtype=torch.long, device='cuda')

    def call(a):
        x = a['x'].detach().requires_grad_()
        y = functional.batch_norm(x, rm, rv, w, b, True, 0.1, EPS, ACT, count)
        return (y,) + torch.autograd.grad(y, (x, w, b), a['g'])

    static, new = make(), make()
    state = lambda: (rm.clone(), rv.clone(), count.clone())
    graph, got = contracts.capture_and_replay(call, static, new)                # (three warm-ups, the capture, one replay)
    after = state()
    assert int(count) == 4, int(count)                                          # a capture runs nothing
    for t, v in zip((rm, rv, count), (torch.zeros(C), torch.ones(C), torch.zeros((), dtype=torch.long))):
        t.copy_(v)
    want = call(new)
    contracts.same_bits(got, want, 'functional.batch_norm replayed on new contents')
    for k in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(count) == 1 + 3 and torch.isfinite(rm).all() and torch.isfinite(rv).all() and after[0].shape == rm.shape
