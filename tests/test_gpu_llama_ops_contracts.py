"""The alignment, stream and capture clauses of include/vqhip.h for the two modes LlamaTransformer runs on - the RMS mode of
vqhip_add_layer_norm_* (beta / dbeta NULL) and act 3, SwiGLU, of vqhip_row_bias_act_*: entries like those of
tests/contract_cases.py (the ViT rows' shapes, the five dtype rows of the norm and three dtypes of SwiGLU, forward and backward),
run through the property functions of tests/test_gpu_op_contracts.py as they are - placement at element offsets 1 and 3, a side
stream, capture and replay, each to the same bits."""
import pytest
import torch

from vector_quantization_amd import _lib, ops

import contract_cases as table
import test_gpu_op_contracts as contracts

pytestmark = pytest.mark.gpu

# a wave per row with pieces of 8 / 4; single elements either side of nothing; a workgroup per row; the widest row.  SwiGLU reads
# them as F: (5, 12) has pieces that cross a row end in the 16-bit dtypes, (3, 2051) in every dtype
NORM_SHAPES = table.VIT_SHAPES
SWIGLU_SHAPES = ((5, 12), (3, 2051), (3, 2052), (2, 8192))
EPS = 1e-5
F32, P, S, CODE, NAME = table.F32, table.P, table.S, table.CODE, table.NAME


def _rms(shape, xd, yd, with_res, backward):
    R, D = shape

    def make(seed):
        gen = table._gen(seed)
        a = dict(x=table._randn(gen, shape, xd), gamma=torch.randn(D, generator=gen).cuda())
        if with_res:
            a['res'] = table._randn(gen, shape, yd)
        if backward:
            a['g'] = table._randn(gen, shape, yd)
            a['g_skip'] = table._randn(gen, shape, xd)
        return a

    def forward(a):
        return ops.add_rms_norm(a['x'], a.get('res'), a['gamma'], EPS, yd)

    if not backward:
        def call(a):
            s, y, stats = forward(a)
            return (s, y, stats) if with_res else (y, stats)

        def outs(a):
            o = [table.flat(shape, yd), table.flat((R, 2), F32)]
            return [table.flat(shape, xd)] + o if with_res else o

        def call_abi(a, o):
            s = o[0] if with_res else None
            y, stats = o[-2], o[-1]
            _lib.check(_lib.lib().vqhip_add_layer_norm_fwd(P(a['x']), CODE[xd], P(a.get('res')), CODE[yd], R, D, P(a['gamma']), None,
                                                           EPS, P(s), P(y), CODE[yd], P(stats), S()), 'vqhip_add_layer_norm_fwd')
        abi, free = ('vqhip_add_layer_norm_fwd',), ('x', 'res', 'gamma')
    else:
        def call(a):
            s, _, stats = forward(a)
            return ops.add_rms_norm_backward(a['g'], s, table.saved(stats), a['gamma'], a['g_skip'])

        def outs(a):
            return [table.flat(shape, xd), table.flat((D,), F32)]

        def call_abi(a, o):
            s, _, stats = forward(a)
            L = _lib.lib()
            ws = torch.empty(2 * L.vqhip_add_layer_norm_slabs(R, D) * D, dtype=F32, device='cuda')
            _lib.check(L.vqhip_add_layer_norm_bwd(P(a['g']), CODE[yd], P(s), CODE[xd], P(a['g_skip']), R, D, P(a['gamma']),
                                                  P(table.saved(stats)), P(o[0]), P(o[1]), None, P(ws), ws.numel() * 4, S()),
                       'vqhip_add_layer_norm_bwd')
        abi, free = ('vqhip_add_layer_norm_fwd', 'vqhip_add_layer_norm_bwd'), ('x', 'res', 'gamma', 'g', 'g_skip')
    return table.Case(id=f'add_rms_norm{"_backward" if backward else ""}-{R}x{D}-{NAME[xd]}-{NAME[yd]}-{"res" if with_res else "nores"}',
                      family='vit_rows', abi=abi, clause=table.CLAUSE['vit'], make=make, call=call,
                      free=tuple(n for n in free if with_res or n != 'res'), outs=outs, call_abi=call_abi)


def _swiglu(shape, dtype, backward):
    R, F = shape

    def make(seed):
        gen = table._gen(seed)
        a = dict(x=table._randn(gen, (R, 2 * F), dtype, scale=2.0))
        if backward:
            a['g'] = table._randn(gen, shape, dtype)
        return a

    if not backward:
        def call(a):
            return (ops.swiglu(a['x']),)

        def outs(a):
            return [table.flat(shape, dtype)]

        def call_abi(a, o):
            _lib.check(_lib.lib().vqhip_row_bias_act_fwd(P(a['x']), CODE[dtype], R, F, None, _lib.ROW_ACT_SWIGLU, P(o[0]), S()),
                       'vqhip_row_bias_act_fwd')
        abi, free = ('vqhip_row_bias_act_fwd',), ('x',)
    else:
        def call(a):
            return (ops.swiglu_backward(a['g'], a['x']),)

        def outs(a):
            return [table.flat((R, 2 * F), dtype)]

        def call_abi(a, o):
            _lib.check(_lib.lib().vqhip_row_bias_act_bwd(P(a['g']), P(a['x']), CODE[dtype], R, F, None, _lib.ROW_ACT_SWIGLU, P(o[0]), None,
                                                         None, 0, S()), 'vqhip_row_bias_act_bwd')
        abi, free = ('vqhip_row_bias_act_bwd',), ('x', 'g')
    return table.Case(id=f'swiglu{"_backward" if backward else ""}-{R}x{F}-{NAME[dtype]}', family='vit_rows', abi=abi,
                      clause=table.CLAUSE['vit'], make=make, call=call, free=free, outs=outs, call_abi=call_abi)


CASES = [_rms(shape, xd, yd, res, backward) for shape in NORM_SHAPES for xd, yd in table.LN_PAIRS
         for res in ((True, False) if shape in ((5, 24), (2, 8192)) else (True,)) for backward in (False, True)] \
    + [_swiglu(shape, dtype, backward) for shape in SWIGLU_SHAPES for dtype in table.DTYPES for backward in (False, True)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_placement(case):
    contracts.test_placement(case)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_side_stream(case):
    contracts.test_side_stream(case)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_capture_and_replay(case):
    contracts.test_capture_and_replay(case)
