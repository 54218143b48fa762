"""The alignment, stream and capture clauses of include/vqhip.h for vqhip_decode_attention and vqhip_rope_append: entries like those
of tests/contract_cases.py, run through the property functions of tests/test_gpu_op_contracts.py as they are - q, k, v, cos, sin and
the output at element offsets 1 and 3 past a 16-byte boundary (served: they are read and written element by element), a side
stream, capture and replay, each to the same bits.  ``seen`` is passed by value, so a replay recomputes the same position: on the
same contents it must give the same bits, stored key and value included.  The caches are read 16 bytes at a time: a cache one
element off a boundary is refused by name (tests/test_gpu_decode_attention.py holds that clause with the other limits).

(tests/contract_cases.py finds entry points by a parameter called ``stream``; these two call theirs ``hip_stream`` and are held
here instead - tests/test_decode_attention_cpu.py checks that ``CASES`` below reaches both.)"""
import pytest
import torch

from vector_quantization_amd import _lib, ops

import contract_cases as table
import test_gpu_op_contracts as contracts
from test_gpu_decode_attention import problem

pytestmark = pytest.mark.gpu

P, S, CODE, NAME = table.P, table.S, table.CODE, table.NAME
CLAUSE = 'sin and the output are read and written element by element and need the alignment of their element type only'
# GQA 4:1 past one sweep per wave; fewer positions than waves at the widest head
SHAPES = [(3, 8, 2, 64, 70, 73), (2, 2, 1, 128, 5, 8)]
NAMES = ('q', 'k', 'v', 'cos', 'sin', 'store')


def _case(shape, dtype, packed, L, stored):
    B, Hq, Hkv, Dh, seen, cap = shape
    decode = L == 1

    def make(seed):
        p = problem(shape, dtype, packed, seed=seed, L=L)
        return {n: p[n] for n in NAMES}

    def run(a):
        kc, vc = a['store'][0, 0], a['store'][0, 1]
        if decode:
            return ops.decode_attention(a['q'], a['k'], a['v'], a['cos'], a['sin'], kc, vc, seen), kc, vc
        return ops.rope_append(a['q'], a['k'], a['v'], a['cos'], a['sin'], kc, vc, seen), kc, vc

    def call(a):
        out, kc, vc = run(a)
        return (out, kc[:, :, seen:seen + L].clone(), vc[:, :, seen:seen + L].clone()) if stored else (out,)

    def outs(a):
        return [table.flat((B, Hq * Dh) if decode else (B, Hq, L, Dh), dtype)]

    def call_abi(a, o):
        kc, vc = a['store'][0, 0], a['store'][0, 1]
        head = (P(a['q']), a['q'].stride(0), P(a['k']), a['k'].stride(0), P(a['v']), a['v'].stride(0), CODE[dtype], P(a['cos']), P(a['sin']),
                P(kc), P(vc), seen, cap)
        if decode:
            _lib.check(_lib.lib().vqhip_decode_attention(*head, Dh ** -0.5, B, Hq, Hkv, Dh, P(o[0]), S()), 'vqhip_decode_attention')
        else:
            _lib.check(_lib.lib().vqhip_rope_append(*head, B, L, Hq, Hkv, Dh, P(o[0]), S()), 'vqhip_rope_append')

    name = 'decode_attention' if decode else 'rope_append'
    return table.Case(id=f'{name}{"-stored" if stored else ""}-{"x".join(map(str, shape))}-{NAME[dtype]}-{"packed" if packed else "separate"}',
                      family='attention', abi=(f'vqhip_{name}',), clause=CLAUSE, make=make, call=call,
                      free=() if stored else ('q', 'k', 'v', 'cos', 'sin'), outs=None if stored else outs,
                      call_abi=None if stored else call_abi)


CASES = [_case(shape, dtype, packed, L, stored) for shape in SHAPES for dtype in table.DTYPES for packed in (False, True)
         for L in (1, 3) for stored in (False, True) if not (L == 3 and shape[4] + 3 > shape[5])]
PLACED = [c for c in CASES if c.call_abi is not None]


def test_the_quoted_clause_stands_in_the_header():
    with open(_lib.HEADER_PATH) as f:
        words = ' '.join(f.read().replace('*', ' ').split())
    assert ' '.join(CLAUSE.split()) in words


@pytest.mark.parametrize('case', PLACED, ids=lambda c: c.id)
def test_placement(case):
    contracts.test_placement(case)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_side_stream(case):
    contracts.test_side_stream(case)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_capture_and_replay(case):
    contracts.test_capture_and_replay(case)


def test_a_replayed_step_rewrites_the_same_position_with_the_same_bits():
    """One decode step captured and replayed three times on unchanged inputs: ``seen`` is by value, every replay recomputes that
    position, and out, the stored key and the stored value keep their bits."""
    shape = SHAPES[0]
    seen = shape[4]
    a = problem(shape, torch.bfloat16, True)
    want = ops.decode_attention(a['q'], a['k'], a['v'], a['cos'], a['sin'], a['kc'], a['vc'], seen).clone()
    stored = a['store'].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = ops.decode_attention(a['q'], a['k'], a['v'], a['cos'], a['sin'], a['kc'], a['vc'], seen)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        contracts.same_bits([got, a['store']], [want, stored], 'a replayed decode step')
