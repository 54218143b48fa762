"""The CPU twin of tests/test_gpu_decode_attention_geometry.py: what that file takes for granted about its own inputs is settled
here, without a GPU.  The geometry helpers against a literal table; the power condition of the matrix (losing one position leaves
the bound) on the very inputs the GPU test draws; the probe construction of the full length against its own reference assertions;
and the package's torch restatement through the same ``check_out`` / ``check_storage``, so inputs and bounds are satisfiable."""
import pytest
import torch

from vector_quantization_amd import functional
from vector_quantization_amd.kv_cache import StaticKVCache

import decode_attention_ref as ref
from test_gpu_decode_attention import check_out, check_storage

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
HEAD_DIMS = [16, 24, 40, 64, 80, 96, 120, 128]
# (E, C, LP, PP, sweep), by hand from the kernel's comment
TABLE = {
    (16, 4): (4, 4, 4, 16, 64), (24, 4): (4, 6, 8, 8, 32), (40, 4): (4, 10, 16, 4, 16), (64, 4): (4, 16, 16, 4, 16),
    (80, 4): (4, 20, 32, 2, 8), (96, 4): (4, 24, 32, 2, 8), (120, 4): (4, 30, 32, 2, 8), (128, 4): (4, 32, 32, 2, 8),
    (16, 2): (8, 2, 2, 32, 128), (24, 2): (8, 3, 4, 16, 64), (40, 2): (8, 5, 8, 8, 32), (64, 2): (8, 8, 8, 8, 32),
    (80, 2): (8, 10, 16, 4, 16), (96, 2): (8, 12, 16, 4, 16), (120, 2): (8, 15, 16, 4, 16), (128, 2): (8, 16, 16, 4, 16),
}
EDGES = {
    2: [1, 2, 3, 7, 8, 9, 17, 27], 4: [1, 4, 5, 13, 15, 16, 17, 33, 53], 8: [1, 8, 9, 25, 31, 32, 33, 65, 105],
    16: [1, 16, 17, 49, 63, 64, 65, 129, 209], 32: [1, 32, 33, 97, 127, 128, 129, 257, 417],
}


def cache_of(store):
    """A one-layer StaticKVCache whose K and V are ``store[0]`` of a problem's [2, 2, B, Hkv, cap, Dh]"""
    cache = StaticKVCache(1, 1, 1, 1, 16, store.dtype, 'cpu')
    cache._store = store[0:1]
    return cache


def check_storage_of_the_restatement(p, before, shape, dtype, L):
    """``check_storage`` for the torch restatement.  Its rotary is plain fp32 - fl(fl(x cos) + fl(y sin)), three roundings where the
    kernel's compensated one has one - so at an element whose two products cancel it misses the one-ulp rule (by 9.6 ulps on the
    first case of the matrix).  Its k' is therefore held to what those roundings allow, 2 u (|x cos| + |y sin|) more, and every
    other clause to ``check_storage`` itself, on a copy of the cache with the correctly rounded k' in place of it."""
    B, Hq, Hkv, Dh, seen, cap = shape
    k, cos, sin = p['k'].reshape(B, L, Hkv, Dh).to(F64), p['cos'].reshape(1, L, 1, Dh).to(F64), p['sin'].reshape(1, L, 1, Dh).to(F64)
    want = ref.rope64(k, cos, sin).transpose(1, 2)
    products = ((k * cos).abs() + (torch.cat((k[..., Dh // 2:], k[..., :Dh // 2]), -1) * sin).abs()).transpose(1, 2)
    got = p['kc'][:, :, seen:seen + L].to(F64)
    assert bool(((got - want).abs() <= ref.ulp(want, dtype) + 2.0 * ref.U * products).all())
    store = p['store'].clone()
    store[0, 0, :, :, seen:seen + L] = want.to(dtype)
    check_storage(dict(p, store=store, kc=store[0, 0], vc=store[0, 1]), before, shape, dtype, L)


def test_geometry_and_edge_lengths_are_the_table():
    for (Dh, size), want in TABLE.items():
        for dtype in DTYPES:
            if torch.empty((), dtype=dtype).element_size() == size:
                assert ref.geometry(Dh, dtype) == want, (Dh, dtype)
                assert ref.edge_lengths(Dh, dtype) == EDGES[want[3]], (Dh, dtype)
    assert max(max(ref.edge_lengths(Dh, dtype)) for Dh in HEAD_DIMS for dtype in DTYPES) == 417


def test_the_grouped_reference_is_attend64_and_a_dropped_position_is_its_weight():
    gen = torch.Generator().manual_seed(3)
    q, keys, values = torch.randn(2, 6, 24, generator=gen), torch.randn(2, 2, 11, 24, generator=gen), torch.randn(2, 2, 11, 24, generator=gen)
    out, A, vmax = ref.attend64(q, keys, values, 0.2)
    got = ref.attend64_grouped(q, keys, values, 0.2)
    for a, b in zip((out, A, vmax), got):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-13
    weight = torch.softmax(got[3], -1)                                           # out' - out = p_j (out - v_j) / (1 - p_j)
    for j in (0, 4, 10):
        v_j = values[:, :, j].to(F64).repeat_interleave(3, dim=1)
        want = weight[..., j, None] * (out - v_j) / (1.0 - weight[..., j, None])
        assert float((ref.drop_one_shift(q, keys, values, 0.2, j) - want).abs().max()) <= 1e-13
    assert torch.equal(ref.drop_one_shift(q, keys[:, :, :1], values[:, :, :1], 0.2, 0), -ref.attend64_grouped(q, keys[:, :, :1], values[:, :, :1], 0.2)[0])


@pytest.mark.parametrize('Dh', HEAD_DIMS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_matrix_is_satisfiable_and_can_see_one_position(dtype, Dh):
    """Every case of the GPU matrix on its own inputs: the torch restatement passes ``check_out`` and ``check_storage`` (but see
    ``check_storage_of_the_restatement``), and on
    the cache it leaves, removing any one of the watched positions moves every head by more than twice its bound."""
    PP, scale = ref.geometry(Dh, dtype)[3], Dh ** -0.5
    weakest = (float('inf'), (0, 0))
    for G in range(1, 9):
        for n in ref.edge_lengths(Dh, dtype):
            shape = ref.matrix_shape(Dh, G, n)
            p = ref.host_problem(shape, dtype, seed=ref.matrix_seed(G, n), amp=ref.MATRIX_AMP)
            before = p['store'].clone()
            cache = cache_of(p['store'])
            cache._seen = n - 1
            out = functional.decode_attention_torch(p['q'], p['k'], p['v'], p['cos'], p['sin'], cache, 0, scale=scale)
            check_storage_of_the_restatement(p, before, shape, dtype, 1)
            check_out(p, out, shape, dtype, scale)
            q_rot = ref.rope64(p['q'].reshape(2, 2 * G, Dh), p['cos'].reshape(1, 1, Dh), p['sin'].reshape(1, 1, Dh))
            weakest = min(weakest, (ref.power_ratio(q_rot, p['kc'][:, :, :n], p['vc'][:, :, :n], scale, dtype, PP), (G, n)))
    print(f'{dtype} Dh={Dh}: weakest drop-one shift / (2 bound) {weakest[0]:.1f} at (G, n) = {weakest[1]}')
    assert weakest[0] > 1.0, weakest


def stored_key_torch(q, k, v, cos, sin):
    B, Dh = q.shape[0], cos.shape[-1]
    cache = StaticKVCache(1, B, k.shape[1] // Dh, 1, Dh, q.dtype, 'cpu')
    functional.decode_attention_torch(q, k, v, cos, sin, cache, 0)
    return cache.layer(0)[0][:, :, 0].clone()


@pytest.mark.parametrize('n', [4096, 4095])
@pytest.mark.parametrize('Dh,G', [(16, 8), (128, 8), (120, 5), (64, 3)])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_probes_satisfy_their_own_reference(dtype, Dh, G, n):
    scale = Dh ** -0.5
    p, pairs = ref.probe_problem(Dh, G, dtype, n, 4096, stored_key_torch)
    _, _, _, PP, sweep = ref.geometry(Dh, dtype)
    covered = {j for pair in pairs for j in pair}
    assert {0, PP - 1, PP, sweep - 1, sweep, n - sweep, n - 2, n - 1} <= covered and pairs[-1] == (0, n - 1) and len(pairs) == p['q'].shape[0]
    slot = lambda j: ((j % sweep) // PP, j % PP)                                 # noqa: E731  (wave, slot) of a position
    assert any(slot(a) == slot(b) for a, b in pairs) and any(slot(a)[0] != slot(b)[0] for a, b in pairs)
    shape = (len(pairs), 2 * G, 2, Dh, n - 1, 4096)
    before = p['store'].clone()
    cache = cache_of(p['store'])
    cache._seen = n - 1
    out = functional.decode_attention_torch(p['q'], p['k'], p['v'], p['cos'], p['sin'], cache, 0, scale=scale)
    check_storage_of_the_restatement(p, before, shape, dtype, 1)
    want, bound = ref.probe_expectation(p, pairs, n, scale, dtype)
    assert bool(((out.to(F64).reshape(want.shape) - want).abs() <= bound).all())


@pytest.mark.parametrize('heads', [(1, 1, 16), (6, 2, 24), (8, 1, 80), (16, 2, 128), (3, 3, 120)], ids=lambda h: 'x'.join(map(str, h)))
def test_rope_append_torch_on_the_cases_of_the_gpu_test(heads):
    Hq, Hkv, Dh = heads
    for seen, L, cap in ((0, 1, 1), (0, 7, 7), (3, 5, 8), (2, 300, 302)):
        shape = (2, Hq, Hkv, Dh, seen, cap)
        p = ref.host_problem(shape, torch.float32, seed=L, L=L)
        before = p['store'].clone()
        cache = cache_of(p['store'])
        cache._seen = seen
        q_rot = functional.rope_append_torch(p['q'], p['k'], p['v'], p['cos'], p['sin'], cache, 0)
        assert q_rot.shape == (2, Hq, L, Dh) and q_rot.dtype == torch.float32 and q_rot.is_contiguous()
        check_storage_of_the_restatement(p, before, shape, torch.float32, L)
