"""decode_attention_kernel at every lane geometry and group size, against the float64 restatement and the bounds of
tests/decode_attention_ref.py, by the method of tests/test_gpu_decode_attention.py (its ``problem``, ``check_storage`` and
``check_out``): the kernel's control flow is a function of (element size, Dh, G, length) - LP lanes per position, idle lanes where
Dh / E is no power of two, PP positions per wave, a sweep of 4 PP with the next one prefetched, GMAX in {1, 2, 4, 8} with G <= GMAX -
and the matrix below runs each (dtype, Dh) at G = 1 .. 8 and at every length at which that geometry's flow changes.

  a, b  the matrix; and, from the reference alone, that losing one position would leave the bound (the power condition)
  c     the full length of 4096 and 4095 by probes: two positions with one key whose value rows the output must average
  d     ``decode_attention_at`` bit for bit the by-value kernel across the matrix (``table_stride`` at every Dh)
  e     ``rope_append`` off its one shape
  f     the tiny model at Dh = 24 with eight query heads on one kv head, by the yardstick of tests/test_gpu_llama_static_cache.py
"""
import copy

import pytest
import torch

from vector_quantization_amd import ops
from vector_quantization_amd.kv_cache import StaticKVCache
from vector_quantization_amd.quantizers import routes

import decode_attention_ref as ref
from llama_models import build_tiny, exact64
from test_gpu_decode_attention import DTYPES, IDS, bits, check_out, check_storage, problem, tables
from test_gpu_llama_static_cache import PREFILL_THEN_STEPS, TOKENS, cached_error

pytestmark = pytest.mark.gpu

F64 = torch.float64
HEAD_DIMS = [16, 24, 40, 64, 80, 96, 120, 128]
GROUPS = range(1, 9)


def reference_of(p, shape, dtype, scale):
    """(q' in float64, the float64 output on the cache as stored, its bound)"""
    B, Hq, Hkv, Dh, seen, cap = shape
    q_rot = ref.rope64(p['q'].reshape(B, Hq, Dh).cpu(), p['cos'].cpu().reshape(1, 1, Dh), p['sin'].cpu().reshape(1, 1, Dh))
    want, A, vmax, _ = ref.attend64_grouped(q_rot, p['kc'][:, :, :seen + 1].cpu(), p['vc'][:, :, :seen + 1].cpu(), scale)
    return q_rot, want, ref.out_bound(seen + 1, scale, A[..., None], vmax[..., None], want.abs(), dtype)


@pytest.mark.parametrize('Dh', HEAD_DIMS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_every_group_size_at_every_edge_length(dtype, Dh):
    """(a) storage and ``out`` per launch; (b) the power condition on the same inputs.  Every launch runs; the failures are
    listed together."""
    PP, scale = ref.geometry(Dh, dtype)[3], Dh ** -0.5
    failed, worst, weakest = [], (-1.0, (0, 0)), (float('inf'), (0, 0))
    for G in GROUPS:
        for n in ref.edge_lengths(Dh, dtype):
            shape = ref.matrix_shape(Dh, G, n)
            p = problem(shape, dtype, True, seed=ref.matrix_seed(G, n), amp=ref.MATRIX_AMP)
            host = ref.host_problem(shape, dtype, seed=ref.matrix_seed(G, n), amp=ref.MATRIX_AMP)
            assert all(torch.equal(bits(p[name].cpu()), bits(host[name])) for name in ('q', 'k', 'v', 'cos', 'sin', 'store')), \
                'the CPU twin of these inputs has drifted'
            before = p['store'].clone()
            out = ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], n - 1)
            q_rot, want, bound = reference_of(p, shape, dtype, scale)
            ratio = float(((out.cpu().to(F64).reshape(want.shape) - want).abs() / bound).max())
            worst = max(worst, (ratio, (G, n)))
            power = ref.power_ratio(q_rot, p['kc'][:, :, :n].cpu(), p['vc'][:, :, :n].cpu(), scale, dtype, PP)
            weakest = min(weakest, (power, (G, n)))
            try:
                check_storage(p, before, shape, dtype, 1)
                check_out(p, out, shape, dtype, scale)
            except AssertionError as e:
                failed.append((G, n, f'{ratio:.3g}', str(e)[:80]))
    print(f'GEOMETRY {dtype} Dh={Dh}: worst error / bound {worst[0]:.3f} at (G, n) = {worst[1]}; '
          f'weakest drop-one shift / (2 bound) {weakest[0]:.1f} at {weakest[1]}')
    print(f'GEOMETRY {dtype} Dh={Dh}: failing lengths {sorted({n for _, n, _, _ in failed})} of {ref.edge_lengths(Dh, dtype)}')
    assert weakest[0] > 1.0, weakest
    assert not failed, failed


FULL = 4096


def stored_key(q, k, v, cos, sin):
    """k' as the kernel stores it for these rows: one launch into a cache of one position"""
    B, Dh = q.shape[0], cos.shape[-1]
    kc = torch.zeros(B, k.shape[1] // Dh, 1, Dh, dtype=q.dtype, device='cuda')
    ops.decode_attention(q.cuda(), k.cuda(), v.cuda(), cos.cuda(), sin.cuda(), kc, torch.zeros_like(kc), 0)
    return kc[:, :, 0].cpu()


def on_gpu(p):
    """``p`` of the CPU on the GPU, q, k and v views into one packed row again"""
    nq, nk = p['q'].shape[1], p['k'].shape[1]
    rows, store = torch.cat((p['q'], p['k'], p['v']), 1).cuda(), p['store'].cuda()
    return dict(q=rows[:, :nq], k=rows[:, nq:nq + nk], v=rows[:, nq + nk:], cos=p['cos'].cuda(), sin=p['sin'].cuda(), store=store,
                kc=store[0, 0], vc=store[0, 1])


@pytest.mark.parametrize('n', [FULL, FULL - 1])
@pytest.mark.parametrize('Dh,G', [(16, 8), (128, 8), (120, 5), (64, 3)])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_full_length_by_probes(dtype, Dh, G, n):
    """(c) every batch row holds one key twice, far above the rest: ``out`` is the mean of the two value rows"""
    scale = Dh ** -0.5
    host, pairs = ref.probe_problem(Dh, G, dtype, n, FULL, stored_key)
    p = on_gpu(host)
    shape = (len(pairs), 2 * G, 2, Dh, n - 1, FULL)
    before = p['store'].clone()
    out = ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], n - 1)
    check_storage(p, before, shape, dtype, 1)
    want, bound = ref.probe_expectation(p, pairs, n, scale, dtype)
    err = (out.cpu().to(F64).reshape(want.shape) - want).abs()
    print(f'PROBES {dtype} Dh={Dh} G={G} n={n}: worst error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}')
    assert bool(torch.isfinite(out).all()) and bool((err <= bound).all()), [int(b) for b in (err > bound).any(-1).any(-1).nonzero()]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_random_rows_at_the_full_length(dtype):
    """(c) the chain term of the bound at its largest value, on the shortest sweep (Dh = 128)"""
    shape = (2, 6, 2, 128, FULL - 1, FULL)
    p = problem(shape, dtype, True, seed=7)
    before = p['store'].clone()
    out = ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], FULL - 1)
    check_storage(p, before, shape, dtype, 1)
    _, want, bound = reference_of(p, shape, dtype, 128 ** -0.5)
    print(f'FULL {dtype}: worst error / bound {float(((out.cpu().to(F64).reshape(want.shape) - want).abs() / bound).max()):.3f}')
    check_out(p, out, shape, dtype, 128 ** -0.5)


@pytest.mark.parametrize('Dh', HEAD_DIMS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_position_in_memory_gives_the_by_value_bytes(dtype, Dh):
    """(d) ``out`` and both caches, at the edges of this geometry and at the last position of the cache; tables [cap, Dh]"""
    edges = ref.edge_lengths(Dh, dtype)
    cap = edges[-1] + 2
    cos_table, sin_table = tables(range(cap), Dh)
    for G in (3, 8):
        for seen in [n - 1 for n in edges] + [cap - 1]:
            shape = (2, 2 * G, 2, Dh, seen, cap)
            by, at = problem(shape, dtype, True, seed=seen), problem(shape, dtype, True, seed=seen)
            want = ops.decode_attention(by['q'], by['k'], by['v'], cos_table[seen:seen + 1], sin_table[seen:seen + 1], by['kc'], by['vc'], seen)
            pos = torch.tensor([seen], dtype=torch.int32, device='cuda')
            got = ops.decode_attention_at(at['q'], at['k'], at['v'], cos_table, sin_table, at['kc'], at['vc'], pos)
            assert torch.equal(bits(got), bits(want)), (G, seen)
            assert torch.equal(bits(at['store']), bits(by['store'])), (G, seen)
            assert int(pos) == seen


@pytest.mark.parametrize('heads', [(1, 1, 16), (6, 2, 24), (8, 1, 80), (16, 2, 128), (3, 3, 120)], ids=lambda h: 'x'.join(map(str, h)))
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rope_append_off_its_one_shape(dtype, heads):
    """(e) fewer elements in a row than threads, ten trips of the 256 threads, one token into a cache of one, 300 tokens"""
    Hq, Hkv, Dh = heads
    for seen, L, cap in ((0, 1, 1), (0, 7, 7), (3, 5, 8), (2, 300, 302)):
        shape = (2, Hq, Hkv, Dh, seen, cap)
        p = problem(shape, dtype, True, seed=L, L=L)
        before = p['store'].clone()
        q_rot = ops.rope_append(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], seen)
        assert q_rot.shape == (2, Hq, L, Dh) and q_rot.dtype == dtype and q_rot.is_contiguous()
        check_storage(p, before, shape, dtype, L)
        want = ref.append64(p['q'].cpu(), p['k'].cpu(), p['v'].cpu(), p['cos'].cpu(), p['sin'].cpu(),
                            torch.zeros(2, Hkv, cap, Dh, dtype=F64), torch.zeros(2, Hkv, cap, Dh, dtype=F64), seen)
        assert bool(((q_rot.cpu().to(F64) - want).abs() <= ref.ulp(want, dtype)).all()), (seen, L, cap)


@pytest.mark.parametrize('on', [False, True], ids=['fp32', 'bf16-autocast'])
def test_a_model_with_eight_query_heads_of_24_on_one_kv_head(on):
    """(f) hidden 192 over 8 heads: Dh = 24 (three or six pieces, idle lanes) and G = 8; a prefill of 5, then single steps"""
    base = build_tiny(hidden_size=192, num_attention_heads=8, num_key_value_heads=1)
    with torch.no_grad():
        full = exact64(base)._transformer(TOKENS)['logits']
    decode, plain = copy.deepcopy(base).cuda().eval(), copy.deepcopy(base).cuda().eval()
    plain.fused = False
    cache = StaticKVCache.for_model(decode._transformer.config, 3, 9, torch.bfloat16 if on else torch.float32, 'cuda')
    assert (cache.head_dim, cache.kv_heads) == (24, 1)
    e_decode, seen_routes, cache = cached_error(decode, cache, PREFILL_THEN_STEPS, full, on)
    assert len(seen_routes) == 5 and all(r == routes.Route('decode') for r in seen_routes) and cache.get_seq_length() == 9
    e_torch, seen_routes, _ = cached_error(plain, None, PREFILL_THEN_STEPS, full, on)
    assert all(r.name == 'torch' for r in seen_routes)
    print(f'MODEL Dh=24 G=8 ({"autocast" if on else "fp32"}): decode {e_decode:.3e}, torch {e_torch:.3e}')
    assert e_decode <= 2 * e_torch
