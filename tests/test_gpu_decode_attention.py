"""vqhip_decode_attention and vqhip_rope_append on the GPU, through ``ops`` and the C ABI, in fp32, bf16 and fp16, against the
float64 restatement and the derived bounds of tests/decode_attention_ref.py: what is stored (v bit-equal, k' within one ulp),
what is left alone (everything past the new positions, every other cache), ``out`` within the bound of the restatement evaluated on
the cache as stored, equal bits run to run and whatever the other batch rows hold, hostile values, and every LIMITS clause."""
import ctypes
import math

import pytest
import torch

from vector_quantization_amd import _lib, ops

import decode_attention_ref as ref

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
CANARY = 777.0
# (B, Hq, Hkv, Dh, seen, cap): a length of one; GQA 4:1 with a ragged tail past one sweep; 257 positions; fewer positions than
# waves; the last slot of the cache
SHAPES = [(2, 4, 4, 16, 0, 3), (3, 8, 2, 64, 70, 73), (1, 16, 16, 64, 256, 259), (2, 2, 1, 128, 5, 8), (1, 4, 4, 64, 1, 2)]
INT_OF = {4: torch.int32, 2: torch.int16}


def bits(t):
    return t.contiguous().view(INT_OF[t.element_size()])


def tables(positions, Dh, theta=10000.0):
    """cos, sin fp32 [len(positions), Dh] as LlamaRotaryEmbedding computes them"""
    inv = 1.0 / (theta ** (torch.arange(0, Dh, 2, dtype=torch.float32) / Dh))
    f = torch.as_tensor(positions, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((f, f), -1)
    return emb.cos().cuda(), emb.sin().cuda()


def problem(shape, dtype, packed, seed=0, L=1, amp=1.0, tail=CANARY):
    """The inputs of one call: rows of L new tokens per batch row, a cache pair with ``seen`` random positions and ``tail``
    everywhere else, and a second pair next to it that the call must not touch."""
    B, Hq, Hkv, Dh, seen, cap = shape
    gen = torch.Generator().manual_seed(100 + seed)
    nq, nk = Hq * Dh, Hkv * Dh
    rows = (amp * torch.randn(B * L, nq + 2 * nk, generator=gen)).to(dtype).cuda()
    if packed:
        q, k, v = rows[:, :nq], rows[:, nq:nq + nk], rows[:, nq + nk:]
    else:
        q, k, v = rows[:, :nq].contiguous(), rows[:, nq:nq + nk].contiguous(), rows[:, nq + nk:].contiguous()
    store = torch.full((2, 2, B, Hkv, cap, Dh), tail, dtype=dtype).cuda()
    store[0, :, :, :, :seen] = (amp * torch.randn(2, B, Hkv, seen, Dh, generator=gen)).to(dtype).cuda()
    cos, sin = tables(range(seen, seen + L), Dh)
    return dict(q=q, k=k, v=v, cos=cos, sin=sin, store=store, kc=store[0, 0], vc=store[0, 1])


def check_storage(p, before, shape, dtype, L):
    """v bit-equal, k' within one ulp, everything else as it was"""
    B, Hq, Hkv, Dh, seen, cap = shape
    want_k = ref.rope64(p['k'].reshape(B, L, Hkv, Dh).cpu(), p['cos'].cpu().reshape(1, L, 1, Dh), p['sin'].cpu().reshape(1, L, 1, Dh)).transpose(1, 2)
    got_k = p['kc'][:, :, seen:seen + L].cpu().to(F64)
    assert bool(((got_k - want_k).abs() <= ref.ulp(want_k, dtype)).all()), float(((got_k - want_k).abs() / ref.ulp(want_k, dtype)).max())
    assert torch.equal(bits(p['vc'][:, :, seen:seen + L]), bits(p['v'].reshape(B, L, Hkv, Dh).transpose(1, 2)))
    keep = torch.ones(cap, dtype=torch.bool)
    keep[seen:seen + L] = False
    for name in ('kc', 'vc'):
        a, b = p[name][:, :, keep.to(p[name].device)], before[0, 0 if name == 'kc' else 1][:, :, keep.to(before.device)]
        assert torch.equal(bits(a), bits(b)), f'{name}: a position other than the new ones has changed'
    assert torch.equal(bits(p['store'][1]), bits(before[1])), 'the unrelated cache has changed'


def check_out(p, out, shape, dtype, scale):
    B, Hq, Hkv, Dh, seen, cap = shape
    n = seen + 1
    q_rot = ref.rope64(p['q'].reshape(B, Hq, Dh).cpu(), p['cos'].cpu().reshape(1, 1, Dh), p['sin'].cpu().reshape(1, 1, Dh))
    want, A, vmax = ref.attend64(q_rot, p['kc'][:, :, :n].cpu(), p['vc'][:, :, :n].cpu(), scale)
    bound = ref.out_bound(n, scale, A[..., None], vmax[..., None], want.abs(), dtype)
    err = (out.cpu().to(F64).reshape(B, Hq, Dh) - want).abs()
    print(f'{shape} {dtype}: worst error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}')
    assert bool(torch.isfinite(out).all()) and bool((err <= bound).all())
    return want


@pytest.mark.parametrize('packed', [False, True], ids=['separate', 'packed'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_decode_attention(dtype, shape, packed):
    B, Hq, Hkv, Dh, seen, cap = shape
    p = problem(shape, dtype, packed)
    before = p['store'].clone()
    out = ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], seen)
    assert out.shape == (B, Hq * Dh) and out.dtype == dtype
    check_storage(p, before, shape, dtype, 1)
    check_out(p, out, shape, dtype, Dh ** -0.5)
    # the same bits on a second run, from the cache as it was
    again = problem(shape, dtype, packed)
    out2 = ops.decode_attention(again['q'], again['k'], again['v'], again['cos'], again['sin'], again['kc'], again['vc'], seen)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(p['store']), bits(again['store']))
    # and with another batch row behind them
    wide = problem((B + 1,) + shape[1:], dtype, packed, seed=1)
    for name in ('q', 'k', 'v'):
        wide[name][:B] = again[name]
    wide['store'][:, :, :B] = before
    out3 = ops.decode_attention(wide['q'], wide['k'], wide['v'], wide['cos'], wide['sin'], wide['kc'], wide['vc'], seen)
    assert torch.equal(bits(out3[:B]), bits(out)), 'a row\'s result depends on the other rows of the batch'
    assert torch.equal(bits(wide['store'][:, :, :B]), bits(p['store']))


HOSTILE = (3, 8, 2, 64, 70, 73)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_scores_of_order_1e4_saturate_without_overflow(dtype):
    B, Hq, Hkv, Dh, seen, cap = HOSTILE
    p = problem(HOSTILE, dtype, True, amp=100.0)                                 # q . k / 8 of order 1e4
    p['v'].copy_(torch.randn(p['v'].shape, generator=torch.Generator().manual_seed(9)).to(dtype))
    p['vc'][:, :, :seen] = torch.randn(B, Hkv, seen, Dh, generator=torch.Generator().manual_seed(10)).to(dtype).cuda()
    out = ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], seen)
    check_out(p, out, HOSTILE, dtype, Dh ** -0.5)
    q_rot = ref.rope64(p['q'].reshape(B, Hq, Dh).cpu(), p['cos'].cpu().reshape(1, 1, Dh), p['sin'].cpu().reshape(1, 1, Dh))
    keys = p['kc'][:, :, :seen + 1].cpu().to(F64).repeat_interleave(Hq // Hkv, dim=1)
    values = p['vc'][:, :, :seen + 1].cpu().repeat_interleave(Hq // Hkv, dim=1)
    s = torch.einsum('bhd,bhnd->bhn', q_rot, keys) * Dh ** -0.5
    assert float(s.abs().max()) > 5e3
    top = s.topk(2, dim=-1)
    clear = (top.values[..., 0] - top.values[..., 1]) > 150.0                   # every other weight underflows to zero in fp32
    assert int(clear.sum()) >= B * Hq // 2
    winner = torch.gather(values, 2, top.indices[..., :1, None].expand(-1, -1, 1, Dh))[:, :, 0]
    got = out.cpu().reshape(B, Hq, Dh)
    assert torch.equal(bits(got[clear]), bits(winner[clear])), 'a saturated softmax must return the winning v row'


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_equal_scores_average_the_values(dtype):
    B, Hq, Hkv, Dh, seen, cap = HOSTILE
    p = problem(HOSTILE, dtype, False)
    p['q'].zero_()
    out = ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], seen)
    want = check_out(p, out, HOSTILE, dtype, Dh ** -0.5)
    mean = p['vc'][:, :, :seen + 1].cpu().to(F64).mean(2).repeat_interleave(Hq // Hkv, dim=1)
    assert float((want - mean).abs().max()) <= 1e-12


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_nan_in_the_unused_tail_does_not_reach_out(dtype):
    B, Hq, Hkv, Dh, seen, cap = HOSTILE
    p = problem(HOSTILE, dtype, True, tail=math.nan)
    out = ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], seen)
    check_out(p, out, HOSTILE, dtype, Dh ** -0.5)
    assert bool(torch.isnan(p['store'][0][:, :, :, seen + 1:]).all()) and bool(torch.isnan(p['store'][1]).all())


@pytest.mark.parametrize('seen', [0, 3])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rope_append(dtype, seen):
    L = 5
    shape = (2, 8, 2, 64, seen, seen + L + 2)
    B, Hq, Hkv, Dh, _, cap = shape
    for packed in (False, True):
        p = problem(shape, dtype, packed, L=L)
        before = p['store'].clone()
        q_rot = ops.rope_append(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], seen)
        assert q_rot.shape == (B, Hq, L, Dh) and q_rot.dtype == dtype and q_rot.is_contiguous()
        check_storage(p, before, shape, dtype, L)
        want = ref.append64(p['q'].cpu(), p['k'].cpu(), p['v'].cpu(), p['cos'].cpu(), p['sin'].cpu(),
                            torch.zeros(B, Hkv, cap, Dh, dtype=F64), torch.zeros(B, Hkv, cap, Dh, dtype=F64), seen)
        assert bool(((q_rot.cpu().to(F64) - want).abs() <= ref.ulp(want, dtype)).all())


def test_a_cancelling_rotation_keeps_one_ulp_in_fp32():
    """x cos - y sin with the two products equal to 2^-12: plain fp32 arithmetic would leave no correct bit."""
    shape = (1, 1, 1, 16, 0, 1)
    p = problem(shape, torch.float32, False)
    cos, sin = p['cos'].clone(), p['sin'].clone()
    gen = torch.Generator().manual_seed(4)
    cos.copy_(torch.rand(1, 16, generator=gen) + 0.5)
    sin.copy_(torch.rand(1, 16, generator=gen) + 0.5)
    x = torch.rand(8, generator=gen) + 1.0
    y = (x * cos[0, :8].cpu() / sin[0, :8].cpu()) * (1.0 + 2.0 ** -12)         # x cos - y sin is about -2^-12 x cos
    p['k'][0, :8], p['k'][0, 8:] = x.cuda(), y.cuda()
    before = p['store'].clone()
    ops.decode_attention(p['q'], p['k'], p['v'], cos, sin, p['kc'], p['vc'], 0)
    p['cos'], p['sin'] = cos, sin
    check_storage(p, before, shape, torch.float32, 1)


def _abi(name, p, shape, dt, out, **change):
    """rc and the text of one direct call with the arguments of ``shape``, ``change`` applied"""
    B, Hq, Hkv, Dh, seen, cap = shape
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())          # noqa: E731
    a = dict(q=P(p['q']), qs=p['q'].stride(0), k=P(p['k']), ks=p['k'].stride(0), v=P(p['v']), vs=p['v'].stride(0), dtype=ops.FLOAT_DTYPES[dt],
             cos=P(p['cos']), sin=P(p['sin']), kc=P(p['kc']), vc=P(p['vc']), seen=seen, cap=cap, scale=Dh ** -0.5, B=B, L=1, Hq=Hq,
             Hkv=Hkv, Dh=Dh, out=P(out))
    a.update(change)
    L = _lib.lib()
    head = (a['q'], a['qs'], a['k'], a['ks'], a['v'], a['vs'], a['dtype'], a['cos'], a['sin'], a['kc'], a['vc'], a['seen'], a['cap'])
    if name == 'vqhip_decode_attention':
        rc = L.vqhip_decode_attention(*head, a['scale'], a['B'], a['Hq'], a['Hkv'], a['Dh'], a['out'], ops._stream())
    else:
        rc = L.vqhip_rope_append(*head, a['B'], a['L'], a['Hq'], a['Hkv'], a['Dh'], a['out'], ops._stream())
    return rc, (L.vqhip_last_error() or b'').decode()


CLAUSES = [
    (dict(Dh=20), 'Dh must be a multiple of 8'), (dict(Dh=8), 'Dh must be a multiple of 8'), (dict(Dh=136), 'VQHIP_ATTN_MAX_HEAD_DIM'),
    (dict(Hq=3), 'multiple of Hkv'), (dict(Hq=32, qs=4096), 'VQHIP_ATTN_MAX_GROUP'), (dict(cap=0, seen=0), 'cap must be in 1'),
    (dict(cap=4097), 'VQHIP_ATTN_MAX_LEN'), (dict(seen=73), 'seen + L <= cap'), (dict(seen=-1), 'seen + L <= cap'),
    (dict(qs=8 * 64 - 1), 'row stride'), (dict(ks=2 * 64 - 1), 'row stride'), (dict(vs=0), 'row stride'), (dict(q=None), 'are required'),
    (dict(dtype=2), 'dtype'), (dict(B=0), 'B and L must be >= 1'), ('cache+1', '16-byte aligned'), ('q+1byte', 'alignment of their element type'),
]


@pytest.mark.parametrize('name', ['vqhip_decode_attention', 'vqhip_rope_append'])
def test_every_limit_is_refused_by_name_and_launches_nothing(name):
    dtype = torch.bfloat16
    p = problem(HOSTILE, dtype, False)
    B, Hq, Hkv, Dh, seen, cap = HOSTILE
    out = torch.full((B, Hq * Dh), CANARY, dtype=dtype).cuda()
    before, out_before = p['store'].clone(), out.clone()
    clauses = CLAUSES + ([(dict(scale=math.inf), 'scale must be finite')] if name == 'vqhip_decode_attention' else
                         [(dict(L=0), 'B and L must be >= 1'), (dict(L=4), 'seen + L <= cap')])
    for change, text in clauses:
        if change == 'cache+1':
            change = dict(kc=ctypes.c_void_p(p['kc'].data_ptr() + 2))
        elif change == 'q+1byte':
            change = dict(q=ctypes.c_void_p(p['q'].data_ptr() + 1))
        rc, msg = _abi(name, p, HOSTILE, dtype, out, **change)
        assert rc == -22 and name in msg and text in msg, (change, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(bits(p['store']), bits(before)) and torch.equal(bits(out), bits(out_before))
    rc, msg = _abi(name, p, HOSTILE, dtype, out if name == 'vqhip_decode_attention' else torch.empty(B, Hq, 1, Dh, dtype=dtype).cuda())
    assert rc == 0, msg
    # the host layer names the same clauses before it calls
    with pytest.raises(ValueError, match='not 16-byte aligned'):
        flat = torch.zeros(2 * p['kc'].numel() + 8, dtype=dtype).cuda()
        shifted = flat[1:1 + p['kc'].numel()].view(p['kc'].shape)
        ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], shifted, p['vc'], seen)
    with pytest.raises(ValueError, match='do not fit a capacity'):
        ops.decode_attention(p['q'], p['k'], p['v'], p['cos'], p['sin'], p['kc'], p['vc'], cap)
