"""Pooled code features (tokens -> [B, D] mean of the decoded rows), the parts that need no GPU: the arithmetic contract itself
against the float64 mean, the route decision, and the refusals of the three new entry points."""
import ctypes

import numpy as np
import pytest
import torch

import pooled_ref as PR
import route_variants as RV
from vector_quantization_amd import _lib, ops
from vector_quantization_amd.quantizers import routes


@pytest.fixture(scope='module')
def lib():
    return _lib.lib()


@pytest.mark.parametrize('HW', PR.HW_CASES)
def test_the_contract_lies_within_the_bound_of_the_float64_mean(HW):
    """The restatement (8 partials, the tree, an fp32 division) against the float64 mean, on every (K, D) of the GPU cases:
    the contract, not only a kernel, meets the derived bound."""
    rng = np.random.default_rng(HW)
    for K, D in PR.KD_CASES:
        e = rng.standard_normal((K, D)).astype(np.float32)
        quant = rng.integers(0, K, size=(3, HW))
        v = e[quant]
        out, ref = PR.pooled_tokens(e, quant), PR.mean64(v)
        err = np.abs(out.astype(np.float64) - ref)
        assert (err <= PR.bound(v)).all(), (HW, K, D, float((err / PR.bound(v)).max()))


def test_the_contract_keeps_its_order_and_its_special_values():
    # the order depends on HW alone: 1e8 + 1 - 1e8 over 9 positions, partial 0 holds positions 0 and 8
    v = np.zeros((1, 9, 1), dtype=np.float32)
    v[0, 0, 0], v[0, 1, 0], v[0, 8, 0] = 1e8, 1.0, -1e8
    assert PR.pooled(v)[0, 0] == np.float32(1.0) / np.float32(9)          # (1e8 - 1e8) + 1: the 1 survives
    v[0, 1, 0], v[0, 8, 0], v[0, 2, 0] = -1e8, 1.0, 0.0
    assert PR.pooled(v)[0, 0] == np.float32(0.0)                          # (1e8 + 1) - 1e8: it does not
    z = np.full((1, 3, 1), -0.0, dtype=np.float32)
    assert not np.signbit(PR.pooled(z)[0, 0])                             # +0.0f + -0.0f = +0.0f
    e = np.arange(8, dtype=np.float32).reshape(4, 2)
    out = PR.pooled_tokens(e, np.array([[0, 1], [4, 1], [-1, 0]]))
    assert np.isfinite(out[0]).all() and np.isnan(out[1:]).all()


def _device_tokens(shape=(2, 4, 4), dtype=torch.int64):
    """Tokens that say they live on a GPU, on a machine without one (a fake tensor: metadata only)."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        return torch.empty(shape, dtype=dtype, device='cuda')


@pytest.mark.parametrize('variant', ['vqgan', 'vqkd', 'cvq_cos', 'cvq_l2', 'llamagen', 'fsq'])
def test_shipped_configs_take_the_pooled_route(variant):
    q = RV.build(variant)
    assert routes.pooled_config(q) == ''
    for dtype in (torch.int64, torch.int32):
        assert routes.pooled_entry(q, _device_tokens(dtype=dtype)) == routes.Route('pooled')


@pytest.mark.parametrize('variant', ['vqgan+sub_decode', 'fsq+sub_decode', 'vqgan+cb_after_decode', 'fsq+cb_after_decode'])
def test_a_customised_decode_takes_the_rows(variant):
    q = RV.build(variant)
    route = routes.pooled_entry(q, _device_tokens())
    assert route.name == 'rows' and route.why
    assert ('_decode' if 'sub_decode' in variant else 'after_decode') in route.why


def test_cpu_tokens_other_types_and_other_token_tensors_take_the_rows():
    for variant in ('vqgan', 'fsq'):
        q = RV.build(variant)
        route = routes.pooled_entry(q, torch.zeros(2, 4, 4, dtype=torch.long))
        assert route.name == 'rows' and 'cpu' in route.why
        assert routes.pooled_entry(q, _device_tokens((16,))).name == 'rows'
        assert 'float32' in routes.pooled_entry(q, _device_tokens(dtype=torch.float32)).why
    route = routes.pooled_entry(torch.nn.Identity(), _device_tokens())
    assert route.name == 'rows' and 'Identity' in route.why


def test_pool_from_quant_on_the_rows_route_is_decode_and_mean():
    """CPU tokens, and a decode that needs no device (a subclass that gathers with torch): the caller gets the reference's
    value, the reason is left in last_route, and the memo has the decode stage."""
    from vector_quantization_amd import tokenization as T
    q = RV.build('vqgan')

    class TorchDecode(type(q)):
        def _decode(self, quant, memo):
            return torch.nn.functional.embedding(quant, self.embedding.weight), memo
    q.__class__ = TorchDecode
    quant = torch.randint(0, RV.K, (3, 2, 5), generator=torch.Generator().manual_seed(3))
    features, memo = T.pool_from_quant(q, quant, {})
    assert q.last_route.name == 'rows' and q.last_route.why
    want = q.embedding.weight.detach()[quant].mean(dim=(1, 2))
    assert torch.equal(features.detach(), want) and 'decode' in memo['quantizer']


def test_new_symbols_refuse_bad_arguments_before_any_hip_call(lib):
    fake = ctypes.c_void_p(0x1000)
    I32, I64 = _lib.DTYPE_I32, _lib.DTYPE_I64
    q = ops.fsq_constants([8, 5, 5, 5])
    qp = ctypes.byref(q)

    def fwd(e=fake, K=64, D=8, quant=fake, dt=I64, B=2, HW=16, out=fake):
        return lib.vqhip_decode_pool(e, K, D, quant, dt, B, HW, out, None)

    def bwd(g=fake, quant=fake, dt=I64, B=2, HW=16, K=64, D=8, grad=fake):
        return lib.vqhip_decode_pool_bwd(g, quant, dt, B, HW, K, D, grad, None)

    def fsq(qq=qp, quant=fake, dt=I32, B=2, HW=16, out=fake):
        return lib.vqhip_fsq_decode_pool(qq, quant, dt, B, HW, out, None)

    for name, call, pointers in (('vqhip_decode_pool', fwd, ('e', 'quant', 'out')),
                                 ('vqhip_decode_pool_bwd', bwd, ('g', 'quant', 'grad')),
                                 ('vqhip_fsq_decode_pool', fsq, ('qq', 'quant', 'out'))):
        for p in pointers:
            assert call(**{p: None}) == -22, (name, p)
            assert name.encode() in lib.vqhip_last_error()
        assert call(HW=0) == -22 and name.encode() in lib.vqhip_last_error()
        assert call(B=0) == -22
        assert call(B=1 << 16, HW=1 << 15) == -22 and b'2^31' in lib.vqhip_last_error()      # B * HW = 2^31
        assert call(B=1, HW=1 << 31) == -22
        assert call(B=1 << 40, HW=1 << 40) == -22                                               # (the product would wrap)
        assert call(dt=0) == -22 and b'quant_dtype' in lib.vqhip_last_error()                  # VQHIP_DTYPE_F32 is no token dtype
        assert call(dt=1) == -22 and call(dt=4) == -22
    for call in (fwd, bwd):
        assert call(K=0) == -22 and call(D=0) == -22
    bad = ops.fsq_constants([8, 5, 5, 5])
    bad.struct_bytes -= 1
    assert fsq(qq=ctypes.byref(bad)) == -22 and b'struct_bytes' in lib.vqhip_last_error()


def test_ops_refuse_cpu_tensors():
    e, quant = torch.zeros(8, 8), torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(_lib.VqhipError):
        ops.decode_pool(e, quant)
    with pytest.raises(_lib.VqhipError):
        ops.decode_pool_bwd(torch.zeros(2, 8), quant, 8)
    with pytest.raises(_lib.VqhipError):
        ops.fsq_decode_pool(quant, ops.fsq_constants([3, 3, 3]))
