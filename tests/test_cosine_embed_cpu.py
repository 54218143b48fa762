"""CPU checks of the fused CosineEmbeddingLoss: the float64 restatement the GPU tests hold the kernels to against
``F.cosine_embedding_loss`` and its autograd, the module built from the reference's config, the route decision, the ABI limits,
the bindings and the bound helpers."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cosine_embed_ref as ref
import vector_quantization_amd as vqa
from vector_quantization_amd import _lib
from vector_quantization_amd.registries import VQLossRegistry

CONFIG = dict(type='ModelRegistry.LossRegistry.VQLossRegistry.CosineEmbeddingLoss', cosine_embedding=dict())


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libvqhip.so is not built')
    return _lib.lib()


def test_restatement_is_the_float64_functional_and_its_autograd():
    seen = set()
    for case in ref.cases():
        C, R, pad, dtypes, seed = case
        if R == 300 and C > 520:                                   # (the GPU tests take these; here the small ones carry the point)
            continue
        pred, target = ref.make_case(*case)
        assert pred.shape == target.shape == (R, C) and pred.stride(0) == target.stride(0) == C + pad
        assert (pred.dtype, target.dtype) == dtypes
        p = pred.double().clone().requires_grad_()
        t = target.double()
        want = F.cosine_embedding_loss(p, t, torch.ones(R, dtype=torch.float64), reduction='none')
        want.sum().backward()
        e = ref.expected(case)
        assert np.abs(e['loss'] - want.detach().numpy()).max() <= 1e-14, case
        scale = np.maximum(e['h'], 1.0)[:, None]                   # the gradient scales as 1 / |p|
        assert (np.abs(e['grad_unit'] - p.grad.numpy()) <= 1e-14 * scale).all(), case
        assert abs(e['total'] - float(want.detach().sum())) <= 1e-14 * R
        seen |= {(r + seed) % ref.KINDS for r in range(R)}
    assert seen == set(range(ref.KINDS))
    cs = ref.cases()
    assert {c[0] for c in cs} == set(ref.CS) and {c[1] for c in cs} == set(ref.RS) and {c[2] for c in cs} == set(ref.PADS)
    assert {c[3] for c in cs} == set(ref.DTYPES) and len(cs) == len(ref.CS) * len(ref.RS) * len(ref.PADS) * len(ref.DTYPES)
    assert [c[:3] for c in ref.map_cases()[::2]] == ref.MAP_SHAPES
    # the cancellation rows and the orthogonal rows are what they are meant to be
    pred, target = ref.make_case(512, 5, 0, (torch.bfloat16, torch.float32), 0)
    e = ref.reference(ref.as64(pred), ref.as64(target))
    assert e['loss'][3] == 0.0 or abs(e['loss'][3]) < 1e-12       # kind 3 with a bf16 pred: the target is pred exactly
    assert abs(e['loss'][4] - 2.0) < 1e-12 and abs(e['loss'][0] - 1.0) < 0.5
    pred, target = ref.make_case(512, 1, 0, (torch.float32, torch.float32), 5)
    assert abs(ref.reference(ref.as64(pred), ref.as64(target))['cos'][0]) < 1e-12


@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
def test_module_builds_from_the_reference_config_and_takes_the_torch_route_on_cpu(reduction):
    torch.manual_seed(1)
    m = VQLossRegistry.build(dict(CONFIG, reduction=reduction, weight=0.25))
    assert type(m) is vqa.CosineEmbeddingLoss and 'CosineEmbeddingLoss' in vqa.__all__
    assert type(VQLossRegistry.build(CONFIG)) is vqa.CosineEmbeddingLoss
    pred = torch.randn(2, 5, 12, requires_grad=True)
    target = torch.randn(2, 5, 12)
    got = m(pred, target)
    assert m.last_route.name == 'torch' and 'cpu' in m.last_route.why
    rows = F.cosine_embedding_loss(pred.flatten(0, -2), target.flatten(0, -2), torch.ones(10), reduction='none').reshape(2, 5)
    want = {'mean': rows.mean(), 'sum': rows.sum(), 'none': rows}[reduction] * 0.25
    assert got.shape == want.shape and torch.equal(got, want)
    got.sum().backward()
    assert pred.grad is not None and bool(pred.grad.abs().sum() > 0)
    # the map entry point on the CPU: the rearrangement, then the same composition
    from vector_quantization_amd import tokenization
    pmap = pred.detach().reshape(2, 5, 12).permute(0, 2, 1).contiguous().reshape(2, 12, 5, 1)
    viamap = tokenization.distill_loss(m, pmap, target)
    assert m.last_route.name == 'torch'
    assert torch.allclose(viamap.reshape(want.shape), want.detach(), rtol=0, atol=1e-6)


class Fake:
    """A tensor as the route decision sees it (no GPU here)."""
    def __init__(self, t, cuda=True):
        self.t, self.is_cuda = t, cuda

    def __getattr__(self, n):
        return getattr(self.t, n)


def test_route_reasons():
    from vector_quantization_amd.quantizers import routes
    why = routes.cosine_embedding_why
    p = torch.zeros(4, 9, 32, device='meta')
    t = torch.zeros(4, 9, 32, device='meta')
    assert why(Fake(p), Fake(t)) == routes.Route('fused')
    assert why(Fake(p.bfloat16()), Fake(t)).name == 'fused' and why(Fake(p.half()), Fake(t.bfloat16())).name == 'fused'
    assert why(Fake(torch.zeros(4, 9, 35, device='meta')[..., :32]), Fake(t)).name == 'fused'          # a sliced view: rows of stride 35
    pmap = torch.zeros(4, 32, 3, 3, device='meta')
    assert why(Fake(pmap), Fake(t), layout='map').name == 'fused'
    reasons = {
        'cpu': why(torch.zeros(4, 32), torch.zeros(4, 32)).why,
        'cpu target': why(Fake(p), torch.zeros(4, 9, 32)).why,
        'float64': why(Fake(p.double()), Fake(t)).why,
        'float64 target': why(Fake(p), Fake(t.double())).why,
        'grad': why(Fake(p), Fake(torch.zeros(4, 9, 32, device='meta', requires_grad=True))).why,
        'strides': why(Fake(torch.zeros(4, 32, 9, device='meta').transpose(1, 2)), Fake(t)).why,
        'map strides': why(Fake(pmap.transpose(2, 3)), Fake(t), layout='map').why,
        'shape': why(Fake(p[:, :8]), Fake(t)).why,
        'map shape': why(Fake(torch.zeros(4, 31, 3, 3, device='meta')), Fake(t), layout='map').why,
        'layout': why(Fake(p), Fake(t), layout='nhwc').why,
    }
    assert all(reasons.values()) and len(set(reasons.values())) == len(reasons), reasons
    assert 'cpu' in reasons['cpu'] and 'float64' in reasons['float64'] and 'requires grad' in reasons['grad']
    assert 'stride 1' in reasons['strides'] and 'NCHW-contiguous' in reasons['map strides']

    class Other(vqa.CosineEmbeddingLoss):
        def forward(self, pred_image, image):
            return super().forward(pred_image, image) * 2

    r = why(Fake(p), Fake(t), loss=Other())
    assert r.name == 'torch' and 'overrides forward' in r.why and r.why not in reasons.values()
    assert why(Fake(p), Fake(t), loss=vqa.CosineEmbeddingLoss()).name == 'fused'
    assert 'cosine_embedding_why' in routes.__doc__


def test_abi_limits_are_refused_without_a_gpu(lib):
    fake = ctypes.c_void_p(0x1000)

    def fwd(pred=fake, pdtype=1, layout=0, pstride=35, target=fake, tdtype=0, tstride=32, B=6, P=1, C=32, loss=fake, stats=fake,
            out=fake):
        return lib.vqhip_cosine_embed_fwd(pred, pdtype, layout, pstride, target, tdtype, tstride, B, P, C, loss, stats, out, None)

    def bwd(pred=fake, pdtype=1, layout=0, pstride=35, target=fake, tdtype=0, tstride=32, B=6, P=1, C=32, stats=fake, g=fake,
            per_row=0, mean=1, grad=fake, gstride=32):
        return lib.vqhip_cosine_embed_bwd(pred, pdtype, layout, pstride, target, tdtype, tstride, B, P, C, stats, g, per_row, mean,
                                          grad, gstride, None)

    shared = (dict(pred=None), dict(target=None), dict(pdtype=2), dict(pdtype=3), dict(pdtype=5), dict(pdtype=9), dict(tdtype=2),
              dict(tdtype=-1), dict(layout=2), dict(layout=-1), dict(B=0), dict(P=0), dict(B=-1), dict(B=1 << 31),
              dict(B=1 << 16, P=1 << 15), dict(B=1 << 40, P=1 << 40), dict(C=0), dict(C=-3), dict(C=(1 << 16) + 1, pstride=1 << 17, tstride=1 << 17),
              dict(pstride=31), dict(tstride=31), dict(layout=1, tstride=31))
    for kw in shared + (dict(loss=None), dict(stats=None), dict(out=None)):
        assert fwd(**kw) == -22, kw
        assert b'vqhip_cosine_embed_fwd' in lib.vqhip_last_error(), kw
    for kw in shared + (dict(stats=None), dict(g=None), dict(grad=None), dict(gstride=31)):
        assert bwd(**kw) == -22, kw
        assert b'vqhip_cosine_embed_bwd' in lib.vqhip_last_error(), kw
    assert lib.vqhip_version() == 600


def test_symbols_are_declared_bound_and_the_bounds_are_the_header_macros(lib):
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'vqhip.h')).read()
    for name in ('vqhip_cosine_embed_fwd', 'vqhip_cosine_embed_bwd'):
        assert f'int {name}(' in header and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES['vqhip_cosine_embed_fwd'][1]) == 14 and len(_lib.SIGNATURES['vqhip_cosine_embed_bwd'][1]) == 17
    # the macros as the header spells them, restated: N = C / 32 + 16, u = 2^-24, the second-order factor 1 + 2^-9
    assert '#define VQHIP_COSINE_EMBED_CHAIN(C) ((double)((C) / 32 + 16))' in header
    assert ('#define VQHIP_COSINE_EMBED_BOUND(C) ((2.0 * VQHIP_COSINE_EMBED_CHAIN(C) + 6.0) * 5.9604644775390625e-08 * 1.001953125)'
            in header)
    assert '((4.0 * VQHIP_COSINE_EMBED_CHAIN(C) + 21.0) * 5.9604644775390625e-08 * 1.001953125 * (double)(h))' in header
    assert '#define VQHIP_COSINE_EMBED_MAX_C (1 << 16)' in header and _lib.COSINE_EMBED_MAX_C == 1 << 16
    assert 5.9604644775390625e-08 == 2.0 ** -24 and 1.001953125 == 1 + 2.0 ** -9
    for C, h in ((1, 1.0), (768, 0.03125), (1 << 16, 1.0e6)):
        n = C // 32 + 16
        assert _lib.cosine_embed_chain(C) == ref.chain(C) == n
        assert _lib.cosine_embed_bound(C) == ref.bound(C) == (2.0 * n + 6.0) * 5.9604644775390625e-08 * 1.001953125
        assert _lib.cosine_embed_grad_bound(C, h) == ref.grad_bound(C, h) == (4.0 * n + 21.0) * 5.9604644775390625e-08 * 1.001953125 * h
    assert ref.bound(768) == 86.0 * 2.0 ** -24 * (1 + 2.0 ** -9)


def test_cpu_tensors_are_refused_by_the_ops():
    from vector_quantization_amd import ops
    p, t = torch.zeros(2, 8), torch.zeros(2, 8)
    with pytest.raises(_lib.VqhipError):
        ops.cosine_embedding_forward(p, t)
    with pytest.raises(_lib.VqhipError):
        ops.cosine_embedding_backward(p, t, torch.zeros(2, 3), torch.ones(1))
    with pytest.raises(_lib.VqhipError):
        ops.cosine_embedding_loss(p, t)
    with pytest.raises(ValueError):
        ops.cosine_embedding_loss(p, t, reduction='batchmean')
