"""CPU checks of the token cross-entropy: the ABI limits, the bindings, the route decision, the torch route of the three modules
against ``F.cross_entropy`` and the hand-written compositions, and the float64 restatement the GPU tests hold the kernels to."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_ce_ref as ref
import vector_quantization_amd as vqa
from vector_quantization_amd import _lib, sequence_losses as SL
from vector_quantization_amd.quantizers import routes


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libvqhip.so is not built')
    return _lib.lib()


def test_abi_limits_are_refused_without_a_gpu(lib):
    fake = ctypes.c_void_p(0x1000)

    def fwd(logits=fake, dtype=1, R=6, stride=107, start=0, end=100, targets=fake, tdtype=3, shift=0, ignore=-100, eps=0.1,
            weight=None, loss=fake, lse=fake, hit=None, out=fake):
        return lib.vqhip_token_ce_fwd(logits, dtype, R, stride, start, end, targets, tdtype, shift, ignore, eps, weight, loss, lse,
                                      hit, out, None)

    def bwd(logits=fake, dtype=1, R=6, stride=107, start=0, end=100, targets=fake, tdtype=3, shift=0, ignore=-100, eps=0.1,
            weight=None, lse=fake, g=fake, per_row=0, wsum=None, grad=fake, cols=107, stride_out=107):
        return lib.vqhip_token_ce_bwd(logits, dtype, R, stride, start, end, targets, tdtype, shift, ignore, eps, weight, lse, g,
                                      per_row, wsum, grad, cols, stride_out, None)

    shared = (dict(logits=None), dict(targets=None), dict(dtype=2), dict(dtype=3), dict(dtype=9), dict(tdtype=0), dict(tdtype=1),
              dict(tdtype=4), dict(R=0), dict(R=-1), dict(R=1 << 31), dict(start=-1), dict(start=100), dict(start=50, end=50),
              dict(end=108), dict(stride=(1 << 20) + 10, end=(1 << 20) + 1), dict(eps=-0.1), dict(eps=1.0), dict(eps=float('nan')),
              dict(shift=4), dict(shift=-2), dict(shift=7))
    for kw in shared + (dict(loss=None), dict(lse=None), dict(out=None)):
        assert fwd(**kw) == -22, kw
        assert b'vqhip_token_ce_fwd' in lib.vqhip_last_error(), kw
    for kw in shared + (dict(lse=None), dict(g=None), dict(grad=None), dict(cols=99), dict(cols=108), dict(stride_out=106),
                        dict(cols=1 << 31, stride_out=1 << 32)):
        assert bwd(**kw) == -22, kw
        assert b'vqhip_token_ce_bwd' in lib.vqhip_last_error(), kw
    assert lib.vqhip_version() == 600


def test_symbols_are_declared_and_bound(lib):
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'vqhip.h')).read()
    for name in ('vqhip_token_ce_fwd', 'vqhip_token_ce_bwd'):
        assert f'int {name}(' in header and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES['vqhip_token_ce_fwd'][1]) == 17 and len(_lib.SIGNATURES['vqhip_token_ce_bwd'][1]) == 20
    for name in ('VQHIP_TOKEN_CE_BOUND', 'VQHIP_TOKEN_CE_LSE_BOUND', 'VQHIP_TOKEN_CE_GRAD_BOUND'):
        assert f'#define {name}(V, amax)' in header
    for V, amax in ((1, 0.0), (257, 3.5), (16384, 60.0), (1 << 20, 1000.0)):
        assert _lib.token_ce_bound(V, amax) == ref.bound(V, amax)
        assert _lib.token_ce_lse_bound(V, amax) == ref.lse_bound(V, amax) <= ref.bound(V, amax)
        assert _lib.token_ce_grad_bound(V, amax) == ref.grad_bound(V, amax)
    # the header's figures, spelled out once: N = V / 256 + 20, u = 2^-24
    assert ref.lse_bound(16384, 60.0) == (300.0 + 44.0 + 4 * 84.0) * 2.0 ** -24 * (1 + 2.0 ** -9)
    assert ref.bound(16384, 60.0) == ref.lse_bound(16384, 60.0) + (95.0 * 60.0 + 70.0) * 2.0 ** -24


def test_exports():
    for name in ('CausalTokenLoss', 'LabelSmoothingCrossEntropy', 'MaskedTokenLoss'):
        assert getattr(vqa, name) is getattr(SL, name) and name in vqa.__all__


class Fake:
    """A tensor as the route decision sees it (no GPU here)."""
    def __init__(self, t, cuda=True):
        self.t, self.is_cuda = t, cuda

    def __getattr__(self, n):
        return getattr(self.t, n)


def test_route_reasons():
    x = torch.zeros(4, 32)
    t = torch.zeros(4, dtype=torch.int64)
    r = routes.token_ce_why(x, t)
    assert r.name == 'torch' and 'cpu' in r.why
    meta = torch.zeros(4, 32, device='meta')
    tm = torch.zeros(4, dtype=torch.int64, device='meta')
    assert routes.token_ce_why(Fake(meta), tm) == routes.Route('fused')
    assert routes.token_ce_why(Fake(meta), tm.int(), 1, 31, label_smoothing=0.1, weight=torch.zeros(4)).name == 'fused'
    assert 'float64' in routes.token_ce_why(Fake(torch.zeros(4, 32, dtype=torch.float64, device='meta')), tm).why
    assert 'stride 1' in routes.token_ce_why(Fake(torch.zeros(32, 4, device='meta').t()), tm).why
    cube = torch.zeros(2, 3, 32, device='meta')
    t23 = torch.zeros(2, 3, dtype=torch.int64, device='meta')
    assert routes.token_ce_why(Fake(cube), t23, shift=True).name == 'fused'
    assert 'flatten' in routes.token_ce_why(Fake(cube.transpose(0, 1)), t23.t()).why
    assert 'flatten' in routes.token_ce_why(Fake(cube[:, 1:]), t23[:, 1:]).why           # MAGE's [:, 1:] view, B > 1
    for start, end in ((0, 33), (5, 5), (-1, 4)):
        assert 'slice' in routes.token_ce_why(Fake(meta), tm, start, end).why
    assert '2^20' in routes.token_ce_why(Fake(torch.zeros(1, (1 << 20) + 1, device='meta')), tm[:1]).why
    assert 'overlap' in routes.token_ce_why(Fake(meta[:1].expand(4, 32)), tm).why
    assert 'float32' in routes.token_ce_why(Fake(meta), tm.float()).why and 'int32 or int64' in routes.token_ce_why(Fake(meta), tm.float()).why
    assert 'one per row' in routes.token_ce_why(Fake(meta), tm[:3]).why
    assert 'device' in routes.token_ce_why(Fake(meta), t).why
    assert 'shift' in routes.token_ce_why(Fake(meta[0]), tm[0], shift=True).why
    assert 'label_smoothing' in routes.token_ce_why(Fake(meta), tm, label_smoothing=1.0).why
    assert 'weights' in routes.token_ce_why(Fake(meta), tm, weight=torch.zeros(5)).why


def test_cpu_tensors_are_refused_by_the_op():
    from vector_quantization_amd import ops
    with pytest.raises(_lib.VqhipError):
        ops.token_cross_entropy(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.token_cross_entropy(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64), reduction='batchmean')


@pytest.mark.parametrize('smoothing', [0.0, 0.1])
def test_torch_route_of_the_modules_on_cpu_float64(smoothing):
    torch.manual_seed(3)
    B, L, Vt = 3, 6, 29
    x = torch.randn(B, L, Vt, dtype=torch.float64) * 3
    tokens = torch.randint(0, Vt, (B, L))
    tokens[1, 3] = -100
    # CausalTokenLoss: F.cross_entropy on the explicit shift-and-slice form
    m = SL.CausalTokenLoss(label_smoothing=smoothing)
    loss, memo = m(x, tokens, {})
    assert m.last_route.name == 'torch' and loss.dtype == torch.float64
    sl, st = x[:, :-1].reshape(-1, Vt), tokens[:, 1:].reshape(-1)
    want = F.cross_entropy(sl, st, ignore_index=-100, label_smoothing=smoothing)
    assert abs(float(loss - want)) <= 1e-14 * max(1.0, abs(float(want)))
    keep = st != -100
    assert float(memo['accuracy']) == float((sl.argmax(-1)[keep] == st[keep]).double().mean())
    # ... and the restatement the GPU tests use; there e and 1 - e are the fp32-rounded values (2^-24 relative each) on terms of
    # at most 2 max|a| + ln V
    eps_tol = (2.0 ** -23 * (2 * float(x.abs().max()) + 4) if smoothing else 0.0) + 1e-13
    r = ref.reference(x.reshape(-1, Vt).numpy(), ref.row_targets(tokens.reshape(-1).numpy(), 0, Vt, shift_len=L), smoothing)
    assert abs(r['total'] / r['wsum'] - float(want)) <= eps_tol
    # LabelSmoothingCrossEntropy: per row
    c = SL.LabelSmoothingCrossEntropy(smoothing)
    rows = c(sl[keep], st[keep])
    assert c.last_route.name == 'torch'
    want_rows = F.cross_entropy(sl[keep], st[keep], reduction='none', label_smoothing=smoothing)
    assert float((rows - want_rows).abs().max()) <= 1e-13
    # MaskedTokenLoss: the hand-written MAGE composition
    S, K = L - 1, 16
    gt = torch.randint(0, K, (B, S))
    mask = (torch.rand(B, L) > 0.4).double()
    q = SL.MaskedTokenLoss(K, smoothing)
    got = q(gt, x, mask)
    assert q.last_route.name == 'torch'
    logp = F.log_softmax(x[:, 1:, :K].reshape(B * S, -1), -1)
    per = (1 - smoothing) * -logp.gather(-1, gt.reshape(-1, 1))[:, 0] + smoothing * -logp.mean(-1)
    want = (per.reshape(B, S) * mask[:, 1:]).sum() / mask[:, 1:].sum()
    assert abs(float(got - want)) <= 1e-13
    full = torch.cat([torch.full((B, 1), -100), gt], 1).reshape(-1).numpy()
    w = mask.clone()
    w[:, 0] = 0
    r = ref.reference(x.reshape(-1, Vt)[:, :K].numpy(), ref.row_targets(full, 0, K), smoothing, w.reshape(-1).numpy())
    assert abs(r['total'] / r['wsum'] - float(want)) <= eps_tol


def test_reference_gradient_is_the_autograd_gradient():
    torch.manual_seed(5)
    x = (torch.randn(5, 17, dtype=torch.float64) * 2).requires_grad_()
    t = torch.tensor([3, 0, -100, 16, 7])
    F.cross_entropy(x, t, ignore_index=-100, label_smoothing=0.25, reduction='sum').backward()
    r = ref.reference(x.detach().numpy(), ref.row_targets(t.numpy(), 0, 17), 0.25)
    assert np.abs(r['grad_unit'] - x.grad.numpy()).max() <= 1e-14
    assert np.array_equal(r['live'], [True, True, False, True, True])


def test_case_grid_covers_what_the_issue_lists():
    cs = ref.cases()
    assert {c[0] for c in cs} == set(ref.VS + ref.BOUNDARY_VS + [ref.LONG_V])
    assert {c[1] for c in cs} == set(ref.STARTS) and {c[2] for c in cs} == set(ref.RS) and {c[3] for c in cs} == set(ref.DTYPES)
    kinds = set()
    for (V, start, R, dtype, seed) in cs:
        x, t = ref.make_case(V, start, R, dtype, seed)
        assert x.shape == (R, start + V + ref.PAD) and x.dtype == dtype
        a = ref.slice64(x, start, V)
        kinds |= {(r + seed) % 4 for r in range(R)}
        assert np.isfinite(a).all() and np.abs(a).max() <= 60.0
    assert kinds == {0, 1, 2, 3}
    assert any(np.abs(ref.slice64(*ref.make_case(*c)[:1], c[1], c[0])).max() == 60.0 for c in cs)
