"""CPU checks of LPIPSLoss: the reference's config dicts build, the state-dict keys are the reference's, the VGG16 taps, the
``torch`` route against the float64 restatement the GPU tests hold the kernels to, reductions, float64, where gradients go, the
restatement's analytic gradient against float64 autograd, the route clauses, the ABI limits and the bindings."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lpips_ref as ref
import vector_quantization_amd as vqa
from vector_quantization_amd import _lib, ops, perceptual_losses
from vector_quantization_amd.image_losses import column_of, is_plain
from vector_quantization_amd.quantizers import routes
from vector_quantization_amd.registries import VQIRLossRegistry, VQLossRegistry

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)


@pytest.fixture(scope='module')
def loss():
    torch.manual_seed(7)
    return vqa.LPIPSLoss().eval()


@pytest.fixture(scope='module')
def images():
    gen = torch.Generator().manual_seed(11)
    image = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
    pred = (image + 0.3 * torch.randn(2, 3, 32, 32, generator=gen)).clamp(-1, 1)
    return pred, image


def expected_value(loss, pred, image):
    """float64 restatement on the module's own features: ([B], the summed plain-fp32 margin)."""
    with torch.no_grad():
        pf, tf = loss.extract_features(pred), loss.extract_features(image)
    total, margin = 0.0, 0.0
    for f, g, conv in zip(pf, tf, loss._convs):
        w = conv.weight.double().reshape(-1).numpy()
        total = total + ref.reference(ref.as64(f), ref.as64(g), w)['value']
        margin += ref.plain_fp32_bound(f.shape[1], float(np.abs(w).max()))
    return total, margin + 5 * 2.0 ** -24 * float(np.abs(total).max())


def test_reference_configs_build():
    from vector_quantization_amd import registries
    a = VQIRLossRegistry.build(dict(type='LPIPSLoss'))                          # configs/vqgan/model.py:29
    assert type(a) is vqa.LPIPSLoss and a._reduction == 'mean' and a._weight == 1.0
    runner = dict(type='VQLossRegistry.VQIRLossRegistry.LPIPSLoss')            # configs/vqgan/runner.py:85-87
    for registry in (VQLossRegistry, registries.VQRegistry, registries.ModelRegistry):
        assert type(registry.build(dict(runner))) is vqa.LPIPSLoss
    c = VQIRLossRegistry.build(dict(type='LPIPSLoss', reduction='none', weight=0.5))
    assert c._reduction == 'none' and c._weight == 0.5
    assert not column_of(a) and not is_plain(a)                                 # not a column of ops.image_metrics
    assert a.init_weights(vqa.Config()) is False


def test_state_dict_keys_and_frozen_parameters(loss):
    want = {'_mean', '_std'} | {f'_vgg.features.{i}.{n}' for i in CONV_INDICES for n in ('weight', 'bias')} \
        | {f'_convs.{i}.weight' for i in range(5)}
    sd = loss.state_dict()
    assert set(sd) == want
    assert sd['_mean'].shape == sd['_std'].shape == (1, 3, 1, 1)
    assert torch.allclose(sd['_mean'].flatten(), torch.tensor([-.030, -.088, -.188]))
    assert torch.allclose(sd['_std'].flatten(), torch.tensor([.458, .448, .450]))
    assert [tuple(sd[f'_convs.{i}.weight'].shape) for i in range(5)] == [(1, c, 1, 1) for c in ref.CHANNELS]
    assert len(loss._vgg.features) == 31 and isinstance(loss._dropout, torch.nn.Dropout) and loss._dropout.p == 0.5
    assert not any(p.requires_grad for p in loss.parameters())
    # a reference checkpoint carries the classifier the reference runs and throws away
    extra = dict(sd)
    extra['_vgg.classifier.0.weight'] = torch.zeros(4, 4)
    extra['_vgg.classifier.0.bias'] = torch.zeros(4)
    extra['_vgg.classifier.6.weight'] = torch.zeros(2, 4)
    other = vqa.LPIPSLoss()
    other.load_state_dict(extra)                                                # strict
    assert all(torch.equal(other.state_dict()[k], sd[k]) for k in sd)
    nested = torch.nn.ModuleDict(dict(lpips_r_loss=vqa.LPIPSLoss()))
    nested.load_state_dict({f'lpips_r_loss.{k}': v for k, v in extra.items()})
    with pytest.raises(RuntimeError):
        other.load_state_dict(dict(sd, bogus=torch.zeros(1)))


def test_init_weights_loads_the_convs(tmp_path, loss):
    path = tmp_path / 'vgg.pth.converted'
    torch.save({f'{i}.weight': torch.full((1, c, 1, 1), float(i)) for i, c in enumerate(ref.CHANNELS)}, path)
    fresh = vqa.LPIPSLoss()
    assert fresh.init_weights(vqa.Config(pretrained=str(path))) is False
    assert all(float(conv.weight.mean()) == float(i) for i, conv in enumerate(fresh._convs))
    assert fresh.init_weights(vqa.Config(pretrained=str(tmp_path / 'missing'))) is False


def test_taps(loss, images):
    with torch.no_grad():
        feats = loss.extract_features(images[0])
    assert [tuple(f.shape) for f in feats] == [(2, c, 32 >> i, 32 >> i) for i, c in enumerate(ref.CHANNELS)]
    assert all(float(f.min()) >= 0.0 for f in feats)                             # behind a ReLU each


def test_cpu_route_and_value(loss, images):
    pred, image = images
    with torch.no_grad():
        got = loss(pred, image)
    assert loss.last_route.name == 'torch' and 'cpu' in loss.last_route.why and 'device' in loss.last_route.why
    want, margin = expected_value(loss, pred, image)
    print(f'cpu eval: value {float(got):.6f}, |err| {abs(float(got) - want.mean()):.3e}, margin {margin:.3e}')
    assert got.shape == () and got.dtype == torch.float32
    assert abs(float(got) - float(want.mean())) <= margin


def test_reductions_and_weight(images):
    pred, image = images
    torch.manual_seed(7)
    none = vqa.LPIPSLoss(reduction='none').eval()
    state = none.state_dict()
    with torch.no_grad():
        per = none(pred, image)
        assert per.shape == (2, 1, 1, 1)
        for reduction, fold in (('mean', per.mean()), ('sum', per.sum())):
            other = vqa.LPIPSLoss(reduction=reduction, weight=0.25).eval()
            other.load_state_dict(state)
            out = other(pred, image)
            assert out.shape == () and torch.allclose(out, fold * 0.25, rtol=1e-6, atol=0)
    want, margin = expected_value(none, pred, image)
    assert np.abs(per.flatten().numpy() - want).max() <= margin


def test_float64_goes_through_torch(loss, images):
    pred, image = images
    double = vqa.LPIPSLoss().double().eval()
    double.load_state_dict(loss.state_dict())
    with torch.no_grad():
        got = double(pred.double(), image.double())
    assert got.dtype == torch.float64 and double.last_route.name == 'torch'
    with torch.no_grad():
        pf, tf = double.extract_features(pred.double()), double.extract_features(image.double())
    want = sum(ref.reference(ref.as64(f), ref.as64(g), conv.weight.reshape(-1).numpy(), eps=1e-10)['value']
               for f, g, conv in zip(pf, tf, double._convs))
    assert abs(float(got) - float(want.mean())) <= 1e-12


def test_gradients_reach_pred_image_only(loss, images):
    pred, image = images
    pred = pred.clone().requires_grad_()
    image = image.clone().requires_grad_()
    loss(pred, image).backward()
    assert pred.grad is not None and float(pred.grad.abs().sum()) > 0
    assert image.grad is None
    assert all(p.grad is None for p in loss.parameters())


def test_train_mode_drops(loss, images):
    pred, image = images
    train = vqa.LPIPSLoss()
    train.load_state_dict(loss.state_dict())
    assert train.training and train._dropout.training
    with torch.no_grad():
        torch.manual_seed(0)
        a = train(pred, image)
        b = train(pred, image)
        assert float(a) != float(b)                                             # another mask
        train._dropout.eval()
        assert float(train(pred, image)) == float(loss(pred, image))


@pytest.mark.parametrize('C,B,H,W', [(3, 2, 5, 7), (64, 1, 3, 4), (65, 2, 2, 2)])
def test_analytic_gradient_is_float64_autograd(C, B, H, W):
    pred, target, w = ref.make_layer(C, B, H, W, seed=3)
    f = pred.double().clone().requires_grad_()
    g_out = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
    mask = (torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(5)) < 0.5)
    for m, scale in ((None, 1.0), (mask, 2.0)):
        f.grad = None
        value = ref.torch_composition(f, target.double(), w.double(), m, scale)
        (value * g_out).sum().backward()
        e = ref.reference(ref.as64(pred), ref.as64(target), w.reshape(-1).numpy(), None if m is None else ref.as64(m), scale,
                          eps=1e-10)                                            # float64 torch ops compare with the double
        assert e['clamped'].any() and not e['clamped'].all()                    # a clamped pixel is among them
        assert np.abs(e['value'] - value.detach().numpy()).max() <= 1e-12
        want = f.grad.reshape(B, C, -1).numpy()
        got = e['grad_unit'] * g_out.numpy()[:, None, None]
        assert (np.abs(got - want) <= 1e-12 * np.maximum(e['h'], 1.0)[:, None, :]).all()


def test_route_clauses(loss, images):
    feats = [torch.zeros(2, c, 4, 4) for c in ref.CHANNELS]
    assert 'device cpu' in routes.lpips_why(loss, feats, feats).why

    class Own(vqa.LPIPSLoss):
        def extract_features(self, image):
            return super().extract_features(image)

    class OwnTorch(vqa.LPIPSLoss):
        def forward_torch(self, pred_image, image):
            return super().forward_torch(pred_image, image)

    torch.manual_seed(0)
    assert routes.lpips_why(Own(), feats, feats) == routes.Route('torch', 'Own overrides extract_features')
    assert routes.lpips_why(OwnTorch(), feats, feats).why == 'OwnTorch overrides forward_torch'
    meta = [torch.zeros(2, c, 4, 4, device='meta') for c in ref.CHANNELS]
    # the clauses that read only dtypes, shapes and strides (ops.lpips_refusal)
    f = torch.zeros(2, 64, 4, 4)
    assert ops.lpips_refusal(f, f) == '' and ops.lpips_layout(f, f) == 'map'
    cl = f.contiguous(memory_format=torch.channels_last)
    assert ops.lpips_refusal(cl, cl) == '' and ops.lpips_layout(cl, cl) == 'rows'
    assert 'differ in layout' in ops.lpips_refusal(f, cl)
    assert 'float64' in ops.lpips_refusal(f.double(), f)
    assert 'neither NCHW-contiguous nor channels-last' in ops.lpips_refusal(f[:, :, ::2], f[:, :, ::2])
    assert 'one shape' in ops.lpips_refusal(f, f[:1])
    assert 'weights' in ops.lpips_refusal(f, f, torch.zeros(1, 63, 1, 1))
    one = torch.zeros(2, 1, 4, 4)
    assert ops.lpips_layout(one, one.contiguous(memory_format=torch.channels_last)) == 'map'
    del meta


def test_bounds_restate_the_header():
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'vqhip.h')).read()
    assert '#define VQHIP_LPIPS_CHAIN(C) ((double)((C) / 4 + 12))' in header
    assert '((8.0 * VQHIP_LPIPS_CHAIN(C) + 56.0) * 5.9604644775390625e-08 * 1.001953125 * (double)(wabs))' in header
    assert '((16.0 * VQHIP_LPIPS_CHAIN(C) + 136.0) * 5.9604644775390625e-08 * 1.001953125 * (double)(wabs) * (double)(h))' in header
    for C in (1, 3, 64, 65, 512, 1 << 16):
        assert ref.chain(C) == _lib.lpips_chain(C) == C // 4 + 12
        assert ref.bound(C, 0.75) == _lib.lpips_bound(C, 0.75) == (8 * (C // 4 + 12) + 56) * 5.9604644775390625e-08 * 1.001953125 * 0.75
        assert ref.grad_bound(C, 0.75, 3.0) == _lib.lpips_grad_bound(C, 0.75, 3.0)
    assert ref.EPS == float(np.float32(_lib.LPIPS_EPS))


def test_abi_limits_refuse_before_any_hip_call():
    lib = _lib.lib()
    assert lib.vqhip_version() == _lib.ABI_VERSION
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    F32, MAP = _lib.DTYPE_F32, _lib.LAYOUT_MAP

    def fwd(pred=p, pd=F32, target=p, td=F32, layout=MAP, B=1, C=4, P=4, w=p, seed=None, prob=0.5, layer=0, stats=p, value=p):
        return lib.vqhip_lpips_fwd(pred, pd, target, td, layout, B, C, P, w, seed, prob, layer, stats, value, 0, None)

    def bwd(pred=p, stats=p, g=p, grad=p, C=4, seed=None, prob=0.5):
        return lib.vqhip_lpips_bwd(pred, F32, p, F32, MAP, 1, C, 4, p, seed, prob, 0, stats, g, grad, None)

    EINVAL = 1 if not hasattr(_lib, 'EINVAL') else _lib.EINVAL
    bad = [fwd(pred=None), fwd(target=None), fwd(w=None), fwd(stats=None), fwd(value=None), fwd(pd=_lib.DTYPE_I32), fwd(td=_lib.DTYPE_U8),
           fwd(layout=2), fwd(B=0), fwd(P=0), fwd(C=0), fwd(C=(1 << 16) + 1), fwd(B=1 << 16, P=1 << 15), fwd(layer=-1),
           fwd(layer=(1 << 16) + 1), fwd(seed=p, prob=1.0), fwd(seed=p, prob=-0.1), fwd(seed=p, prob=float('nan')),
           bwd(pred=None), bwd(stats=None), bwd(g=None), bwd(grad=None), bwd(C=0), bwd(seed=p, prob=1.5),
           lib.vqhip_lpips_keep_mask(None, 0.5, 0, 1, 4, 4, p, None), lib.vqhip_lpips_keep_mask(p, 0.5, 0, 1, 4, 4, None, None),
           lib.vqhip_lpips_keep_mask(p, 1.0, 0, 1, 4, 4, p, None), lib.vqhip_lpips_keep_mask(p, 0.5, 0, 0, 4, 4, p, None)]
    assert all(rc != 0 for rc in bad) and len(set(bad)) == 1, bad
    assert b'vqhip_lpips_keep_mask' in lib.vqhip_last_error()
    for name in ('lpips_layer_forward', 'lpips_layer_backward', 'lpips_keep_mask', 'lpips_refusal', 'lpips_distance'):
        assert callable(getattr(ops, name))
    with pytest.raises(_lib.VqhipError):
        ops.lpips_layer_forward(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2), torch.zeros(4))
    assert perceptual_losses.TAPS == (3, 8, 15, 22, 29)
