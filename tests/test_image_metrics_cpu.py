"""CPU checks of the reconstruction metrics: the test reference against an independent restatement of scikit-image's SSIM, the
``torch`` route of the four loss classes against that reference, the registries, the route reasons, the refusals and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import image_metrics_ref as ref
from vector_quantization_amd import _lib, image_losses, ops, registries, runners
from vector_quantization_amd.quantizers import routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


def _bytes(kind, B, C, H, W, dtype):
    pred, image = ref.make_pair(kind, B, C, H, W, dtype)
    return ref.decode(pred).numpy(), ref.decode(image).numpy()


def test_integer_moment_ssim_agrees_with_the_restated_scikit_image_path():
    """(b) against (c) within 1e-12 over the case grid (the two evaluate the same definition in float64; what separates them
    is the cancellation in (c)'s `uxx - ux * ux`, of the order of 1e-16 / C2)."""
    worst = 0.0
    for (B, C, H, W) in ref.grid():
        for kind in ref.KINDS:
            for dtype in (torch.float32, torch.uint8):
                p, q = _bytes(kind, B, C, H, W, dtype)
                b = ref.expected(kind, B, C, H, W, dtype)['ssim']
                c = np.array([ref.ssim_restated(pi / 255.0, qi / 255.0) for pi, qi in zip(p, q)])
                worst = max(worst, float(np.abs(b - c).max()))
                assert np.abs(b - c).max() <= 1e-12, (kind, B, C, H, W, dtype, b, c)
    print(f'largest |(b) - (c)| = {worst:.3e}')


def test_reference_extremes():
    e = ref.expected('identical', 5, 3, 16, 20, torch.float32)
    assert (e['abs_sum'] == 0).all() and (e['sq_sum'] == 0).all() and (e['ssim'] == 1.0).all() and np.isposinf(e['psnr']).all()
    e = ref.expected('black_white', 1, 3, 16, 20, torch.float32)
    assert e['l1'][0] == 1.0 and e['mse'][0] == 1.0 and e['psnr'][0] == 0.0
    assert abs(e['ssim'][0] - ref.C1 / (1.0 + ref.C1)) <= 1e-15                 # flat windows: only the luminance term is left


def test_skimage_itself_where_it_exists():
    metrics = pytest.importorskip('skimage.metrics')
    for kind in ('noise', 'near', 'black_white'):
        p, q = _bytes(kind, 5, 3, 33, 65, torch.float32)
        b = ref.expected(kind, 5, 3, 33, 65, torch.float32)['ssim']
        for i in range(5):
            got = metrics.structural_similarity((p[i] / 255).astype(np.float32), (q[i] / 255).astype(np.float32), channel_axis=0, data_range=1)
            assert abs(got - b[i]) <= 1e-6, (kind, i, got, b[i])


@pytest.mark.parametrize('kind', ref.KINDS)
def test_torch_route_of_the_four_classes(kind):
    """fp32 arithmetic on image / 255: every element of |x - y| and (x - y)^2 carries at most 3 roundings (the two divisions,
    the difference; the square one more) and torch's pairwise mean adds less than one more on this size: 4 * 2^-24 relative.
    SSIMLoss is float64 on float64 images: 1e-12 (its avg_pool2d form cancels like (c))."""
    B, C, H, W = 5, 3, 33, 65
    p, q = _bytes(kind, B, C, H, W, torch.float32)
    e = ref.expected(kind, B, C, H, W, torch.float32)
    x, y = torch.from_numpy(p).float() / 255, torch.from_numpy(q).float() / 255
    for klass, name in ((image_losses.L1Loss, 'l1'), (image_losses.MSELoss, 'mse')):
        loss = klass(reduction='none')
        got = loss(x, y)
        assert got.shape == (B, C, H, W) and loss.last_route.name == 'torch'
        got = got.reshape(B, -1).mean(1).double().numpy()
        assert (np.abs(got - e[name]) <= 4 * U32 * e[name]).all(), (name, got, e[name])
        assert abs(float(klass()(x, y)) - e[name].mean()) <= 5 * U32 * e[name].mean()
    psnr = image_losses.PSNRLoss(reduction='none')(x, y).double().numpy()
    finite = np.isfinite(e['psnr'])
    assert (np.isposinf(psnr) == ~finite).all()
    # d psnr = (10 / ln 10) d mse / mse, plus log10 and the product in fp32
    assert (np.abs(psnr[finite] - e['psnr'][finite]) <= (10 / np.log(10)) * 4 * U32 + 4 * U32 * np.abs(e['psnr'][finite]) + U32).all()
    ssim = image_losses.SSIMLoss(reduction='none')(torch.from_numpy(p).double() / 255, torch.from_numpy(q).double() / 255)
    assert ssim.dtype == torch.float64 and (np.abs(ssim.numpy() - e['ssim']) <= 1e-12).all()
    # uint8 images on the CPU: per image, the same composition
    got = image_losses.L1Loss(reduction='none')(torch.from_numpy(p), torch.from_numpy(q))
    assert got.shape == (B,) and (np.abs(got.double().numpy() - e['l1']) <= 4 * U32 * e['l1']).all()


def test_l1_mse_psnr_keep_autograd_on_the_torch_route():
    x = torch.rand(2, 3, 8, 8, requires_grad=True)
    y = torch.rand(2, 3, 8, 8)
    for klass in (image_losses.L1Loss, image_losses.MSELoss, image_losses.PSNRLoss):
        (g,) = torch.autograd.grad(klass()(x, y), x)
        assert g.shape == x.shape and bool(g.abs().sum() > 0)


# configs/vqgan/runner.py:93-116 of the reference, as written there (f-strings expanded)
SHIPPED = dict(
    l1_image_loss=dict(type='VQMetricRegistry.ImageLossMetric', loss=dict(type='VQLossRegistry.VQIRLossRegistry.L1Loss'),
                       pred_image='["pred_image"]', image='["image"]'),
    mse_image_loss=dict(type='VQMetricRegistry.ImageLossMetric', loss=dict(type='VQLossRegistry.VQIRLossRegistry.MSELoss'),
                        pred_image='["pred_image"]', image='["image"]'),
    psnr=dict(type='VQMetricRegistry.ImageLossMetric', loss=dict(type='VQLossRegistry.VQIRLossRegistry.PSNRLoss'),
              pred_image='["pred_image"]', image='["image"]'),
    ssim=dict(type='VQMetricRegistry.ImageLossMetric', loss=dict(type='VQLossRegistry.VQIRLossRegistry.SSIMLoss'),
              pred_image='["pred_image"]', image='["image"]'),
)
COLUMN = dict(l1_image_loss='l1', mse_image_loss='mse', psnr='psnr', ssim='ssim')


def test_shipped_metric_configs_build_and_run_on_cpu():
    """The four dicts build through the registries unchanged; on CPU tensors each takes the torch route on decode(v) / 255 and
    accumulates the per-image values; summary() is their mean over both batches."""
    assert issubclass(registries.VQIRLossRegistry, registries.VQLossRegistry) and issubclass(registries.VQITMetricRegistry, registries.VQMetricRegistry)
    built = {k: registries.VQMetricRegistry.build(v) for k, v in SHIPPED.items()}
    batches = [ref.make_pair(kind, 5, 3, 16, 20, torch.float32) for kind in ('noise', 'near')]
    want = {k: np.concatenate([ref.expected(kind, 5, 3, 16, 20, torch.float32)[c] for kind in ('noise', 'near')]) for k, c in COLUMN.items()}
    for name, m in built.items():
        assert isinstance(m, runners.ImageLossMetric) and type(m._loss).__name__ == SHIPPED[name]['loss']['type'].rsplit('.', 1)[-1]
        for pred, image in batches:
            memo = m.forward({}, dict(pred_image=pred, image=image))
            assert m.last_route.name == 'torch' and 'not on a GPU' in m.last_route.why and m.last.shape == (5,)
            assert 'image_metrics' not in memo
        # the route runs on fp32 images (decode(v) / 255 is fp32): 1e-5 here; the routes' own bounds are held above
        assert abs(m.summary({}) - want[name].mean()) <= 1e-5 * max(1.0, abs(want[name].mean())), name


def test_a_dataset_with_its_own_decode_is_asked_once_per_pair():
    class Dataset:
        calls = 0

        @classmethod
        def decode(cls, images):
            cls.calls += 1
            return (images * 255).clamp(0, 255).to(torch.uint8)

    runner = type('Runner', (), dict(dataset=Dataset()))()
    built = {k: registries.VQMetricRegistry.build(v) for k, v in SHIPPED.items()}
    x = torch.rand(2, 3, 8, 8)
    memo = dict(pred_image=x, image=x.flip(0), other=x.roll(1, 2))
    for m in built.values():
        m.bind(runner)
        assert m._decode()[1] is False
        memo = m.forward({}, memo)
        assert m.last.shape == (2,)
    assert Dataset.calls == 2                                                     # four metrics, one decode of each image
    # another pair of the same shape in the same memo is decoded on its own and gets its own values
    other = registries.VQMetricRegistry.build(dict(SHIPPED['l1_image_loss'], pred_image='["other"]'))
    other.bind(runner)
    other.forward({}, memo)
    assert Dataset.calls == 4 and not torch.equal(other.last, built['l1_image_loss'].last)
    want = (Dataset.decode(memo['other']).float() / 255 - Dataset.decode(memo['image']).float() / 255).abs().mean((1, 2, 3))
    assert torch.allclose(other.last, want, rtol=1e-6)
    # the kernel's decode stands for the dataset's only where that is declared: on the dataset or on the metric
    m = built['l1_image_loss']
    m.bind(type('Runner', (), dict(dataset=runners.ImageRangeMixin()))())
    assert m._decode()[1] is True
    Dataset.image_range_decode = True
    m.bind(runner)
    assert m._decode()[1] is True
    del Dataset.image_range_decode
    declared = registries.VQMetricRegistry.build(dict(SHIPPED['l1_image_loss'], image_range_decode=True))
    declared.bind(runner)
    assert declared._decode()[1] is True and m._decode()[1] is False


def test_route_reasons():
    x = torch.zeros(2, 3, 16, 16)

    class Meta:
        """A stand-in with a tensor's metadata on a GPU: the route is decided without touching the data."""
        def __init__(self, t, cuda=True):
            self.t, self.is_cuda, self.device = t, cuda, 'cuda:0' if cuda else t.device
        def __getattr__(self, k):
            return getattr(self.t, k)

    g = Meta(x)
    assert routes.image_metrics_why(g, g).name == 'fused'
    assert routes.image_metrics_why(Meta(x.to(torch.uint8)), Meta(x.bfloat16())).name == 'fused'
    assert routes.image_metrics_why(Meta(x.contiguous(memory_format=torch.channels_last)), g).name == 'fused'
    r = routes.image_metrics_why(x, x)
    assert r.name == 'torch' and 'not on a GPU' in r.why
    r = routes.image_metrics_why(Meta(x.double()), Meta(x.double()))
    assert r.name == 'torch' and 'float64' in r.why
    r = routes.image_metrics_why(Meta(x[:, :, ::2]), Meta(x[:, :, ::2]))
    assert r.name == 'torch' and 'neither NCHW-contiguous nor channels-last' in r.why
    big = Meta(torch.empty(1, 3, 1200, 1200, dtype=torch.uint8))
    r = routes.image_metrics_why(big, big)
    assert r.name == 'torch' and 'size cap' in r.why
    assert routes.image_metrics_why(big, big, ssim=False).name == 'fused'

    class Custom(image_losses.L1Loss):
        def forward(self, pred_image, image):
            return super().forward(pred_image, image) * 2

    r = routes.image_metrics_why(g, g, loss=Custom())
    assert r.name == 'torch' and 'overrides forward' in r.why
    assert routes.image_metrics_why(g, g, loss=image_losses.PSNRLoss()).name == 'fused'
    r = routes.image_metrics_why(g, g, loss=torch.nn.L1Loss())
    assert r.name == 'torch' and 'none of L1Loss, MSELoss, PSNRLoss and SSIMLoss' in r.why and 'overrides' not in r.why


def test_refusals_raise_value_error():
    x, low, narrow = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 6, 16), torch.zeros(2, 3, 16, 6)
    big = torch.empty(1, 3, 1200, 1200, dtype=torch.uint8)
    for pred, image, word in ((x, x[:1], 'must both be'), (x, x[:, :, :8], 'must both be'), (x[0], x[0], 'must both be'),
                              (x.double(), x.double(), 'float64'), (x[:, :, ::2], x[:, :, ::2], 'neither'),
                              (low, low, '7 x 7'), (narrow, narrow, '7 x 7'), (big, big, 'size cap')):
        with pytest.raises(ValueError, match=word):
            ops.image_metrics(pred, image)
    with pytest.raises(_lib.VqhipError):                                          # fine but for the device: there is no CPU path
        ops.image_metrics(low, low, ssim=False)


def test_c_abi_refuses_before_any_launch():
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    c1, c2 = ops.SSIM_C1, ops.SSIM_C2

    def call(B=2, C=3, H=16, W=16, want=1, pd=0, pl=0, qd=0, ql=0, ws_bytes=None, pred=fake, out=fake):
        need = L.vqhip_image_metrics_workspace_bytes(B, C, H, W)
        return L.vqhip_image_metrics(pred, pd, pl, fake, qd, ql, B, C, H, W, want, c1, c2, fake, need if ws_bytes is None else ws_bytes,
                                     out, fake, fake, None)

    assert L.vqhip_image_metrics_workspace_bytes(2, 3, 16, 16) == 2 * 3 * 1 * 32
    assert L.vqhip_image_metrics_workspace_bytes(4, 3, 128, 128) == 4 * 3 * 16 * 32
    assert L.vqhip_image_metrics_workspace_bytes(1, 1, 33, 65) == 2 * 3 * 32
    assert L.vqhip_image_metrics_workspace_bytes(0, 3, 16, 16) == 0
    assert call(pred=None) == -22 and call(out=None) == -22
    assert call(pd=2) == -22 and b'dtype' in L.vqhip_last_error()
    assert call(qd=3) == -22 and call(pd=6) == -22
    assert call(pl=2) == -22 and b'layout' in L.vqhip_last_error()
    assert call(ql=-1) == -22
    assert call(H=6) == -22 and b'7 x 7' in L.vqhip_last_error()
    assert call(W=6) == -22
    assert call(B=1, H=1200, W=1200) == -22 and b'2^22' in L.vqhip_last_error()
    assert call(B=0) == -22 and call(C=0) == -22 and call(H=0, want=0) == -22
    assert call(ws_bytes=2 * 3 * 32 - 1) == -22 and b'ws too small' in L.vqhip_last_error()
    assert call(B=1 << 20, C=1 << 12) == -22 and b'2^31' in L.vqhip_last_error()


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, 'include', 'vqhip.h')).read()

    def macro(name):
        return re.search(r'#define\s+' + name + r'\s+(\S+)', text).group(1)

    assert int(macro('VQHIP_DTYPE_U8')) == _lib.DTYPE_U8 == ops.IMAGE_DTYPES[torch.uint8]
    assert (int(macro('VQHIP_IMAGE_NCHW')), int(macro('VQHIP_IMAGE_NHWC'))) == (_lib.IMAGE_NCHW, _lib.IMAGE_NHWC)
    assert int(macro('VQHIP_IMAGE_METRICS_TILE')) == _lib.IMAGE_METRICS_TILE == ref.T
    assert float(macro('VQHIP_IMAGE_SSIM_BOUND')) == _lib.IMAGE_SSIM_BOUND == ref.SSIM_BOUND == 2.0 ** -40
    assert _lib.IMAGE_SSIM_MAX_WINDOWS == 1 << 22 and '(1ll << 22)' in text
    assert (ops.SSIM_C1, ops.SSIM_C2) == (ref.C1, ref.C2)
    decl = re.search(r'int vqhip_image_metrics\((.*?)\);', re.sub(r'/\*.*?\*/', '', text, flags=re.S), flags=re.S).group(1)
    kinds = []
    for arg in decl.split(','):
        arg = arg.strip()
        kinds.append(ctypes.c_void_p if '*' in arg else {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double}[arg.split()[0]])
    res, args = _lib.SIGNATURES['vqhip_image_metrics']
    assert res is ctypes.c_int and args == kinds
    assert _lib.SIGNATURES['vqhip_image_metrics_workspace_bytes'] == (ctypes.c_int64, [ctypes.c_int64] * 4)
