"""GPU checks of the fused reconstruction metrics (vqhip_image_metrics) against tests/image_metrics_ref.py: the integer sums
exactly (which pins the decode bit for bit), l1 and mse bit for bit, psnr within 2 double ulp, ssim within the bound derived in
include/vqhip.h.  No tolerance below is fitted to an output."""
import numpy as np
import pytest
import torch

import image_metrics_ref as ref
from vector_quantization_amd import image_losses, ops, registries, runners

pytestmark = pytest.mark.gpu
LAYOUTS = ['nchw', 'channels_last']


def _device(t: torch.Tensor, layout: str) -> torch.Tensor:
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if layout == 'channels_last' else t


def _host(out: dict) -> dict:
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got: dict, e: dict, what, ssim: bool = True) -> float:
    """Every assertion of the contract on one call; returns the largest ssim error as a share of the bound."""
    assert np.array_equal(got['abs_sum'], e['abs_sum']) and np.array_equal(got['sq_sum'], e['sq_sum']), what
    v = got['values64']
    assert np.array_equal(v[:, 0], e['l1']) and np.array_equal(v[:, 1], e['mse']), what
    assert (ref.ulps(v[:, 2], e['psnr']) <= 2).all(), (what, v[:, 2], e['psnr'])
    err = np.abs(v[:, 3] - e['ssim']) if ssim else np.zeros(1)
    assert (err <= ref.SSIM_BOUND).all() if ssim else np.isnan(v[:, 3]).all(), (what, v[:, 3], e['ssim'])
    assert np.array_equal(got['values32'], v.astype(np.float32), equal_nan=True), what
    for k, name in enumerate(ops.IMAGE_METRIC_COLUMNS):
        assert np.array_equal(got[name], got['values32'][:, k], equal_nan=True)
    return float(err.max() / ref.SSIM_BOUND)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', ref.DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_every_output_against_the_reference(dtype, layout):
    worst = 0.0
    for (B, C, H, W) in ref.grid():
        for kind in ref.KINDS:
            pred, image = ref.make_pair(kind, B, C, H, W, dtype)
            got = _host(ops.image_metrics(_device(pred, layout), _device(image, layout)))
            share = _check(got, ref.expected(kind, B, C, H, W, dtype), (kind, B, C, H, W, dtype, layout))
            worst = max(worst, share)
            if kind == 'identical':
                assert (got['values64'][:, 3] == 1.0).all() and np.isposinf(got['values64'][:, 2]).all()
                assert not got['abs_sum'].any() and not got['sq_sum'].any()
    print(f'{dtype} {layout}: largest ssim error {worst:.4f} of the bound 2^-40')


def test_mixed_dtypes_and_layouts_and_no_ssim():
    """Each tensor has its own dtype and layout; want_ssim = 0 takes images below 7 pixels."""
    B, C, H, W = 5, 3, 33, 65
    pred, _ = ref.make_pair('noise', B, C, H, W, torch.bfloat16)
    _, image = ref.make_pair('noise', B, C, H, W, torch.float32)
    e = ref.metrics(ref.decode(pred).numpy(), ref.decode(image).numpy())
    _check(_host(ops.image_metrics(_device(pred, 'channels_last'), _device(image, 'nchw'))), e, 'mixed')
    _check(_host(ops.image_metrics(_device(ref.decode(pred), 'nchw'), _device(image, 'channels_last'))), e, 'mixed u8')
    for (h, w) in ((1, 1), (3, 70), (6, 6), (33, 65)):
        pred, image = ref.make_pair('noise', 2, 3, h, w, torch.float16)
        got = _host(ops.image_metrics(pred.cuda(), image.cuda(), ssim=False))
        _check(got, ref.expected('noise', 2, 3, h, w, torch.float16, 0, False), ('no ssim', h, w), ssim=False)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: str(d).split('.')[-1])
def test_a_nan_pixel_marks_its_image_only(dtype):
    B, C, H, W = 5, 3, 33, 65
    pred, image = ref.make_pair('noise', B, C, H, W, dtype)
    clean = _host(ops.image_metrics(pred.cuda(), image.cuda()))
    for where in ((1, 2, 32, 64), (1, 0, 0, 0), (1, 1, 31, 33)):                  # image 2 of 5: a corner, the origin, a halo pixel
        for side in (0, 1):
            pair = [pred.clone(), image.clone()]
            pair[side][where] = float('nan')
            for layout in LAYOUTS:
                got = _host(ops.image_metrics(_device(pair[0], layout), _device(pair[1], layout)))
                assert np.isnan(got['values64'][1]).all() and np.isnan(got['values32'][1]).all()
                keep = [0, 2, 3, 4]
                for name in ('values64', 'values32', 'abs_sum', 'sq_sum'):
                    assert np.array_equal(got[name][keep], clean[name][keep]), (where, side, layout, name)
                e = ref.metrics(ref.decode(pair[0]).numpy(), ref.decode(pair[1]).numpy())     # the NaN counts as byte 0 in the sums
                assert np.array_equal(got['abs_sum'], e['abs_sum']) and np.array_equal(got['sq_sum'], e['sq_sum'])


@pytest.mark.parametrize('dtype', ref.DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_bit_equality_across_runs_layouts_and_batches(dtype):
    for (H, W) in ref.SHAPES:
        pred, image = ref.make_pair('near', 5, 3, H, W, dtype)
        a = _host(ops.image_metrics(pred.cuda(), image.cuda()))
        b = _host(ops.image_metrics(pred.cuda(), image.cuda()))
        c = _host(ops.image_metrics(_device(pred, 'channels_last'), _device(image, 'channels_last')))
        for name in ('values64', 'values32', 'abs_sum', 'sq_sum'):
            assert np.array_equal(a[name], b[name]) and np.array_equal(a[name], c[name]), (H, W, name)
        for i in (0, 3):
            alone = _host(ops.image_metrics(pred[i:i + 1].cuda(), image[i:i + 1].cuda()))
            for name in ('values64', 'values32', 'abs_sum', 'sq_sum'):
                assert np.array_equal(alone[name][0], a[name][i]), (H, W, i, name)


def _peak_beyond(fn, *tensors) -> int:
    """Peak allocation while fn runs, beyond what is allocated before it (the inputs) and what it returns."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(*tensors)
    torch.cuda.synchronize()
    peak, after = torch.cuda.max_memory_allocated(), torch.cuda.memory_allocated()     # after: the inputs and what fn returned
    del out
    assert after >= before
    return peak - after


def _torch_composition(pred, image):
    """The four metrics as the reference's validation loop composes them, SSIM through the torch route."""
    decode = runners.ImageRangeMixin.decode
    out = []
    for loss in (image_losses.L1Loss(reduction='none'), image_losses.MSELoss(reduction='none'),
                 image_losses.PSNRLoss(reduction='none'), image_losses.SSIMLoss(reduction='none')):
        v = loss(decode(pred) / 255, decode(image) / 255)
        out.append(v.reshape(v.shape[0], -1).mean(1))
    return out


def test_no_image_sized_intermediate():
    """At 4 x 3 x 128 x 128 the fused call allocates less than a quarter of one input beyond inputs and outputs; the torch
    composition on the same shape exceeds that, so the cap can tell the two apart."""
    pred, image = (t.cuda() for t in ref.make_pair('noise', 4, 3, 128, 128, torch.float32))
    cap = pred.numel() * pred.element_size() // 4
    ops.image_metrics(pred, image)                                                # (loads the library outside the measurement)
    fused = _peak_beyond(ops.image_metrics, pred, image)
    composed = _peak_beyond(_torch_composition, pred, image)
    print(f'peak beyond inputs and outputs: fused {fused} B, torch composition {composed} B, cap {cap} B')
    assert fused < cap
    assert composed > cap


SHIPPED = {name: dict(type='VQMetricRegistry.ImageLossMetric', loss=dict(type=f'VQLossRegistry.VQIRLossRegistry.{loss}'),
                      pred_image='["pred_image"]', image='["image"]')
           for name, loss in (('l1', 'L1Loss'), ('mse', 'MSELoss'), ('psnr', 'PSNRLoss'), ('ssim', 'SSIMLoss'))}


def test_four_metrics_share_one_launch_pair(monkeypatch):
    calls = []
    real = ops.image_metrics

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, 'image_metrics', counted)
    metrics = {k: registries.VQMetricRegistry.build(v) for k, v in SHIPPED.items()}
    total = {k: [] for k in metrics}
    for n, kind in enumerate(('noise', 'near')):
        pred, image = ref.make_pair(kind, 5, 3, 33, 65, torch.bfloat16)
        e = ref.expected(kind, 5, 3, 33, 65, torch.bfloat16)
        memo = dict(pred_image=_device(pred, 'channels_last'), image=image.cuda())
        direct = _host(real(memo['pred_image'], memo['image']))
        _check(direct, e, kind)
        for name, m in metrics.items():
            memo = m.forward({}, memo)
            assert m.last_route.name == 'fused', m.last_route.why
            assert np.array_equal(m.last.cpu().numpy(), direct[name], equal_nan=True), name    # its own column, bit for bit
            total[name].append(direct[name].astype(np.float64))
        assert len(calls) == n + 1                                                # one call per batch for all four
    for name, m in metrics.items():                                               # the float64 mean of the fp32 values: its own roundings only
        want = np.concatenate(total[name]).mean()
        assert abs(m.summary({}) - want) <= 16 * 2.0 ** -53 * abs(want), name


class _OwnDecode:
    """A dataset whose decode is not the kernel's: images in [0, 1]."""
    calls = 0

    @classmethod
    def decode(cls, images):
        cls.calls += 1
        return (images * 255).clamp(0, 255).to(torch.uint8)


def test_a_dataset_decode_is_asked_once_and_pairs_of_one_shape_stay_apart(monkeypatch):
    """With a dataset that decodes for itself the kernel gets uint8 temporaries.  Four metrics still make one call (and one
    decode per image); a second pair of the same shape in the same memo - whose temporaries the caching allocator would place
    at the addresses of the first pair's, were those freed - gets its own values."""
    calls = []
    real = ops.image_metrics

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, 'image_metrics', counted)
    monkeypatch.setattr(_OwnDecode, 'calls', 0)
    runner = type('Runner', (), dict(dataset=_OwnDecode()))()
    g = torch.Generator().manual_seed(7)
    image, pred, ema = (torch.rand(5, 3, 33, 65, generator=g).cuda() for _ in range(3))
    memo = dict(image=image, pred_image=pred, ema_pred_image=ema)
    want = {k: _host(real(_OwnDecode.decode(memo[k]), _OwnDecode.decode(image))) for k in ('pred_image', 'ema_pred_image')}
    _check(want['pred_image'], ref.metrics(_OwnDecode.decode(pred).cpu().numpy(), _OwnDecode.decode(image).cpu().numpy()), 'own decode')
    monkeypatch.setattr(_OwnDecode, 'calls', 0)
    for n, which in enumerate(('pred_image', 'ema_pred_image')):
        for name, config in SHIPPED.items():
            m = registries.VQMetricRegistry.build(dict(config, pred_image=f'["{which}"]'))
            m.bind(runner)
            memo = m.forward({}, memo)
            assert m.last_route.name == 'fused', m.last_route.why
            assert np.array_equal(m.last.cpu().numpy(), want[which][name]), (which, name)
        assert len(calls) == n + 1 and _OwnDecode.calls == 2 * (n + 1)
    assert not np.array_equal(want['pred_image']['l1'], want['ema_pred_image']['l1'])


def test_an_overridden_forward_takes_the_torch_route():
    class Doubled(image_losses.L1Loss):
        def forward(self, pred_image, image):
            return 2 * super().forward(pred_image, image)

    m = runners.ImageLossMetric(pred_image='["pred_image"]', image='["image"]', loss=Doubled(reduction='none'))
    pred, image = ref.make_pair('noise', 5, 3, 16, 20, torch.float32)
    memo = m.forward({}, dict(pred_image=pred.cuda(), image=image.cuda()))
    assert m.last_route.name == 'torch' and 'overrides forward' in m.last_route.why and 'image_metrics' not in memo
    e = ref.expected('noise', 5, 3, 16, 20, torch.float32)
    assert np.abs(m.last.double().cpu().numpy() - 2 * e['l1']).max() <= 8 * 2.0 ** -24 * 2 * e['l1'].max()


def test_uint8_images_take_the_fused_route_through_the_loss_classes():
    pred, image = ref.make_pair('near', 5, 3, 33, 65, torch.uint8)
    e = ref.expected('near', 5, 3, 33, 65, torch.uint8)
    for klass in (image_losses.L1Loss, image_losses.MSELoss, image_losses.PSNRLoss, image_losses.SSIMLoss):
        loss = klass(reduction='none')
        got = loss(pred.cuda(), image.cuda())
        assert loss.last_route.name == 'fused' and got.shape == (5,)
        assert np.array_equal(got.cpu().numpy(), ops.image_metrics(pred.cuda(), image.cuda())[klass.COLUMN].cpu().numpy())
        assert np.abs(got.double().cpu().numpy() - e[klass.COLUMN]).max() <= 2.0 ** -23 * np.abs(e[klass.COLUMN]).max()
