"""The fused LPIPS tail on the GPU, held to the float64 restatement of tests/lpips_ref.py: every tolerance is a bound of
include/vqhip.h plus the rounding into the output dtype.  Worst error / bound ratios are printed (profiles/lpips.txt).

Measured on an MI355X (worst error / bound over each grid): see the table in profiles/lpips.txt."""
import gc

import numpy as np
import pytest
import torch

import lpips_ref as ref
import vector_quantization_amd as vqa
from vector_quantization_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(autouse=True)
def leave_no_device_memory_behind():
    """Autograd graphs over the VGG16 features die with the collector, not with the test: collect here, so that the device
    memory this module held is back before any later test measures its own."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def dev(*ts):
    """CPU tensors on the GPU with their strides kept."""
    out = []
    for t in ts:
        fmt = torch.channels_last if t.dim() == 4 and not t.is_contiguous() else torch.contiguous_format
        out.append(t.cuda().contiguous(memory_format=fmt))
    return out


def guarded_like(pred: torch.Tensor):
    """(a NaN-prefilled buffer with the shape and strides of ``pred`` inside a flat allocation, the guard region behind it)."""
    flat = torch.full((pred.numel() + GUARD,), float('nan'), dtype=pred.dtype, device=pred.device)
    flat[pred.numel():] = 7.0
    return flat[:pred.numel()].as_strided(pred.shape, pred.stride()), flat[pred.numel():]


def check_layer(case, seed=None, p=0.5, layer=0):
    """Forward and backward of one layer against float64: the worst error / bound ratios (s, value, accumulated value, gradient)."""
    C, (B, H, W), dtypes, layout = case
    pred, target, w = ref.make_layer(C, B, H, W, dtypes, seed=C + B, layout=layout)
    f, g, wd = dev(pred, target, w)
    P = H * W
    mask, scale = None, 1.0
    if seed is not None:
        mask = ops.lpips_keep_mask(seed, p, layer, B, C, P).cpu().numpy()
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    wn = w.reshape(-1).double().numpy()
    e = ref.reference(ref.as64(pred), ref.as64(target), wn, mask, scale)
    wabs = float(np.abs(wn).max())
    fb = ref.bound(C, wabs) * scale
    out = ops.lpips_layer_forward(f, g, wd, seed=seed, p=p, layer=layer)
    s, value = out['s'].double().cpu().numpy(), out['value'].double().cpu().numpy()
    assert out['stats'].shape == (B, P, 4) and out['value'].shape == (B,)
    r_s, r_v = np.abs(s - e['s']).max() / fb, np.abs(value - e['value']).max() / fb
    twice = ops.lpips_layer_forward(f, g, wd, seed=seed, p=p, layer=layer, value=out['value'].clone())['value']
    r_a = np.abs(twice.double().cpu().numpy() - 2.0 * e['value']).max() / (2.0 * fb)
    g_out = torch.linspace(0.5, 1.5, B, device='cuda')
    buf, guard = guarded_like(f)
    grad = ops.lpips_layer_backward(f, g, wd, out['stats'], g_out, seed=seed, p=p, layer=layer, out=buf)
    assert grad.data_ptr() == buf.data_ptr() and not torch.isnan(buf).any(), case   # every element overwritten
    assert bool((guard == 7.0).all()), case                                         # nothing beyond it
    gn = g_out.double().cpu().numpy()[:, None, None]
    want = e['grad_unit'] * gn
    tol32 = ref.grad_bound(C, wabs, e['h'])[:, None, :] * scale * gn / P
    got = ref.as64(grad)
    tol = tol32 + ref.half_ulp(np.abs(want) + tol32, dtypes[0])
    ok = ref.grad_ok(got, want, tol, dtypes[0])
    finite = np.isfinite(got)
    r_g = (np.abs(got - want)[finite] / tol[finite]).max()
    assert ok.all(), (case, r_g)
    assert r_s <= 1.0 and r_v <= 1.0 and r_a <= 1.0, (case, r_s, r_v, r_a)
    return r_s, r_v, r_a, r_g


@pytest.mark.parametrize('dtypes', ref.DTYPES, ids=lambda d: f'{d[0]}-{d[1]}'.replace('torch.', ''))
def test_forward_and_backward_grid(dtypes):
    worst = np.zeros(4)
    for C in ref.CS:
        for bp in ref.BPS:
            for layout in ref.LAYOUTS:
                worst = np.maximum(worst, check_layer((C, bp, dtypes, layout)))
    print(f'lpips grid {dtypes[0]}/{dtypes[1]}: worst error / bound: s {worst[0]:.3f}  value {worst[1]:.3f}  '
          f'accumulated {worst[2]:.3f}  gradient (bound + half ulp) {worst[3]:.3f}')


def test_reproducibility():
    for layout in ref.LAYOUTS:
        for dtypes in (ref.DTYPES[0], ref.DTYPES[2]):
            pred, target, w = ref.make_layer(65, 3, 9, 29, dtypes, seed=1, layout=layout)
            f, g, wd = dev(pred, target, w)
            g_out = torch.tensor([0.5, 1.0, 1.5], device='cuda')
            a = ops.lpips_layer_forward(f, g, wd)
            b = ops.lpips_layer_forward(f, g, wd)
            assert torch.equal(a['stats'], b['stats']) and torch.equal(a['value'], b['value'])
            ga = ops.lpips_layer_backward(f, g, wd, a['stats'], g_out)
            assert torch.equal(ga, ops.lpips_layer_backward(f, g, wd, a['stats'], g_out))
            for i in range(3):                                                   # an image alone has the bits it has in the batch
                fi, gi = dev(pred[i:i + 1], target[i:i + 1])
                alone = ops.lpips_layer_forward(fi, gi, wd)
                assert torch.equal(alone['stats'][0], a['stats'][i]) and torch.equal(alone['value'][0], a['value'][i])
                assert torch.equal(ops.lpips_layer_backward(fi, gi, wd, alone['stats'], g_out[i:i + 1])[0], ga[i])
    # two autograd.grad calls on one graph
    feats = [ref.make_layer(c, 2, 4, 4, (torch.bfloat16, torch.bfloat16), seed=i) for i, c in enumerate(ref.CHANNELS)]
    preds = [t[0].cuda().requires_grad_() for t in feats]
    targets, weights = [t[1].cuda() for t in feats], [t[2].cuda() for t in feats]
    seed = torch.tensor([123, 456], dtype=torch.int32, device='cuda')
    for sd in (None, seed):
        value = ops.lpips_distance(preds, targets, weights, sd)
        assert value.shape == (2,) and value.dtype == torch.float32
        one = torch.autograd.grad(value.sum(), preds, retain_graph=True)
        two = torch.autograd.grad(value.sum(), preds, retain_graph=True)
        assert all(torch.equal(x, y) and x.dtype == torch.bfloat16 for x, y in zip(one, two))
        want = sum(ref.reference(ref.as64(f), ref.as64(g), w.reshape(-1).double().numpy(),
                                 None if sd is None else ops.lpips_keep_mask(sd, 0.5, i, 2, f.shape[1], 16).cpu().numpy(),
                                 1.0 if sd is None else 2.0)['value'] for i, (f, g, w) in enumerate(feats))
        margin = sum(ref.bound(c, float(w.abs().max())) for c, (_, _, w) in zip(ref.CHANNELS, feats)) * (1.0 if sd is None else 2.0)
        assert np.abs(value.detach().double().cpu().numpy() - want).max() <= margin


@pytest.mark.parametrize('layout', ref.LAYOUTS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_degenerate_and_non_finite_table(layout, dtype):
    C, H, W = 65, 5, 7
    cases = ['clean', 'zero', 'sub_eps', 'nan_pred', 'pinf_pred', 'ninf_pred', 'nan_target']
    B, P, pix, ch = len(cases), H * W, 17, 33
    gen = torch.Generator().manual_seed(5)
    pred = torch.randn(B, C, P, generator=gen).clamp_min(0.0) + 0.0
    target = (pred + 0.5 * torch.randn(B, C, P, generator=gen)).clamp_min(0.0)
    w = torch.randn(1, C, 1, 1, generator=gen)
    clean_pred, clean_target = pred.clone(), target.clone()
    pred[1, :, pix] = 0.0
    pred[2, :, pix] *= 1e-12
    pred[3, ch, pix] = float('nan')
    pred[4, ch, pix] = float('inf')
    pred[5, ch, pix] = float('-inf')
    target[6, ch, pix] = float('nan')
    fmt = torch.channels_last if layout == 'rows' else torch.contiguous_format

    def run(p_, t_):
        f = p_.view(B, C, H, W).to(dtype).cuda().contiguous(memory_format=fmt)
        g = t_.view(B, C, H, W).to(dtype).cuda().contiguous(memory_format=fmt)
        out = ops.lpips_layer_forward(f, g, w.cuda())
        grad = ops.lpips_layer_backward(f, g, w.cuda(), out['stats'], torch.ones(B, device='cuda'))
        e = ref.reference(ref.as64(f), ref.as64(g), w.reshape(-1).double().numpy())
        return out, grad.reshape(B, C, P), e

    out, grad, e = run(pred, target)
    base, base_grad, _ = run(clean_pred, clean_target)
    s, value, gn = out['s'].cpu().numpy(), out['value'].cpu().numpy(), grad.float().cpu().numpy()
    assert np.array_equal(np.isnan(s), np.isnan(e['s'])) and np.array_equal(np.isnan(value), np.isnan(e['value']))
    assert np.array_equal(np.isnan(gn), np.isnan(e['grad_unit']))
    assert np.isnan(value).tolist() == [False, False, False, True, True, True, True]
    for b in (3, 4, 5, 6):                                                      # the whole gradient column of the pixel, only it
        assert np.isnan(gn[b, :, pix]).all() and np.isnan(gn[b]).sum() == C and np.isnan(s[b]).sum() == 1
    assert e['clamped'][1, pix] and e['clamped'][2, pix] and e['clamped'].sum() == 2
    wabs, g0 = float(w.abs().max()), e['grad_unit']
    for b in (1, 2):                                                            # finite, huge, within the bound at h = 1 / e
        assert abs(s[b, pix] - e['s'][b, pix]) <= ref.bound(C, wabs)
        tol = ref.grad_bound(C, wabs, 1.0 / ref.EPS) / P
        tol = tol + ref.half_ulp(np.abs(g0[b, :, pix]) + tol, dtype)
        assert (np.abs(gn[b, :, pix] - g0[b, :, pix]) <= tol).all() and np.abs(gn[b, :, pix]).max() > 1e6
    # untouched images and pixels keep the bits of the clean run
    assert torch.equal(out['value'][0], base['value'][0]) and torch.equal(grad[0], base_grad[0])
    others = [i for i in range(P) if i != pix]
    assert torch.equal(out['stats'][:, others], base['stats'][:, others]) and torch.equal(grad[:, :, others], base_grad[:, :, others])


@pytest.mark.parametrize('p', [0.5, 0.25])
def test_dropout(p):
    seed = torch.tensor([20240611, -77], dtype=torch.int32, device='cuda')
    other = torch.tensor([20240612, -77], dtype=torch.int32, device='cuda')
    worst = np.zeros(4)
    for C, bp in ((3, ref.BPS[1]), (65, ref.BPS[2]), (512, ref.BPS[1])):
        for dtypes in (ref.DTYPES[0], ref.DTYPES[2]):
            for layout in ref.LAYOUTS:                                           # both layouts are held to ONE mask, the logical one
                worst = np.maximum(worst, check_layer((C, bp, dtypes, layout), seed=seed, p=p, layer=2))
    print(f'lpips dropout p={p}: worst error / bound: s {worst[0]:.3f}  value {worst[1]:.3f}  accumulated {worst[2]:.3f}  '
          f'gradient (bound + half ulp) {worst[3]:.3f}')
    # the same seed gives the same bits, another seed or layer another mask; NCHW and channels-last draw the same mask
    pred, target, w = ref.make_layer(64, 2, 9, 29, seed=2)
    f, g, wd = dev(pred, target, w)
    a = ops.lpips_layer_forward(f, g, wd, seed=seed, p=p, layer=1)
    b = ops.lpips_layer_forward(f, g, wd, seed=seed, p=p, layer=1)
    assert torch.equal(a['stats'], b['stats']) and torch.equal(a['value'], b['value'])
    g_out = torch.ones(2, device='cuda')
    assert torch.equal(ops.lpips_layer_backward(f, g, wd, a['stats'], g_out, seed=seed, p=p, layer=1),
                       ops.lpips_layer_backward(f, g, wd, a['stats'], g_out, seed=seed, p=p, layer=1))
    assert not torch.equal(a['value'], ops.lpips_layer_forward(f, g, wd, seed=other, p=p, layer=1)['value'])
    m = ops.lpips_keep_mask(seed, p, 1, 2, 64, 261)
    assert not torch.equal(m, ops.lpips_keep_mask(other, p, 1, 2, 64, 261)) and not torch.equal(m, ops.lpips_keep_mask(seed, p, 0, 2, 64, 261))
    fr, gr = dev(pred.contiguous(memory_format=torch.channels_last), target.contiguous(memory_format=torch.channels_last))
    rows = ops.lpips_layer_forward(fr, gr, wd, seed=seed, p=p, layer=1)
    e = ref.reference(ref.as64(pred), ref.as64(target), w.reshape(-1).double().numpy(), m.cpu().numpy(), float(np.float32(1) / np.float32(1 - p)))
    fb = ref.bound(64, float(w.abs().max())) / (1 - p)
    assert np.abs(rows['s'].double().cpu().numpy() - e['s']).max() <= fb and np.abs(a['s'].double().cpu().numpy() - e['s']).max() <= fb
    # the kept share over n = 131 072 elements, and per channel over its 2 048: within 5 sigma, sigma = sqrt(p (1 - p) / n)
    big = ops.lpips_keep_mask(seed, p, 0, 2, 64, 32 * 32).double()
    n = big.numel()
    assert n == 131072 and abs(float(big.mean()) - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5
    per = big.mean(dim=(0, 2))
    assert float((per - (1 - p)).abs().max()) <= 5 * (p * (1 - p) / (n // 64)) ** 0.5


def module_reference(loss, pred, image):
    with torch.no_grad():
        pf, tf = loss.extract_features(pred), loss.extract_features(image)
    total, margin = 0.0, 0.0
    for f, g, conv in zip(pf, tf, loss._convs):
        w = conv.weight.double().reshape(-1).cpu().numpy()
        total = total + ref.reference(ref.as64(f), ref.as64(g), w)['value']
        margin += ref.bound(f.shape[1], float(np.abs(w).max()))
    return total, margin + 5 * 2.0 ** -24 * float(np.abs(total).max())       # the four fp32 additions of the layers


def test_module():
    torch.manual_seed(3)
    loss = vqa.LPIPSLoss(reduction='none').cuda()
    gen = torch.Generator().manual_seed(4)
    image = (torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1).cuda()
    pred = (image + 0.3 * torch.randn(2, 3, 32, 32, generator=gen).cuda()).clamp(-1, 1)
    for autocast in (False, True):
        for train in (False, True):
            loss.train(train)
            x = pred.clone().requires_grad_()
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
                out = loss(x, image)
                if not train:
                    want, margin = module_reference(loss, pred, image)
            assert loss.last_route == ('fused', ''), loss.last_route
            assert out.shape == (2, 1, 1, 1) and out.dtype == torch.float32
            if not train:
                assert np.abs(out.detach().flatten().double().cpu().numpy() - want).max() <= margin
            out.sum().backward()
            assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().sum()) > 0
            assert all(p.grad is None for p in loss.parameters())
    loss.eval()
    with torch.no_grad():
        last_pred = pred.contiguous(memory_format=torch.channels_last)
        out = loss(last_pred, image)                                            # the image follows pred's memory format
        assert loss.last_route.name == 'fused'
        want, margin = module_reference(loss, last_pred, image.contiguous(memory_format=torch.channels_last))
        assert np.abs(out.flatten().double().cpu().numpy() - want).max() <= margin
    double = vqa.LPIPSLoss().double().cuda().eval()
    with torch.no_grad():
        out = double(pred.double(), image.double())
    assert double.last_route.name == 'torch' and 'float64' in double.last_route.why and out.dtype == torch.float64
