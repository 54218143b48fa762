"""GPU checks of the StyleGAN2 discriminator ops and module: the kernels against the float64 restatement of tests/stylegan2_ref.py
within the bounds derived in include/vqhip.h (through _lib, never fitted), the adjoint identity, reproducible gbias, and the fused
route of the module against its torch route.

Module tolerance: the disagreement of the torch route with ITSELF between NCHW and channels-last inputs on the same GPU, times a
margin of 4 for the different convolution algorithms the two routes' shapes select (the fused shortcut convolves at stride 1 a
quarter-size map).  Both numbers are printed; profiles/stylegan2.txt records a run."""
import itertools

import pytest
import torch

from vector_quantization_amd import _lib, ops, functional
from vector_quantization_amd.discriminators import StyleGAN2Discriminator
from vector_quantization_amd.gan_losses import R1GradientPenalty

import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
CODE = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def store(value, dtype):
    """Half an ulp of the output dtype on top of a bound for |value| (VQHIP_SG2_STORE_U)."""
    return _lib.sg2_store_u(CODE[dtype]) * value + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def layouts(t):
    yield 'nchw', t.contiguous()
    if t.dim() == 4:
        yield 'nhwc', t.contiguous(memory_format=torch.channels_last)


def within(got, want, bound, what):
    """|got - want| <= bound wherever want is finite; the same non-finite class elsewhere.  Returns the largest error / bound."""
    got, want = got.double(), want.double()
    finite = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f'{what}: NaNs differ'
    assert torch.equal(got[~finite & ~torch.isnan(want)], want[~finite & ~torch.isnan(want)]), f'{what}: infinities differ'
    err = (got - want).abs()[finite]
    b = bound.expand_as(want)[finite] if torch.is_tensor(bound) else torch.full_like(err, bound)
    ratio = torch.where(err > 0, err / b, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f'{what}: worst error / bound = {worst:.3f}')
    assert worst <= 1.0, f'{what}: error / bound = {worst}'
    return worst


# the issue's shapes, and one whose planes (4900 positions) and rows (9800) cross the backward's 4096-position chunk and 256-row slab
BIAS_ACT_SHAPES = [(1, 1), (3, 513), (1, 1, 1, 1), (2, 3, 5, 7), (3, 130, 4, 4), (1, 513, 9, 2), (2, 3, 70, 70)]


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape', BIAS_ACT_SHAPES, ids=str)
def test_bias_act_forward_and_backward(shape, dtype):
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen).to(dtype)
    bias = torch.randn(shape[1], generator=gen)
    flat = x.view(-1)
    n = flat.numel()
    if n >= 8:
        chan = torch.arange(shape[1]).view((1, -1) + (1,) * (len(shape) - 2)).expand(shape).flatten()
        bias[chan[0]] = 0.5                                                     # exact in every dtype: x + bias == 0 exactly
        flat[0] = -0.5
        flat[1], flat[2], flat[3] = float('inf'), float('-inf'), float('nan')
        bias[chan[4]] = bias[chan[4]].to(dtype).float()
        flat[4] = -bias[chan[4]].to(dtype)
    for name, xs in layouts(x):
        xd, bd = xs.cuda(), bias.cuda()
        y = ops.bias_act(xd, bd)
        assert y.dtype == dtype and y.stride() == xd.stride()
        want = ref.bias_act(xd, bd)
        bound = _lib.bias_act_bound(1.0) * want.abs().nan_to_num(0, 0, 0)
        within(y, want, bound + store(want.abs().nan_to_num(0, 0, 0) + bound, dtype), f'bias_act {shape} {dtype} {name} y')
        if n >= 8:
            assert float(y.flatten()[0]) == 0.0 and float(y.flatten()[4]) == 0.0    # (flatten walks the logical order in both layouts)
        # backward from the saved output as the kernel wrote it, finite gradients
        g = torch.randn(shape, generator=gen).to(dtype)
        g = (g.contiguous(memory_format=torch.channels_last) if name == 'nhwc' else g).cuda()
        gx, gbias = ops.bias_act_backward(g, y)
        gx2, gbias2 = ops.bias_act_backward(g, y)
        assert torch.equal(gbias, gbias2) and torch.equal(gx, gx2), 'gbias is not reproducible'
        want_gx, want_gb = ref.bias_act_grad(g, y)
        bound = _lib.bias_act_bound(1.0) * want_gx.abs()
        within(gx, want_gx, bound + store(want_gx.abs() + bound, dtype), f'bias_act {shape} {dtype} {name} gx')
        B, C = shape[:2]
        P = n // (B * C)
        layout = _lib.LAYOUT_ROWS if name == 'nhwc' else _lib.LAYOUT_MAP
        slabs = _lib.lib().vqhip_bias_act_slabs(layout, B, C, P)
        dims = [d for d in range(len(shape)) if d != 1]
        within(gbias, want_gb, _lib.sg2_gbias_bound(slabs, 4, 1.0) * want_gx.abs().sum(dims), f'bias_act {shape} {dtype} {name} gbias')
        assert ops.bias_act_backward(g, y, need_gbias=False)[1] is None


def test_bias_act_zero_and_nan_rows():
    """x + bias == 0 gives y == 0 and the slope branch; a NaN stays a NaN and takes the slope branch too."""
    x = torch.tensor([[-0.5, 0.5, float('nan'), 2.0]], device='cuda')
    bias = torch.tensor([0.5, -0.5, 0.0, 0.0], device='cuda')
    y = ops.bias_act(x, bias)
    assert y[0, 0] == 0 and y[0, 1] == 0 and torch.isnan(y[0, 2]) and y[0, 3] > 0
    gx, gbias = ops.bias_act_backward(torch.ones_like(x), y)
    s = ref.SCALE
    assert torch.allclose(gx.double().cpu(), torch.tensor([[s * 0.2, s * 0.2, s * 0.2, s]], dtype=torch.float64), rtol=1e-6)


FIR_SIZES = [(4, 4), (5, 7), (16, 16), (33, 65), (1, 9)]
FIR_PADS = [(1, 1, 1, 1), (2, 2, 2, 2), (0, 3, 2, 1)]


def fir_cases():
    for (H, W), pad, down in itertools.product(FIR_SIZES, FIR_PADS, (1, 2)):
        if H + pad[0] + pad[1] < 4 or W + pad[2] + pad[3] < 4:
            continue                                                            # 1 x 9 needs padding >= 2 along H: the issue's note
        yield H, W, pad, down


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('B,C', [(1, 1), (3, 1), (1, 3), (3, 3), (1, 130), (3, 130)], ids=str)
def test_fir4_forward_and_adjoint(B, C, dtype):
    gen = torch.Generator().manual_seed(B * 1000 + C)
    worst = 0.0
    for H, W, pad, down in fir_cases():
        x = torch.randn(B, C, H, W, generator=gen).to(dtype)
        for name, xs in layouts(x):
            xd = xs.cuda()
            out = ops.fir4(xd, pad, down)
            want = ref.blur(xd, pad, down)
            assert out.shape == want.shape and out.dtype == dtype
            bound = _lib.fir4_bound(1.0) * ref.blur(xd.abs(), pad, down)
            tol_out = bound + store(want.abs() + bound, dtype)
            tag = f'fir4 {B}x{C}x{H}x{W} pad={pad} d={down} {dtype} {name}'
            worst = max(worst, within(out, want, tol_out, tag))
            g = torch.randn(out.shape, generator=gen).to(dtype)
            g = (g.contiguous(memory_format=torch.channels_last) if name == 'nhwc' else g).cuda()
            gx = ops.fir4_backward(g, (H, W), pad, down)
            want_gx = ref.blur_adjoint(g, (H, W), pad, down)
            bound = _lib.fir4_bound(1.0) * ref.blur_adjoint(g.abs(), (H, W), pad, down)
            tol_gx = bound + store(want_gx.abs() + bound, dtype)
            within(gx, want_gx, tol_gx, tag + ' adjoint')
            # <fir4(x), g> == <x, fir4_backward(g)> in float64 on the kernels' outputs: each side is within its bound of the exact
            # bilinear form, so they differ by at most sum |g| tol_out + sum |x| tol_gx
            lhs = (out.double() * g.double()).sum()
            rhs = (xd.double() * gx.double()).sum()
            slack = (g.double().abs() * tol_out).sum() + (xd.double().abs() * tol_gx).sum()
            assert abs(float(lhs - rhs)) <= float(slack), (tag, float(lhs), float(rhs), float(slack))
    print(f'fir4 {B}x{C} {dtype}: worst forward error / bound {worst:.3f}')


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('B,C', [(1, 1), (3, 1), (1, 3), (3, 3), (1, 130), (3, 130)], ids=str)
def test_bias_act_blur_forward_and_backward(B, C, dtype):
    gen = torch.Generator().manual_seed(B * 1000 + C + 7)
    pad = (2, 2, 2, 2)
    for H, W in FIR_SIZES:
        x = torch.randn(B, C, H, W, generator=gen).to(dtype)
        bias = torch.randn(C, generator=gen).cuda()
        for name, xs in layouts(x):
            xd = xs.cuda()
            tag = f'bias_act_blur {B}x{C}x{H}x{W} {dtype} {name}'
            out = ops.fir4(xd, pad, 1, bias=bias)
            act = ref.bias_act(xd, bias)
            want = ref.blur(act, pad)
            bound = _lib.fir4_bound(1.0, fused=True) * ref.blur(act.abs(), pad)
            within(out, want, bound + store(want.abs() + bound, dtype), tag)
            g = torch.randn(out.shape, generator=gen).to(dtype)
            g = (g.contiguous(memory_format=torch.channels_last) if name == 'nhwc' else g).cuda()
            gx, gbias = ops.fir4_backward(g, (H, W), pad, 1, x=xd, bias=bias)
            gx2, gbias2 = ops.fir4_backward(g, (H, W), pad, 1, x=xd, bias=bias)
            assert torch.equal(gbias, gbias2) and torch.equal(gx, gx2)
            f = ref.act_factor(xd, bias)
            want_gx = ref.blur_adjoint(g, (H, W), pad) * f
            a = ref.blur_adjoint(g.abs(), (H, W), pad) * f
            bound = _lib.fir4_bound(1.0, fused=True) * a
            within(gx, want_gx, bound + store(want_gx.abs() + bound, dtype), tag + ' gx')
            layout = _lib.LAYOUT_ROWS if xd.is_contiguous(memory_format=torch.channels_last) and not xd.is_contiguous() else _lib.LAYOUT_MAP
            slabs = _lib.lib().vqhip_fir4_slabs(layout, B, C, H, W)
            within(gbias, want_gx.sum((0, 2, 3)), _lib.sg2_gbias_bound(slabs, 12, 1.0) * a.sum((0, 2, 3)), tag + ' gbias')


def _pair(image_size=16):
    torch.manual_seed(5)
    fused = StyleGAN2Discriminator(image_size=image_size).cuda()
    fused.init_weights({})
    with torch.no_grad():
        for name, p in fused.named_parameters():
            if name.endswith('bias'):
                p.normal_(0, 0.1)
    plain = StyleGAN2Discriminator(image_size=image_size, fused=False).cuda()
    plain.load_state_dict(fused.state_dict(), strict=True)
    return fused, plain


def _run(module, image, penalty=False):
    module.zero_grad()
    if penalty:
        out = R1GradientPenalty()(module, image)
        out.backward()
    else:
        out = module(image)
        out.square().sum().backward()
    grads = {n: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for n, p in module.named_parameters()}
    return out.detach().clone(), grads


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('penalty,B', [(False, 4), (True, 2)], ids=['logits', 'r1_penalty'])
def test_module_fused_route_matches_torch_route(penalty, B):
    fused, plain = _pair()
    image = torch.randn(B, 3, 16, 16, device='cuda')
    base_out, base = _run(plain, image, penalty)
    assert plain.last_route.name == 'torch' and plain.last_route.why == 'fused=False'
    cl_out, cl = _run(plain, image.contiguous(memory_format=torch.channels_last), penalty)
    self_dis = max([_rel(cl_out, base_out)] + [_rel(cl[n], base[n]) for n in base])
    tol = 4 * max(self_dis, 2.0 ** -23)                                          # (never below one fp32 ulp of the largest element)
    for layout, x in (('NCHW', image), ('channels-last', image.contiguous(memory_format=torch.channels_last))):
        out, grads = _run(fused, x, penalty)
        assert fused.last_route.name == 'fused', fused.last_route
        dis = max([_rel(out, base_out)] + [_rel(grads[n], base[n]) for n in base])
        print(f'module penalty={penalty}: torch route NCHW vs channels-last {self_dis:.3e}, fused {layout} vs torch {dis:.3e}, tolerance {tol:.3e}')
        assert torch.isfinite(out).all() and dis <= tol, (layout, dis, tol)
    if penalty:
        assert any(float(g.abs().max()) > 0 for n, g in grads.items() if n.endswith('_original_weight'))


def test_module_under_bf16_autocast_and_state_dict_round_trip():
    fused, plain = _pair()
    image = torch.randn(4, 3, 16, 16, device='cuda')
    with torch.autocast('cuda', torch.bfloat16):
        out = fused(image.contiguous(memory_format=torch.channels_last))
        out.float().square().sum().backward()
    assert fused.last_route.name == 'fused' and torch.isfinite(out).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in fused.parameters())
    back = StyleGAN2Discriminator(image_size=16).cuda()
    back.load_state_dict(plain.state_dict(), strict=True)
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in fused.state_dict().items())


def test_double_backward_of_the_ops_matches_the_definition():
    """d/dg of bias_act's backward is gg * scale * mask; of the blur's adjoint the blur; both through autograd."""
    x = torch.randn(2, 5, 6, 7, device='cuda', requires_grad=True)
    bias = torch.randn(5, device='cuda', requires_grad=True)
    y = functional.bias_act_blur(x, bias, 2)
    g = torch.randn_like(y).requires_grad_()
    gx, = torch.autograd.grad(y, x, g, create_graph=True)
    gg = torch.randn_like(gx)
    got, = torch.autograd.grad(gx, g, gg)
    masked = gg.double() * ref.act_factor(x.detach(), bias.detach())
    want = ref.blur(masked, (2, 2, 2, 2))
    # gg * factor (3 u) into the blur (8 u): inside VQHIP_FIR4_ACT_BOUND of blur(|gg factor|); fp32, so no store term
    within(got, want, _lib.fir4_bound(1.0, fused=True) * ref.blur(masked.abs(), (2, 2, 2, 2)), 'double backward of bias_act_blur')


@pytest.mark.parametrize('fmt', [torch.contiguous_format, torch.channels_last], ids=['nchw', 'nhwc'])
def test_an_expanded_gradient_is_made_dense(fmt):
    """``.sum().backward()`` hands the backward a gradient of zero strides: blur, bias_act_blur and bias_act take it (fp32)."""
    x = torch.randn(2, 5, 6, 7, device='cuda').contiguous(memory_format=fmt).requires_grad_()
    bias = torch.randn(5, device='cuda', requires_grad=True)
    ones = lambda t: torch.ones_like(t, dtype=torch.float64)
    functional.blur(x, 1, 2).sum().backward()
    want = ref.blur_adjoint(ones(ref.blur(x.detach(), (1, 1, 1, 1), 2)), (6, 7), (1, 1, 1, 1), 2)
    within(x.grad, want, _lib.fir4_bound(1.0) * want.abs(), 'blur, expanded gradient')
    x.grad = None
    functional.bias_act_blur(x, bias, 2).sum().backward()
    f = ref.act_factor(x.detach(), bias.detach())
    want = ref.blur_adjoint(ones(ref.blur(x.detach(), (2, 2, 2, 2))), (6, 7), (2, 2, 2, 2)) * f
    within(x.grad, want, _lib.fir4_bound(1.0, fused=True) * want.abs(), 'bias_act_blur, expanded gradient')
    slabs = _lib.lib().vqhip_fir4_slabs(_lib.LAYOUT_ROWS if fmt == torch.channels_last else _lib.LAYOUT_MAP, 2, 5, 6, 7)
    within(bias.grad, want.sum((0, 2, 3)), _lib.sg2_gbias_bound(slabs, 12, 1.0) * want.abs().sum((0, 2, 3)), 'bias_act_blur, expanded gradient, gbias')
    x.grad = bias.grad = None
    functional.bias_act(x, bias).sum().backward()
    want = f                                                                    # (the sign of y is the sign of x + bias here: no underflow in fp32)
    within(x.grad, want, _lib.bias_act_bound(1.0) * want.abs(), 'bias_act, expanded gradient')
    # the double backward with an expanded second-order gradient
    y = functional.blur(x, 2)
    g = torch.randn_like(y).requires_grad_()
    gx, = torch.autograd.grad(y, x, g, create_graph=True)
    gx.sum().backward()
    want = ref.blur(ones(gx), (2, 2, 2, 2))
    within(g.grad, want, _lib.fir4_bound(1.0) * want.abs(), 'blur, expanded second-order gradient')
