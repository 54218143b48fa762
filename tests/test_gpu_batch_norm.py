"""GPU checks of the batch-statistics mode of vqhip_group_norm_* (BatchNorm2d in training mode + LeakyReLU(0.2)) and of
PatchGANDiscriminator on it: the kernels against the float64 restatement of tests/batch_norm_ref.py within the bounds derived in
include/vqhip.h (through _lib, never fitted) plus half an ulp of the output dtype; the hostile inputs of the contract; equal bits
run to run; the running statistics; the module against a float64 copy of itself; the routes.

Launch shapes crossed (include/vqhip.h, BATCH STATISTICS, LAUNCH SHAPE), as (B, C, P):
  NCHW           one launch up to n = B P = 8192: (2, 3, 1), (3, 5, 49), (2, 16, 50), (2, 16, 150), (2, 136, 70), (3, 4, 2051) with
                 n = 6153; three launches beyond: (5, 3, 2051) with n = 10255, a ragged second chunk, and (2, 130, 961) never (n = 1922),
                 with runs of 961 that start at odd elements and pieces that cross from one image to the next.
  channels-last  one launch up to 1024 / PW positions, PW = 8, 4 or 1 elements (16 bytes, 8 bytes, one element, whichever divides
                 C): (2, 16, 50) is one launch for every dtype (n = 100 <= 128), (2, 16, 150) is split for every dtype (n = 300 > 256),
                 (2, 136, 70) has three tiles of channels in bf16 / fp16 (PW = 8, the last tile 8 channels wide) and is split there
                 (n = 140 > 128) but not in fp32 (PW = 4, five tiles, 140 <= 256); C = 3, 5, 130 take PW = 1: (3, 5, 49) in one launch,
                 (2, 130, 961), (3, 4, 2051) (PW = 4) and (5, 3, 2051) split, the last in 11 slabs of 1024 with a ragged one.
The seeds are fixed so that no value of the restatement has |u| <= E_u (test_batch_norm_cpu.py checks that without a GPU, this
file asserts it again): the LeakyReLU branch of every element is determined and E_d = 0.

``functional.group_norm(x, 32, .., act='leaky_relu')`` has no test here: act 2 with G >= 1 stays VQHIP_EINVAL (an earlier test holds
the library to it), and the Python layer raises for it."""
import copy

import pytest
import torch

from vector_quantization_amd import _lib, functional, gan_losses, ops
from vector_quantization_amd.discriminators import PatchGANDiscriminator

import batch_norm_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
CODE = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
SHAPES = [(2, 3, 1), (3, 5, 49), (2, 130, 961), (3, 4, 2051), (5, 3, 2051), (2, 16, 50), (2, 16, 150), (2, 136, 70)]
EPS = 1e-5
# seed per (shape, dtype) for which every branch is determined (found by trying 0, 1, 2, .. on the CPU); 0 where not listed
SEEDS = {((2, 130, 961), torch.float16): 3}


def inputs(shape, dtype, device='cpu'):
    """(x, g, gamma, beta): the activation and the incoming gradient [B, C, P, 1] in ``dtype``, the parameters in fp32."""
    B, C, P = shape
    gen = torch.Generator().manual_seed(SEEDS.get((shape, dtype), 0) * 1000 + B + C + P)
    x = torch.randn(B, C, P, 1, generator=gen).to(dtype)
    gamma = (1.0 + 0.3 * torch.randn(C, generator=gen))
    beta = 0.5 * torch.randn(C, generator=gen)
    g = torch.randn(B, C, P, 1, generator=gen).to(dtype)
    return x.to(device), g.to(device), gamma.to(device), beta.to(device)


def store(value, dtype):
    """Half an ulp of the output dtype on top of a bound for |value| (VQHIP_SG2_STORE_U)."""
    return _lib.sg2_store_u(CODE[dtype]) * value + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def layouts(t):
    yield 'nchw', t.contiguous()
    if t.shape[1] > 1 and t.shape[2] * t.shape[3] > 1:
        yield 'nhwc', t.contiguous(memory_format=torch.channels_last)
    else:                                                                       # (strides alone do not tell the two apart: both are both)
        yield 'nhwc', t.contiguous()


def within(got, want, bound, what):
    got, want = got.double(), want.double()
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), f'{what}: not finite'
    err = (got - want).abs()
    b = bound.expand_as(want) if torch.is_tensor(bound) else torch.full_like(err, bound)
    ratio = torch.where(err > 0, err / b, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f'{what}: worst error / bound = {worst:.3f}')
    assert worst <= 1.0, f'{what}: error / bound = {worst}'
    return worst


def check_case(xd, gd, gamma, beta, act, dtype, tag, need_margin=True):
    """Forward and backward of one tensor as it lies in memory against the restatement; returns the kernel's outputs."""
    C = xd.shape[1]
    y, stats, mean, var = ops.batch_norm(xd, gamma, beta, EPS, act)
    assert y.dtype == dtype and y.stride() == xd.stride() and stats.shape == (C, 2) and mean.shape == var.shape == (C,)
    want, _, p = ref.forward(xd, gamma, beta, EPS, act)
    if act == 'leaky_relu' and need_margin:
        margin = ref.branch_margin(gamma, p)
        print(f'{tag}: min |u| / E_u = {margin:.3f}')
        assert margin > 1.0, f'{tag}: a branch is undetermined; choose another seed'
    bound = ref.forward_bound(xd, gamma, p, act)
    within(y, want, bound + store(want.abs() + bound, dtype), tag + ' y')
    within(stats[:, :1], p['mean'], ref.mean_bound(p), tag + ' mean')
    within(stats[:, 1:], p['rstd'], ref.rstd_bound(p), tag + ' rstd')
    within(mean.view(C, 1), p['mean'], ref.mean_bound(p), tag + ' block mean')
    within(var.view(C, 1), p['unbiased'], ref.unbiased_bound(p, EPS), tag + ' block unbiased var')
    assert torch.equal(mean, stats[:, 0])
    gx, dg, db = ops.batch_norm_backward(gd, xd, stats, gamma, beta, act)
    assert gx.dtype == dtype and gx.stride() == xd.stride() and dg.dtype == db.dtype == torch.float32
    wgx, wdg, wdb, p = ref.backward(gd, xd, gamma, beta, EPS, act)
    e_gx, e_dg, e_db = ref.backward_bounds(gd, xd, gamma, p)
    within(gx, wgx, e_gx + store(wgx.abs() + e_gx, dtype), tag + ' gx')
    within(dg, wdg, e_dg + 1e-45, tag + ' dgamma')
    within(db, wdb, e_db + 1e-45, tag + ' dbeta')
    # the same bits on a second call
    y2, stats2, mean2, var2 = ops.batch_norm(xd, gamma, beta, EPS, act)
    gx2, dg2, db2 = ops.batch_norm_backward(gd, xd, stats, gamma, beta, act)
    for a, b in ((y, y2), (stats, stats2), (mean, mean2), (var, var2), (gx, gx2), (dg, dg2), (db, db2)):
        assert torch.equal(a, b), f'{tag}: two calls differ'
    return y, stats, gx, dg, db


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_backward_within_the_derived_bound(shape, dtype):
    x, g, gamma, beta = inputs(shape, dtype)
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        for act in (None, 'leaky_relu'):
            check_case(xs.cuda(), gs.cuda(), gamma.cuda(), beta.cuda(), act, dtype, f'batch_norm {shape} {dtype} {name} act={act}')


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_zero_gamma_and_beta_take_the_slope_branch(dtype):
    """u == 0 in the whole channel: y == 0, and d is the slope, so dbeta = 0.2 sum g within its bound."""
    shape = (3, 6, 700)
    x, g, gamma, beta = inputs(shape, dtype)
    gamma[2] = 0.0
    beta[2] = 0.0
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        y, _, gx, dg, db = check_case(xs.cuda(), gs.cuda(), gamma.cuda(), beta.cuda(), 'leaky_relu', dtype, f'zero channel {dtype} {name}')
        assert float(y[:, 2].abs().max()) == 0.0 and float(gx[:, 2].abs().max()) == 0.0
        gsum, gabs = g[:, 2].double().sum(), g[:, 2].double().abs().sum()
        n = shape[0] * shape[2]
        assert abs(float(db[2]) - ref.SLOPE * float(gsum)) <= (_lib.gn_chain(n) + 1.0) * _lib.GN_U * ref.SLOPE * float(gabs)


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_a_constant_channel(dtype):
    shape = (2, 6, 5000)
    x, g, gamma, beta = inputs(shape, dtype)
    x[:, 1] = 0.3
    x[:, 4] = -7.0
    beta[1], beta[4] = 0.4, -0.6                                                 # far from zero: E_u is gamma q here, up to 1e-2
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        y, stats, gx, _, _ = check_case(xs.cuda(), gs.cuda(), gamma.cuda(), beta.cuda(), 'leaky_relu', dtype, f'constant channel {dtype} {name}')
        assert torch.isfinite(gx).all()
        u = beta.double()
        want = torch.where(u > 0, u, ref.SLOPE * u)
        for c, value in ((1, 0.3), (4, 7.0)):
            q = _lib.gn_q(10000, value, EPS ** -0.5)
            tol = _lib.gn_u_bound(10000, q, 0.0, abs(float(gamma[c])), abs(float(beta[c]))) + 2.0 * _lib.GN_U * abs(float(want[c]))
            assert float((y[:, c].double().cpu() - want[c]).abs().max()) <= tol + float(store(abs(float(want[c])) + tol, dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_a_mean_of_a_thousand_deviations(dtype):
    """x = 1000 + randn, rounded to the dtype first: the q term of the bound carries the fp32 error of the mean."""
    shape = (4, 6, 3000)
    gen = torch.Generator().manual_seed(7)
    x = (1000.0 + torch.randn(shape[0], shape[1], shape[2], 1, generator=gen)).to(dtype)
    gamma, beta = 1.0 + 0.1 * torch.randn(6, generator=gen), 0.1 * torch.randn(6, generator=gen)
    g = torch.randn(x.shape, generator=gen).to(dtype)
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        check_case(xs.cuda(), gs.cuda(), gamma.cuda(), beta.cuda(), None, dtype, f'1000 + randn {dtype} {name}')
        if dtype == torch.float32:
            want, _, p = ref.forward(xs, gamma, beta, EPS, None)
            assert float(ref.forward_bound(xs, gamma, p, None).max()) < 0.05


@pytest.mark.parametrize('shape', [(3, 6, 49), (2, 6, 9000)], ids=str)
def test_nan_stays_in_its_channel(shape):
    x, _, gamma, beta = inputs(shape, torch.float32)
    bad = x.clone()
    bad[1, 3, shape[2] // 2, 0] = float('nan')
    for (name, xs), (_, bs) in zip(layouts(x), layouts(bad)):
        y0, s0, m0, v0 = ops.batch_norm(xs.cuda(), gamma.cuda(), beta.cuda(), EPS, 'leaky_relu')
        y1, s1, m1, v1 = ops.batch_norm(bs.cuda(), gamma.cuda(), beta.cuda(), EPS, 'leaky_relu')
        keep = torch.arange(shape[1], device='cuda') != 3
        assert torch.isnan(y1[:, 3]).all(), f'{name}: the channel of the NaN is not NaN everywhere'
        assert torch.equal(y1[:, keep], y0[:, keep]), f'{name}: another channel changed'
        assert torch.equal(s1[keep], s0[keep]) and torch.equal(m1[keep], m0[keep]) and torch.equal(v1[keep], v0[keep])


@pytest.mark.parametrize('shape', [(3, 5, 49), (5, 3, 2051)], ids=str)
def test_running_statistics_and_the_counter(shape):
    x, _, gamma, beta = inputs(shape, torch.float32, 'cuda')
    C, m = shape[1], 0.1
    gen = torch.Generator().manual_seed(9)
    rm0, rv0 = torch.randn(C, generator=gen).cuda(), (0.5 + torch.rand(C, generator=gen)).cuda()
    rm, rv, count = rm0.clone(), rv0.clone(), torch.tensor(4, device='cuda')
    y = functional.batch_norm(x, rm, rv, gamma, beta, True, m, EPS, 'leaky_relu', count)
    _, _, p = ref.forward(x, gamma, beta, EPS, 'leaky_relu')
    want_m = (1 - m) * rm0.double() + m * p['mean'].reshape(-1)
    want_v = (1 - m) * rv0.double() + m * p['unbiased'].reshape(-1)
    within(rm, want_m, m * ref.mean_bound(p).reshape(-1) + _lib.GN_U * want_m.abs(), f'running_mean {shape}')
    within(rv, want_v, m * ref.unbiased_bound(p, EPS).reshape(-1) + _lib.GN_U * want_v.abs(), f'running_var {shape}')
    assert int(count) == 5 and y.shape == x.shape


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def _grads(d, image):
    d.zero_grad()
    out = d(image)
    out.square().mean().backward()
    return out.detach(), {n: p.grad.detach().clone() for n, p in d.named_parameters()}


def test_module_fused_route_against_float64():
    """Both routes are fp32 pipelines that differ in summation order only, so the fused route's largest error against a float64
    copy of the module is at most twice the torch route's; a wrong formula shows as orders of magnitude."""
    torch.manual_seed(3)
    fused = PatchGANDiscriminator(width=8).cuda()
    fused.init_weights(None)
    plain = PatchGANDiscriminator(width=8, fused=False).cuda()
    plain.load_state_dict(fused.state_dict(), strict=True)
    exact = copy.deepcopy(plain).double()
    image = torch.randn(3, 3, 32, 32, device='cuda')
    want_out, want = _grads(exact, image.double())
    out_f, got_f = _grads(fused, image)
    out_p, got_p = _grads(plain, image)
    assert fused.last_route.name == 'fused' and plain.last_route == ('torch', 'fused=False'), (fused.last_route, plain.last_route)
    err_f = max([_rel(out_f, want_out)] + [_rel(got_f[n], want[n]) for n in want])
    err_p = max([_rel(out_p, want_out)] + [_rel(got_p[n], want[n]) for n in want])
    print(f'PatchGANDiscriminator(width=8) fp32 [3, 3, 32, 32]: largest relative error against float64: fused {err_f:.3e}, torch {err_p:.3e}')
    assert err_f <= 2.0 * err_p, (err_f, err_p)
    for k, v in fused.state_dict().items():                                     # the buffers moved as the plain module's did
        w = exact.state_dict()[k]
        assert _rel(v, w) <= 1e-5 if v.is_floating_point() else torch.equal(v, w), k


def test_eval_mode_and_r1_penalty_take_the_torch_route():
    torch.manual_seed(5)
    d = PatchGANDiscriminator(width=8).cuda()
    image = torch.randn(3, 3, 32, 32, device='cuda')
    d.eval()
    out = d(image)
    assert d.last_route.name == 'torch' and 'eval mode' in d.last_route.why
    assert torch.equal(out, d._discriminator(image))
    d.train()
    penalty = gan_losses.R1GradientPenalty()(d, image)
    assert d.last_route.name == 'torch' and 'eval mode' in d.last_route.why and d.training
    assert torch.isfinite(penalty).all()
    penalty.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in d.parameters() if p.grad is not None)
    assert int(d._discriminator[3].num_batches_tracked) == 0


def test_a_second_derivative_through_the_fused_backward_raises():
    torch.manual_seed(6)
    d = PatchGANDiscriminator(width=8).cuda()
    image = torch.randn(3, 3, 32, 32, device='cuda', requires_grad=True)
    out = d(image)
    assert d.last_route.name == 'fused'
    with pytest.raises(RuntimeError, match='once_differentiable'):
        gi, = torch.autograd.grad(out.sum(), image, create_graph=True)
        gi.square().sum().backward()
