"""GPU checks of the fused GroupNorm (+ SiLU) and of VQGANEncoder / VQGANDecoder on it: the kernels against the float64 restatement
of tests/group_norm_ref.py within the bounds derived in include/vqhip.h (through _lib, never fitted) plus half an ulp of the output
dtype, the hostile inputs of the contract (a large mean, a constant group, NaN and infinity), equal bits run to run, the adjoint
identity, and the fused route of the modules against their torch route.

Launch shapes crossed (include/vqhip.h, LAUNCH SHAPE): n <= 2048 takes one wave per group ((2, 512, 4, 4): n = 256, and the smaller
ones), 2048 < n <= 8192 one workgroup per group ((1, 64, 40, 40): n = 3200, added for this), beyond 8192 a group is split into
chunks of 8192 with partials in the workspace ((1, 128, 70, 70): n = 19600 is 3 chunks whose edges 8192 and 16384 fall inside
channels, planes of 4900).  Pieces are 16 bytes: (3, 96, 3, 3) starts its groups at odd element offsets in NCHW and has 3 channels
per group in channels-last (single-element pieces); (2, 512, 4, 4) has 16 (16-byte pieces), (1, 128, 70, 70) has 4 (8-byte pieces in
bf16 / fp16).

Module tolerance: the disagreement of the torch route with ITSELF between NCHW and channels-last inputs on the same GPU, times a
margin of 4 for the convolution algorithms the two routes select.  Both numbers are printed; profiles/vqgan_autoencoder.txt
records a run."""
import pytest
import torch

from vector_quantization_amd import _lib, functional, ops
from vector_quantization_amd.autoencoders import VQGANDecoder, VQGANEncoder

import group_norm_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
CODE = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
SHAPES = [((1, 32, 1, 1), 32), ((2, 32, 5, 7), 32), ((3, 96, 3, 3), 32), ((2, 64, 1, 1), 32), ((1, 128, 70, 70), 32), ((2, 512, 4, 4), 32),
          ((1, 64, 40, 40), 32), ((2, 12, 5, 5), 4)]
EPS = 1e-6


def store(value, dtype):
    """Half an ulp of the output dtype on top of a bound for |value| (VQHIP_SG2_STORE_U)."""
    return _lib.sg2_store_u(CODE[dtype]) * value + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def layouts(t):
    yield 'nchw', t.contiguous()
    yield 'nhwc', t.contiguous(memory_format=torch.channels_last)


def within(got, want, bound, what):
    """|got - want| <= bound everywhere (all finite).  Returns the largest error / bound."""
    got, want = got.double(), want.double()
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), f'{what}: not finite'
    err = (got - want).abs()
    b = bound.expand_as(want) if torch.is_tensor(bound) else torch.full_like(err, bound)
    ratio = torch.where(err > 0, err / b, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f'{what}: worst error / bound = {worst:.3f}')
    assert worst <= 1.0, f'{what}: error / bound = {worst}'
    return worst


def check_case(xd, g, G, gamma, beta, act, dtype, tag):
    """Forward and backward of one tensor as it lies in memory against the restatement; returns the kernel's outputs."""
    y, stats = ops.group_norm(xd, G, gamma, beta, EPS, act)
    assert y.dtype == dtype and y.stride() == xd.stride() and stats.shape == (xd.shape[0], G, 2)
    want, wstats, p = ref.forward(xd, G, gamma, beta, EPS, act)
    n = p['n']
    bound = ref.forward_bound(xd, G, gamma, beta, EPS, act, want, p)
    within(y, want, bound + store(want.abs() + bound, dtype), tag + ' y')
    q = _lib.gn_q(n, p['mabs'], p['rstd'])
    within(stats[..., :1], p['mean'], _lib.gn_chain(n) * _lib.GN_U * p['mabs'] + 1e-45, tag + ' mean')
    within(stats[..., 1:], p['rstd'], _lib.gn_rho(n, q) * p['rstd'], tag + ' rstd')
    gx, dg, db = ops.group_norm_backward(g, xd, stats, G, gamma, beta, act)
    assert gx.dtype == dtype and gx.stride() == xd.stride() and dg.dtype == db.dtype == torch.float32
    wgx, wdg, wdb, p = ref.backward(g, xd, G, gamma, beta, EPS, act)
    B, C = xd.shape[:2]
    e_gx, e_dg, e_db = ref.backward_bounds(g, xd, G, gamma, beta, EPS, act, wgx, p, ref.slabs(B, C, xd.numel() // (B * C), G))
    within(gx, wgx, e_gx + store(wgx.abs() + e_gx, dtype), tag + ' gx')
    within(dg, wdg, e_dg, tag + ' dgamma')
    within(db, wdb, e_db, tag + ' dbeta')
    # the same bits on a second call
    y2, stats2 = ops.group_norm(xd, G, gamma, beta, EPS, act)
    gx2, dg2, db2 = ops.group_norm_backward(g, xd, stats, G, gamma, beta, act)
    for a, b in ((y, y2), (stats, stats2), (gx, gx2), (dg, dg2), (db, db2)):
        assert torch.equal(a, b), f'{tag}: two calls differ'
    return y, stats, gx, dg, db


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape,G', SHAPES, ids=str)
def test_forward_and_backward_within_the_derived_bound(shape, G, dtype):
    gen = torch.Generator().manual_seed(sum(shape) + G)
    x = torch.randn(shape, generator=gen).to(dtype)
    gamma = torch.randn(shape[1], generator=gen).cuda()
    beta = torch.randn(shape[1], generator=gen).cuda()
    g = torch.randn(shape, generator=gen).to(dtype)
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        for act in (None, 'silu'):
            check_case(xs.cuda(), gs.cuda(), G, gamma, beta, act, dtype, f'group_norm {shape} G={G} {dtype} {name} act={act}')


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape', [(2, 64, 24, 24), (1, 32, 100, 100)], ids=str)
def test_a_mean_of_a_thousand_deviations(shape, dtype):
    """x = 1000 + randn, rounded to the dtype first: var from E[x^2] - mean^2 loses every digit here (1e6 against 1 in fp32); the
    second pass does not, and the bound - whose q term is the fp32 error of the mean itself - holds."""
    gen = torch.Generator().manual_seed(7)
    x = (1000.0 + torch.randn(shape, generator=gen)).to(dtype)
    gamma = (1.0 + 0.1 * torch.randn(shape[1], generator=gen)).cuda()
    beta = (0.1 * torch.randn(shape[1], generator=gen)).cuda()
    g = torch.randn(shape, generator=gen).to(dtype)
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        xd = xs.cuda()
        check_case(xd, gs.cuda(), 32, gamma, beta, 'silu', dtype, f'1000 + randn {shape} {dtype} {name}')
        # what the bound allows is far below what the forbidden formula loses, a relative error of var of 2^-24 * 1e6 / var and so
        # of order 1 in y.  (bf16 keeps multiples of 4 and 8 here: its groups are nearly constant, rstd and with it q are large, and
        # the comparison says nothing.)
        if dtype != torch.bfloat16:
            want, _, p = ref.forward(xd, 32, gamma, beta, EPS, 'silu')
            assert float(ref.forward_bound(xd, 32, gamma, beta, EPS, 'silu', want, p).max()) < 0.05


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_a_constant_group(dtype):
    shape, G = (2, 64, 6, 6), 32
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=gen)
    x[0, 4:6] = 0.3                                                             # group 2 of image 0
    x[1, 62:64] = -7.0                                                          # group 31 of image 1
    x = x.to(dtype)
    gamma, beta = torch.randn(64, generator=gen).cuda(), torch.randn(64, generator=gen).cuda()
    g = torch.randn(shape, generator=gen).to(dtype)
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        y, stats, gx, _, _ = check_case(xs.cuda(), gs.cuda(), G, gamma, beta, 'silu', dtype, f'constant group {dtype} {name}')
        assert torch.isfinite(gx).all()
        # y = act(beta) by name: xh = 0, so the bound is what the mean's error q leaves, with rstd = eps^-1/2
        want = torch.nn.functional.silu(beta.double())
        for b, c, value in ((0, 4, 0.3), (0, 5, 0.3), (1, 62, 7.0), (1, 63, 7.0)):
            q = _lib.gn_q(72, value, EPS ** -0.5)
            tol = _lib.gn_y_bound(72, q, 0.0, abs(float(gamma[c])), abs(float(beta[c])), abs(float(want[c])), 1)
            assert float((y[b, c].double() - want[c]).abs().max()) <= tol + float(store(abs(float(want[c])) + tol, dtype))


@pytest.mark.parametrize('shape', [(2, 64, 9, 9), (1, 128, 70, 70)], ids=str)
def test_nan_and_infinity_stay_in_their_group(shape):
    G = 32
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=gen)
    gamma, beta = torch.randn(shape[1], generator=gen).cuda(), torch.randn(shape[1], generator=gen).cuda()
    cpg = shape[1] // G
    bad = x.clone()
    bad[0, 3 * cpg, 1, 2] = float('nan')
    bad[0, 3 * cpg + cpg - 1, shape[2] - 1, shape[3] - 1] = float('inf')
    for (name, xs), (_, bs) in zip(layouts(x), layouts(bad)):
        for act in (None, 'silu'):
            y0, s0 = ops.group_norm(xs.cuda(), G, gamma, beta, EPS, act)
            y1, s1 = ops.group_norm(bs.cuda(), G, gamma, beta, EPS, act)
            hit = torch.zeros(shape, dtype=torch.bool, device='cuda')
            hit[0, 3 * cpg:4 * cpg] = True
            assert torch.isnan(y1[hit]).all(), f'{name}: the group of the NaN is not NaN everywhere'
            assert torch.equal(y1[~hit], y0[~hit]), f'{name}: another group changed'
            keep = torch.ones(shape[0], G, dtype=torch.bool, device='cuda')
            keep[0, 3] = False
            assert torch.equal(s1[keep], s0[keep]), f'{name}: the stats of another group changed'


@pytest.mark.parametrize('act', [None, 'silu'])
def test_adjoint_identity(act):
    """<g, J v> == <J^T g, v>: J v by forward-mode differentiation of the restatement in float64, J^T g the kernel's gx in fp32;
    the two sides differ by at most sum |v| E_gx."""
    shape, G = (2, 64, 11, 13), 32
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen).cuda()
    gamma, beta = torch.randn(64, generator=gen).cuda(), torch.randn(64, generator=gen).cuda()
    g, v = torch.randn(shape, generator=gen).cuda(), torch.randn(shape, generator=gen).cuda()
    f = lambda t: ref.forward(t, G, gamma, beta, EPS, act)[0]
    _, jv = torch.autograd.functional.jvp(f, x.double(), v.double())
    for (name, xs), (_, gs) in zip(layouts(x), layouts(g)):
        _, stats = ops.group_norm(xs, G, gamma, beta, EPS, act)
        gx, _, _ = ops.group_norm_backward(gs, xs, stats, G, gamma, beta, act)
        wgx, _, _, p = ref.backward(g, x, G, gamma, beta, EPS, act)
        e_gx, _, _ = ref.backward_bounds(g, x, G, gamma, beta, EPS, act, wgx, p, ref.slabs(2, 64, 143, G))
        lhs, rhs = (g.double() * jv).sum(), (gx.double() * v.double()).sum()
        slack = (v.double().abs() * e_gx).sum() + 1e-12 * (g.double() * jv).abs().sum()
        print(f'adjoint {name} act={act}: lhs {float(lhs):.9e} rhs {float(rhs):.9e} slack {float(slack):.3e}')
        assert abs(float(lhs - rhs)) <= float(slack)


def test_functional_gradients_and_the_torch_route():
    """functional.group_norm: gradients to x, weight and bias through autograd on a GPU tensor; float64 takes the torch route."""
    x = torch.randn(2, 64, 8, 8, device='cuda', requires_grad=True)
    w = torch.randn(64, device='cuda', requires_grad=True)
    b = torch.randn(64, device='cuda', requires_grad=True)
    g = torch.randn(2, 64, 8, 8, device='cuda')
    gx, gw, gb = torch.autograd.grad(functional.group_norm(x, 32, w, b, EPS, 'silu'), (x, w, b), g)
    wx, ww, wb, _ = ref.backward(g, x.detach(), 32, w.detach(), b.detach(), EPS, 'silu')
    for got, want in ((gx, wx), (gw, ww), (gb, wb)):
        assert float((got.double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    xd = x.detach().double()
    assert torch.equal(functional.group_norm(xd, 32, w.double(), b.double(), EPS, 'silu'),
                       functional.group_norm_torch(xd, 32, w.double(), b.double(), EPS, 'silu'))


SMALL_ENCODER, SMALL_DECODER = dict(width=32, width_mults=(1, 2)), dict(width=32, width_mults=(2, 1))


def _pair():
    torch.manual_seed(5)
    fused = torch.nn.ModuleList([VQGANEncoder(**SMALL_ENCODER), VQGANDecoder(**SMALL_DECODER)]).cuda()
    with torch.no_grad():
        for m in fused.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
    plain = torch.nn.ModuleList([VQGANEncoder(**SMALL_ENCODER, fused=False), VQGANDecoder(**SMALL_DECODER, fused=False)]).cuda()
    plain.load_state_dict(fused.state_dict(), strict=True)
    return fused, plain


def _run(pair, image, autocast):
    pair.zero_grad()
    image = image.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
        z, _ = pair[0](image, {})
        out, _ = pair[1](z, {})
    out.float().square().mean().backward()
    grads = {n: p.grad.detach().clone() for n, p in pair.named_parameters()}
    grads['image'] = image.grad.detach().clone()
    return out.detach().float().clone(), z.detach().float().clone(), grads


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16_autocast'])
def test_modules_fused_route_matches_torch_route(autocast):
    fused, plain = _pair()
    image = torch.randn(2, 3, 32, 32, device='cuda')
    base_out, base_z, base = _run(plain, image, autocast)
    assert plain[0].last_route.name == 'torch' and plain[1].last_route.why == 'fused=False'
    cl_out, cl_z, cl = _run(plain, image.contiguous(memory_format=torch.channels_last), autocast)
    # Gradients that are zero in exact arithmetic carry rounding noise only, and the torch route disagrees with itself on them by
    # order 1: the key bias inside in_proj_bias (a softmax ignores a shift of its logits), and the bias of a convolution in front
    # of a GroupNorm with one channel per group (width 32 in 32 groups).  No route can be compared on them; they are recognised
    # by a self-disagreement above one half (not one digit in common), listed, and left out of both numbers.  They must stay a
    # minority.
    noise = sorted(n for n in base if _rel(cl[n], base[n]) > 0.5)
    print(f'modules autocast={autocast}: {len(noise)} of {len(base)} gradients are rounding noise on the torch route: {noise}')
    assert 4 * len(noise) < len(base) and 'image' not in noise
    base = {n: v for n, v in base.items() if n not in noise}
    self_dis = max([_rel(cl_out, base_out), _rel(cl_z, base_z)] + [_rel(cl[n], base[n]) for n in base])
    tol = 4 * max(self_dis, 2.0 ** -23)                                          # (never below one fp32 ulp of the largest element)
    for layout, x in (('NCHW', image), ('channels-last', image.contiguous(memory_format=torch.channels_last))):
        out, z, grads = _run(fused, x, autocast)
        assert fused[0].last_route.name == 'fused' and fused[1].last_route.name == 'fused', (fused[0].last_route, fused[1].last_route)
        dis = max([_rel(out, base_out), _rel(z, base_z)] + [_rel(grads[n], base[n]) for n in base])
        print(f'modules autocast={autocast}: torch route NCHW vs channels-last {self_dis:.3e}, fused {layout} vs torch {dis:.3e}, tolerance {tol:.3e}')
        assert torch.isfinite(out).all() and dis <= tol, (layout, dis, tol)


def test_last_parameter_gradient_twice_and_backward():
    """What VQGAN._aglw does: autograd.grad(loss, decoder.last_parameter, retain_graph=True) twice, then the real backward."""
    fused, _ = _pair()
    z = torch.randn(2, 256, 16, 16, device='cuda')
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                                   # the convolution's weight gradient: no atomics there either
    try:
        out, _ = fused[1](z, {})
        assert fused[1].last_route.name == 'fused'
        loss = out.square().mean()
        last = fused[1].last_parameter
        g1, = torch.autograd.grad(loss, last, retain_graph=True)
        g2, = torch.autograd.grad(loss, last, retain_graph=True)
        loss.backward()
    finally:
        torch.backends.cudnn.deterministic = keep
    assert torch.equal(g1, g2), float((g1 - g2).abs().max())
    assert torch.equal(g1, last.grad), float((g1 - last.grad).abs().max())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in fused[1].parameters())
