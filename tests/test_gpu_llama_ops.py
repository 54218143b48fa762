"""GPU checks of the two row modes LlamaTransformer runs on - add + RMS norm and SwiGLU: the kernels against the float64 restatement
of tests/llama_ops_ref.py within the bounds derived in include/vqhip.h (through _lib, never fitted) plus half an ulp of the output
dtype; NaN and infinity contained, an all-zero row, |gate| up to 100 (beyond the 88 the exponential's argument is held at),
subnormals, sum_out bit for bit, equal bits run to run and the adjoint identity.

Launch shapes crossed (include/vqhip.h, LAUNCH SHAPE).  The norm: (33, 1024) is the shipped width, one wave per row and three
slabs of 16 rows; (17, 2048) and (3, 2056) sit either side of the wave / workgroup boundary; (2, 8192) is the widest row; pieces of
8 ((1, 8), 1024, 2048, 2056, 8192 in the 16-bit rows), 4 ((5, 12); every fp32 row) and 1 are all taken, (5, 12) with a spare wave.
SwiGLU: (1, 1) is one element of a piece, (5, 12) has pieces that cross a row end in the 16-bit dtypes (12 % 8 != 0), (33, 2816) is
the shipped width, (257, 8) many short rows; test_swiglu_grid_edge sits either side of the 2 097 152 pieces one launch
covers with a thread each, forward and backward, in fp32 and in bf16, with F = 3072 as the existing activation test."""
import pytest
import torch

from vector_quantization_amd import _lib, functional, ops

import llama_ops_ref as ref
from test_gpu_vit_ops import BF16, COMBOS, F16, F32, store, within

pytestmark = pytest.mark.gpu

NORM_SHAPES = [(1, 8), (5, 12), (33, 1024), (17, 2048), (3, 2056), (2, 8192)]
SWIGLU_SHAPES = [(1, 1), (5, 12), (33, 2816), (257, 8)]
EPS = 1e-5


def check_norm(x, res, g, g_skip, gamma, ydt, tag):
    """Forward and backward of one call against the restatement; equal bits on a second call.  Returns the kernel's outputs."""
    s, y, stats = ops.add_rms_norm(x, res, gamma, EPS, ydt)
    R, D = x.shape
    assert y.dtype == ydt and s.dtype == x.dtype and stats.shape == (R, 2)
    ws = ref.rounded_sum(x, res)
    assert (s is x) if res is None else torch.equal(s, ws), f'{tag}: sum_out is not x + res bit for bit'
    want, wstats, p = ref.rms_forward(ws, gamma, EPS)
    bound = ref.rms_forward_bound(gamma, want, p)
    within(y, want, bound + store(want.abs() + bound, ydt), tag + ' y')
    assert not stats[:, 0].any(), f'{tag}: stats[2 r] is not 0'
    within(stats[:, 1:], p['rstd'], _lib.gn_rho(D, 0.0) * p['rstd'], tag + ' rstd')
    gx, dg = ops.add_rms_norm_backward(g, s, stats, gamma, g_skip)
    assert gx.dtype == x.dtype and dg.dtype == F32
    wgx, wdg, p = ref.rms_backward(g, ws, gamma, EPS, g_skip)
    e_gx, e_dg = ref.rms_backward_bounds(g, gamma, wgx, p, g_skip)
    within(gx, wgx, e_gx + store(wgx.abs() + e_gx, x.dtype), tag + ' gx')
    within(dg, wdg, e_dg, tag + ' dgamma')
    s2, y2, stats2 = ops.add_rms_norm(x, res, gamma, EPS, ydt)
    gx2, dg2 = ops.add_rms_norm_backward(g, s, stats, gamma, g_skip)
    for a, b in ((s, s2), (y, y2), (stats, stats2), (gx, gx2), (dg, dg2)):
        assert torch.equal(a, b), f'{tag}: two calls differ'
    return y, stats, gx


def check_swiglu(x, g, tag):
    y = ops.swiglu(x)
    want, p = ref.swiglu_forward(x)
    bound = ref.swiglu_forward_bound(want, p)
    within(y, want, bound + store(want.abs() + bound, x.dtype), tag + ' y')
    gx = ops.swiglu_backward(g, x)
    assert y.dtype == gx.dtype == x.dtype and gx.shape == x.shape and y.shape == g.shape
    wgx, p = ref.swiglu_backward(g, x)
    e_gx = ref.swiglu_backward_bound(wgx, p)
    within(gx, wgx, e_gx + store(wgx.abs() + e_gx, x.dtype), tag + ' gx')
    assert torch.equal(y, ops.swiglu(x)) and torch.equal(gx, ops.swiglu_backward(g, x)), f'{tag}: two calls differ'
    return y, gx


@pytest.mark.parametrize('xdt,ydt', COMBOS, ids=str)
@pytest.mark.parametrize('R,D', NORM_SHAPES, ids=str)
def test_add_rms_norm_within_the_derived_bound(R, D, xdt, ydt):
    gen = torch.Generator().manual_seed(R * 10000 + D)
    x = torch.randn(R, D, generator=gen).to(xdt).cuda()
    res = torch.randn(R, D, generator=gen).to(ydt).cuda()
    g = torch.randn(R, D, generator=gen).to(ydt).cuda()
    g_skip = torch.randn(R, D, generator=gen).to(xdt).cuda()
    gamma = torch.randn(D, generator=gen).cuda()
    check_norm(x, res, g, g_skip, gamma, ydt, f'add_rms_norm ({R}, {D}) {xdt} {ydt} res+skip')
    check_norm(x, None, g, None, gamma, ydt, f'add_rms_norm ({R}, {D}) {xdt} {ydt} plain')


@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=str)
@pytest.mark.parametrize('R,F', SWIGLU_SHAPES, ids=str)
def test_swiglu_within_the_derived_bound(R, F, dtype):
    gen = torch.Generator().manual_seed(R * 10000 + F + 1)
    x = (2.0 * torch.randn(R, 2 * F, generator=gen)).to(dtype).cuda()
    g = torch.randn(R, F, generator=gen).to(dtype).cuda()
    check_swiglu(x, g, f'swiglu ({R}, {F}) {dtype}')


@pytest.mark.parametrize('R,dtype', [(2730, F32), (2732, F32), (5461, BF16), (5462, BF16)], ids=str)
def test_swiglu_grid_edge(R, dtype):
    """Either side of the 2 097 152 pieces one launch covers with a thread each, forward and backward (both run on that grid):
    beyond it a thread takes a second piece, whose gate and up columns - and, backward, whose two gx pieces - must be those of its
    own elements.  Every shipped training shape is beyond it."""
    F = 3072
    W = 4 if dtype == F32 else 8
    assert (R * F // W <= _lib.ROW_ACT_GRID_PIECES) == (R in (2730, 5461)) and (R * F // W > _lib.ROW_ACT_GRID_PIECES) == (R in (2732, 5462))
    gen = torch.Generator(device='cuda').manual_seed(R)
    x = (2.0 * torch.randn(R, 2 * F, generator=gen, device='cuda')).to(dtype)
    g = torch.randn(R, F, generator=gen, device='cuda').to(dtype)
    check_swiglu(x, g, f'grid edge ({R}, {F}) {dtype}')


def test_the_two_norm_modes_are_paired_by_the_caller():
    """No call of the library sees both beta and dbeta, so stats of one mode fed to the backward of the other are not refused
    (include/vqhip.h says so); ops pairs them.  What the kernels then do is defined: the RMS backward does not read the mean (LayerNorm
    stats give the bits of (0, rstd)), and the LayerNorm backward on RMS stats is its own formula at mean 0."""
    gen = torch.Generator().manual_seed(13)
    x, g = torch.randn(19, 200, generator=gen).cuda(), torch.randn(19, 200, generator=gen).cuda()
    gamma, beta = torch.randn(200, generator=gen).cuda(), torch.randn(200, generator=gen).cuda()
    _, _, ln_stats = ops.add_layer_norm(x, None, gamma, beta, EPS)
    _, _, rms_stats = ops.add_rms_norm(x, None, gamma, EPS)
    assert ln_stats[:, 0].any() and not rms_stats[:, 0].any()
    no_mean = torch.stack([torch.zeros_like(ln_stats[:, 0]), ln_stats[:, 1]], 1)
    for a, b in zip(ops.add_rms_norm_backward(g, x, ln_stats, gamma), ops.add_rms_norm_backward(g, x, no_mean, gamma)):
        assert torch.equal(a, b)
    gx, dg, db = ops.add_layer_norm_backward(g, x, rms_stats, gamma)
    xh = x.double() * rms_stats[:, 1:].double()
    t = g.double() * gamma.double()
    want = rms_stats[:, 1:].double() * (t - t.mean(1, keepdim=True) - xh * (t * xh).mean(1, keepdim=True))
    assert float((gx.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert float((db.double() - g.double().sum(0)).abs().max()) <= 1e-5 * float(g.double().sum(0).abs().max())


@pytest.mark.parametrize('D', [1024, 2816], ids=str)
def test_nan_and_infinity_stay_in_their_row_and_a_zero_row_gives_zero(D):
    gen = torch.Generator().manual_seed(11)
    x, res = torch.randn(9, D, generator=gen).cuda(), torch.randn(9, D, generator=gen).cuda()
    gamma, g = torch.randn(D, generator=gen).cuda(), torch.randn(9, D, generator=gen).cuda()
    x[1], res[1] = 0.0, 0.0
    bad = x.clone()
    bad[3, 5] = float('nan')
    bad[6, D - 1] = float('inf')
    s0, y0, st0 = ops.add_rms_norm(x, res, gamma, EPS)
    s1, y1, st1 = ops.add_rms_norm(bad, res, gamma, EPS)
    keep = torch.ones(9, dtype=torch.bool, device='cuda')
    keep[3] = keep[6] = False
    assert torch.equal(y1[keep], y0[keep]) and torch.equal(st1[keep], st0[keep]) and torch.equal(s1[keep], s0[keep])
    # a NaN makes its row NaN; an infinity makes ms infinite and rstd 0: zeros, and a NaN where the infinity stood
    assert torch.isnan(y1[3]).all() and torch.isnan(y1[6, D - 1]) and not y1[6, :D - 1].any() and float(st1[6, 1]) == 0.0
    assert not y0[1].any() and float(st0[1, 1]) == pytest.approx(EPS ** -0.5, rel=1e-6)
    gx0, dg0 = ops.add_rms_norm_backward(g, s0, st0, gamma)
    gx1, _ = ops.add_rms_norm_backward(g, s1, st1, gamma)
    assert torch.isnan(gx1[~keep]).all() and torch.equal(gx1[keep], gx0[keep]) and torch.isfinite(gx0).all() and torch.isfinite(dg0).all()


@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=str)
def test_swiglu_range_subnormals_and_nan(dtype):
    """The gate over [-100, 100] on a fine grid (the exponential's argument is held at -88 beyond |a| = 88), the subnormals of fp32
    and of the dtype in either half, and a NaN or an infinity that stays in its element (backward: in its pair)."""
    F = 1024
    grid = torch.linspace(-100.0, 100.0, 6 * F).reshape(6, F)
    tiny = torch.tensor([2.0 ** -149, -2.0 ** -149, 2.0 ** -140, -2.0 ** -130, 2.0 ** -127, 6e-8, -6e-8, 1e-40]).repeat(F // 8)
    gate = torch.cat([grid, tiny.reshape(1, F), -tiny.reshape(1, F), grid[:2]])
    gen = torch.Generator().manual_seed(2)
    up = torch.cat([torch.randn(8, F, generator=gen), tiny.reshape(1, F), -tiny.reshape(1, F)])
    x = torch.cat([gate, up], 1).to(dtype).cuda()
    g = torch.randn(10, F, generator=gen).to(dtype).cuda()
    y, gx = check_swiglu(x, g, f'range {dtype}')
    for value, col in ((float('nan'), 17), (float('inf'), 17), (float('nan'), F + 17)):
        bad = x.clone()
        bad[4, col] = value
        y1, gx1 = ops.swiglu(bad), ops.swiglu_backward(g, bad)
        hit = torch.zeros_like(y, dtype=torch.bool)
        hit[4, 17] = True
        pair = torch.cat([hit, hit], 1)
        assert not torch.isfinite(y1[hit]).any() and torch.equal(y1[~hit], y[~hit]) and torch.equal(gx1[~pair], gx[~pair])
        assert not torch.isfinite(gx1[pair]).all()


def test_adjoint_identity():
    """<g, J v> == <J^T g, v>: J v by forward-mode differentiation of the restatement in float64, J^T g the kernels' gx in fp32;
    the two sides differ by at most sum |v| E_gx."""
    R, D = 37, 200
    gen = torch.Generator().manual_seed(5)
    x, g, v = (torch.randn(R, D, generator=gen).cuda() for _ in range(3))
    gamma = torch.randn(D, generator=gen).cuda()
    _, jv = torch.autograd.functional.jvp(lambda t: ref.rms_forward(t, gamma, EPS)[0], x.double(), v.double())
    _, _, stats = ops.add_rms_norm(x, None, gamma, EPS)
    gx, _ = ops.add_rms_norm_backward(g, x, stats, gamma)
    wgx, _, p = ref.rms_backward(g, x, gamma, EPS)
    cases = [('rms norm', g, jv, gx, v, ref.rms_backward_bounds(g, gamma, wgx, p)[0])]
    gh = g[:, :D // 2].contiguous()
    _, jv = torch.autograd.functional.jvp(lambda t: ref.swiglu_forward(t)[0], x.double(), v.double())
    gx = ops.swiglu_backward(gh, x)
    wgx, p = ref.swiglu_backward(gh, x)
    cases.append(('swiglu', gh, jv, gx, v, ref.swiglu_backward_bound(wgx, p)))
    for name, gg, jv, gx, vv, e_gx in cases:
        lhs, rhs = (gg.double() * jv).sum(), (gx.double() * vv.double()).sum()
        slack = (vv.double().abs() * e_gx).sum() + 1e-12 * (gg.double() * jv).abs().sum()
        print(f'adjoint {name}: lhs {float(lhs):.9e} rhs {float(rhs):.9e} slack {float(slack):.3e}')
        assert abs(float(lhs - rhs)) <= float(slack), name


def test_functional_gradients_autocast_and_the_torch_route():
    """functional.add_rms_norm / swiglu through autograd: gradients to x, res and weight, the gradient arriving at s as g_skip; the
    mixed autocast row (fp32 stream, bf16 branch, bf16 y); float64 takes the torch route."""
    gen = torch.Generator().manual_seed(9)
    x, r = torch.randn(4, 10, 96, generator=gen).cuda().requires_grad_(), torch.randn(4, 10, 96, generator=gen).cuda().bfloat16().requires_grad_()
    w = torch.randn(96, generator=gen).cuda().requires_grad_()
    g, gs = torch.randn(4, 10, 96, generator=gen).cuda().bfloat16(), torch.randn(4, 10, 96, generator=gen).cuda()
    s, y = functional.add_rms_norm(x, r, w, EPS, torch.bfloat16, strict=True)
    assert s.dtype == F32 and y.dtype == BF16 and torch.equal(s, x.detach() + r.detach())
    near = functional.add_rms_norm_torch(s.detach(), None, w.detach(), EPS)[1]                   # torch's fp32 norm, rounded once
    assert float((y.detach().float() - near).abs().max()) <= 2.0 ** -8 * float(near.abs().max())
    gx, gr, gw = torch.autograd.grad((y, s), (x, r, w), (g, gs))
    flat = lambda t: t.detach().reshape(-1, t.shape[-1])
    wgx, wdg, _ = ref.rms_backward(flat(g), flat(s), w.detach(), EPS, flat(gs))
    assert gr.dtype == BF16 and torch.equal(gr, gx.bfloat16())
    for got, want in ((flat(gx), wgx), (gw, wdg)):
        assert float((got.double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    h = torch.randn(4, 10, 192, generator=gen).cuda().requires_grad_()
    gh, = torch.autograd.grad(functional.swiglu(h, strict=True), h, gs)
    wgh, _ = ref.swiglu_backward(flat(gs), flat(h))
    assert float((flat(gh).double() - wgh).abs().max()) <= 1e-5
    xd = x.detach().double()
    s, y = functional.add_rms_norm(xd, xd, w.detach().double())
    assert torch.equal(y, functional.add_rms_norm_torch(xd, xd, w.detach().double())[1])
    assert torch.equal(functional.swiglu(h.detach().double()), functional.swiglu_torch(h.detach().double()))
