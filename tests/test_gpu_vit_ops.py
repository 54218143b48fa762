"""GPU checks of the row ops of VQKDEncoder / VQKDDecoder (add + LayerNorm, bias + GELU / tanh): the kernels against the float64
restatement of tests/vit_ops_ref.py within the bounds derived in include/vqhip.h (through _lib, never fitted) plus half an ulp of
the output dtype, the hostile inputs of the contract (a large mean, a constant row, NaN and infinity, subnormals), sum_out bit
for bit, equal bits run to run and the adjoint identity.

Launch shapes crossed (include/vqhip.h, LAUNCH SHAPE).  The norm: D <= 2048 takes one wave per row, beyond it one workgroup per
row: (3, 2048) and (3, 2052) sit either side, (2, 8192) is the widest row.  Pieces: D % 8 == 0 (8 elements where every tensor is
16-bit: (1, 8), (5, 24), 768, 3072), D % 4 == 0 only ((7, 100), (3, 2052)), single elements ((5, 7), (3, 2051)).  The forward has
four rows per workgroup ((5, 24), (7, 100): a workgroup with spare waves); the backward 16 rows per slab ((17, 24): two slabs, the
second with one row; (394, 768): 25 slabs, which is also two workgroups' worth of 256 rows for the activation's backward, whose
column blocks of 64 pieces end inside (3, 3072) fp32 at 256 columns and inside (7, 100)).  The activation's forward gives every
16-byte piece a thread up to 8192 workgroups x 256 threads = 2 097 152 pieces and strides beyond: fp32 (2730, 3072) is 2 096 640
pieces, (2732, 3072) 2 098 176; bf16 (5461, 3072) is 2 097 024, (5462, 3072) 2 097 408 (test_forward_grid_edge; every shipped width
at a training batch is beyond it)."""
import pytest
import torch

from vector_quantization_amd import _lib, functional, ops

import vit_ops_ref as ref

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CODE = {F32: _lib.DTYPE_F32, BF16: _lib.DTYPE_BF16, F16: _lib.DTYPE_F16}
COMBOS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)]         # (x, res = y): the table of include/vqhip.h
SHAPES = [(1, 8), (5, 24), (7, 100), (3, 768), (394, 768), (3, 3072), (5, 7), (17, 24), (3, 2048), (3, 2052), (3, 2051), (2, 8192)]
EPS = 1e-6


def store(value, dtype):
    """Half an ulp of the output dtype on top of a bound for |value| (VQHIP_SG2_STORE_U), and half an ulp of its subnormals: 2^-25 for
    fp16, 2^-134 for bf16 (the activation tests store subnormal results)."""
    return _lib.sg2_store_u(CODE[dtype]) * value + {F16: 2.0 ** -25, BF16: 2.0 ** -134}.get(dtype, 0.0)


def within(got, want, bound, what):
    got, want = got.double(), want.double()
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), f'{what}: not finite'
    err = (got - want).abs()
    b = bound.expand_as(want) if torch.is_tensor(bound) else torch.full_like(err, bound)
    ratio = torch.where(err > 0, err / b, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f'{what}: worst error / bound = {worst:.3f}')
    assert worst <= 1.0, f'{what}: error / bound = {worst}'


def check_norm(x, res, g, g_skip, gamma, beta, ydt, tag):
    """Forward and backward of one call against the restatement; equal bits on a second call.  Returns the kernel's outputs."""
    s, y, stats = ops.add_layer_norm(x, res, gamma, beta, EPS, ydt)
    R, D = x.shape
    assert y.dtype == ydt and s.dtype == x.dtype and stats.shape == (R, 2)
    ws = ref.rounded_sum(x, res)
    assert (s is x) if res is None else torch.equal(s, ws), f'{tag}: sum_out is not x + res bit for bit'
    want, wstats, p = ref.ln_forward(ws, gamma, beta, EPS)
    bound = ref.ln_forward_bound(ws, gamma, beta, EPS, want, p)
    within(y, want, bound + store(want.abs() + bound, ydt), tag + ' y')
    q = _lib.gn_q(D, p['mabs'], p['rstd'])
    within(stats[:, :1], p['mean'].squeeze(2), (_lib.gn_chain(D) * _lib.GN_U * p['mabs'] + 1e-45).squeeze(2), tag + ' mean')
    within(stats[:, 1:], p['rstd'].squeeze(2), (_lib.gn_rho(D, q) * p['rstd']).squeeze(2), tag + ' rstd')
    gx, dg, db = ops.add_layer_norm_backward(g, s, stats, gamma, g_skip)
    assert gx.dtype == x.dtype and dg.dtype == db.dtype == F32
    wgx, wdg, wdb, p = ref.ln_backward(g, ws, gamma, beta, EPS, g_skip)
    e_gx, e_dg, e_db = ref.ln_backward_bounds(g, ws, gamma, beta, EPS, wgx, p, g_skip)
    within(gx, wgx, e_gx + store(wgx.abs() + e_gx, x.dtype), tag + ' gx')
    within(dg, wdg, e_dg, tag + ' dgamma')
    within(db, wdb, e_db, tag + ' dbeta')
    s2, y2, stats2 = ops.add_layer_norm(x, res, gamma, beta, EPS, ydt)
    gx2, dg2, db2 = ops.add_layer_norm_backward(g, s, stats, gamma, g_skip)
    for a, b in ((s, s2), (y, y2), (stats, stats2), (gx, gx2), (dg, dg2), (db, db2)):
        assert torch.equal(a, b), f'{tag}: two calls differ'
    return y, stats, gx


def check_act(x, g, bias, act, tag):
    y = ops.row_bias_act(x, bias, act)
    want, p = ref.act_forward(x, bias, act)
    bound = ref.act_forward_bound(act, want, p)
    within(y, want, bound + store(want.abs() + bound, x.dtype), tag + ' y')
    gx, dbias = ops.row_bias_act_backward(g, x, bias, act)
    assert y.dtype == gx.dtype == x.dtype and dbias.dtype == F32
    wgx, wdb, p = ref.act_backward(g, x, bias, act)
    e_gx, e_db = ref.act_backward_bounds(act, g, wgx, p)
    within(gx, wgx, e_gx + store(wgx.abs() + e_gx, x.dtype), tag + ' gx')
    within(dbias, wdb, e_db + 1e-45, tag + ' dbias')
    gx2, dbias2 = ops.row_bias_act_backward(g, x, bias, act)
    assert torch.equal(y, ops.row_bias_act(x, bias, act)) and torch.equal(gx, gx2) and torch.equal(dbias, dbias2), f'{tag}: two calls differ'
    assert torch.equal(ops.row_bias_act_backward(g, x, bias, act, need_dbias=False)[0], gx)
    return y, gx


@pytest.mark.parametrize('xdt,ydt', COMBOS, ids=str)
@pytest.mark.parametrize('R,D', SHAPES, ids=str)
def test_add_layer_norm_within_the_derived_bound(R, D, xdt, ydt):
    gen = torch.Generator().manual_seed(R * 10000 + D)
    x = torch.randn(R, D, generator=gen).to(xdt).cuda()
    res = torch.randn(R, D, generator=gen).to(ydt).cuda()
    g = torch.randn(R, D, generator=gen).to(ydt).cuda()
    g_skip = torch.randn(R, D, generator=gen).to(xdt).cuda()
    gamma, beta = torch.randn(D, generator=gen).cuda(), torch.randn(D, generator=gen).cuda()
    check_norm(x, res, g, g_skip, gamma, beta, ydt, f'add_layer_norm ({R}, {D}) {xdt} {ydt} res+skip')
    check_norm(x, None, g, None, gamma, beta, ydt, f'add_layer_norm ({R}, {D}) {xdt} {ydt} plain')


@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=str)
@pytest.mark.parametrize('act', ['gelu', 'tanh'])
@pytest.mark.parametrize('R,D', SHAPES, ids=str)
def test_row_bias_act_within_the_derived_bound(R, D, act, dtype):
    gen = torch.Generator().manual_seed(R * 10000 + D + 1)
    x = (2.0 * torch.randn(R, D, generator=gen)).to(dtype).cuda()
    g = torch.randn(R, D, generator=gen).to(dtype).cuda()
    bias = torch.randn(D, generator=gen).cuda()
    check_act(x, g, bias, act, f'row_bias_act ({R}, {D}) {act} {dtype}')


@pytest.mark.parametrize('R,dtype', [(2730, F32), (2732, F32), (5461, BF16), (5462, BF16)], ids=str)
@pytest.mark.parametrize('act', ['gelu', 'tanh'])
def test_forward_grid_edge(act, R, dtype):
    """Either side of the 2 097 152 pieces one launch covers with a thread each: beyond it a thread takes a second piece, whose
    bias column must be that of its own element."""
    D = 3072
    W = 4 if dtype == F32 else 8
    assert (R * D // W <= _lib.ROW_ACT_GRID_PIECES) == (R in (2730, 5461)) and (R * D // W > _lib.ROW_ACT_GRID_PIECES) == (R in (2732, 5462))
    gen = torch.Generator(device='cuda').manual_seed(R)
    x = (2.0 * torch.randn(R, D, generator=gen, device='cuda')).to(dtype)
    bias = torch.randn(D, generator=gen, device='cuda')
    y = ops.row_bias_act(x, bias, act)
    want, p = ref.act_forward(x, bias, act)
    bound = ref.act_forward_bound(act, want, p)
    within(y, want, bound + store(want.abs() + bound, dtype), f'grid edge ({R}, {D}) {act} {dtype} y')
    assert torch.equal(y, ops.row_bias_act(x, bias, act))


@pytest.mark.parametrize('xdt,ydt', COMBOS, ids=str)
def test_a_mean_of_a_thousand_deviations_and_a_constant_row(xdt, ydt):
    """x + res = 1000 + randn: E[x^2] - mean^2 would lose every digit, the second pass does not.  A constant row has var = 0 and
    y = beta within the bound, whose q term is the fp32 error of the mean in units of eps^1/2."""
    R, D = 6, 768
    gen = torch.Generator().manual_seed(7)
    x = (1000.0 + torch.randn(R, D, generator=gen)).to(xdt)
    res = (0.01 * torch.randn(R, D, generator=gen)).to(ydt)
    x[2], res[2] = 0.3, 0.0
    x[5], res[5] = -7.0, 0.0
    x, res = x.cuda(), res.cuda()
    g, g_skip = torch.randn(R, D, generator=gen).to(ydt).cuda(), torch.randn(R, D, generator=gen).to(xdt).cuda()
    gamma, beta = (1.0 + 0.1 * torch.randn(D, generator=gen)).cuda(), (0.1 * torch.randn(D, generator=gen)).cuda()
    y, _, gx = check_norm(x, res, g, g_skip, gamma, beta, ydt, f'1000 + randn {xdt} {ydt}')
    assert torch.isfinite(gx).all()
    for r in (2, 5):
        value = abs(float(x[r, 0]))
        tol = _lib.gn_y_bound(D, _lib.gn_q(D, value, EPS ** -0.5), 0.0, gamma.double().abs(), beta.double().abs(), beta.double().abs(), 0)
        assert bool(((y[r].double() - beta.double()).abs() <= tol + store(beta.double().abs() + tol, ydt)).all()), r


@pytest.mark.parametrize('D', [768, 3072], ids=str)
def test_nan_and_infinity_stay_in_their_row(D):
    gen = torch.Generator().manual_seed(11)
    x, res = torch.randn(9, D, generator=gen).cuda(), torch.randn(9, D, generator=gen).cuda()
    gamma, beta = torch.randn(D, generator=gen).cuda(), torch.randn(D, generator=gen).cuda()
    g = torch.randn(9, D, generator=gen).cuda()
    bad = x.clone()
    bad[3, 5] = float('nan')
    bad[6, D - 1] = float('inf')
    s0, y0, st0 = ops.add_layer_norm(x, res, gamma, beta, EPS)
    s1, y1, st1 = ops.add_layer_norm(bad, res, gamma, beta, EPS)
    keep = torch.ones(9, dtype=torch.bool, device='cuda')
    keep[3] = keep[6] = False
    assert torch.isnan(y1[~keep]).all() and torch.equal(y1[keep], y0[keep]) and torch.equal(st1[keep], st0[keep]) and torch.equal(s1[keep], s0[keep])
    gx0, _, _ = ops.add_layer_norm_backward(g, s0, st0, gamma)
    gx1, _, _ = ops.add_layer_norm_backward(g, s1, st1, gamma)
    assert torch.isnan(gx1[~keep]).all() and torch.equal(gx1[keep], gx0[keep])


@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=str)
@pytest.mark.parametrize('act', ['gelu', 'tanh'])
def test_activation_range_subnormals_and_nan(act, dtype):
    """t over [-12, 12] on a fine grid (bias 0 and a bias that shifts it), the subnormals of fp32 and of the dtype, and a NaN that
    stays in its element."""
    D = 1024
    grid = torch.linspace(-12.0, 12.0, 6 * D).reshape(6, D)
    tiny = torch.tensor([2.0 ** -149, -2.0 ** -149, 2.0 ** -140, -2.0 ** -130, 2.0 ** -127, 6e-8, -6e-8, 1e-40]).repeat(D // 8)
    x = torch.cat([grid, tiny.reshape(1, D), -tiny.reshape(1, D)]).to(dtype).cuda()
    g = torch.randn(8, D, generator=torch.Generator().manual_seed(2)).to(dtype).cuda()
    for bias in (torch.zeros(D), 0.25 * torch.randn(D, generator=torch.Generator().manual_seed(3))):
        y, gx = check_act(x, g, bias.cuda(), act, f'range {act} {dtype}')
        bad = x.clone()
        bad[4, 17] = float('nan')
        y1 = ops.row_bias_act(bad, bias.cuda(), act)
        gx1, _ = ops.row_bias_act_backward(g, bad, bias.cuda(), act)
        hit = torch.zeros_like(bad, dtype=torch.bool)
        hit[4, 17] = True
        assert torch.isnan(y1[hit]).all() and torch.isnan(gx1[hit]).all() and torch.equal(y1[~hit], y[~hit]) and torch.equal(gx1[~hit], gx[~hit])


def test_adjoint_identity():
    """<g, J v> == <J^T g, v>: J v by forward-mode differentiation of the restatement in float64, J^T g the kernels' gx in fp32;
    the two sides differ by at most sum |v| E_gx."""
    R, D = 37, 200
    gen = torch.Generator().manual_seed(5)
    x, g, v = (torch.randn(R, D, generator=gen).cuda() for _ in range(3))
    gamma, beta = torch.randn(D, generator=gen).cuda(), torch.randn(D, generator=gen).cuda()
    _, jv = torch.autograd.functional.jvp(lambda t: ref.ln_forward(t, gamma, beta, EPS)[0], x.double(), v.double())
    _, _, stats = ops.add_layer_norm(x, None, gamma, beta, EPS)
    gx, _, _ = ops.add_layer_norm_backward(g, x, stats, gamma)
    wgx, _, _, p = ref.ln_backward(g, x, gamma, beta, EPS)
    e_gx, _, _ = ref.ln_backward_bounds(g, x, gamma, beta, EPS, wgx, p)
    cases = [('norm', jv, gx, e_gx)]
    for act in ('gelu', 'tanh'):
        _, jv = torch.autograd.functional.jvp(lambda t: ref.act_forward(t, beta, act)[0], x.double(), v.double())
        gx, _ = ops.row_bias_act_backward(g, x, beta, act)
        wgx, _, p = ref.act_backward(g, x, beta, act)
        cases.append((act, jv, gx, ref.act_backward_bounds(act, g, wgx, p)[0]))
    for name, jv, gx, e_gx in cases:
        lhs, rhs = (g.double() * jv).sum(), (gx.double() * v.double()).sum()
        slack = (v.double().abs() * e_gx).sum() + 1e-12 * (g.double() * jv).abs().sum()
        print(f'adjoint {name}: lhs {float(lhs):.9e} rhs {float(rhs):.9e} slack {float(slack):.3e}')
        assert abs(float(lhs - rhs)) <= float(slack), name


def test_functional_gradients_autocast_and_the_torch_route():
    """functional.add_layer_norm / row_bias_act through autograd: gradients to x, res, weight and bias, the gradient arriving at s
    as g_skip; the mixed autocast combination; float64 takes the torch route."""
    gen = torch.Generator().manual_seed(9)
    x, r = torch.randn(4, 10, 96, generator=gen).cuda().requires_grad_(), torch.randn(4, 10, 96, generator=gen).cuda().bfloat16().requires_grad_()
    w, b = torch.randn(96, generator=gen).cuda().requires_grad_(), torch.randn(96, generator=gen).cuda().requires_grad_()
    g, gs = torch.randn(4, 10, 96, generator=gen).cuda().bfloat16(), torch.randn(4, 10, 96, generator=gen).cuda()
    s, y = functional.add_layer_norm(x, r, w, b, EPS, torch.bfloat16)
    assert s.dtype == F32 and y.dtype == BF16 and torch.equal(s, x.detach() + r.detach())
    near = torch.nn.functional.layer_norm(s, (96,), w, b, EPS).detach()                          # torch's fp32 norm, rounded once
    assert float((y.detach().float() - near).abs().max()) <= 2.0 ** -8 * float(near.abs().max())
    gx, gr, gw, gb = torch.autograd.grad((y, s), (x, r, w, b), (g, gs))
    flat = lambda t: t.detach().reshape(-1, 96)
    wgx, wdg, wdb, _ = ref.ln_backward(flat(g), flat(s), w.detach(), b.detach(), EPS, flat(gs))
    assert gr.dtype == BF16 and torch.equal(gr, gx.bfloat16())
    for got, want in ((flat(gx), wgx), (gw, wdg), (gb, wdb)):
        assert float((got.double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    h = torch.randn(4, 10, 96, generator=gen).cuda().requires_grad_()
    for act in ('gelu', 'tanh'):
        gh, gbias = torch.autograd.grad(functional.row_bias_act(h, b, act), (h, b), gs)
        wgh, wgb, _ = ref.act_backward(flat(gs), flat(h), b.detach(), act)
        assert float((flat(gh).double() - wgh).abs().max()) <= 1e-5 and float((gbias.double() - wgb).abs().max()) <= 1e-4
    xd = x.detach().double()
    s, y = functional.add_layer_norm(xd, xd, w.detach().double(), b.detach().double())
    assert torch.equal(y, functional.add_layer_norm_torch(xd, xd, w.detach().double(), b.detach().double())[1])
