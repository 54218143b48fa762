"""GPU checks of the fused token cross-entropy (vqhip_token_ce_fwd / _bwd) against the float64 restatement of tests/token_ce_ref.py
and the bounds derived in include/vqhip.h.  Every tolerance below is one of those bounds; none is fitted to an output."""
import functools

import numpy as np
import pytest
import torch

import token_ce_ref as ref
from vector_quantization_amd import ops, sequence_losses as SL

pytestmark = pytest.mark.gpu
U = ref.U


@functools.lru_cache(maxsize=None)
def _weights(R, seed):
    return np.random.default_rng(50 + seed).uniform(0.0, 2.0, size=R).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _expected(case, eps, weighted):
    """The float64 reference of a case, computed once and shared: (reference dict, amax per row)."""
    V, start, R, dtype, seed = case
    x, t = ref.make_case(*case)
    a = ref.slice64(x, start, V)
    w = _weights(R, seed).astype(np.float64) if weighted else None
    return ref.reference(a, ref.row_targets(t.numpy(), start, V), eps, w), np.abs(a).max(-1)


def _scalar_tolerances(e, row_bound):
    """Bounds of sum_r w_r loss_r and of the mean, from the header: the rows' own errors, the products w_r * loss_r, the chain
    of the R-sum; the mean adds W's chain and the division."""
    live, w = e['live'], np.abs(e['w'])
    R = len(live)
    mass = (w[live] * np.abs(e['loss'][live])).sum()
    tol_sum = (w[live] * row_bound[live]).sum() + (ref.chain(R) + 1) * U * mass
    mean = e['total'] / e['wsum']
    return tol_sum, tol_sum / e['wsum'] + abs(mean) * (ref.chain(R) + 2) * U


@pytest.mark.parametrize('tdtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_forward_rows_and_reductions_within_the_bound(eps, weighted, tdtype):
    worst = 0.0
    for case in ref.cases():
        V, start, R, dtype, seed = case
        x, t = ref.make_case(*case)
        e, amax = _expected(case, eps, weighted)
        xd, td = x.cuda(), t.to(tdtype).cuda()
        wd = torch.from_numpy(_weights(R, seed)).cuda() if weighted else None
        kw = dict(label_smoothing=eps, weight=wd)
        f = ops.token_ce_forward(xd, td, start, start + V, **kw)
        b = np.array([ref.bound(V, am) for am in amax])
        for name in ('lse', 'loss'):
            err = np.abs(f[name].double().cpu().numpy() - e[name])
            print(f'{case} eps={eps} w={weighted} {name}: max err {err.max():.3e} bound {b.min():.3e}')
            worst = max(worst, float((err / b).max()))
            assert (err <= b).all(), (case, name, err.max(), b)
        assert np.array_equal(f['hit'].cpu().numpy(), e['hit']), case
        tol_sum, tol_mean = _scalar_tolerances(e, b)
        got_sum = float(ops.token_cross_entropy(xd, td, start, start + V, reduction='sum', **kw))
        got_mean, stats = ops.token_cross_entropy(xd, td, start, start + V, reduction='mean', want_stats=True, **kw)
        got_none = ops.token_cross_entropy(xd, td, start, start + V, reduction='none', **kw)
        assert abs(got_sum - e['total']) <= tol_sum, (case, got_sum, e['total'], tol_sum)
        assert abs(float(got_mean) - e['total'] / e['wsum']) <= tol_mean, (case, float(got_mean), e['total'] / e['wsum'], tol_mean)
        assert abs(float(stats['weight_sum']) - e['wsum']) <= (ref.chain(R) + 1) * U * e['wsum'] and float(stats['hits']) == e['hits']
        want_none = e['w'] * e['loss']
        assert got_none.shape == (R,) and got_none.dtype == torch.float32
        assert (np.abs(got_none.double().cpu().numpy() - want_none) <= np.abs(e['w']) * b + U * np.abs(want_none)).all(), case
    print(f'worst error / bound over the grid: {worst:.4f}')


@pytest.mark.parametrize('reduction', ['mean', 'none'])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_backward_within_the_bound_and_zeros_where_nothing_flows(eps, reduction):
    worst = 0.0
    for case in ref.cases():
        V, start, R, dtype, seed = case
        x, t = ref.make_case(*case)
        e, amax = _expected(case, eps, True)
        xd, td = x.cuda(), t.cuda()
        wd = torch.from_numpy(_weights(R, seed)).cuda()
        g = np.random.default_rng(90 + seed).normal(size=R if reduction == 'none' else 1).astype(np.float32)
        leaf = xd.clone().requires_grad_()
        loss = ops.token_cross_entropy(leaf, td, start, start + V, label_smoothing=eps, weight=wd, reduction=reduction)
        loss.backward(torch.from_numpy(g).cuda().reshape(loss.shape))
        grad = leaf.grad
        assert grad.dtype == dtype and grad.shape == x.shape
        gd = grad.double().cpu().numpy()
        c = g.astype(np.float64) * e['w'] / (e['wsum'] if reduction == 'mean' else 1.0)
        c = np.where(e['live'], c, 0.0)
        want = c[:, None] * e['grad_unit']
        # per unit |c_r|: the fp32 bound of an element, and c_r's own error (two roundings and W's chain); then the rounding
        per_c = np.array([ref.grad_bound(V, am) for am in amax]) + (ref.chain(R) + 3) * U
        tol32 = np.abs(c)[:, None] * per_c[:, None] * np.ones((1, V))
        tol = tol32 + ref.half_ulp(np.abs(want) + tol32, dtype)
        err = np.abs(gd[:, start:start + V] - want)
        worst = max(worst, float((err / tol).max()))
        print(f'{case} eps={eps} {reduction}: max grad err {err.max():.3e}, max err / tol {(err / tol).max():.3f}')
        assert (err <= tol).all(), (case, err.max())
        assert not gd[:, :start].any() and not gd[:, start + V:].any() and not gd[~e['live']].any(), case
        # the same into a buffer pre-filled with NaN: every element is written by the kernel
        buf = torch.full_like(xd, float('nan'))
        f = ops.token_ce_forward(xd, td, start, start + V, label_smoothing=eps, weight=wd)
        ops.token_ce_backward(xd, td, f['lse'], torch.from_numpy(g).cuda(), start, start + V, label_smoothing=eps, weight=wd,
                              weight_sum=f['out'][1:2] if reduction == 'mean' else None, out=buf)
        assert torch.equal(buf, grad), case
    print(f'worst gradient error / tolerance over the grid: {worst:.4f}')


@pytest.mark.parametrize('B,L', [(3, 5), (2, 257)])
def test_shift_equals_explicitly_rolled_targets(B, L):
    Vt = 41
    g = torch.Generator().manual_seed(B * L)
    x = (torch.randn(B, L, Vt, generator=g) * 3).to(torch.bfloat16).cuda()
    tokens = torch.randint(0, Vt, (B, L), generator=g)
    tokens[0, 2] = -100
    rolled = torch.roll(tokens, -1, dims=1)
    rolled[:, -1] = -100
    a = ops.token_ce_forward(x, tokens.cuda(), shift=True)
    b = ops.token_ce_forward(x, rolled.cuda())
    for k in ('loss', 'lse', 'hit', 'out'):
        assert torch.equal(a[k], b[k]), k
    # CausalTokenLoss against HF's semantics in float64
    m = SL.CausalTokenLoss()
    loss, memo = m(x, tokens.cuda(), {})
    assert m.last_route.name == 'fused', m.last_route
    a64 = ref.slice64(x.cpu(), 0, Vt)
    e = ref.reference(a64, ref.row_targets(tokens.reshape(-1).numpy(), 0, Vt, shift_len=L), 0.0)
    want = torch.nn.functional.cross_entropy(torch.from_numpy(a64).reshape(B, L, Vt)[:, :-1].reshape(-1, Vt), tokens[:, 1:].reshape(-1))
    assert abs(e['total'] / e['wsum'] - float(want)) <= 1e-12
    _, tol_mean = _scalar_tolerances(e, np.array([ref.bound(Vt, am) for am in np.abs(a64).max(-1)]))
    assert abs(float(loss) - float(want)) <= tol_mean
    assert float(memo['accuracy']) == pytest.approx(e['hits'] / e['wsum'], rel=2 ** -22)


def test_hit_breaks_ties_towards_the_lowest_index():
    x = torch.zeros(4, 70, dtype=torch.float16)
    x[0, [5, 9, 40]] = 3.0                     # tied maximum: the arg-max is 5
    x[1, [5, 9, 40]] = 3.0
    x[2] = 1.5                                 # all equal: the arg-max is the slice's first element
    x[3] = 1.5
    t = torch.tensor([5, 9, 3, 4])
    for start, want in ((0, [1, 0, 0, 0]), (3, [1, 0, 1, 0]), (4, [1, 0, 0, 1])):
        f = ops.token_ce_forward(x.cuda(), t.cuda(), start, 70)
        assert f['hit'].tolist() == want and float(f['out'][2]) == sum(want)
    m = SL.CausalTokenLoss()
    seq = torch.zeros(1, 4, 8, dtype=torch.bfloat16)
    seq[0, 0, [2, 6]] = 1.0                    # next token 2: hit;  position 1: all equal, next token 0: hit;  position 2: next 5: miss
    _, memo = m(seq.cuda(), torch.tensor([[7, 2, 0, 5]]).cuda(), {})
    assert float(memo['accuracy']) == pytest.approx(2 / 3, rel=2 ** -22)


def test_reproducible_and_independent_of_layout_target_dtype_and_other_rows():
    for case in [c for c in ref.cases() if c[2] == 6]:
        V, start, R, dtype, seed = case
        x, t = ref.make_case(*case)
        xd, td = x.cuda(), t.cuda()
        kw = dict(label_smoothing=0.1, weight=torch.from_numpy(_weights(R, seed)).cuda())
        a = ops.token_ce_forward(xd, td, start, start + V, **kw)
        again = ops.token_ce_forward(xd, td, start, start + V, **kw)
        i32 = ops.token_ce_forward(xd, td.int(), start, start + V, **kw)
        # the slice as a contiguous tensor of its own: other row stride, other alignment of every row
        copy = xd[:, start:start + V].contiguous()
        assert copy.stride(0) == V
        dense = ops.token_ce_forward(copy, td - start, 0, V, **dict(kw, ignore_index=ref.IGNORE - start))
        for k in ('loss', 'lse', 'hit', 'out'):
            assert torch.equal(a[k], again[k]) and torch.equal(a[k], i32[k]) and torch.equal(a[k], dense[k]), (case, k)
        g = torch.ones(1, device='cuda')
        ga = ops.token_ce_backward(xd, td, a['lse'], g, start, start + V, weight_sum=a['out'][1:2], **kw)
        gb = ops.token_ce_backward(copy, td - start, a['lse'], g, 0, V, weight_sum=a['out'][1:2], **dict(kw, ignore_index=ref.IGNORE - start))
        assert torch.equal(ga[:, start:start + V], gb), case
        for r in range(R):                                   # a row alone: its per-row outputs do not depend on the other rows
            alone = ops.token_ce_forward(xd[r:r + 1].clone(), td[r:r + 1], start, start + V, label_smoothing=0.1)
            for k in ('loss', 'lse', 'hit'):
                assert torch.equal(alone[k], a[k][r:r + 1]), (case, r, k)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_non_finite_rows_follow_the_table_and_stay_in_their_row(eps, dtype):
    start, V = 1, 100
    inf, nan = float('inf'), float('nan')
    x = torch.randn(9, start + V + ref.PAD, generator=torch.Generator().manual_seed(11)) * 2
    t = torch.randint(start, start + V, (9,), generator=torch.Generator().manual_seed(12))
    x[1, 40] = nan
    x[2, 17] = inf
    x[3, [3, 50, 99]] = -inf
    t[3] = 10
    x[4, [20, 60]] = -inf
    t[4] = 20                                  # a_t = -inf
    x[5, start:start + V] = -inf
    t[6] = 0                                   # outside the slice (below it)
    t[7] = start + V + 3                       # outside the slice (above it)
    x = x.to(dtype)
    a64 = ref.slice64(x, start, V)
    e = ref.reference(a64, ref.row_targets(t.numpy(), start, V), eps)
    xd, td = x.cuda(), t.cuda()
    f = ops.token_ce_forward(xd, td, start, start + V, label_smoothing=eps)
    lse, loss = f['lse'].double().cpu().numpy(), f['loss'].double().cpu().numpy()
    # the header's table
    assert np.isnan(lse[[1, 2, 5]]).all() and np.isfinite(lse[[0, 3, 4, 6, 7, 8]]).all()
    assert np.isnan(loss[[1, 2, 5, 6, 7]]).all() and loss[4] == inf and np.isfinite(loss[[0, 8]]).all()
    assert (loss[3] == inf) if eps else np.isfinite(loss[3])
    assert f['hit'][[1, 2, 5, 6, 7]].tolist() == [0] * 5
    # ... which is the float64 reference's pattern, and the finite values are within the bound
    with np.errstate(all='ignore'):
        amax = np.where(np.isfinite(a64), np.abs(a64), 0.0).max(-1)
    b = np.array([ref.bound(V, am) for am in amax])
    for got, want in ((lse, e['lse']), (loss, e['loss'])):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isneginf(got).any() and not np.isneginf(want).any()
        fin = np.isfinite(want)
        assert (np.abs(got[fin] - want[fin]) <= b[fin]).all()
    assert np.isnan(float(f['out'][0])) and np.isnan(float(f['out'][3])) and float(f['out'][1]) == 9.0
    grad = ops.token_ce_backward(xd, td, f['lse'], torch.ones(1, device='cuda'), start, start + V, label_smoothing=eps)
    gd = grad.double().cpu().numpy()
    assert not gd[:, :start].any() and not gd[:, start + V:].any()
    gs, want = gd[:, start:start + V], e['grad_unit']
    assert np.array_equal(np.isnan(gs), np.isnan(want)) and np.isnan(gs[[1, 2, 5, 6, 7]]).all() and np.isfinite(gs[[0, 3, 4, 8]]).all()
    fin = np.isfinite(want)
    tol = np.broadcast_to(np.array([ref.grad_bound(V, am) for am in amax])[:, None], want.shape)
    tol = tol + ref.half_ulp(np.abs(np.where(fin, want, 0.0)) + tol, dtype)
    assert (np.abs(gs - want)[fin] <= tol[fin]).all()
    if not eps:
        assert not gs[3][[2, 49, 98]].any()                                        # p = 0 at the -inf entries


def test_modules_take_the_fused_route_and_carry_gradients():
    torch.manual_seed(2)
    # MaskedTokenLoss on [2, 9, 40], codebook_size 32, against the float64 restatement of forward_loss
    B, S, Vt, K = 2, 8, 40, 32
    logits = (torch.randn(B, S + 1, Vt) * 2).to(torch.bfloat16).cuda().requires_grad_()
    gt = torch.randint(0, K, (B, S)).cuda()
    mask = (torch.rand(B, S + 1) > 0.4).float().cuda()
    q = SL.MaskedTokenLoss(K, 0.1)
    loss = q(gt, logits, mask)
    assert q.last_route.name == 'fused', q.last_route
    a64 = logits.detach().double().cpu()
    want = q.forward_torch(gt.cpu(), a64, mask.double().cpu())
    amax = float(a64[:, 1:, :K].abs().max())
    n = float(mask[:, 1:].sum())
    # rows within the bound, their 0 / 1-weighted sum and the division (header: the scalars)
    tol = ref.bound(K, amax) + abs(float(want)) * (2 * ref.chain(B * (S + 1)) + 3 + 2) * U + 2.0 ** -23 * (2 * amax + 4)
    assert n > 0 and abs(float(loss) - float(want)) <= tol, (float(loss), float(want), tol)
    loss.backward()
    gd = logits.grad.double().cpu()
    assert logits.grad.dtype == torch.bfloat16 and not gd[:, 0].any() and not gd[:, :, K:].any() and gd[:, 1:, :K].any()
    leaf = a64.clone().requires_grad_()
    q.forward_torch(gt.cpu(), leaf, mask.double().cpu()).backward()
    c = 1.0 / n
    tol32 = c * (ref.grad_bound(K, amax) + (ref.chain(B * (S + 1)) + 3) * U + 2.0 ** -23)
    err = (gd - leaf.grad).abs().numpy()
    assert (err <= tol32 + ref.half_ulp(leaf.grad.abs().numpy() + tol32, torch.bfloat16)).all(), err.max()
    # LabelSmoothingCrossEntropy: per-row, the reference's signature
    crit = SL.LabelSmoothingCrossEntropy(0.1)
    rows = crit(logits.detach()[:, :, :K].reshape(-1, K).contiguous(), torch.randint(0, K, (B * (S + 1),)).cuda())
    assert crit.last_route.name == 'fused' and rows.shape == (B * (S + 1),) and bool(torch.isfinite(rows).all())
    # CausalTokenLoss: a requires_grad leaf behind a bf16 head, plain and under autocast
    head = torch.nn.Linear(16, Vt).cuda()
    h = torch.randn(B, S + 1, 16, device='cuda')
    tokens = torch.randint(0, Vt, (B, S + 1)).cuda()
    m = SL.CausalTokenLoss()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = head(h)
        loss, memo = m(out, tokens, {})
    assert out.dtype == torch.bfloat16 and m.last_route.name == 'fused' and loss.dtype == torch.float32
    loss.backward()
    assert head.weight.grad is not None and bool(torch.isfinite(head.weight.grad).all()) and bool(head.weight.grad.abs().sum() > 0)
    leaf = (torch.randn(B, S + 1, Vt, device='cuda') * 2).to(torch.bfloat16).requires_grad_()
    loss, _ = m(leaf, tokens, {})
    loss.backward()
    assert m.last_route.name == 'fused' and leaf.grad.dtype == torch.bfloat16 and not leaf.grad[:, -1].any() and leaf.grad[:, :-1].any()
    # each live row of the gradient sums to zero up to its rounding (sum_j p_j = 1, one target)
    assert float(leaf.grad.double().sum(-1).abs().max()) <= Vt * 2.0 ** -9 / (B * S)
