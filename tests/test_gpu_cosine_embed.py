"""GPU checks of the fused CosineEmbeddingLoss (vqhip_cosine_embed_fwd / _bwd) against the float64 restatement of
tests/cosine_embed_ref.py and the bounds derived in include/vqhip.h.  Every tolerance below is one of those bounds plus half an
ulp of the output dtype; none is fitted to an output."""
import numpy as np
import pytest
import torch

import cosine_embed_ref as ref
import vector_quantization_amd as vqa
from vector_quantization_amd import ops, tokenization

pytestmark = pytest.mark.gpu
U = ref.U


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    """The grid allocates a few hundred device buffers and autograd graphs: collect them and hand the cached blocks back when the
    module is done, so that the peak-memory checks of later modules start from what they allocate themselves."""
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _dev_view(t: torch.Tensor) -> torch.Tensor:
    """``t`` on the GPU with the strides it has on the CPU (a sliced view stays a sliced view of a buffer of the same shape)."""
    if t.is_contiguous():
        return t.cuda()
    R, C = t.shape
    buf = torch.full((R, t.stride(0)), ref.GARBAGE, dtype=t.dtype, device='cuda')
    buf[:, :C] = t.cuda()
    return buf[:, :C]


def _check_forward(f, e, C, R, tag):
    """loss within the bound of every row; out[0], out[1] within the rows' bounds plus the R-chain.  Returns worst err / bound."""
    b = ref.bound(C)
    err = np.abs(f['loss'].double().cpu().numpy() - e['loss'])
    print(f'{tag} loss: max err {err.max():.3e} bound {b:.3e}')
    assert (err <= b).all(), (tag, err.max(), b)
    cos_err = np.abs(f['stats'][:, 1].double().cpu().numpy() - e['cos'])
    assert (cos_err <= b).all(), (tag, cos_err.max(), b)
    tol_sum = R * b + ref.sum_chain(R) * U * np.abs(e['loss']).sum()
    out = f['out'].double().cpu().numpy()
    assert abs(out[0] - e['total']) <= tol_sum, (tag, out[0], e['total'], tol_sum)
    assert abs(out[1] - e['total'] / R) <= tol_sum / R + 2 * U * abs(e['total'] / R), (tag, out[1], e['total'] / R)
    return float(err.max() / b)


def _grad_tolerance(e, c, C, dtype):
    """|c_r| times the fp32 bound of an element, plus half an ulp of pred's dtype at the value."""
    want = c[:, None] * e['grad_unit']
    tol32 = np.abs(c)[:, None] * ref.grad_bound(C, e['h'])[:, None] * np.ones((1, C))
    return want, tol32 + ref.half_ulp(np.abs(want) + tol32, dtype)


def _g(R, reduction, seed):
    return np.random.default_rng(90 + seed).normal(size=R if reduction == 'none' else 1).astype(np.float32)


def test_rows_forward_within_the_bound():
    worst = 0.0
    for case in ref.cases():
        C, R, pad, dtypes, seed = case
        pred, target = ref.make_case(*case)
        f = ops.cosine_embedding_forward(_dev_view(pred), _dev_view(target))
        assert f['loss'].shape == (R,) and f['stats'].shape == (R, 3) and f['out'].shape == (2,)
        worst = max(worst, _check_forward(f, ref.expected(case), C, R, case))
    print(f'worst error / bound over the rows grid: {worst:.4f}')


@pytest.mark.parametrize('reduction', ['mean', 'none'])
def test_rows_backward_within_the_bound_every_element_written(reduction):
    worst = 0.0
    for case in ref.cases():
        C, R, pad, dtypes, seed = case
        pred, target = ref.make_case(*case)
        e = ref.expected(case)
        pd, td = _dev_view(pred), _dev_view(target)
        g = _g(R, reduction, seed)
        gd = torch.from_numpy(g).cuda()
        leaf = pd.detach().requires_grad_()
        loss = ops.cosine_embedding_loss(leaf, td, reduction)
        assert loss.dtype == torch.float32 and loss.shape == (() if reduction == 'mean' else (R,))
        loss.backward(gd.reshape(loss.shape))
        grad = leaf.grad
        assert grad.dtype == dtypes[0] and grad.shape == pred.shape
        c = g.astype(np.float64) / (R if reduction == 'mean' else 1.0) * np.ones(R)
        want, tol = _grad_tolerance(e, c, C, dtypes[0])
        err = np.abs(grad.double().cpu().numpy() - want)
        worst = max(worst, float((err / tol).max()))
        print(f'{case} {reduction}: max grad err {err.max():.3e}, max err / tol {(err / tol).max():.3f}')
        assert (err <= tol).all(), (case, err.max())
        # the same into a buffer pre-filled with NaN, of pred's strides: every element is written, the padding is not touched
        buf = torch.full((R, C + pad), float('nan'), dtype=dtypes[0], device='cuda')
        f = ops.cosine_embedding_forward(pd, td)
        got = ops.cosine_embedding_backward(pd, td, f['stats'], gd, mean=reduction == 'mean', out=buf[:, :C])
        assert got.data_ptr() == buf.data_ptr() and torch.equal(buf[:, :C], grad), case
        assert bool(torch.isnan(buf[:, C:]).all()), case
    print(f'worst gradient error / tolerance over the rows grid: {worst:.4f}')


def test_map_layout_against_the_same_reference():
    worst = worst_g = 0.0
    for case in ref.map_cases():
        B, C, P, dtypes, seed = case
        R = B * P
        pmap, prow, target = ref.make_map_case(*case)
        e = ref.expected_map(case)
        md, td = pmap.cuda(), target.cuda()
        f = ops.cosine_embedding_forward(md, td, layout='map')
        worst = max(worst, _check_forward(f, e, C, R, case))
        frows = ops.cosine_embedding_forward(prow.cuda(), td.reshape(R, C))               # both layouts within the bound of float64
        _check_forward(frows, e, C, R, (case, 'rows'))
        for reduction in ('mean', 'none'):
            g = _g(R, reduction, seed)
            gd = torch.from_numpy(g).cuda()
            leaf = md.detach().requires_grad_()
            loss = ops.cosine_embedding_loss(leaf, td, reduction, layout='map')
            assert loss.shape == (() if reduction == 'mean' else (B, P))
            loss.backward(gd.reshape(loss.shape))
            assert leaf.grad.dtype == dtypes[0] and leaf.grad.shape == (B, C, P) and leaf.grad.is_contiguous()
            c = g.astype(np.float64) / (R if reduction == 'mean' else 1.0) * np.ones(R)
            want, tol = _grad_tolerance(e, c, C, dtypes[0])
            got = leaf.grad.permute(0, 2, 1).reshape(R, C).double().cpu().numpy()
            err = np.abs(got - want)
            worst_g = max(worst_g, float((err / tol).max()))
            assert (err <= tol).all(), (case, reduction, err.max())
            buf = torch.full_like(md, float('nan'))
            ops.cosine_embedding_backward(md, td, f['stats'], gd, layout='map', mean=reduction == 'mean', out=buf)
            assert torch.equal(buf, leaf.grad), case
    print(f'worst error / bound over the map grid: {worst:.4f}; gradient error / tolerance: {worst_g:.4f}')


def test_reproducible_and_independent_of_strides_and_other_rows():
    one = torch.ones(1, device='cuda')
    for case in [c for c in ref.cases() if c[1] == 5 and c[2] == 3]:
        C, R, pad, dtypes, seed = case
        pred, target = ref.make_case(*case)
        pd, td = _dev_view(pred), _dev_view(target)
        a, again = ops.cosine_embedding_forward(pd, td), ops.cosine_embedding_forward(pd, td)
        pc, tc = pd.contiguous(), td.contiguous()                              # other row stride, other alignment of every row
        assert pd.stride(0) == C + 3 and pc.stride(0) == C
        dense = ops.cosine_embedding_forward(pc, tc)
        for k in ('loss', 'stats', 'out'):
            assert torch.equal(a[k], again[k]) and torch.equal(a[k], dense[k]), (case, k)
        ga = ops.cosine_embedding_backward(pd, td, a['stats'], one, mean=True)
        assert torch.equal(ga, ops.cosine_embedding_backward(pc, tc, a['stats'], one, mean=True)), case
        assert torch.equal(ga, ops.cosine_embedding_backward(pd, td, a['stats'], one, mean=True)), case
        for r in range(R):                                                     # a row alone has the bits it has inside the batch
            alone = ops.cosine_embedding_forward(pd[r:r + 1].clone(), td[r:r + 1].clone())
            assert torch.equal(alone['loss'], a['loss'][r:r + 1]) and torch.equal(alone['stats'], a['stats'][r:r + 1]), (case, r)
    for case in ref.map_cases():
        B, C, P, dtypes, seed = case
        R = B * P
        pmap, _, target = ref.make_map_case(*case)
        md, td = pmap.cuda(), target.cuda()
        ts = _dev_view(ref._strided(target.reshape(R, C), 3))                  # the target rows as a strided view
        a, again = ops.cosine_embedding_forward(md, td, layout='map'), ops.cosine_embedding_forward(md, td, layout='map')
        strided = ops.cosine_embedding_forward(md, ts, layout='map')
        for k in ('loss', 'stats', 'out'):
            assert torch.equal(a[k], again[k]) and torch.equal(a[k], strided[k]), (case, k)
        ga = ops.cosine_embedding_backward(md, td, a['stats'], one, layout='map', mean=True)
        assert torch.equal(ga, ops.cosine_embedding_backward(md, ts, a['stats'], one, layout='map', mean=True)), case
        for r in sorted({0, R // 2, R - 1}):                                   # a position alone: B = 1, P = 1
            b, p = divmod(r, P)
            alone = ops.cosine_embedding_forward(md[b, :, p].reshape(1, C, 1).contiguous(), td[b, p].reshape(1, 1, C).clone(), layout='map')
            assert torch.equal(alone['loss'], a['loss'][r:r + 1]) and torch.equal(alone['stats'], a['stats'][r:r + 1]), (case, r)


@pytest.mark.parametrize('layout', ['rows', 'map'])
@pytest.mark.parametrize('dtypes', [(torch.bfloat16, torch.float32), (torch.float32, torch.float32)])
def test_degenerate_and_non_finite_rows_follow_the_table_and_stay_in_their_row(dtypes, layout):
    R, C = 9, 100
    inf, nan = float('inf'), float('nan')
    gen = torch.Generator().manual_seed(21)
    clean_p = torch.randn(R, C, generator=gen).to(dtypes[0])
    clean_t = torch.randn(R, C, generator=gen).to(dtypes[1])
    clean_p[1] = 0                                                             # a zero pred row
    clean_t[2] = 0                                                             # a zero target row
    clean_p[8] = 0
    clean_t[8] = 0                                                             # both zero
    p, t = clean_p.clone(), clean_t.clone()
    p[3, 40] = nan
    p[4, 17] = inf
    p[5, 99] = -inf
    t[6, 0] = nan
    t[7, 63] = -inf
    t[7, 64] = inf
    poisoned = [3, 4, 5, 6, 7]
    rest = [0, 1, 2, 8]

    def run(pp, tt):
        if layout == 'map':
            pm = pp.reshape(3, 3, C).permute(0, 2, 1).contiguous().cuda()
            f = ops.cosine_embedding_forward(pm, tt.reshape(3, 3, C).cuda(), layout='map')
            g = ops.cosine_embedding_backward(pm, tt.reshape(3, 3, C).cuda(), f['stats'], torch.ones(1, device='cuda'), layout='map')
            return f, g.permute(0, 2, 1).reshape(R, C)
        f = ops.cosine_embedding_forward(pp.cuda(), tt.cuda())
        return f, ops.cosine_embedding_backward(pp.cuda(), tt.cuda(), f['stats'], torch.ones(1, device='cuda'))

    f, grad = run(p, t)
    e = ref.reference(ref.as64(p), ref.as64(t))
    loss, gd = f['loss'].double().cpu().numpy(), grad.double().cpu().numpy()
    # the header's table
    assert loss[1] == 1.0 and loss[2] == 1.0 and loss[8] == 1.0 and np.isnan(loss[poisoned]).all() and np.isfinite(loss[rest]).all()
    assert np.isnan(gd[poisoned]).all() and np.isfinite(gd[rest]).all() and not gd[8].any() and not gd[2].any() and gd[1].any()
    # ... which is the float64 reference's pattern, and the finite values are within the bounds
    assert np.array_equal(np.isnan(loss), np.isnan(e['loss'])) and np.array_equal(np.isnan(gd), np.isnan(e['grad_unit']))
    assert (np.abs(loss[rest] - e['loss'][rest]) <= ref.bound(C)).all()
    want = e['grad_unit'][rest]
    tol32 = ref.grad_bound(C, e['h'][rest])[:, None] * np.ones((1, C))
    assert (np.abs(gd[rest] - want) <= tol32 + ref.half_ulp(np.abs(want) + tol32, dtypes[0])).all()
    assert np.isnan(float(f['out'][0])) and np.isnan(float(f['out'][1]))
    # the other rows are unchanged bit for bit against a run without the poison
    fc, gc = run(clean_p, clean_t)
    assert torch.equal(f['loss'][rest], fc['loss'][rest]) and torch.equal(f['stats'][rest], fc['stats'][rest])
    assert torch.equal(grad[rest], gc[rest]) and bool(torch.isfinite(fc['loss']).all()) and bool(torch.isfinite(fc['out']).all())


def test_module_routes_autocast_and_the_map_entry_point():
    torch.manual_seed(4)
    B, L, C = 2, 49, 96
    m = vqa.CosineEmbeddingLoss()
    head = torch.nn.Linear(32, C).cuda()
    h = torch.randn(B, L, 32, device='cuda')
    target = torch.randn(B, L, C, device='cuda')
    with torch.autocast('cuda', dtype=torch.bfloat16):
        pred = head(h)
        loss = m(pred, target)
    assert pred.dtype == torch.bfloat16 and m.last_route.name == 'fused', m.last_route
    assert loss.dtype == torch.float32 and loss.shape == ()
    e = ref.reference(ref.as64(pred.detach().cpu()), ref.as64(target.cpu()))
    R = B * L
    tol = ref.bound(C) + ref.sum_chain(R) * U * np.abs(e['loss']).sum() / R + 2 * U * abs(e['total'] / R)
    assert abs(float(loss.detach()) - e['total'] / R) <= tol
    loss.backward()
    gw = head.weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and bool(gw.abs().sum() > 0)
    # float64: the reference's composition, with the reason
    got = m(pred.detach().double(), target.double())
    assert m.last_route.name == 'torch' and 'float64' in m.last_route.why and got.dtype == torch.float64
    assert abs(float(got) - e['total'] / R) <= 1e-12
    # the map entry point against the rows entry point on the rearranged tensor
    pmap = torch.randn(B, C, 7, 7, device='cuda').to(torch.bfloat16).requires_grad_()
    via_map = tokenization.distill_loss(m, pmap, target)
    assert m.last_route.name == 'fused', m.last_route
    rows = pmap.detach().flatten(2).transpose(1, 2).contiguous().requires_grad_()
    via_rows = m(rows, target)
    assert m.last_route.name == 'fused'
    e = ref.reference(ref.as64(rows.detach().cpu()), ref.as64(target.cpu()))
    tol = ref.bound(C) + ref.sum_chain(R) * U * np.abs(e['loss']).sum() / R + 2 * U * abs(e['total'] / R)
    assert abs(float(via_map) - e['total'] / R) <= tol and abs(float(via_rows) - e['total'] / R) <= tol
    via_map.backward()
    via_rows.backward()
    assert pmap.grad.shape == pmap.shape and pmap.grad.dtype == torch.bfloat16
    c = np.full(R, 1.0 / R)
    want, tol = _grad_tolerance(e, c, C, torch.bfloat16)
    for got in (pmap.grad.flatten(2).transpose(1, 2).reshape(R, C), rows.grad.reshape(R, C)):
        assert (np.abs(got.double().cpu().numpy() - want) <= tol).all()
    # 'none' and a weight, as BaseReconstructLoss has them
    n = vqa.CosineEmbeddingLoss(reduction='none', weight=0.5)
    per = n(rows.detach(), target)
    assert n.last_route.name == 'fused' and per.shape == (B, L) and per.dtype == torch.float32
    assert (np.abs(per.double().cpu().numpy().reshape(-1) - 0.5 * e['loss']) <= 0.5 * ref.bound(C)).all()
