"""The fused sampler on the GPU against the numpy restatement (tests/sampler_ref.py): top-k exactly, top-p up to the ambiguous
run at the header's delta, the draw against float64 intervals over the kernel's own kept set, the distribution without an RNG,
CFG keys bit for bit, bad rows, run-to-run identity, and the modules.

Shapes (sampler_ref.cases): not the full product of V, start, R and dtype.  Every V in {1, 2, 63, 64, 65, 257, 1024, 4099, 16384}
meets every start in {0, 1, 1001} and every dtype (81 cases), with R cycling through {1, 2, 6} over them instead of every R for
every combination; the long rows (the LDS-resident limit, one more, 64 000) get three (start, dtype) pairs each at R = 2.  What R
could interact with is the alignment of a row's slice, which start, dtype and the odd row stride (end + 7) already vary."""
import numpy as np
import pytest
import torch

import sampler_ref as ref
from vector_quantization_amd import _lib, ops, samplers

pytestmark = pytest.mark.gpu

TORCH_DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float16': torch.float16}
_CASES = {}


def case(V, start, R, dtype, seed):
    """(device logits in ``dtype``, a fp32 [R, V] of the restatement), computed once and shared."""
    key = (V, start, R, dtype, seed)
    if key not in _CASES:
        full = ref.make_logits(V, start, R, dtype, seed)
        dev = torch.from_numpy(full).cuda().to(TORCH_DTYPES[dtype])
        assert np.array_equal(dev.float().cpu().numpy(), full)
        _CASES[key] = (dev, full)
    return _CASES[key]


def run(dev, start, V, u, **kw):
    tokens, cut = ops.sample_tokens(dev, start, start + V, u=u, want_cut=True, **kw)
    return tokens.cpu().numpy(), ops.sample_cut_fields(cut)


def uniforms(Ro, seed):
    u = np.random.default_rng(seed).random(Ro).astype(np.float32)
    u[u >= 1.0] = 0.5
    return u


def check_z(a_row, kept, z, dlt):
    """cut.z is the kept mass in units of exp(0): every mass is within delta / 2 of its float64 value relatively and loses less than
    2^-40 to truncation (Z >= 1), so the sum is within delta relatively; the fp32 store adds 2^-24."""
    Z = ref.masses(a_row, kept).sum()
    assert abs(float(z) / Z - 1.0) <= dlt + 2.0 ** -23, (float(z), Z)


def check_draw(a_row, kept, token, u, dlt, start):
    j = int(token) - start
    assert 0 <= j < a_row.shape[0] and kept[j], (j, 'not a kept token')
    lo, hi = ref.draw_interval(a_row, kept, j)
    assert lo - dlt <= float(u) <= hi + dlt, (j, lo, hi, float(u))


def cases_of(V):
    return [c for c in ref.cases() if c[0] == V]


@pytest.mark.parametrize('V', ref.VS + ref.BIG_VS)
def test_top_k_is_exact(V):
    """cut.topk_kept and the set the cut describes equal the restatement for every top_k, on random rows, rows with ties at the
    k-th value (values rounded to integers) and all-equal rows; top-p off."""
    dlt = ref.delta(V)
    for (v, start, R, dtype, seed) in cases_of(V):
        dev, full = case(v, start, R, dtype, seed)
        tied = torch.round(dev.float() * 2).to(dev.dtype)
        flat = torch.full_like(dev, 0.25)
        u = uniforms(R, seed)
        ud = torch.from_numpy(u).cuda()
        for variant in (dev, tied, flat):
            a = ref.keys(variant.float().cpu().numpy()[:, start:start + v])
            for top_k in ref.TOP_KS + (v, v + 5):
                tokens, cut = run(variant, start, v, ud, top_k=top_k)
                for r in range(R):
                    surv = ref.topk_set(a[r], top_k)
                    assert cut['topk_kept'][r] == surv.sum() == cut['kept'][r], (v, start, dtype, top_k, r)
                    kept = ref.kept_from_cut(a[r], cut['cut_value'][r], cut['cut_index'][r])
                    assert np.array_equal(kept, surv), (v, start, dtype, top_k, r)
                    assert cut['max'][r] == a[r].max()
                    check_draw(a[r], kept, tokens[r], u[r], dlt, start)
                    check_z(a[r], kept, cut['z'][r], dlt)


@pytest.mark.parametrize('V', ref.VS + ref.BIG_VS)
def test_top_p_cut_lies_in_the_ambiguous_run(V):
    dlt = ref.delta(V)
    for (v, start, R, dtype, seed) in cases_of(V):
        dev, full = case(v, start, R, dtype, seed)
        a = ref.keys(full[:, start:start + v])
        u = uniforms(R, seed + 1)
        ud = torch.from_numpy(u).cuda()
        for top_k in ref.TOP_P_KS:
            for top_p in ref.TOP_PS:
                tokens, cut = run(dev, start, v, ud, top_k=top_k, top_p=top_p)
                for r in range(R):
                    rc = ref.RowCut(a[r], top_k, top_p, dlt)
                    kept = ref.kept_from_cut(a[r], cut['cut_value'][r], cut['cut_index'][r])
                    # (rebuilt from the cut record, so an upper set by construction; that the kernel's DRAW honours this set is
                    #  what check_draw's kept[j] and interval, and check_z's kept mass, show)
                    assert kept.sum() == cut['kept'][r] and cut['topk_kept'][r] == rc.surv.sum(), (v, start, dtype, top_k, top_p, r)
                    assert not (kept & ~rc.surv).any()
                    pos = rc.n - int(kept.sum())                    # position, in ascending rank, of the kernel's lowest kept token
                    assert rc.asc[pos] == cut['cut_index'][r] and a[r][rc.asc[pos]] == cut['cut_value'][r]
                    if rc.ambiguous == 0:
                        assert pos == rc.pos, (v, start, dtype, top_k, top_p, r, pos, rc.pos)
                    else:
                        assert rc.run[0] <= pos <= rc.run[1], (v, start, dtype, top_k, top_p, r, pos, rc.run)
                    if top_p == 0.0:                                # exactly the top-ranked token: the lowest index among the maxima
                        assert kept.sum() == 1 and cut['cut_index'][r] == int(np.argmax(a[r]))
                    check_draw(a[r], kept, tokens[r], u[r], dlt, start)
                    check_z(a[r], kept, cut['z'][r], dlt)


def test_p_zero_keeps_the_lowest_index_among_tied_maxima():
    V, start = 4099, 1
    x = torch.zeros(3, start + V + 3)
    x[:, start + 17] = 2.0
    x[:, start + 3000] = 2.0
    x[2] = 1.5                                                      # an all-equal row
    u = torch.tensor([0.0, 0.999, 0.5]).cuda()
    for dtype in TORCH_DTYPES.values():
        tokens, cut = run(x.cuda().to(dtype), start, V, u, top_p=0.0, top_k=600)
        assert tokens.tolist() == [start + 17, start + 17, start] and cut['kept'].tolist() == [1, 1, 1]
        assert cut['cut_index'].tolist() == [17, 17, 0]


@pytest.mark.parametrize('V', (64, 4099, ref.RESIDENT_MAX + 1))
def test_draw_end_points(V):
    """u = 0 gives the first kept token in index order, u = nextafter(1, 0) the last (every kept token of these rows holds more
    than delta + 2^-24 of the mass: top_k = 20 on a narrow spread)."""
    start, R = 1001, 4
    g = np.random.default_rng(V)
    full = np.full((R, start + V + 5), 9.0, dtype=np.float32)
    full[:, start:] = g.normal(0, 0.5, size=(R, V + 5))
    dev = torch.from_numpy(full).cuda().bfloat16()
    a = ref.keys(dev.float().cpu().numpy()[:, start:start + V])
    for uval, pick in ((0.0, 0), (float(np.nextafter(np.float32(1), np.float32(0))), -1)):
        u = torch.full((R,), uval).cuda()
        tokens, cut = run(dev, start, V, u, top_k=20, top_p=2.0)
        for r in range(R):
            kept = ref.kept_from_cut(a[r], cut['cut_value'][r], cut['cut_index'][r])
            m = ref.masses(a[r], kept)
            assert (m[kept] / m.sum()).min() > ref.delta(V) + 2.0 ** -24
            assert tokens[r] - start == np.nonzero(kept)[0][pick]


def test_distribution_without_an_rng():
    """4096 rows of the same logits, u_i = (i + 0.5) / 4096: each token's count is within 1 + 2 delta 4096 of 4096 p_j."""
    V, N = 64, 4096
    row = np.random.default_rng(11).normal(0, 1.5, size=V).astype(np.float32)
    dev = torch.from_numpy(np.tile(row, (N, 1))).cuda()
    u = torch.from_numpy(((np.arange(N) + 0.5) / N).astype(np.float32)).cuda()
    tokens = ops.sample_tokens(dev, 0, V, u=u).cpu().numpy()
    p = ref.masses(row, np.ones(V, dtype=bool))
    p = p / p.sum()
    counts = np.bincount(tokens, minlength=V)
    assert counts.sum() == N
    assert np.abs(counts - N * p).max() <= 1 + 2 * ref.delta(V) * N, np.abs(counts - N * p).max()


@pytest.mark.parametrize('alpha', (0.0, 1.0, 1.75))
@pytest.mark.parametrize('dtype', ('float32', 'bfloat16', 'float16'))
def test_cfg_keys_bit_for_bit(alpha, dtype):
    for (V, start, R, temperature) in ((257, 1001, 6, 1.0), (4099, 1, 2, 0.7), (ref.RESIDENT_MAX + 1, 1001, 2, 1.3)):
        dev, full = case(V, start, R, dtype, 77)
        a = ref.keys(full[:, start:start + V], cfg_alpha=alpha, temperature=temperature)
        Ro = R // 2
        u = uniforms(Ro, 3)
        tokens, cut = run(dev, start, V, torch.from_numpy(u).cuda(), top_k=50, cfg_alpha=alpha, temperature=temperature)
        assert np.array_equal(tokens[:Ro], tokens[Ro:])
        for r in range(Ro):
            assert cut['max'][r].view(np.uint32) == a[r].max().view(np.uint32)
            kth = np.sort(a[r])[-50]
            assert cut['cut_value'][r].view(np.uint32) == kth.view(np.uint32)
            kept = ref.kept_from_cut(a[r], cut['cut_value'][r], cut['cut_index'][r])
            assert np.array_equal(kept, ref.topk_set(a[r], 50))
            check_draw(a[r], kept, tokens[r], u[r], ref.delta(V), start)
            check_z(a[r], kept, cut['z'][r], ref.delta(V))


def test_the_op_never_copies_and_never_reads_past_the_last_dimension():
    x = torch.zeros(2, 3, 64).cuda()
    with pytest.raises(ValueError):
        ops.sample_tokens(x.transpose(0, 1), 0, 64, u=torch.zeros(6).cuda())       # does not flatten as a view
    with pytest.raises(ValueError):
        ops.sample_tokens(x[..., :32], 0, 40, u=torch.zeros(6).cuda())             # end beyond the narrowed view
    with pytest.raises(ValueError):
        ops.sample_tokens(x[0, :1].expand(4, 64), 0, 64, u=torch.zeros(4).cuda())  # overlapping rows
    s = samplers.TopKTopPSampler(top_k=4)
    tokens, _ = s(x[0, :1].expand(4, 64), 0, 64, {})                               # the module falls back with a reason
    assert s.last_route.name == 'torch' and 'overlap' in s.last_route.why and tokens.shape == (4,)


def test_odd_r_is_refused_under_cfg():
    x = torch.zeros(3, 64).cuda()
    with pytest.raises(_lib.VqhipError):
        ops.sample_tokens(x, 0, 64, u=torch.zeros(1).cuda(), cfg_alpha=1.5)


@pytest.mark.parametrize('V', (65, 4099, ref.RESIDENT_MAX + 1))
def test_bad_rows(V):
    start = 1
    g = np.random.default_rng(V)
    x = g.normal(0, 1, size=(8, start + V + 2)).astype(np.float32)
    x[1, start + V // 2] = np.nan
    x[3, start + V - 1] = np.inf
    x[5, start:start + V] = -np.inf
    x[6, start:start + V:2] = -np.inf                                # masked entries: never drawn
    x[0, 0] = np.nan                                                 # outside the slice: not read
    x[2, start + V] = np.inf
    u = uniforms(8, 9)
    for dtype in TORCH_DTYPES.values():
        dev = torch.from_numpy(x).cuda().to(dtype)
        a = ref.keys(dev.float().cpu().numpy()[:, start:start + V])
        for kw in (dict(), dict(top_k=50, top_p=0.92)):
            tokens, cut = run(dev, start, V, torch.from_numpy(u).cuda(), **kw)
            assert tokens[[1, 3, 5]].tolist() == [-1, -1, -1] and cut['cut_index'][[1, 3, 5]].tolist() == [-1, -1, -1]
            for r in (0, 2, 4, 6, 7):
                kept = ref.kept_from_cut(a[r], cut['cut_value'][r], cut['cut_index'][r])
                check_draw(a[r], kept, tokens[r], u[r], ref.delta(V), start)
                check_z(a[r], kept, cut['z'][r], ref.delta(V))
                assert np.isfinite(a[r][tokens[r] - start])
            good, _ = run(dev[[0, 2, 4, 6, 7]], start, V, torch.from_numpy(u[[0, 2, 4, 6, 7]]).cuda(), **kw)
            assert np.array_equal(good, tokens[[0, 2, 4, 6, 7]])     # the neighbours of bad rows are unaffected
    # under CFG a bad half makes both halves -1
    dev = torch.from_numpy(x).cuda()
    tokens, _ = run(dev, start, V, torch.from_numpy(u[:4]).cuda(), cfg_alpha=1.75)
    assert tokens[1] == tokens[5] == -1 and tokens[3] == tokens[7] == -1 and np.array_equal(tokens[:4], tokens[4:])


def test_two_identical_calls_give_identical_results():
    for (V, start, R, dtype, seed) in (cases_of(16384)[1], cases_of(64000)[0], cases_of(257)[2]):
        dev, _ = case(V, start, R, dtype, seed)
        u = torch.from_numpy(uniforms(R, 1)).cuda()
        outs = [ops.sample_tokens(dev, start, start + V, u=u, top_k=600, top_p=0.92, want_cut=True) for _ in range(3)]
        for t, c in outs[1:]:
            assert torch.equal(t, outs[0][0]) and torch.equal(c, outs[0][1])


def test_resident_and_streamed_rows_agree():
    """The same slice values read from LDS (V = the resident limit) and re-read from memory (one more column that cannot win):
    the same cut and the same token."""
    V, start, R = ref.RESIDENT_MAX, 1, 2
    dev, full = case(V, start, R, 'bfloat16', 5)
    wide = dev.clone()
    wide[:, start + V] = -float('inf')
    u = torch.from_numpy(uniforms(R, 2)).cuda()
    t0, c0 = run(dev, start, V, u, top_k=600, top_p=0.92)
    t1, c1 = run(wide, start, V + 1, u, top_k=600, top_p=0.92)
    assert np.array_equal(t0, t1)
    for f in ('kept', 'topk_kept', 'cut_index'):
        assert np.array_equal(c0[f], c1[f])
    for f in ('cut_value', 'max', 'z'):
        assert np.array_equal(c0[f].view(np.uint32), c1[f].view(np.uint32))


def test_modules_take_the_fused_route():
    torch.manual_seed(0)
    x = torch.randn(2, 3, 17385, device='cuda').bfloat16()
    start, end = 1001, 17385
    u6, u3 = torch.rand(6, device='cuda'), torch.rand(3, device='cuda')
    s = samplers.TopKTopPSampler()
    tokens, memo = s(x, start, end, {'u': u6})
    assert s.last_route.name == 'fused' and tokens.shape == (2, 3) and tokens.dtype == torch.int64
    assert torch.equal(tokens, ops.sample_tokens(x, start, end, u=u6, temperature=1.0, top_k=600, top_p=0.92))
    c = samplers.CFGSampler(sampler=samplers.TopKTopPSampler(temperature=0.9), alpha=1.75)
    tokens, _ = c(x, start, end, {'u': u3})
    assert c.last_route.name == 'fused' and tokens.shape == (2, 3)
    assert torch.equal(tokens, ops.sample_tokens(x, start, end, u=u3, temperature=0.9, top_k=600, top_p=0.92, cfg_alpha=1.75))
    assert torch.equal(tokens[0], tokens[1])
    b = samplers.BaseSampler()
    tokens, _ = b(x.float(), start, end, {'u': u6})
    assert b.last_route.name == 'fused' and torch.equal(tokens, ops.sample_tokens(x.float(), start, end, u=u6))
    # a strided view is read in place
    view = x[:, :, :9000]
    tokens, _ = s(view, start, 9000, {'u': u6})
    assert s.last_route.name == 'fused' and torch.equal(tokens, ops.sample_tokens(view.contiguous(), start, 9000, u=u6, top_k=600, top_p=0.92))
    # a seeded generator gives the same tokens twice, and the block of uniforms is advanced between steps
    runs = []
    for _ in range(2):
        torch.manual_seed(123)
        s2 = samplers.TopKTopPSampler()
        runs.append(torch.stack([s2(x, start, end, {})[0] for _ in range(3)]))
    assert torch.equal(runs[0], runs[1])
    assert not torch.equal(runs[0][0], runs[0][1])


def test_a_step_allocates_less_than_one_logit_matrix():
    R, Vt = 128, 17385
    x = torch.randn(R, Vt, device='cuda').bfloat16()
    c = samplers.CFGSampler(sampler=samplers.TopKTopPSampler(), alpha=1.75)
    c(x, 1001, Vt, {})                                              # the block of uniforms exists from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    tokens, _ = c(x, 1001, Vt, {})
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < R * (Vt - 1001) * 4
    assert c.last_route.name == 'fused' and tokens.shape == (R,)
