"""The bounds of tests/update_ref.py, proven on the CPU for every row of the case table the GPU tests use:

1. ATen's fp32 evaluation of the same ``oracle.torch_ref`` compositions differs from the float64 one by at most the derived
   tolerance, no element excluded; so do ``oracle.c_oracle.ema`` / ``cvq_decay`` / ``kmeans_centroids`` and, where the
   reference checkout is present, the reference's own ``CVQVAECallback.after_encode`` / ``VQKDCallback.after_encode`` at two
   non-default settings;
2. the bound has teeth: every deliberately wrong float64 restatement of update_ref lies outside it on at least one case;
3. no case is vacuous: each has an element with a tolerance above the floor and a non-zero reference;
4. the kernels' own expressions, restated in numpy fp32 in the kernels' operation order (``update_ref.k_*``), lie inside too, and
   the listed set they give passes the assertions the GPU test makes of ``ops.cvq_rows`` on the same nine settings.

It also measures the one known difference between the kernels and the reference's arithmetic (``1 - g`` formed in double and
then rounded, against the kernels' fp32 ``1.0f - g``) in units of the bound; profiles/update_parity.txt keeps the figures.
No GPU is involved; tests/test_gpu_updates.py holds the HIP kernels to the same ``compare`` and the same tolerances.
"""
import numpy as np
import pytest
import torch

import update_ref as ur
from oracle import c_oracle, ref_import

F64 = torch.float64
# largest |decay(double g) - decay(fp32 g)| over the CVQ-VAE case table in units of decay's bound: the figures DESIGN.md §4.5
# and profiles/update_parity.txt state (float64 on the CPU)
DOUBLE_G_RECORDED = {0.9: 0.418, 0.99: 1.742, 0.999: 24.17}


def _one_rank(inp):
    r = inp['ranks'][0]
    return r['x'], r['col']


def _three_ranks(inp):
    """The all-reduced payload of three ranks as the kernel receives it: fp32 sums of the anchors, counts and token counts."""
    s = (inp['ranks'][0]['x'][inp['ranks'][0]['col']] + inp['ranks'][1]['x'][inp['ranks'][1]['col']]) + inp['ranks'][2]['x'][inp['ranks'][2]['col']]
    hist = sum(r['hist32'].to(torch.int64) for r in inp['ranks'])
    return s, torch.arange(s.shape[0]), hist, sum(r['numel'] for r in inp['ranks'])


def _cvq_check(name, got, ref, tol, keys=('p', 'decay', 'w')):
    for k in keys:
        v = ur.compare(got[k], ref[k], tol[k])
        assert v.ok, v.line(f'{name} {k}')


@pytest.mark.parametrize('c', ur.CVQ_CASES, ids=lambda c: c.name)
def test_cvq_bound(c):
    inp = ur.cvq_inputs(c)
    for world in (1, 3):
        if world == 1:
            (x, col), hist, numel = _one_rank(inp), inp['hist'], inp['numel']
        else:
            x, col, hist, numel = _three_ranks(inp)
        for stage in (1, 2, 3):
            ref = ur.cvq_reference(inp['w'], inp['p'], hist, numel, x, col, c.g, c.eps, world, stage=stage)
            a_abs = x[col].double().abs() / world
            tol = ur.cvq_tolerance(inp['w'], inp['p'], hist, numel, a_abs, c.g, c.eps, stage=stage, c_anchor=int(world > 1))
            got = ur.cvq_reference(inp['w'], inp['p'], hist, numel, x, col, c.g, c.eps, world, dtype=torch.float32, stage=stage)
            _cvq_check(f'{c.name} world={world} stage={stage} ATen fp32', got, ref, tol)
        assert ur.not_vacuous(ref['w'], tol['w']) and ur.not_vacuous(ref['p'], tol['p']), c.name
    # the C oracle's elementwise formulas, from the fp32 p' of ATen
    x, col = _one_rank(inp)
    ref = ur.cvq_reference(inp['w'], inp['p'], inp['hist'], inp['numel'], x, col, c.g, c.eps, stage=2)
    tol = ur.cvq_tolerance(inp['w'], inp['p'], inp['hist'], inp['numel'], x[col].double().abs(), c.g, c.eps, stage=2)
    p0 = torch.nan_to_num(inp['p'], nan=0.0).numpy()
    decay = c_oracle.cvq_decay(p0, c.K, ur.f32(c.g), ur.f32(c.eps))
    v = ur.compare(torch.from_numpy(decay).reshape(-1), ref['decay'], tol['decay'])
    assert v.ok, v.line(f'{c.name} c_oracle.cvq_decay')
    w_new = c_oracle.ema(inp['w'].numpy(), x[col].numpy(), decay)
    v = ur.compare(torch.from_numpy(w_new), ref['w'], tol['w'])
    assert v.ok, v.line(f'{c.name} c_oracle.ema')


@pytest.mark.parametrize('c', ur.KD_CASES, ids=lambda c: c.name)
def test_vqkd_bound(c):
    inp = ur.kd_inputs(c)
    for mode in ('full', 'centroid'):
        ref = ur.kd_reference(inp['w'], inp['hist'], inp['sums'], c.g, mode)
        tol = ur.kd_tolerance(inp['w'], inp['hist'], inp['sums'], c.g, mode)
        v = ur.compare(ur.kd_reference(inp['w'], inp['hist'], inp['sums'], c.g, mode, dtype=torch.float32), ref, tol)
        print(v.line(f'{c.name} {mode}: ATen fp32'))
        assert v.ok, v.line(f'{c.name} {mode}')
        assert ur.not_vacuous(ref, tol), f'{c.name} {mode}'
    cent_ref = ur.kd_reference(inp['w'], inp['hist'], inp['sums'], c.g, 'centroid')
    cent_tol = ur.kd_tolerance(inp['w'], inp['hist'], inp['sums'], c.g, 'centroid')
    cent = c_oracle.kmeans_centroids(None, None, inp['w'].numpy(), hist=inp['hist'].numpy(), sums=inp['sums'].numpy())
    v = ur.compare(torch.from_numpy(cent), cent_ref, cent_tol)
    assert v.ok, v.line(f'{c.name} c_oracle.kmeans_centroids')


def test_every_mutation_lies_outside_somewhere():
    """Every mutation of the list is rejected by the bound on at least one case of the table (the table is walked here)."""
    seen_cvq, seen_kd = set(), set()
    for c in ur.CVQ_CASES:
        inp = ur.cvq_inputs(c)
        for world in (1, 3):
            if world == 1:
                (x, col), hist, numel = _one_rank(inp), inp['hist'], inp['numel']
            else:
                x, col, hist, numel = _three_ranks(inp)
            ref = ur.cvq_reference(inp['w'], inp['p'], hist, numel, x, col, c.g, c.eps, world)
            tol = ur.cvq_tolerance(inp['w'], inp['p'], hist, numel, x[col].double().abs() / world, c.g, c.eps, c_anchor=int(world > 1))
            for name, m in ur.cvq_mutations(c, inp, x, col, hist, numel, world).items():
                if not (ur.compare(m['p'], ref['p'], tol['p']).ok and ur.compare(m['w'], ref['w'], tol['w']).ok):
                    seen_cvq.add(name)
    for c in ur.KD_CASES:
        inp = ur.kd_inputs(c)
        ref = ur.kd_reference(inp['w'], inp['hist'], inp['sums'], c.g)
        tol = ur.kd_tolerance(inp['w'], inp['hist'], inp['sums'], c.g)
        for name, m in ur.kd_mutations(c, inp).items():
            if not ur.compare(m, ref, tol).ok:
                seen_kd.add(name)
    assert seen_cvq == ur.CVQ_MUTATIONS, ur.CVQ_MUTATIONS - seen_cvq
    assert seen_kd == ur.KD_MUTATIONS, ur.KD_MUTATIONS - seen_kd


def test_header_round_trip_and_listed_predicate():
    hist = torch.tensor([0, 1, 65535, 65536, ur.BIG_A, ur.BIG_B], dtype=torch.int64)
    numel = 2 ** 41 + 5
    back = ur.unpack_header(ur.pack_header(hist, numel), 6)
    assert torch.equal(back[:6], hist) and int(back[6]) == numel
    three = ur.pack_header(hist[:4], 70000) * 3                             # three equal ranks summed: still exact
    assert torch.equal(ur.unpack_header(three, 4), torch.cat([hist[:4] * 3, torch.tensor([210000])]))
    K, g, eps = 1000, 0.9, 0.5
    ps = ur.threshold_p(K, g, eps)
    p = torch.tensor([0.0, ps * 0.5, ps * 2, 1.0, float('nan'), -1.0], dtype=torch.float32)
    assert ur.listed(p, K, g, eps).tolist() == [True, True, False, False, True, True]
    assert ur.c_exponent(0.25) == 5 and ur.c_exponent(0.5) == 4 and ur.tree(63) == 7


needs_reference = pytest.mark.skipif(not ref_import.available(), reason='the reference checkout is not present on this machine')


@needs_reference
@pytest.mark.parametrize('g,eps', [(0.9, 1e-2), (0.5, 0.0)])
@pytest.mark.parametrize('dist', ['L2', 'Cosine'])
def test_reference_cvq_callback_lies_inside(g, eps, dist):
    """The reference's own CVQVAECallback.after_encode (two training steps of its module) against the float64 reference of each
    step, evaluated from the module's own tokens and column indices.  The hyperparameters are given at their fp32 values."""
    from oracle import make_golden as mg, synth
    N, K, D = 700, 130, 24
    x, w = synth.make_inputs('normal', 77, N, K, D)
    cb = [dict(type='CVQVAECallback', ema=dict(decay=ur.f32(g)), eps=ur.f32(eps), anchor=dict(type='NearestAnchor', sync=False))]
    q = mg.ref_quantizer(K, D, dist, 'vqgan', cb, w, train=True)
    xt = torch.from_numpy(x)
    w_old, p_old = torch.from_numpy(w).clone(), torch.zeros(K)
    for step in range(2):
        with torch.no_grad():
            _, _, memo = q(xt, {})
        col = memo['encode']['distance'].argmin(0)
        hist = torch.bincount(memo['quant'].reshape(-1), minlength=K)
        ref = ur.cvq_reference(w_old, p_old, hist, N, xt, col, g, eps)
        tol = ur.cvq_tolerance(w_old, p_old, hist, N, xt[col].double().abs(), g, eps)
        got = dict(p=q.get_buffer('_probability').clone(), w=q.embedding.weight.detach().clone())
        _cvq_check(f'reference CVQVAECallback {dist} g={g} eps={eps} step {step}', got, ref, tol, keys=('p', 'w'))
        w_old, p_old = got['w'], got['p']


@needs_reference
@pytest.mark.parametrize('g', [0.9, 0.5])
def test_reference_vqkd_callback_lies_inside(g):
    """The reference's own VQKDCallback.after_encode, called on normalised rows with the module's own tokens; the centroid sums
    are the float64 sums of those rows, and the tolerance carries the m - 1 fp32 additions of the reference's scatter-add."""
    from oracle import make_golden as mg, synth
    import torch.nn.functional as F
    N, K, D = 700, 130, 24
    x, w = synth.make_inputs('normal', 78, N, K, D)
    w = synth.unit_rows(w)
    q = mg.ref_quantizer(K, D, 'Cosine', 'commitment_norm', [dict(type='VQKDCallback', ema=dict(decay=ur.f32(g)))], w, train=True)
    xn = F.normalize(torch.from_numpy(x))
    quant = torch.from_numpy(synth.rng(5).integers(0, K // 2, N))
    with torch.no_grad():
        q._callbacks.after_encode(xn, quant, {})                            # (the composed callback hands it to VQKDCallback)
    hist = torch.bincount(quant, minlength=K)
    x2 = F.normalize(xn.double())
    sums = torch.zeros(K, D, dtype=F64).index_add_(0, quant, x2)
    a_sums = torch.zeros(K, D, dtype=F64).index_add_(0, quant, x2.abs())
    tol_sums = (hist.double().reshape(-1, 1) + ur.tree(D) / 2 + 2) * ur.U * a_sums
    w_old = torch.from_numpy(w)
    ref = ur.kd_reference(w_old, hist, sums, g)
    tol = ur.kd_tolerance(w_old, hist, sums, g, tol_sums=tol_sums)
    v = ur.compare(q.embedding.weight.detach(), ref, tol)
    assert v.ok, v.line(f'reference VQKDCallback g={g}')


def test_double_g_difference_is_measured():
    """Gap between 1 - g formed in double and rounded (the reference, oracle.c_oracle.cvq_decay) and the kernels' fp32
    ``1.0f - g``, in units of decay's bound: printed, and held to the figures the documents state.  Not folded into any count."""
    for g in (0.9, 0.99, 0.999):
        f = ur.double_g_figure(g)
        print(f"double-g g={g}: denominators differ by {f['denominators_differ_by_u']:.3g} u; "
              f"largest |decay(double g) - decay(fp32 g)| = {f['ratio']:.4g} x bound at {f['case']} (CPU, float64; not a device run)")
        assert f['ratio'] == pytest.approx(DOUBLE_G_RECORDED[g], rel=2e-3), 'the recorded figure (DESIGN.md, profiles) has drifted'


# ------------------------------------------------------------------------------------------------------------------
# the kernels' expressions restated in numpy fp32 (update_ref.k_*): inside the bounds, and the listed set's assertions
# ------------------------------------------------------------------------------------------------------------------

def test_fp32_restatement_of_the_kernels_lies_inside():
    """The kernels' own operation order in fp32 (not ATen's) under the same bounds, on every case; prints the worst err/tol per
    form (CPU figures of profiles/update_parity.txt; the device's come from tests/test_gpu_updates.py)."""
    worst = {}

    def note(form, name, got, ref, tol):
        v = ur.compare(got, ref, tol)
        assert v.ok, v.line(f'{form} {name}')
        if v.worst >= worst.get(form, (0.0, ''))[0]:
            worst[form] = (v.worst, name)
    for c in ur.CVQ_CASES:
        inp = ur.cvq_inputs(c)
        p0 = torch.nan_to_num(inp['p'], nan=0.0)
        for world in (1, 3):
            if world == 1:
                (x, col), hist, numel = _one_rank(inp), inp['hist'], inp['numel']
            else:
                x, col, hist, numel = _three_ranks(inp)
            ref = ur.cvq_reference(inp['w'], inp['p'], hist, numel, x, col, c.g, c.eps, world)
            tol = ur.cvq_tolerance(inp['w'], inp['p'], hist, numel, x[col].double().abs() / world, c.g, c.eps, c_anchor=int(world > 1))
            got = ur.k_cvq(inp['w'], p0, hist, numel, x[col], c.g, c.eps, world)
            for k in ('p', 'decay', 'w'):
                note(f'cvq world={world} {k}', c.name, got[k], ref[k], tol[k])
    for c in ur.KD_CASES:
        inp = ur.kd_inputs(c)
        for mode in ('full', 'centroid'):
            note(f'vqkd {mode}', c.name, ur.k_vqkd(inp['w'], inp['hist'], inp['sums'], c.g, mode),
                 ur.kd_reference(inp['w'], inp['hist'], inp['sums'], c.g, mode), ur.kd_tolerance(inp['w'], inp['hist'], inp['sums'], c.g, mode))
    for form, (v, name) in worst.items():
        print(f'fp32 restatement {form}: worst err/tol={v:.4g} at {name} (CPU; not a device run)')


@pytest.mark.parametrize('K,g,eps', ur.ROWS_SETTINGS)
def test_fp32_restatement_of_the_listed_set(K, g, eps):
    """cvq_may_need_anchor restated in numpy fp32 on the probabilities the GPU test uses, through the same assertions: soundness
    for freq in {0, 1/N, 1} with the restated p' and decay, band-limited agreement with the float64 predicate, the margin."""
    p = ur.rows_p(K, g, eps)
    is_listed = torch.from_numpy(ur.k_listed(p.numpy(), K, g, eps))
    p_freq0 = None
    for h in (0, 1, ur.ROWS_N):
        p2 = ur.k_pnew(p.numpy(), np.full(K, h, np.int64), ur.ROWS_N, g)
        decay = torch.from_numpy(ur.k_decay(p2, K, g, eps))
        assert bool((decay[~is_listed] == 1.0).all()), f'hist={h}: an unlisted code has decay != 1'
        if h == 0:
            p_freq0 = torch.from_numpy(p2)
    print(ur.check_listed_set(p, K, g, eps, is_listed, p_freq0) + ' (CPU restatement; not a device run)')
