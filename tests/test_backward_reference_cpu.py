"""The bounds of tests/backward_ref.py, proven on the CPU for every row of the case table the GPU tests use:

1. the reference alone stays inside: the same ``oracle.torch_ref`` composition evaluated in fp32 differs from the float64 one
   by at most the derived tolerance, no element excluded;
2. the bound has teeth: every deliberately wrong float64 restatement that applies to a case (loss term x 1.01, beta 0.26,
   2/(N (D+1)), a token left out of grad_W, two swapped channels, an unclamped zero row, g_xn dropped) lies outside it on at
   least one element, and ``compare`` says so.

No GPU is involved; tests/test_gpu_backward.py holds the HIP kernels to the same ``compare`` and the same tolerances.
"""
import pytest
import torch

import backward_ref as br

ALL_MUTATIONS = {'loss_term_x1.01', 'beta_0.26', 'nd_plus_one', 'dropped_token_last', 'dropped_token_8192',
                 'swapped_channels', 'unclamped_zero_row', 'unclamped_tiny_row', 'g_xn_dropped'}
SEEN = set()


def _mask(c, gx, gw):
    """What the case asks the kernel for."""
    return (gx if c.need_x else None), (gw if c.need_w else None)


def _check_pair(name, got, ref, tol, expect_ok):
    worst = 0.0
    any_bad = False
    for part, g, r, t in zip(('grad_x', 'grad_w'), got, ref, tol):
        if r is None:
            continue
        v = br.compare(g, r, t)
        worst = max(worst, v.worst)
        any_bad |= not v.ok
        if expect_ok:
            assert v.ok, v.line(f'{name} {part}')
    if not expect_ok:
        assert any_bad, f'{name}: the mutation is inside the bound (worst err/tol {worst:.3g})'
    return worst


@pytest.mark.parametrize('c', br.VQ_CASES + br.MAP_CASES + br.NORM_CASES, ids=lambda c: c.name)
def test_vq_tail_bound(c):
    inp = br.vq_inputs(c)
    gx, gw = br.vq_value(c, inp)
    tx, tw = br.vq_tolerance(c, inp)
    gx32, gw32 = br.vq_value(c, inp, dtype=torch.float32)
    if c.form == 'map':
        tol = (br.map_tolerance(c, gx, tx), None)
        conv = lambda t: br.to_map(t, c)
        got32 = br.to_map(gx32, c)
        if c.out_dtype == 'bf16':
            got32 = got32.bfloat16()
        w = _check_pair(c.name, (got32, None), (conv(gx), None), tol, True)
        muts = {k: ((br.round_bf16(conv(v[0])) if c.out_dtype == 'bf16' else conv(v[0])), None)
                for k, v in br.vq_mutations(c, inp, gx, gw).items()}
        ref = (conv(gx), None)
    else:
        ref, tol = _mask(c, gx, gw), (tx, tw)
        w = _check_pair(c.name, (gx32, gw32), ref, tol, True)
        muts = br.vq_mutations(c, inp, gx, gw)
    print(f'{c.name}: fp32 reference err/tol={w:.3g}')
    for name, got in muts.items():
        _check_pair(f'{c.name} [{name}]', got, ref, tol, False)
        SEEN.add('dropped_token_last' if name == f'dropped_token_{c.N - 1}' else name)
    # kw == 0: the reference's grad_W is exactly zero, and so is its tolerance (the kernel must return exact zeros)
    if c.form == 'tok' and c.scal[0] is None and c.scal[2] is None:
        assert not gw.any() and not tw.any()
    # the planted outliers are what makes a dropped token visible under the worst-case grad_W bound
    if c.form == 'tok' and c.need_w and br.kw_signed(c) != 0:
        assert any(k.startswith('dropped_token') for k in muts)


@pytest.mark.parametrize('c', br.KD_CASES, ids=lambda c: c.name)
def test_vqkd_tail_bound(c):
    inp = br.kd_inputs(c)
    gx = br.kd_value(c, inp)
    tol = br.kd_tolerance(c, inp)
    v = br.compare(br.kd_value(c, inp, dtype=torch.float32), gx, tol)
    print(v.line(f'{c.name}: fp32 reference'))
    assert v.ok, v.line(c.name)
    for name, got in br.kd_mutations(c, inp, gx).items():
        m = br.compare(got, gx, tol)
        assert not m.ok, f'{c.name} [{name}]: inside the bound ({m.worst:.3g})'
        SEEN.add(name)


@pytest.mark.parametrize('c', br.NB_CASES, ids=lambda c: c.name)
def test_normalize_backward_bound(c):
    inp = br.nb_inputs(c)
    gv = br.nb_value(inp)
    tol = br.nb_tolerance(c, inp)
    v = br.compare(br.nb_value(inp, dtype=torch.float32), gv, tol)
    print(v.line(f'{c.name}: fp32 reference'))
    assert v.ok, v.line(c.name)
    for name, got in br.nb_mutations(c, inp, gv).items():
        m = br.compare(got, gv, tol)
        assert not m.ok, f'{c.name} [{name}]: inside the bound ({m.worst:.3g})'
        SEEN.add(name)


@pytest.mark.parametrize('c', br.EL_CASES, ids=lambda c: c.name)
def test_elementwise_bounds(c):
    inp = br.el_inputs(c)
    ref, tol, f32 = br.el_values(inp), br.el_tolerances(c, inp), br.el_values(inp, dtype=torch.float32)
    for k in ('diff', 'sse', 'ste'):
        v = br.compare(f32[k], ref[k], tol[k])
        assert v.ok, v.line(f'{c.name} {k}')
        # teeth: a scale wrong by 1e-5 (diff), one element left out of the sum, the straight-through value taken from x
    assert not br.compare(ref['diff'] * (1 + 1e-5), ref['diff'], tol['diff']).ok
    d2 = (inp['a'].double() - inp['b'].double()) ** 2
    assert not br.compare(ref['sse'] - d2.max(), ref['sse'], tol['sse']).ok
    assert not br.compare(inp['a'].double(), ref['ste'], tol['ste']).ok


def test_compare_reports_position_nan_and_floor():
    ref = torch.zeros(3, 4, dtype=torch.float64)
    tol = torch.zeros(3, 4, dtype=torch.float64)
    got = ref.clone()
    assert br.compare(got, ref, tol).ok                                     # exact zeros against a zero tolerance
    got[1, 2] = 1e-30
    v = br.compare(got, ref, tol)
    assert not v.ok and v.pos == (1, 2) and v.bad == 1
    got[1, 2] = 2.0 ** -127
    v = br.compare(got, ref, tol)
    assert v.ok and v.floor_needed                                          # below the smallest normal fp32: the floor
    got[2, 3] = float('nan')
    v = br.compare(got, ref, tol + 1.0)
    assert not v.ok and v.pos == (2, 3) and v.worst == float('inf')


def test_rounding_counts_are_the_documented_ones():
    assert br.tree(1) == 7 and br.tree(64) == 7 and br.tree(65) == 8 and br.tree(1030) == 23
    assert br.C_GRAD_X == 8 and br.c_normalize_bwd(64) == 26.5
    assert br.vqkd_count(32) == 101.0 and br.vq_norm_count(8) == 41.0


def test_every_mutation_was_seen_somewhere():
    """Runs last in this file: every mutation of the issue's list applied to (and was rejected for) at least one case."""
    if len(SEEN) == 0:
        return                                                              # the case tests were deselected
    assert SEEN == ALL_MUTATIONS, ALL_MUTATIONS - SEEN
