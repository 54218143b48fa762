"""The bounds of tests/forward_ref.py, proven on the CPU for every row of the case table the GPU tests use:

1. an fp32 restatement of the tail stays inside: the C oracle's ``gather_ste`` / ``mse`` / ``vqgan_loss`` where they apply (the
   plain tails), and the ``oracle.torch_ref`` composition in float32 with the kernel's summation grouping (every case); the
   decoded rows and the straight-through output of the C oracle are the bits ``forward_ref.exact_outputs`` asks the kernels for;
2. the bound has teeth: every mutation that applies to a case (the last row dropped or counted twice, the elements past
   4 (D // 4) dropped, the last 16-row block dropped, the divisor (N - 1) D, and from N D = 2^22 on a sequential fp32 running
   sum) lies outside it.

No GPU is involved; tests/test_gpu_forward.py holds the HIP kernels to the same bounds through the same ``compare``.
"""
import numpy as np
import pytest
import torch

import forward_ref as fr
from oracle import c_oracle as co

def _bound(c, inp, ref):
    if c.tail == 'normalised':
        return fr.normalised_bound(inp['x'], inp['w'], inp['idx'], ref)
    return fr.loss_bound(ref, fr.c_plain(c.D), c.N * c.D, fp32_out=(c.tail == 'plain_mse'))


@pytest.mark.parametrize('c', fr.ALL_CASES, ids=lambda c: c.name)
def test_forward_bound(c):
    inp = fr.inputs(c)
    x, w, idx = inp['x'], inp['w'], inp['idx']
    vals = fr.reference(x, w, idx, c.tail, c.beta)
    ref = vals['commitment']
    tol = _bound(c, inp, ref)
    if c.tail != 'normalised':
        assert vals['codebook'] == ref                              # one value, two graph nodes
    if c.tok == 'exact':
        assert ref == 0.0 and tol == 0.0
    else:
        assert ref > 0.0 and np.float32((c.scale * 8.0) ** 2) < np.finfo(np.float32).max     # squares stay normal fp32 numbers
    # 1. fp32 restatements
    got = fr.restate_fp32(x, w, idx, c.tail)
    if c.tail != 'plain':
        got = float(np.float32(got))                                # the kernels of these kinds return the mean as fp32
    v = fr.check(got, ref, tol)
    print('\n' + v.line(f'{c.name}: fp32 restatement'), end='')
    assert v.ok, v.line(c.name)
    if c.tail != 'normalised':
        x32 = x.float().numpy()
        z_o, zs_o = co.gather_ste(x32, w.numpy(), idx.numpy())
        z_e, zs_e = fr.exact_outputs(x, w, idx)
        assert np.array_equal(z_o, z_e.numpy()) and np.array_equal(zs_o, zs_e.numpy())
        if c.tok == 'exact':
            assert np.array_equal(zs_o.view(np.uint32), x32.view(np.uint32))       # the bits of x
        if c.tail == 'plain_mse':
            m = co.mse(z_o, x32)
            v = fr.check(float(m), ref, tol)
            print('\n' + v.line(f'{c.name}: C oracle'), end='')
            assert v.ok, v.line(c.name)
            assert co.vqgan_loss(z_o, x32, c.beta) == fr.combine_fp32(m, c.beta)
            vc = fr.check(float(fr.combine_fp32(m, c.beta)), vals['vqgan'], fr.combined_bound(ref, tol, c.beta))
            assert vc.ok, vc.line(f'{c.name}: combined')
    # 2. mutations
    if c.tok == 'exact':
        return
    muts = fr.mutations(x, w, idx, c.tail)
    assert set(muts) == {name for name in fr.MUTATIONS if fr.applies(name, c)}
    for name, wrong in muts.items():
        m = fr.check(wrong, ref, tol)
        print(f'\n{c.name} [{name}]: err/tol={m.worst:.4g}', end='')
        if fr.must_reject(name, c.N, c.D):
            assert not m.ok, f'{c.name} [{name}]: inside the bound (err/tol {m.worst:.3g})'


def test_counts_and_helpers_are_the_documented_ones():
    assert fr.c_plain(256) == 5 and fr.c_plain(30) == 3 and fr.a_normalize(32) == 5.5 and fr.a_normalize(768) == 11.0
    assert fr.half_ulp_fp32(1.0) == 2.0 ** -24 and fr.half_ulp_fp32(1.5) == 2.0 ** -24 and fr.half_ulp_fp32(0.75) == 2.0 ** -25
    assert fr.half_ulp_fp32(0.0) == 0.0 and fr.half_ulp_fp32(2.0 ** -140) == 2.0 ** -150
    assert fr.combine_fp32(np.float32(0.1), 0.25) == np.float32(np.float32(0.1) + np.float32(0.25) * np.float32(0.1))
    out_bytes = fr.STREAM_N * fr.STREAM_D * 4
    assert out_bytes <= (192 << 20) < 2 * out_bytes and fr.STREAM_N % 16 == 1        # one output stays below the threshold, two pass it
    for n in (1, 15, 17, 4097, 8193):
        for d in (3, 4, 30, 252, 256, 260, 1030):
            for dt in ('f32', 'bf16'):
                assert any(c.N == n and c.dtype == dt for c in fr.TAIL_CASES) and any(c.D == d and c.dtype == dt for c in fr.TAIL_CASES)
    assert {c.scale for c in fr.TAIL_CASES} == {1e-3, 1.0, 1e3} and {c.tok for c in fr.TAIL_CASES} == {'uniform', 'same', 'exact'}


def test_every_mutation_is_required_of_some_case():
    """From the table alone: every mutation applies to, and must be rejected at, some case (test_forward_bound asserts the rejection
    itself, case by case), and the normalised cases are the whole D x N product."""
    required = {name for c in fr.ALL_CASES for name in fr.MUTATIONS if fr.applies(name, c) and fr.must_reject(name, c.N, c.D)}
    assert required == set(fr.MUTATIONS), set(fr.MUTATIONS) - required
    assert {(c.N, c.D) for c in fr.NORM_CASES} == {(n, d) for n in (63, 3000, 32769) for d in (8, 16, 24, 32, 64, 768)}
    assert any(c.N % 16 == 15 and c.N > 4096 for c in fr.TAIL_CASES)             # a last block that is not the last row alone
