"""tests/entropy_ref.py proven on the CPU (no GPU involved):

1. the chunked float64 evaluator of the closed form equals float64 autograd of ``oracle.torch_ref.entropy_loss`` on every small
   case (to a thousandth of the fp32 bound), whatever the chunk size;
2. ATen's fp32 evaluation of the reference's composition stays inside the derived bounds, no element excluded;
3. the bounds have teeth: every mutation of ``entropy_ref.MUTATIONS`` lies outside them on at least one case;
4. tests/golden/entropy/*.npz regenerate byte for byte from the reference's own EntropyLoss where the reference is present.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import entropy_ref as er
from oracle import make_golden, ref_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'entropy')
TOOL = os.path.join(ROOT, 'tools', 'make_golden_entropy.py')


@pytest.mark.parametrize('c', er.SMALL_CASES, ids=lambda c: c.name)
def test_evaluator_is_the_reference_and_fp32_stays_inside(c):
    inp = er.inputs(c)
    ref = er.evaluate(c, inp)
    auto = er.autograd_reference(c, inp)
    for name, v in er.verdicts(auto, ref, scale=1e-3).items():
        print(v.line(f'{c.name} float64 autograd vs evaluator {name} (1e-3 of the bound)'))
        assert v.ok, v.line(f'{c.name} {name}')
    small = er.evaluate(c, inp, tol=False, chunk=7)
    for k in ('loss', 'grad_x', 'grad_w'):
        assert torch.allclose(small[k], ref[k], rtol=1e-12, atol=1e-300 + 1e-13 * float(ref[k].abs().max())), k
    aten = er.autograd_reference(c, inp, dtype=torch.float32)
    if c.dtype == 'bf16':
        aten['grad_x'] = aten['grad_x'].bfloat16()
    for name, v in er.verdicts(aten, ref).items():
        print(v.line(f'{c.name} ATen fp32 {name}'))
        assert v.ok, v.line(f'{c.name} ATen fp32 {name}')


def test_every_mutation_falls_outside_on_some_case():
    """Over ALL small cases, computed here (no state shared with another test): each deliberately wrong restatement lies
    outside the bound of loss, grad_x or grad_w on at least one case."""
    caught = {m: False for m in er.MUTATIONS}
    for c in er.SMALL_CASES:
        inp = er.inputs(c)
        ref = er.evaluate(c, inp)
        for m in er.mutations_for(c, inp):
            mut = er.evaluate(c, inp, tol=False, mutation=m)
            if c.dtype == 'bf16':
                mut['grad_x'] = mut['grad_x'].float().bfloat16()
            vs = er.verdicts(mut, ref)
            print(f'{c.name} mutation {m}: worst err/tol {max(v.worst for v in vs.values()):.4g}')
            caught[m] = caught[m] or any(not v.ok for v in vs.values())
    inside = sorted(m for m, hit in caught.items() if not hit)
    assert not inside, f'mutations inside the bound on every case: {inside}'


def test_case_tables_cover_the_grid():
    cs = er.GPU_CASES
    assert {1, 127, 1000, 8193} <= {c.N for c in cs} and {1, 64, 1000, 4096} <= {c.K for c in cs}
    assert {8, 30, 32, 256, 768, 1030} <= {c.D for c in cs} and {0.5, 0.01, -1.0} <= {c.T for c in cs}
    assert {(c.metric, c.dtype) for c in cs} == {(m, d) for m in ('L2', 'Cosine') for d in ('f32', 'bf16')}
    assert any(c.block_rows and c.N % c.block_rows for c in cs) and any(c.block_rows == c.N for c in cs)
    assert any(c.plant == 'equal' for c in cs) and any(c.plant == 'zero' and c.metric == 'Cosine' for c in cs)
    assert len({c.name for c in cs}) == len(cs)


@pytest.mark.skipif(not ref_import.available(), reason='the reference checkout is not present on this machine')
def test_entropy_fixtures_are_the_reference_outputs(tmp_path):
    if not make_golden.host_has_avx512():
        pytest.skip('the fixtures were written with AVX-512 kernels; this processor has no AVX-512')
    res = subprocess.run([sys.executable, TOOL, str(tmp_path)], env=make_golden.pinned_env(), cwd=ROOT, capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    fresh = sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(tmp_path), '*.npz')))
    committed = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, '*.npz')))
    assert fresh == committed and len(committed) >= 4
    for name in fresh:
        a, b = np.load(os.path.join(str(tmp_path), name)), np.load(os.path.join(GOLD, name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            if k == 'spec':
                sa, sb = json.loads(str(a[k])), json.loads(str(b[k]))
                assert sb['source'] == 'reference-import' and sb['reference'], name
                sa.pop('torch', None), sb.pop('torch', None)
                assert sa == sb, name
            else:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f'{name}:{k} drifted from the reference'
