"""The networks, the discriminator and the GAN losses against the reference's OWN modules (CPU).

tests/golden/networks/*.npz are written by oracle/make_network_golden.py from the reference's source files behind
``ref_import.load_networks()``: float64 outputs, input gradients, parameter gradients and running statistics of seeded modules
(tests/network_cases.py).  Here

(a) with the reference checkout present, every fixture is regenerated and compared byte by byte (which also re-runs the recipe's
    check of this package's ``init_weights``), and the loaded classes are the reference's files;
(b) this package's modules with ``fused=False``, float64, CPU, the same seeded state dict loaded with ``strict=True``: within 1e-10
    relative of the fixture - the two sides differ in the summation order of the same ATen ops only;
(c) the same in fp32, within ``4 * max(fp32_self, 2**-23)`` per tensor, ``fp32_self`` being the reference's own fp32 run against
    its float64 run;
(d) ``init_weights`` after the same ``torch.manual_seed``: mean and standard deviation of every parameter equal to the bit (every
    parameter of the three modules is drawn by the same ATen initialiser in the same order; ``VQGANEncoder`` / ``VQGANDecoder`` have
    no ``init_weights`` on either side);
(e) the four GAN losses in float64, ``R1GradientPenalty`` with its gradient to every parameter and the modes it restores.
"""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

import vector_quantization_amd as vqa
from oracle import ref_import

import network_cases as nc

needs_reference = pytest.mark.skipif(not ref_import.available(), reason='the reference checkout is not present on this machine')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'networks')
F64_TOL = 1e-10
EPS32 = 2.0 ** -23


def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return z, json.loads(str(z['spec']))


def test_fixtures_hold_the_cases_of_this_tree():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, '*.npz')))
    assert names == sorted(list(nc.CASES) + ['init_' + n for n in nc.INIT_CASES] + ['gan_losses'])
    for name, case in nc.CASES.items():
        z, spec = fixture(name)
        assert spec['cls'] == case['cls'] and spec['kwargs'] == json.loads(json.dumps(case['kwargs']))
        assert spec['input'] == list(case['input']) and spec['seed'] == case['seed'] and spec['train'] == case['train']
        assert sorted(spec['names'] + ['fp32_self', 'spec']) == sorted(z.files) and len(z['fp32_self']) == len(spec['names'])
        assert 8 * len(spec['zero']) <= len(spec['names'])
        assert spec['source'] == 'reference-import' and spec['reference']
        assert all(z[n].dtype == np.float64 for n in spec['names'])
    for p in glob.glob(os.path.join(GOLDEN, '*.npz')):
        assert os.path.getsize(p) < 330_000, p                 # below the largest fixture committed before these


@needs_reference
def test_loaded_classes_are_the_reference_files():
    ref = ref_import.load_networks()
    want = {'vq/models/autoencoders.py', 'vq/algorithms/vqgan/autoencoder.py', 'vq/algorithms/vqkd/autoencoder.py',
            'vq/algorithms/vqgan/discriminators/base.py', 'vq/algorithms/vqgan/discriminators/patchgan.py',
            'vq/algorithms/vqgan/losses/registries.py', 'vq/algorithms/vqgan/losses/generator.py',
            'vq/algorithms/vqgan/losses/discriminator.py'}
    assert want <= set(ref.files.values())
    for name in ('VQGANEncoder', 'VQGANDecoder', 'VQKDEncoder', 'VQKDDecoder', 'PatchGANDiscriminator', 'VQGANGeneratorLoss',
                 'NonSaturatingLoss', 'VQGANDiscriminatorLoss', 'R1GradientPenalty'):
        cls = getattr(ref, name)
        for base in cls.__mro__:
            if base.__module__.startswith('vq.'):
                assert sys.modules[base.__module__].__file__.startswith(ref_import.REFERENCE_ROOT), (name, base)
    assert ref.VQGANEncoder is not vqa.VQGANEncoder


@needs_reference
def test_committed_fixtures_are_the_reference_outputs(tmp_path):
    """(a): regenerated in a fresh process under make_golden.PINNED_ENV, key by key, byte by byte."""
    import subprocess
    from oracle import make_golden
    if not make_golden.host_has_avx512():
        pytest.skip('the fixtures were written with AVX-512 kernels; this processor has no AVX-512')
    root = os.path.dirname(os.path.dirname(os.path.dirname(GOLDEN)))
    res = subprocess.run([sys.executable, '-c', 'import sys; from oracle import make_network_golden as m; m.main(out_dir=sys.argv[1], quiet=True)',
                          str(tmp_path)], env=make_golden.pinned_env(), cwd=root, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    fresh = sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(tmp_path), '*.npz')))
    committed = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, '*.npz')))
    assert fresh == committed
    for name in fresh:
        a, b = np.load(os.path.join(str(tmp_path), name)), np.load(os.path.join(GOLDEN, name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            if k == 'spec':
                assert json.loads(str(a[k])) == json.loads(str(b[k])), name
            else:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f'{name}:{k} drifted from the reference'


def ours(case, dtype):
    module = getattr(vqa, case['cls'])(**case['kwargs'], fused=False)
    res = nc.run_case(module, case, dtype=dtype)
    assert module.last_route.name == 'torch'
    return res


def compare(name, res, tol_of):
    z, spec = fixture(name)
    assert list(res) == spec['names'], 'the state dict or the outputs are not the reference\'s'
    worst = []
    for i, n in enumerate(spec['names']):
        if n in spec['zero']:
            continue
        got, want = nc.stored(n, res[n], spec['seed']), z[n]
        assert got.shape == want.shape, n
        err, tol = nc.rel_err(got, want), tol_of(float(z['fp32_self'][i]))
        worst.append((err / tol, n, err, tol))
    bad = [w for w in worst if not w[0] <= 1]
    assert not bad, f'{name}: ' + '; '.join(f'{n} err {e:.3e} > tol {t:.3e}' for _, n, e, t in sorted(bad, reverse=True)[:6])
    return max(worst)


@pytest.mark.parametrize('name', list(nc.CASES))
def test_float64_cpu_equals_the_reference(name):
    """(b)"""
    compare(name, ours(nc.CASES[name], torch.float64), lambda self_err: F64_TOL)


@pytest.mark.parametrize('name', list(nc.CASES))
def test_fp32_cpu_is_as_close_as_the_reference_is_to_itself(name):
    """(c)"""
    compare(name, ours(nc.CASES[name], torch.float32), lambda self_err: 4 * max(self_err, EPS32))


@pytest.mark.parametrize('name', list(nc.INIT_CASES))
def test_init_weights_draws_what_the_reference_draws(name):
    """(d)"""
    case = nc.INIT_CASES[name]
    z, spec = fixture('init_' + name)
    torch.manual_seed(case['seeds'][0])
    module = getattr(vqa, case['cls'])(**case['kwargs'])
    stats = nc.init_statistics(module, case['seeds'], vqa.Config())
    assert list(stats) == spec['names'] and spec['seeds'] == list(case['seeds'])
    for n, v in stats.items():
        assert v.tobytes() == z['stat/' + n].tobytes(), f'{n}: (mean, std) {v}, the reference {z["stat/" + n]}'
    if case['cls'] != 'PatchGANDiscriminator':                    # the per-depth rescale is in the numbers: block i against block 0
        std = {i: z[f'stat/blocks.{i}.attn.proj.weight'][1] for i in range(case['kwargs']['depth'])}
        assert std[1] / std[0] == pytest.approx(2 ** -0.5, rel=0.05)


def test_gan_losses_equal_the_reference():
    """(e)"""
    z, spec = fixture('gan_losses')
    assert spec['settings'] == list(nc.LOSS_SETTINGS) and spec['shapes'] == [list(s) for s in nc.LOSS_SHAPES]
    classes = {n: getattr(vqa, n) for n in nc.LOSS_CLASSES + ('R1GradientPenalty',)}
    classes['PatchGANDiscriminator'] = lambda **kw: vqa.PatchGANDiscriminator(**kw, fused=False)
    res = nc.run_losses(classes)
    assert list(res) == spec['names']
    assert res['r1/modes_restored'].item() == 1.0
    for n in spec['names']:
        got, want = nc.stored(n, res[n], nc.R1_CASE['seed']), z[n]
        assert got.shape == want.shape, n
        if n.startswith('r1/buffer/') or not np.abs(want).max() > 0:
            assert np.array_equal(got, want), n
        else:
            assert nc.rel_err(got, want) <= F64_TOL, (n, nc.rel_err(got, want))
