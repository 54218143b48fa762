"""The recipe of tests/golden/networks/*.npz (TEST INFRASTRUCTURE - needs the reference checkout).

    python -m oracle.make_network_golden            # rewrites tests/golden/networks/

Every file comes from the reference's OWN modules (``ref_import.load_networks()``): ``VQGANEncoder`` / ``VQGANDecoder``,
``VQKDEncoder`` / ``VQKDDecoder``, ``PatchGANDiscriminator`` and the four GAN losses, run by ``tests/network_cases.py`` (the cases,
the seeded state dict, the seeded input and the scalar ``sum(out * g)``), the same code the tests then run on this package's
modules.  A fixture holds data only: the kwargs, seeds and shapes (``spec``), the reference's float64 output, input gradient,
parameter gradients (``network_cases.stored``: all of a tensor of at most 512 elements, 512 seeded positions of a larger one) and
running statistics, ``fp32_self`` (per tensor ``max|fp32 - f64| / max|f64|`` of the reference's own fp32 CPU run against its float64
run, over the stored elements), and ``zero``: the names of the parameter gradients that are zero in exact arithmetic, found from
the reference alone (float64 maximum below 1e-9 of the case's largest parameter-gradient maximum).  No weights, no program text.

``init_<module>.npz`` holds the mean and standard deviation of every parameter after the reference's ``init_weights``;
``gan_losses.npz`` the values and gradients of the losses.  The process runs under ``make_golden.PINNED_ENV``, as every fixture does.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from . import make_golden, ref_import

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import network_cases as nc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'networks')
MAX_BYTES = 330_000                      # below the largest fixture committed before these (tests/golden/update_8rank.npz)
ZERO_BELOW = 1e-9

CITE = {
    'VQGANEncoder': ['vq/algorithms/vqgan/autoencoder.py:18-276', 'vq/models/autoencoders.py:14-27'],
    'VQGANDecoder': ['vq/algorithms/vqgan/autoencoder.py:18-248,279-304', 'vq/models/autoencoders.py:30-47'],
    'VQKDEncoder': ['vq/algorithms/vqkd/autoencoder.py:23-314', 'vq/models/autoencoders.py:14-27'],
    'VQKDDecoder': ['vq/algorithms/vqkd/autoencoder.py:23-268,317-367', 'vq/models/autoencoders.py:30-47'],
    'PatchGANDiscriminator': ['vq/algorithms/vqgan/discriminators/patchgan.py:15-99', 'vq/algorithms/vqgan/discriminators/base.py:11-15'],
    'losses': ['vq/algorithms/vqgan/losses/generator.py:16-42', 'vq/algorithms/vqgan/losses/discriminator.py:17-69',
               'vq/algorithms/vqgan/losses/registries.py:9-14'],
}


def jsonable(kwargs: dict) -> dict:
    return json.loads(json.dumps(kwargs))


def network_case(ref, name: str, case: dict) -> dict:
    cls = getattr(ref, case['cls'])
    f64 = nc.run_case(cls(**case['kwargs']), case, dtype=torch.float64)
    f32 = nc.run_case(cls(**case['kwargs']), case, dtype=torch.float32)
    assert list(f64) == list(f32)
    grads = [n for n in f64 if n.startswith('grad/')]
    top = max(f64[n].abs().max().item() for n in grads)
    zero = sorted(n for n in grads if f64[n].abs().max().item() < ZERO_BELOW * top)
    assert 8 * len(zero) <= len(f64), f'{name}: {len(zero)} of {len(f64)} tensors are zero in exact arithmetic: {zero}'
    rec, names, self_err = {}, [], []
    for n, t in f64.items():
        assert torch.isfinite(t).all(), (name, n)
        rec[n] = nc.stored(n, t, case['seed'])
        names.append(n)
        self_err.append(0.0 if n in zero else nc.rel_err(nc.stored(n, f32[n], case['seed']), rec[n]))
    rec['fp32_self'] = np.array(self_err, dtype=np.float64)
    rec['spec'] = json.dumps(dict(
        cls=case['cls'], kwargs=jsonable(case['kwargs']), input=list(case['input']), train=case['train'], seed=case['seed'],
        seeds=dict(weights=case['seed'], input=case['seed'] + 1, g=case['seed'] + 2), names=names, zero=zero,
        source='reference-import', reference=CITE[case['cls']]))
    return rec


def init_case(ref, name: str, case: dict) -> dict:
    torch.manual_seed(case['seeds'][0])
    module = getattr(ref, case['cls'])(**case['kwargs'])
    stats = nc.init_statistics(module, case['seeds'], ref.Config())
    rec = {'stat/' + n: v for n, v in stats.items()}
    rec['spec'] = json.dumps(dict(cls=case['cls'], kwargs=jsonable(case['kwargs']), seeds=list(case['seeds']), names=list(stats),
                                  source='reference-import', reference=CITE[case['cls']]))
    return rec


def loss_case(ref) -> dict:
    classes = {n: getattr(ref, n) for n in nc.LOSS_CLASSES + ('R1GradientPenalty', 'PatchGANDiscriminator')}
    res = nc.run_losses(classes)
    assert res['r1/modes_restored'].item() == 1.0
    rec = {n: nc.stored(n, t, nc.R1_CASE['seed']) for n, t in res.items()}
    rec['spec'] = json.dumps(dict(shapes=[list(s) for s in nc.LOSS_SHAPES], settings=list(nc.LOSS_SETTINGS), classes=list(nc.LOSS_CLASSES),
                                  r1=dict(kwargs=jsonable(nc.R1_CASE['kwargs']), input=list(nc.R1_CASE['input']), seed=nc.R1_CASE['seed']),
                                  seed=nc.LOSS_SEED, names=list(res), source='reference-import',
                                  reference=CITE['losses'] + CITE['PatchGANDiscriminator']))
    return rec


def check_ours_against(rec_by_name: dict) -> None:
    """Section (d) of tests/test_network_reference_cpu.py on generation: this package's ``init_weights`` after the same seeds."""
    import vector_quantization_amd as vqa
    for name, case in nc.INIT_CASES.items():
        torch.manual_seed(case['seeds'][0])
        module = getattr(vqa, case['cls'])(**case['kwargs'])
        stats = nc.init_statistics(module, case['seeds'], vqa.Config())
        for n, v in stats.items():
            want = rec_by_name['init_' + name]['stat/' + n]
            assert v.tobytes() == want.tobytes(), f'{name}: init_weights of {n} gives {v}, the reference {want}'


def main(out_dir=None, quiet=False) -> None:
    if not ref_import.available():
        sys.exit('oracle/make_network_golden.py needs the reference checkout')
    make_golden.check_pinned()
    out = OUT if out_dir is None else out_dir
    os.makedirs(out, exist_ok=True)
    torch.set_num_threads(make_golden.FIXTURE_THREADS)
    ref = ref_import.load_networks()
    recs = {}
    for name, case in nc.CASES.items():
        recs[name] = network_case(ref, name, case)
    for name, case in nc.INIT_CASES.items():
        recs['init_' + name] = init_case(ref, name, case)
    recs['gan_losses'] = loss_case(ref)
    check_ours_against(recs)
    for name, rec in recs.items():
        path = os.path.join(out, name + '.npz')
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, f'{path}: {size} bytes'
        if not quiet:
            spec = json.loads(rec['spec'])
            worst = float(np.max(rec['fp32_self'])) if 'fp32_self' in rec else float('nan')
            print(f"{name:18s} {size:7d} bytes  {len(spec['names']):3d} tensors  zero {len(spec.get('zero', []))}  "
                  f"worst fp32_self {worst:.2e}", flush=True)


if __name__ == '__main__':
    if any(os.environ.get(k) != v for k, v in make_golden.PINNED_ENV.items()):      # a fresh child process with the pinned numerics
        import subprocess
        sys.exit(subprocess.run([sys.executable, '-m', 'oracle.make_network_golden'] + sys.argv[1:],
                                env=make_golden.pinned_env()).returncode)
    main()
