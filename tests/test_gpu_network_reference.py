"""The fused route of the networks on the GPU against the reference's own float64 outputs (tests/golden/networks/*.npz, written by
oracle/make_network_golden.py from the reference's source files; nothing but the fixtures is read here).

For every case of tests/network_cases.py the module loads the seeded state dict with ``strict=True`` and runs forward and backward
in fp32 on the fused route - NCHW and channels-last inputs for the convolutional networks, contiguous rows for VQ-KD - and once
under bf16 autocast per network.  Every output, the input gradient, every parameter gradient not on the fixture's zero list and
PatchGAN's running statistics are held to the fixture's float64 values in ``max|got - want| / max|want|``.

The tolerance per tensor is 4 x the larger of

1. ``fp32_self`` of the fixture: the reference's own fp32 CPU run against its float64 run;
2. the error, against the same fixture, of the ``fused=False`` route on the same GPU with the same input layout and autocast
   setting - that route runs no kernel of this package and tests/test_network_reference_cpu.py pins it to the reference;

and never below 4 x 2**-23.  The factor 4 is the margin tests/test_gpu_group_norm.py grants for the convolution algorithms two
routes select.  Both numbers and the fused error are printed for every case; profiles/network_reference.txt records a run.

``patchgan_eval`` cannot take the kernels (eval mode normalises with the running statistics): the module is built with
``fused=True``, ``last_route`` has to name that reason, and the same tolerance holds.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import vector_quantization_amd as vqa

import network_cases as nc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'networks')
EPS32 = 2.0 ** -23
MARGIN = 4
AUTOCAST_CASES = ('vqgan_encoder', 'vqgan_decoder', 'vqkd_encoder_48', 'vqkd_decoder_3', 'patchgan_train')


@functools.lru_cache(None)
def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    spec = json.loads(str(z['spec']))
    return {n: z[n] for n in spec['names']}, dict(zip(spec['names'], z['fp32_self'])), spec


def errors(name, fused, channels_last, autocast):
    """name of tensor -> error against the fixture of one GPU run, and the route the module reported."""
    case = nc.CASES[name]
    want, _, spec = fixture(name)
    module = getattr(vqa, case['cls'])(**case['kwargs'], fused=fused)
    res = nc.run_case(module, case, device='cuda', dtype=torch.float32, channels_last=channels_last, autocast=autocast)
    assert list(res) == spec['names']
    out = {}
    for n in spec['names']:
        if n in spec['zero']:
            continue
        got = nc.stored(n, res[n], spec['seed'])
        assert got.shape == want[n].shape and np.isfinite(got).all(), n
        out[n] = nc.rel_err(got, want[n])
    return out, module.last_route


def check(name, channels_last=False, autocast=None):
    case = nc.CASES[name]
    _, fp32_self, _ = fixture(name)
    torch_err, torch_route = errors(name, False, channels_last, autocast)
    fused_err, route = errors(name, True, channels_last, autocast)
    assert torch_route.name == 'torch' and torch_route.why == 'fused=False'
    if case['train'] or case['cls'] != 'PatchGANDiscriminator':
        assert route.name == 'fused', route
    else:
        assert route.name == 'torch' and route.why.startswith('eval mode'), route
    tag = f"{name} {'nhwc' if channels_last else 'rows' if case.get('rows') else 'nchw'} {'bf16 autocast' if autocast else 'fp32'}"
    rows = []
    for n, err in fused_err.items():
        floor = max(float(fp32_self[n]), torch_err[n], EPS32)
        rows.append((err / (MARGIN * floor), n, float(fp32_self[n]), torch_err[n], err))
    worst = max(rows)
    print(f'{tag}: {len(rows)} tensors; largest fp32_self {max(r[2] for r in rows):.3e}, largest fused=False error '
          f'{max(r[3] for r in rows):.3e}, largest fused error {max(r[4] for r in rows):.3e}; worst error / tolerance '
          f'{worst[0]:.3f} at {worst[1]} (fp32_self {worst[2]:.3e}, fused=False {worst[3]:.3e}, fused {worst[4]:.3e})')
    bad = sorted((r for r in rows if not r[0] <= 1), reverse=True)
    assert not bad, f'{tag}: ' + '; '.join(f'{n}: fused {e:.3e} > 4 x max(fp32_self {s:.3e}, fused=False {t:.3e})' for _, n, s, t, e in bad[:6])


@pytest.mark.parametrize('name', list(nc.CASES))
def test_fused_route_fp32_against_the_reference(name):
    check(name)


@pytest.mark.parametrize('name', [n for n, c in nc.CASES.items() if not c.get('rows')])
def test_fused_route_fp32_channels_last_against_the_reference(name):
    check(name, channels_last=True)


@pytest.mark.parametrize('name', AUTOCAST_CASES)
def test_fused_route_bf16_autocast_against_the_reference(name):
    check(name, autocast=torch.bfloat16)
