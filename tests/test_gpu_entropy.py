"""The fused EntropyLoss (LazyDistance.entropy -> ops.entropy_loss / entropy_loss_backward -> vqhip_entropy_*) on the GPU,
held to the float64 evaluator and the derived bounds of tests/entropy_ref.py (proven on the CPU by
tests/test_entropy_reference_cpu.py), to the reference's own values (tests/golden/entropy), and to its memory contract:
no allocation that grows with N * K.

Measured on an MI355X (worst err/tol over the case table: see profiles/entropy_loss.txt)."""
import ctypes
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import backward_ref as br
import entropy_ref as er
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'entropy')
EMB = 'torch_nn_modules_sparse_Embedding'
MIB = float(1 << 20)


def _distance(metric):
    from vector_quantization_amd import quantizers as Q
    return Q.L2Distance() if metric == 'L2' else Q.CosineDistance(autocast=None)


def _run(c, inp, fused=True):
    """loss, grad_x, grad_w of the case on the device through LazyDistance + EntropyLoss; also the handle."""
    from vector_quantization_amd.quantizers.distances import LazyDistance
    from vector_quantization_amd.quantizers.losses import EntropyLoss
    x = inp['x'].cuda().requires_grad_(True)
    w = inp['w'].cuda().requires_grad_(True)
    d = LazyDistance(_distance(c.metric), x, w)
    if fused and c.block_rows is not None:
        loss = d.entropy(c.T, c.block_rows)
    else:
        loss = EntropyLoss(temperature=c.T, fused=None if fused else False)(None, x, dict(distance=d))
    (loss * c.upstream).backward()
    return dict(loss=(loss.detach() * c.upstream).cpu(), grad_x=x.grad.cpu(), grad_w=w.grad.cpu()), d


def _assert_inside(name, got, ref, scale=1.0):
    vs = er.verdicts(got, ref, scale)
    for part, v in vs.items():
        print(v.line(f'{name} {part}'))
    for part, v in vs.items():
        assert v.ok, v.line(f'{name} {part}')


@pytest.mark.parametrize('c', er.GPU_CASES, ids=lambda c: c.name)
def test_fused_entropy_matches_float64_evaluator(c):
    inp = er.inputs(c)
    ref = er.evaluate(c, inp)
    got, d = _run(c, inp)
    assert d._value is None, 'the fused route materialised the handle'
    assert got['grad_x'].dtype == inp['x'].dtype and got['grad_w'].dtype == torch.float32
    _assert_inside(f'{c.name} fused', got, ref)
    again, _ = _run(c, inp)
    for k in ('loss', 'grad_x', 'grad_w'):
        assert torch.equal(got[k], again[k]), f'{c.name}: {k} differs between two runs'
    old, d_old = _run(c, inp, fused=False)
    assert d_old._value is not None
    _assert_inside(f'{c.name} fused=False', old, ref)


@pytest.mark.parametrize('path', sorted(glob.glob(os.path.join(GOLD, '*.npz'))), ids=os.path.basename)
def test_fused_entropy_matches_reference_fixture(path):
    """The reference's own fp32 values lie within the bound of the float64 value (CPU test), the fused route's too: the two
    differ by at most twice the bound."""
    g = np.load(path)
    spec = json.loads(str(g['spec']))
    c = er.Case(spec['name'], spec['N'], spec['K'], spec['D'], spec['metric'], 'f32', spec['temperature'], plant=spec['plant'])
    inp = dict(x=torch.from_numpy(g['x']), w=torch.from_numpy(g['w']),
               zero_pairs=[(spec['plant_row'], spec['plant_code'])] if spec['plant'] == 'equal' else [])
    ref = er.evaluate(c, inp)
    got, d = _run(c, inp)
    assert d._value is None
    gold = dict(loss=torch.tensor(float(g['loss'])), grad_x=torch.from_numpy(g['grad_x']), grad_w=torch.from_numpy(g['grad_w']))
    _assert_inside(f'{c.name} fixture vs float64', gold, ref)
    _assert_inside(f'{c.name} fused vs float64', got, ref)
    ref2 = dict(ref, **{k: gold[k].double() for k in gold})
    _assert_inside(f'{c.name} fused vs fixture (2x)', got, ref2, scale=2.0)


def _build(K, D, dist, T, fused=None):
    from vector_quantization_amd import Config, build_quantizer
    cfg = dict(type='VQGANQuantizer', embedding=dict(type=EMB, num_embeddings=K, embedding_dim=D),
               distance=dict(type=f'{dist}Distance'),
               losses=dict(vqgan_loss=dict(type='VQGANLoss'), entropy=dict(type='EntropyLoss', temperature=T)))
    if fused is not None:
        cfg['losses']['entropy']['fused'] = fused
    q = build_quantizer(cfg)
    q.train(True)
    q.init_weights(Config(dict(type='vqgan')))
    return q.cuda()


@pytest.mark.parametrize('dist', ['L2', 'Cosine'])
def test_module_with_vqgan_and_entropy_losses(dist):
    """A VQGANQuantizer with losses = {vqgan_loss, entropy}: encode, decode, both losses, one backward; the handle stays
    unmaterialised and the gradients of both terms add up to the float64 reference of the sum."""
    c = er.Case('module', 300, 96, 16, dist, T=0.5)
    inp = er.inputs(c)
    q = _build(c.K, c.D, dist, c.T)
    with torch.no_grad():
        q.embedding.weight.copy_(inp['w'])
    x = inp['x'].cuda().requires_grad_(True)
    x2, quant, memo = q.encode(x, {})
    d = memo['encode']['distance']
    z, memo = q.decode(quant, memo)
    ent = q._losses['entropy'](None, x2, dict(distance=d))        # the reference reads memo['distance'] (losses.py:145)
    assert d._value is None
    vq = q._losses['vqgan_loss'](z, x2, memo)
    (ent + vq).backward()
    ref = er.evaluate(c, inp)
    idx = quant.reshape(-1).cpu()
    x64 = inp['x'].double().requires_grad_(True)
    w64 = inp['w'].double().requires_grad_(True)
    lv = tr.vqgan_loss(tr.decode(idx, w64), x64, 0.25)
    gvx, gvw = torch.autograd.grad(lv, (x64, w64))
    vc = br.VqCase('module', c.N, c.K, c.D, mix='loss', scal=(None, None, 1.0))
    tvx, tvw = br.vq_tolerance(vc, dict(x=inp['x'], w=inp['w'], idx=idx, g_zste=None, g_xn=None))
    tot = dict(loss=ref['loss'] + lv.detach(), grad_x=ref['grad_x'] + gvx, grad_w=ref['grad_w'] + gvw,
               tol_loss=ref['tol_loss'] + (br.C_SSE + 4) * er.U * float(lv.detach()) + er.U * (abs(float(ref['loss'])) + float(lv.detach())),
               tol_x=ref['tol_x'] + tvx + er.U * (ref['grad_x'].abs() + gvx.abs()),
               tol_w=ref['tol_w'] + tvw + er.U * (ref['grad_w'].abs() + gvw.abs()))
    got = dict(loss=(ent + vq).detach().cpu(), grad_x=x.grad.cpu(), grad_w=q.embedding.weight.grad.cpu())
    _assert_inside(f'module {dist}', got, tot)


def test_routes_and_refusals():
    from vector_quantization_amd import _lib, ops
    from vector_quantization_amd.quantizers.distances import CosineDistance, L2Distance, LazyDistance
    from vector_quantization_amd.quantizers.losses import EntropyLoss
    x = torch.randn(64, 16, device='cuda')
    e = torch.randn(32, 16, device='cuda')
    for T in (0.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            ops.entropy_loss(x, e, 'L2', T)
        with pytest.raises(ValueError):
            LazyDistance(L2Distance(), x, e).entropy(T)
    with pytest.raises(ValueError):
        ops.entropy_loss(x, e, 'CosineBF16', 0.5)
    # the bf16-autocast cosine, a materialised handle and a plain tensor keep the matrix route
    d16 = LazyDistance(CosineDistance(autocast='bf16'), x, e)
    assert d16.metric == 'CosineBF16'
    v16 = EntropyLoss(temperature=0.5)(None, x, dict(distance=d16))
    assert d16._value is not None and torch.isfinite(v16)
    d = LazyDistance(L2Distance(), x, e)
    mat = d.materialize()
    a = EntropyLoss(temperature=0.5)(None, x, dict(distance=d))
    b = EntropyLoss(temperature=0.5)(None, x, dict(distance=mat))
    assert torch.equal(a, b)
    # weight stays applied on the fused route
    lazy = LazyDistance(L2Distance(), x, e)
    w3 = EntropyLoss(temperature=0.5, weight=3.0)(None, x, dict(distance=lazy))
    assert lazy._value is None and torch.allclose(w3, 3.0 * ops.entropy_loss(x, e, 'L2', 0.5)[0])
    # bad sizes: VQHIP_EINVAL, nothing launched
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    need = L.vqhip_entropy_workspace_bytes(100, 64)
    assert need == math.ceil(100 / 32) * 64 * 8
    assert L.vqhip_entropy_rows(fake, 100, 64, 0.5, fake, fake, fake, 1, fake, need - 1, None) == -22
    assert b'ws too small' in L.vqhip_last_error()
    assert L.vqhip_entropy_rows(fake, 0, 64, 0.5, fake, fake, fake, 1, fake, need, None) == -22
    assert L.vqhip_entropy_rows(fake, 100, 64, 0.0, fake, fake, fake, 1, fake, need, None) == -22
    assert L.vqhip_entropy_rows(None, 100, 64, 0.5, fake, fake, fake, 1, fake, need, None) == -22
    assert L.vqhip_entropy_grad(fake, 100, 64, 0.5, fake, fake, fake, 1.0, None, 0, fake, fake, 1, fake, need - 1, None) == -22
    assert L.vqhip_entropy_grad(fake, 100, 64, 0.5, fake, fake, fake, 1.0, None, 5, fake, fake, 1, fake, need, None) == -22
    assert L.vqhip_entropy_grad(fake, 100, 64, float('nan'), fake, fake, fake, 1.0, None, 0, fake, fake, 1, fake, need, None) == -22
    assert L.vqhip_entropy_finish(fake, fake, fake, 0, 64, fake, fake, fake, None) == -22
    torch.cuda.synchronize()


def _peak(c, inp, fused):
    from vector_quantization_amd.quantizers.distances import LazyDistance
    from vector_quantization_amd.quantizers.losses import EntropyLoss
    x = inp['x'].cuda().requires_grad_(True)
    w = inp['w'].cuda().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    d = LazyDistance(_distance(c.metric), x, w)
    loss = EntropyLoss(temperature=c.T, fused=None if fused else False)(None, x, dict(distance=d))
    loss.backward()
    torch.cuda.synchronize()
    outputs = x.grad.numel() * x.grad.element_size() + w.grad.numel() * 4
    peak = torch.cuda.max_memory_allocated() - base - outputs
    return dict(loss=loss.detach().cpu(), grad_x=x.grad.cpu(), grad_w=w.grad.cpu()), peak, d


def test_memory_stays_bounded_at_65536_by_16384():
    """N = 65 536, K = 16 384, D = 256, L2, bf16 latents: one matrix would be 4 GiB; forward + backward of the fused route
    must stay below N K 4 / 8 = 512 MiB beyond inputs and outputs, and its values inside the bounds of the float64 evaluator
    (loss, grad_w, and grad_x on 256 evenly spaced rows plus the first and last row of every block)."""
    from vector_quantization_amd import ops
    c = er.Case('mem_65536', 65536, 16384, 256, 'L2', 'bf16', 0.5)
    inp = er.inputs(c)
    got, peak, d = _peak(c, inp, True)
    print(f'{c.name}: peak beyond inputs and outputs {peak / MIB:.1f} MiB (limit 512)')
    assert d._value is None
    assert peak < c.N * c.K * 4 / 8, f'{peak / MIB:.1f} MiB'
    ref = er.evaluate(c, inp, chunk=2048)
    R = ops.entropy_block_rows(c.N, c.K)
    rows = sorted(set(np.linspace(0, c.N - 1, 256).astype(int).tolist()
                      + [r for b in range(0, c.N, R) for r in (b, min(c.N, b + R) - 1)]))
    sub = lambda t: t[rows]                                                     # noqa: E731
    _assert_inside(c.name, dict(loss=got['loss'], grad_x=sub(got['grad_x']), grad_w=got['grad_w']),
                   dict(ref, grad_x=sub(ref['grad_x']), tol_x=sub(ref['tol_x'])))


@pytest.mark.parametrize('shape', [(12544, 16384, 256, 'L2'), (3072, 8192, 32, 'Cosine')], ids=lambda s: f'n{s[0]}_k{s[1]}_d{s[2]}')
def test_training_shapes_both_routes(shape):
    N, K, D, metric = shape
    c = er.Case(f'train_{N}', N, K, D, metric, 'bf16', 0.5)
    inp = er.inputs(c)
    ref = er.evaluate(c, inp, chunk=2048)
    got, peak, d = _peak(c, inp, True)
    old, peak_old, _ = _peak(c, inp, False)
    print(f'{c.name}: peak fused {peak / MIB:.1f} MiB, matrix route {peak_old / MIB:.1f} MiB (one matrix {N * K * 4 / MIB:.0f} MiB)')
    # one tile of at most 64 MiB, and as much again for everything that does not grow with N K (distance scratch, column
    # partials, the fp32 / normalised operands and block temporaries of [R, D] and [K, D])
    assert d._value is None and peak < 128 * MIB, f'{peak / MIB:.1f} MiB'
    _assert_inside(f'{c.name} fused', got, ref)
    _assert_inside(f'{c.name} fused=False', old, ref)
