"""Every forward loss scalar and straight-through output against the float64 reference, under the derived bounds of
tests/forward_ref.py.

The token-major tail (``gather_ste_loss_kernel<DT, NT>``) is called directly through ``ops.gather_ste_loss`` / ``ops.gather_ste_mse``
so that each form can be forced; the VQ-KD tails (``vqkd_tail_small_kernel<L>``, ``vqkd_tail_kernel``, ``vqkd_tail_finish``) and the
one-call forwards with their hook-by-hook twins run through the modules.  Every loss is compared with ``oracle.torch_ref`` in
float64 on the step's own tokens and codebook — never with another route of the library — and the decoded rows and
straight-through outputs bit for bit.  The case table, the bounds and the mutations are those
tests/test_forward_reference_cpu.py proves on the CPU.  Each comparison prints its err / tol (run with ``-s``);
profiles/forward_parity.txt keeps one run's record.
"""
import numpy as np
import pytest
import torch

import forward_ref as fr
from oracle import synth

pytestmark = pytest.mark.gpu

EMB = 'torch_nn_modules_sparse_Embedding'
ON_DEVICE_FROM = 1 << 20       # N D from which the float64 reference is evaluated on the device


def _report(name, got, ref, tol):
    v = fr.check(got, ref, tol)
    print('\n' + v.line(f'forward {name}'), end='')
    assert v.ok, v.line(name) + f' got={float(got)!r} ref={float(ref)!r} tol={float(tol)!r}'
    return v


def _reference(c, x, w, idx, inp):
    """float64 values of the case, on the device where N D is large."""
    if c.N * c.D >= ON_DEVICE_FROM:
        return fr.reference(x, w, idx, c.tail, c.beta)
    return fr.reference(inp['x'], inp['w'], inp['idx'], c.tail, c.beta)


def _exact(x, w, idx, z, z_ste):
    z_e, zs_e = fr.exact_outputs(x, w, idx)
    if z is not None:
        assert z.dtype == torch.float32 and torch.equal(z, z_e), 'z != e[idx] bit for bit'
    if z_ste is not None:
        assert z_ste.dtype == torch.float32 and torch.equal(z_ste.view(torch.int32), zs_e.view(torch.int32)), 'z_ste != fl(x + fl(z - x))'


def _check_mse(name, c, mse, ref):
    """mse fp32[4] of the ticket form: [0] within the bound, [1] its bits, [2] = fl([0] + fl(beta [1])) bit for bit, [3] = 0."""
    m = mse.cpu().numpy()
    assert m.dtype == np.float32 and m.shape == (4,)
    tol = fr.loss_bound(ref, fr.c_plain(c.D), c.N * c.D)
    v = _report(name, float(m[0]), ref, tol)
    assert m[0].tobytes() == m[1].tobytes() and m[3] == 0.0
    assert m[2].tobytes() == fr.combine_fp32(m[0], c.beta).tobytes(), (m, c.beta)
    return v


def _check_sse(name, c, sse, ref):
    assert sse.dtype == torch.float64 and sse.shape == (1,)
    return _report(name, float(sse) / (c.N * c.D), ref, fr.loss_bound(ref, fr.c_plain(c.D), c.N * c.D, fp32_out=False))


def _run_tail(c, x, w, idx, need_z=True, need_ste=True):
    from vector_quantization_amd import ops
    if c.tail == 'plain':
        return ops.gather_ste_loss(x, w, idx, need_z=need_z, need_ste=need_ste, need_sse=True)
    return ops.gather_ste_mse(x, w, idx, need_z=need_z, need_ste=need_ste, beta=c.beta)


def _check_tail(name, c, out, x, w, idx, ref):
    z, z_ste, s = out
    _exact(x, w, idx, z, z_ste)
    v = _check_sse(name, c, s, ref) if c.tail == 'plain' else _check_mse(name, c, s, ref)
    if c.tok == 'exact':
        assert float(s[0]) == 0.0 and torch.equal(z_ste.view(torch.int32), x.float().view(torch.int32))     # exactly 0.0; the bits of x
    return v


# ------------------------------------------------------------------------------------------------------------------
# gather_ste_loss_kernel<DT, 0>: the token-major tail
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', fr.TAIL_CASES, ids=lambda c: c.name)
def test_token_major_tail(c):
    inp = fr.inputs(c)
    x, w, idx = inp['x'].cuda(), inp['w'].cuda(), inp['idx'].cuda()
    ref = _reference(c, x, w, idx, inp)['commitment']
    _check_tail(c.name, c, _run_tail(c, x, w, idx), x, w, idx, ref)


def test_need_combinations_of_gather_ste_loss():
    from vector_quantization_amd import ops
    c = fr.by_name('n4097_d252_f32_plain')
    inp = fr.inputs(c)
    x, w, idx = inp['x'].cuda(), inp['w'].cuda(), inp['idx'].cuda()
    ref = fr.reference(inp['x'], inp['w'], inp['idx'], c.tail)['commitment']
    for bits in range(8):
        need_z, need_ste, need_sse = bool(bits & 1), bool(bits & 2), bool(bits & 4)
        z, z_ste, sse = ops.gather_ste_loss(x, w, idx, need_z=need_z, need_ste=need_ste, need_sse=need_sse)
        assert (z is None) == (not need_z) and (z_ste is None) == (not need_ste) and (sse is None) == (not need_sse)
        _exact(x, w, idx, z, z_ste)
        if need_sse:
            _check_sse(f'{c.name} need_z={int(need_z)} need_ste={int(need_ste)}', c, sse, ref)


def test_ticket_scratch_comes_back_zeroed():
    """gather_ste_mse twice in a row and then at another N: the 16-byte scratch (sum, ticket) is handed back zeroed, so all three
    results are within the bound, and the two equal calls are bit-identical only if nothing was left in it.  (The double
    atomics of one launch arrive in any order: the equal calls are compared through the fp32 mean, whose half ulp is 2^29 times
    the spread of the double sums.)"""
    a, b = fr.by_name('n8193_d256_f32_plain_mse'), fr.by_name('n4097_d1030_f32_plain_mse')
    outs = []
    for c in (a, a, b, a):
        inp = fr.inputs(c)
        x, w, idx = inp['x'].cuda(), inp['w'].cuda(), inp['idx'].cuda()
        ref = _reference(c, x, w, idx, inp)['commitment']
        out = _run_tail(c, x, w, idx, need_z=False)
        _check_tail(f'{c.name} call {len(outs)}', c, out, x, w, idx, ref)
        outs.append(out[2].clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[3])


# ------------------------------------------------------------------------------------------------------------------
# gather_ste_loss_kernel<DT, 1>: the streamed form
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', fr.STREAM_CASES, ids=lambda c: c.name)
def test_streamed_and_resident_form_at_one_shape(c):
    """Both outputs of 98 321 x 256 are just over 192 MiB: gather_ste_impl takes the streamed form (non-temporal accesses, grid
    cap 512).  With ONE output the same N is below the threshold and stays on the non-streamed form: both are run here, so
    both forms are checked at one shape (N = 16 * 6145 + 1: the last workgroup's block holds one row)."""
    assert 2 * c.N * c.D * 4 > (192 << 20) >= c.N * c.D * 4
    inp = fr.inputs(c)
    x, w, idx = inp['x'].cuda(), inp['w'].cuda(), inp['idx'].cuda()
    ref = fr.reference(x, w, idx, c.tail, c.beta)['commitment']
    out = _run_tail(c, x, w, idx, need_z=True, need_ste=True)
    _check_tail(f'{c.name} streamed', c, out, x, w, idx, ref)
    del out
    out = _run_tail(c, x, w, idx, need_z=False, need_ste=True)
    _check_tail(f'{c.name} resident', c, out, x, w, idx, ref)
    del out, x, w, idx
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------
# the bound sees on the device what it is for
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['n4097_d1030_f32_plain_mse', 'n4111_d260_bf16_plain'])
def test_mutated_reference_rejects_the_kernel(name):
    """The CPU mutations on the REFERENCE side: against a reference that drops or repeats a row, leaves out the elements past
    4 (D // 4) or the last block, divides by (N - 1) D or sums sequentially in fp32, the kernel's value is out of bound."""
    c = fr.by_name(name)
    inp = fr.inputs(c)
    x, w, idx = inp['x'].cuda(), inp['w'].cuda(), inp['idx'].cuda()
    s = _run_tail(c, x, w, idx, need_z=False, need_ste=False)[2]
    got = float(s[0]) / (c.N * c.D) if c.tail == 'plain' else float(s[0])
    ref = fr.reference(inp['x'], inp['w'], inp['idx'], c.tail, c.beta)['commitment']
    assert fr.check(got, ref, fr.loss_bound(ref, fr.c_plain(c.D), c.N * c.D, c.tail != 'plain')).ok
    muts = fr.mutations(inp['x'], inp['w'], inp['idx'], c.tail)
    assert ('tail_elements_dropped' in muts) == (c.D % 4 != 0)
    assert fr.must_reject('sequential_fp32_sum', c.N, c.D) == (c.D == 1030)      # required from N D = 2^22 on: the first of the two cases
    if c.N % 16 != 1:
        assert muts['last_block_dropped'] != muts['last_row_dropped']           # a last block of 15 rows: a mutation of its own
    for mut, wrong in muts.items():
        v = fr.check(got, wrong, fr.loss_bound(wrong, fr.c_plain(c.D), c.N * c.D, c.tail != 'plain'))
        print(f'\nforward {name} [reference: {mut}]: err/tol={v.worst:.4g}', end='')
        if fr.must_reject(mut, c.N, c.D):
            assert not v.ok, f'{name}: the kernel is within the bound of the mutated reference {mut}'


# ------------------------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------------------------

def build(cfg, w, train=True, no_grad_params=False):
    from vector_quantization_amd import Config, build_quantizer
    q = build_quantizer(cfg)
    q.train(True)
    q.init_weights(Config(type='vqgan') if cfg['type'] == 'VQGANQuantizer' else Config())
    q = q.cuda()
    q._forward_pre_hooks.clear()
    with torch.no_grad():
        q.embedding.weight.copy_(torch.from_numpy(w))
    if no_grad_params:
        for p in q.parameters():
            p.requires_grad_(False)
    q.train(train)
    return q


def vqkd_cfg(K, D):
    return dict(type='VQKDQuantizer', embedding=dict(type=EMB, num_embeddings=K, embedding_dim=D),
                distance=dict(type='CosineDistance'), callbacks=[dict(type='VQKDCallback', ema=dict())],
                losses=dict(commitment_loss=dict(type='CommitmentLoss', mse=dict(norm=True))))


def batches(N, K, D, w0, steps, seed, bf16=False, plant=False):
    g = synth.rng(seed)
    out = []
    for _ in range(steps):
        x = g.standard_normal((N, D), dtype=np.float32) * np.float32(0.3) + w0[g.integers(0, max(1, K // 8), N)]
        if plant:                                # a zero-norm row and a tiny-norm row: the eps clamps (backward_ref's zero_rows / tiny_rows)
            x[0] = 0.0
            x[1] = 0.0
            x[1, D - 1] = 1e-13
        t = torch.from_numpy(x).cuda()
        out.append(t.bfloat16() if bf16 else t)
    return out


@pytest.mark.parametrize('N,D', [(c.N, c.D) for c in fr.NORM_CASES], ids=[c.name for c in fr.NORM_CASES])
def test_vqkd_tails_through_the_one_call_forward(N, D):
    """vqkd_tail_small_kernel<8|16|32> (D = 24 leaves lanes of a group idle), vqkd_tail_kernel (D = 64, 768) and
    vqkd_tail_finish: ``loss`` and ``memo['loss']`` against the float64 CommitmentLoss(norm=True) of the module's own tokens,
    normalised rows and POST-update codebook; z bit for bit."""
    from vector_quantization_amd.quantizers import routes
    K = 1024
    w0 = synth.unit_rows(synth.rng(8).standard_normal((K, D), dtype=np.float32))
    q = build(vqkd_cfg(K, D), w0, no_grad_params=True)
    for step, x in enumerate(batches(N, K, D, w0, 2, 34 + D, plant=True)):
        z, loss, memo = q(x, {})
        assert q.last_route == routes.Route('one_call_vqkd'), q.last_route       # (the reason it was refused is in the route)
        rows, quant, w_new = memo['x'].detach(), memo['quant'], q.embedding.weight.detach()
        assert rows.dtype == torch.float32 and not rows[0].any() and float(rows[1].abs().sum()) == pytest.approx(0.1, rel=1e-6)
        ref = fr.reference(rows, w_new, quant, 'normalised')['commitment']
        tol = fr.normalised_bound(rows, w_new, quant, ref)
        _report(f'vqkd n{N}_d{D} step {step} loss', float(loss), ref, tol)
        assert list(memo['loss'].keys()) == ['commitment_loss']
        for name, value in memo['loss'].items():
            _report(f'vqkd n{N}_d{D} step {step} memo {name}', float(value), ref, tol)
        assert torch.equal(z.detach(), rows + (w_new[quant] - rows)), 'z != x + (w_new[quant] - x) bit for bit'


def _module_cfg(kind, K, D, fused):
    cfg = dict(type='VQGANQuantizer', embedding=dict(type=EMB, num_embeddings=K, embedding_dim=D),
               distance=dict(type=f'{kind.distance}Distance'), losses=dict(the_loss=dict(type=kind.loss)))
    if kind.callback == 'CVQVAECallback':
        cfg['callbacks'] = [dict(type='CVQVAECallback', ema=dict(), anchor=dict(type='NearestAnchor'))]
    else:
        cfg['callbacks'] = [dict(type=kind.callback)] if kind.callback else []
    if not fused:
        cfg['fused'] = False
    return cfg


def _expected_route(kind, D, route):
    """The Route each (kind, D) must take, reason included (routes.py): the one-call forward of its family, except the CVQ-VAE
    flow at a D without a proposal image (D = 30), which keeps the fused tail behind a hook-by-hook encode."""
    from vector_quantization_amd.quantizers import routes
    if route != 'one_call':
        return routes.Route(route, 'one_call_steps=False')
    if kind.callback != 'CVQVAECallback':
        return routes.Route('one_call_plain')
    why = routes.proposal_image(D)
    assert bool(why) == (D == 30)
    return routes.Route('fused_tail', why) if why else routes.Route('one_call_cvq')


@pytest.mark.parametrize('shape', fr.MODULE_SHAPES, ids=lambda s: f'n{s[0]}_k{s[1]}_d{s[2]}_{s[3]}')
@pytest.mark.parametrize('kind', fr.MODULE_KINDS, ids=lambda k: k.name)
def test_module_forwards_on_every_route(kind, shape):
    """The one-call forward (vqhip_vq_forward / vqhip_cvq_forward), the fused tail behind a hook-by-hook encode and the
    hook-by-hook route (fused=False), two steps each with the codebook moved in between (the callback's update; an SGD step
    where there is a gradient): every loss term against the float64 reference of that step's own rows (``memo['x']``), tokens
    and codebook, and z bit for bit."""
    N, K, D, dtype = shape
    beta = 0.25
    w0 = synth.rng(11).standard_normal((K, D), dtype=np.float32)
    if kind.callback == 'CVQVAECallback':
        w0 = synth.unit_rows(w0)
    xs = batches(N, K, D, synth.unit_rows(w0), 2, 37, dtype == 'bf16')
    for route, one_call, fused in (('one_call', True, True), ('fused_tail', False, True), ('hooks', False, False)):
        q = build(_module_cfg(kind, K, D, fused), w0, train=kind.train)
        q.one_call_steps = one_call
        for step, x in enumerate(xs):
            xin = x.clone().requires_grad_(kind.train)
            z, loss, memo = q(xin, {})
            took = q.last_route
            assert took == _expected_route(kind, D, route), (took, _expected_route(kind, D, route))
            rows, quant, w_now = memo['x'].detach(), memo['quant'].reshape(-1), q.embedding.weight.detach().clone()
            ref = fr.reference(rows, w_now, quant, 'plain', beta)
            b_m = fr.loss_bound(ref['commitment'], fr.c_plain(D), N * D)
            want, tol = (ref['vqgan'], fr.combined_bound(ref['commitment'], b_m, beta)) if kind.loss == 'VQGANLoss' else (ref['codebook'], b_m)
            tag = f'{kind.name} n{N}_d{D}_{dtype} {route}[{took.name}] step {step}'
            _report(f'{tag} loss', float(loss.detach()), want, tol)
            assert list(memo['loss'].keys()) == ['the_loss']
            _report(f'{tag} memo the_loss', float(memo['loss']['the_loss'].detach()), want, tol)
            zd = z.detach()
            assert zd.dtype == torch.float32 and torch.equal(zd, rows.float() + (w_now[quant] - rows.float())), f'{tag}: z'
            if kind.train:
                q.zero_grad(set_to_none=True)
                loss.backward()
                g = q.embedding.weight.grad
                if g is not None:
                    with torch.no_grad():
                        q.embedding.weight.add_(g, alpha=-50.0)
