"""Every backward kernel against float64 autograd of the reference, under the derived bounds of tests/backward_ref.py.

The kernels are called directly (``ops.*`` / ``train_step.vqkd_backward``) so that each form can be forced, and once per
shipped config family through the modules and autograd.  The case table, the float64 references, the tolerances and
``compare`` are those tests/test_backward_reference_cpu.py proves on the CPU (the fp32 reference stays inside, every mutation
falls outside).  Each case prints its worst err / tol (run with ``-s``); profiles/backward_parity.txt keeps one run's record.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_ref as br
from oracle import synth

pytestmark = pytest.mark.gpu

EMB = 'torch_nn_modules_sparse_Embedding'


def _dev(t):
    return None if t is None else t.cuda()


def _scalars(c):
    return [None if v is None else torch.tensor(v, dtype=torch.float32, device='cuda') for v in c.scal]


def _report(name, got, ref, tol):
    v = br.compare(got, ref, tol)
    print('\n' + v.line(name), end='')
    assert v.ok, v.line(name)
    return v


# ------------------------------------------------------------------------------------------------------------------
# vq_backward_kernel<0|1>, the ordered grad_W kernels
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', br.VQ_CASES, ids=lambda c: c.name)
def test_vq_backward(c):
    from vector_quantization_amd import ops
    inp = br.vq_inputs(c)
    gx_ref, gw_ref = br.vq_value(c, inp)
    tx, tw = br.vq_tolerance(c, inp)
    g_cb, g_cm, g_comb = _scalars(c)
    if c.ordered is None:
        assert ops.use_ordered(c.K, c.D, None, c.N, backward=True) == (c.D % 4 == 0 and c.N >= 32768)
    x, w, idx, gz = _dev(inp['x']), _dev(inp['w']), _dev(inp['idx']), _dev(inp['g_zste'])

    def run():
        return ops.vq_backward(x, w, idx, gz, g_cb, g_cm, c.need_x, c.need_w, ordered=c.ordered, g_comb=g_comb, beta=c.beta)
    gx, gw = run()
    assert (gx is None) == (not c.need_x) and (gw is None) == (not c.need_w)
    if c.need_x:
        _report(f'vq_backward {c.name} grad_x', gx, gx_ref, tx)
    if c.need_w:
        _report(f'vq_backward {c.name} grad_w', gw, gw_ref, tw)
        unused = br.vq_counts(c, inp) == 0
        assert not gw.cpu()[unused].any(), 'rows of codes no token chose must be exactly zero'
        if br.kw_signed(c) == 0:
            assert not gw.any(), 'kw == 0: grad_W must be exactly zero'
    # determinism where the design promises it: grad_x always, grad_W on the ordered route
    gx2, gw2 = run()
    if c.need_x:
        assert torch.equal(gx, gx2)
    if c.need_w and ops.use_ordered(c.K, c.D, c.ordered, c.N, backward=True):
        assert torch.equal(gw, gw2)


# ------------------------------------------------------------------------------------------------------------------
# vq_backward_map256_kernel<DT, ODT>
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', br.MAP_CASES, ids=lambda c: c.name)
def test_vq_backward_map(c):
    from vector_quantization_amd import ops
    inp = br.vq_inputs(c)
    gx_ref, _ = br.vq_value(c, inp)
    tx, _ = br.vq_tolerance(c, inp)
    B, hw = c.N // c.hw, c.hw
    assert ops.backward_map_supported(c.D, hw)
    _, g_cm, g_comb = _scalars(c)
    g_map = None if inp['g_zste'] is None else br.to_map(inp['g_zste'], c).reshape(B, c.D, 16, hw // 16).cuda()
    out = ops.vq_backward_map(_dev(inp['x']), _dev(inp['w']), _dev(inp['idx']), (B, c.D, 16, hw // 16), g_map, g_cm, g_comb, c.beta,
                              torch.bfloat16 if c.out_dtype == 'bf16' else torch.float32)
    assert out.dtype == (torch.bfloat16 if c.out_dtype == 'bf16' else torch.float32)
    _report(f'vq_backward_map {c.name}', out.reshape(B, c.D, hw), br.to_map(gx_ref, c), br.map_tolerance(c, gx_ref, tx))


@pytest.mark.parametrize('D,hw', [(48, 256), (32, 128), (30, 100)])
def test_vq_backward_map_refuses_other_shapes_and_functional_takes_the_transpose_route(D, hw):
    """The ABI refuses the shape on the host (VQHIP_EINVAL, nothing launched); functional.py goes through vq_backward and two
    transposes, and that route meets the same float64 reference."""
    from vector_quantization_amd import _lib, functional as Fn, ops
    assert not ops.backward_map_supported(D, hw)
    B, K = 2, 64
    h = 4
    c = br.VqCase(f'transpose_route_d{D}_hw{hw}', B * hw, K, D, form='map', hw=hw, tok='uniform', scal=(None, None, 1.0), seed=140)
    inp = br.vq_inputs(c)
    x, w, idx = _dev(inp['x']), _dev(inp['w']), _dev(inp['idx'])
    with pytest.raises(_lib.VqhipError) as e:
        ops.vq_backward_map(x, w, idx, (B, D, h, hw // h), None, None, torch.ones((), device='cuda'), c.beta, torch.float32)
    assert 'failed with code -22' in str(e.value) and 'HW % 256 == 0' in str(e.value)       # VQHIP_EINVAL, refused on the host
    x_map = br.to_map(inp['x'], c).reshape(B, D, h, hw // h).cuda().requires_grad_(True)
    wp = w.clone().requires_grad_(True)
    z_map, m_cb, m_cm, comb = Fn.fused_map_decode_loss(x_map, x, wp, idx, c.beta)
    g_map = br.to_map(inp['g_zste'], c).reshape(B, D, h, hw // h).cuda()
    torch.autograd.backward([z_map, comb], [g_map, torch.ones((), device='cuda')])
    gx_ref, gw_ref = br.vq_value(c, inp)
    tx, tw = br.vq_tolerance(c, inp)
    _report(f'{c.name} grad_x', x_map.grad.reshape(B, D, hw), br.to_map(gx_ref, c), br.to_map(tx, c))
    _report(f'{c.name} grad_w', wp.grad, gw_ref, tw)


# ------------------------------------------------------------------------------------------------------------------
# vqkd_backward_small_kernel<DT, 8|16|32>, vqkd_backward_kernel<DT>
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', br.KD_CASES, ids=lambda c: c.name)
def test_vqkd_backward(c):
    from vector_quantization_amd import ops, train_step
    inp = br.kd_inputs(c)
    ref = br.kd_value(c, inp)
    x = _dev(inp['x'])
    xn = ops.normalize_rows(x)                                  # as in the product
    g = inp['g_zste']
    if inp['g_xn'] is not None:                                 # what _VqkdStep.backward forms: g_zste + g_xn (either may be absent)
        g = inp['g_xn'] if g is None else g + inp['g_xn']
    g_loss = None if inp['g_loss'] is None else torch.tensor(inp['g_loss'], device='cuda')
    gx = train_step.vqkd_backward(x, xn, _dev(inp['w']), _dev(inp['idx']), _dev(g), g_loss)
    tol = br.kd_tolerance(c, inp)
    if inp['g_zste'] is not None and inp['g_xn'] is not None:   # the host-side fp32 sum g_zste + g_xn: one more rounding
        tol = tol * (br.vqkd_count(c.D) + 1) / br.vqkd_count(c.D)
    _report(f'vqkd_backward {c.name}', gx, ref, tol)
    assert torch.equal(gx, train_step.vqkd_backward(x, xn, _dev(inp['w']), _dev(inp['idx']), _dev(g), g_loss))


# ------------------------------------------------------------------------------------------------------------------
# normalize_bwd_kernel<0|1>, diff_kernel<DTA, DTB>, ste_kernel<DT>
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', br.NB_CASES, ids=lambda c: c.name)
def test_normalize_rows_bwd(c):
    from vector_quantization_amd import ops
    inp = br.nb_inputs(c)
    gv = ops.normalize_rows_bwd(_dev(inp['v']), _dev(inp['g']))
    _report(f'normalize_rows_bwd {c.name}', gv, br.nb_value(inp), br.nb_tolerance(c, inp))


@pytest.mark.parametrize('c', br.EL_CASES, ids=lambda c: c.name)
def test_elementwise(c):
    from vector_quantization_amd import ops
    inp = br.el_inputs(c)
    ref, tol = br.el_values(inp), br.el_tolerances(c, inp)
    a, b = _dev(inp['a']), _dev(inp['b'])
    sd = torch.tensor(br.EL_SCALE_DEV, device='cuda')
    _report(f'diff_scale {c.name}', ops.diff_scale(a, b, br.EL_SCALE, sd), ref['diff'], tol['diff'])
    _report(f'sse {c.name}', ops.sse(a, b), ref['sse'], tol['sse'])
    if c.db == 'f32':                                          # ste_kernel: z is fp32, x fp32 or bf16
        _report(f'ste {c.name}', ops.ste(a, b), ref['ste'], tol['ste'])
    # without scale_dev: the host scalar alone
    plain = (inp['a'].double() - inp['b'].double()) * br.EL_SCALE
    _report(f'diff_scale(no scale_dev) {c.name}', ops.diff_scale(a, b, br.EL_SCALE), plain, tol['diff'])


# ------------------------------------------------------------------------------------------------------------------
# the normalised tail as _VqStep chains it: normalize_rows -> vq_backward -> (+ g_xn) -> normalize_rows_bwd
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', br.NORM_CASES, ids=lambda c: c.name)
def test_normalised_tail_through_the_autograd_node(c):
    from vector_quantization_amd import functional as Fn, ops
    inp = br.vq_inputs(c)
    gx_ref, gw_ref = br.vq_value(c, inp)
    tx, tw = br.vq_tolerance(c, inp)
    x = _dev(inp['x']).requires_grad_(True)
    w = _dev(inp['w']).requires_grad_(True)
    idx = _dev(inp['idx'])
    xn = ops.normalize_rows(x.detach())
    _, z_ste, mse = ops.gather_ste_mse(xn, w.detach(), idx, beta=c.beta)
    done = Fn._Computed(xn=xn, idx=idx, z_ste=z_ste, mse=mse)
    xn_out, zs, m_cb, m_cm, comb = Fn.vq_step(x, w, done, c.beta)
    outs, grads = [], []
    for t, g in ((zs, inp['g_zste']), (xn_out, inp['g_xn'])):
        if g is not None:
            outs.append(t)
            grads.append(g.cuda().to(t.dtype))
    for t, v in zip((m_cb, m_cm, comb), c.scal):
        if v is not None:
            outs.append(t)
            grads.append(torch.tensor(v, device='cuda'))
    torch.autograd.backward(outs, grads)
    if c.dtype == 'bf16':                                       # the node returns the latents' gradient in their dtype: one bf16 rounding
        tx = tx + br.half_bf16_ulp(gx_ref.abs() + tx)
    _report(f'_VqStep {c.name} grad_x', x.grad, gx_ref, tx)
    _report(f'_VqStep {c.name} grad_w', w.grad, gw_ref, tw)


# ------------------------------------------------------------------------------------------------------------------
# autograd glue on the modules
# ------------------------------------------------------------------------------------------------------------------

def _build(cfg, w, one_call=None, train=True):
    from vector_quantization_amd import Config, build_quantizer
    q = build_quantizer(cfg)
    q.train(train)
    q.init_weights(Config(type='vqgan') if cfg['type'] == 'VQGANQuantizer' else Config())
    q = q.cuda()
    q._forward_pre_hooks.clear()
    with torch.no_grad():
        q.embedding.weight.copy_(torch.from_numpy(w))
    if one_call is not None:
        q.one_call_steps = one_call
    return q


def _vq_cfg(K, D, dist='L2', callbacks=(), **extra):
    return dict(type='VQGANQuantizer', embedding=dict(type=EMB, num_embeddings=K, embedding_dim=D), distance=dict(type=f'{dist}Distance'),
                losses=dict(vqgan_loss=dict(type='VQGANLoss')), callbacks=list(callbacks), **extra)


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('N,D,dtype', [(777, 256, 'bf16'), (1001, 30, 'f32')])
@pytest.mark.parametrize('mix', ['loss', 'commensurate', 'z_only'])
def test_vqgan_module_gradients(fused, N, D, dtype, mix):
    """VQGANQuantizer, fused and op by op: only the loss back-propagated (no gradient for z), both, and only z (no gradient
    for the loss) — the set_materialize_grads(False) branches of the autograd nodes."""
    K = 64
    x_np, w_np = synth.make_inputs('normal', 900, N, K, D)
    q = _build(_vq_cfg(K, D, fused=fused), w_np)
    x0 = br.to_dtype(x_np, dtype)
    xd = x0.cuda().requires_grad_(True)
    z, loss, memo = q(xd, {})
    c = br.VqCase(f'vqgan_fused{int(fused)}_d{D}_{dtype}_{mix}', N, K, D, dtype, mix='commensurate' if mix == 'z_only' else mix,
                  scal=(None, None, None if mix == 'z_only' else 1.0), seed=900)
    gz = br.upstream(c.mix, 911, N, D)
    inp = dict(x=x0, w=torch.from_numpy(w_np), idx=memo['quant'].cpu(), g_zste=None if gz is None else torch.from_numpy(gz), g_xn=None)
    outs = [t for t, use in ((loss, mix != 'z_only'), (z, gz is not None)) if use]
    grads = [g for g, use in ((torch.ones((), device='cuda'), mix != 'z_only'), (None if gz is None else torch.from_numpy(gz).cuda().to(z.dtype), gz is not None)) if use]
    torch.autograd.backward(outs, grads)
    gx_ref, gw_ref = br.vq_value(c, inp)
    tx, tw = br.vq_tolerance(c, inp)
    if dtype == 'bf16' and not fused and mix == 'commensurate':
        # op by op, every node returns its gradient in the latents' dtype as the reference's ops do: the straight-through term
        # and the commitment term are each rounded to bf16 and autograd adds them in bf16 — three roundings
        ste_part = inp['g_zste'].double()
        tx = tx + br.half_bf16_ulp(ste_part) + br.half_bf16_ulp((gx_ref - ste_part).abs() + tx)
    if dtype == 'bf16':                                         # the latents' gradient is returned in their dtype: one bf16 rounding
        tx = tx + br.half_bf16_ulp(gx_ref.abs() + tx)
    # op by op (fused=False): diff_kernel per loss term (3 roundings, one more for beta) and autograd's accumulation of the
    # terms (2): 6, inside the same count of 8
    _report(f'{c.name} grad_x', xd.grad, gx_ref, tx)
    gw = q.embedding.weight.grad
    if mix == 'z_only':
        assert gw is None or not gw.any()
    else:
        _report(f'{c.name} grad_w', gw, gw_ref, tw)


@pytest.mark.parametrize('one_call', [True, False])
@pytest.mark.parametrize('mix', ['loss', 'commensurate'])
def test_normalize_callback_with_a_second_consumer_of_the_normalised_rows(one_call, mix):
    """NormalizeCallback (LlamaGen shape): memo['x'] = F.normalize(x) feeds a second consumer, whose gradient g_xn must reach x."""
    N, K, D = 1500, 128, 8
    x_np, w_np = synth.make_inputs('normal', 920, N, K, D)
    q = _build(_vq_cfg(K, D, callbacks=[dict(type='NormalizeCallback')]), w_np, one_call=one_call)
    xd = torch.from_numpy(x_np).cuda().requires_grad_(True)
    z, loss, memo = q(xd, {})
    assert (q._one_call_step(xd) is not None) == one_call
    c = br.VqCase(f'normalize_callback_onecall{int(one_call)}_{mix}', N, K, D, mix=mix, scal=(None, None, 1.0), form='norm', g_xn=True, seed=920)
    gz = br.upstream(mix, 921, N, D)
    gxn = (synth.normal(923, N, D) * np.float32(2.0 / (N * D))).astype(np.float32)
    outs, grads = [loss, memo['x']], [torch.ones((), device='cuda'), torch.from_numpy(gxn).cuda()]
    if gz is not None:
        outs.append(z)
        grads.append(torch.from_numpy(gz).cuda())
    torch.autograd.backward(outs, grads)
    # the module decodes from F.normalize(w): the float64 reference normalises the codebook itself, and the fp32 rows the
    # kernel read carry tree/2 + 2 more roundings in z
    wn = F.normalize(torch.from_numpy(w_np).double())
    inp = dict(x=torch.from_numpy(x_np), w=wn, idx=memo['quant'].cpu(), g_zste=None if gz is None else torch.from_numpy(gz),
               g_xn=torch.from_numpy(gxn))
    gx_ref, _ = br.vq_value(c, inp)
    tx, _ = br.vq_tolerance(c, inp)
    extra = br.tree(D) / 2 + 2
    _report(f'{c.name} grad_x', xd.grad, gx_ref, tx * (br.vq_norm_count(D) + extra) / br.vq_norm_count(D))


@pytest.mark.parametrize('mix', ['loss', 'commensurate'])
def test_vqkd_one_call_with_a_second_consumer_of_the_normalised_rows(mix):
    N, K, D = 2048, 64, 32
    x_np, w_np = synth.make_inputs('normal', 930, N, K, D)
    cfg = dict(type='VQKDQuantizer', embedding=dict(type=EMB, num_embeddings=K, embedding_dim=D), distance=dict(type='CosineDistance'),
               callbacks=[dict(type='VQKDCallback', ema=dict())], losses=dict(commitment_loss=dict(type='CommitmentLoss', mse=dict(norm=True))))
    q = _build(cfg, synth.unit_rows(w_np), one_call=True)
    xd = torch.from_numpy(x_np).cuda().requires_grad_(True)
    assert q._one_call_step(xd) is not None
    z, loss, memo = q(xd, {})
    c = br.KdCase(f'vqkd_module_{mix}', N, D, mix=mix, g_xn=True, K=K)
    gz = br.upstream(mix, 931, N, D)
    gxn = (synth.normal(933, N, D) * np.float32(2.0 / (N * D))).astype(np.float32)
    outs, grads = [loss, memo['x']], [torch.ones((), device='cuda'), torch.from_numpy(gxn).cuda()]
    if gz is not None:
        outs.append(z)
        grads.append(torch.from_numpy(gz).cuda())
    torch.autograd.backward(outs, grads)
    inp = dict(x=torch.from_numpy(x_np), w=q.embedding.weight.detach().cpu(), idx=memo['quant'].cpu(),      # decoded from the UPDATED codebook
               g_zste=None if gz is None else torch.from_numpy(gz), g_xn=torch.from_numpy(gxn), g_loss=1.0, zero_rows=(), tiny_rows=())
    tol = br.kd_tolerance(c, inp) * (br.vqkd_count(D) + 1) / br.vqkd_count(D)                                 # g_zste + g_xn on the host side
    _report(f'{c.name} grad_x', xd.grad, br.kd_value(c, inp), tol)
    assert q.embedding.weight.grad is None or not q.embedding.weight.grad.any()


@pytest.mark.parametrize('mix', ['loss', 'commensurate'])
def test_cvq_one_call_gradients(mix):
    N, K, D = 1200, 64, 64
    x_np, w_np = synth.make_inputs('normal', 940, N, K, D)
    q = _build(_vq_cfg(K, D, callbacks=[dict(type='CVQVAECallback', ema=dict(), anchor=dict(type='NearestAnchor'))]), w_np, one_call=True)
    xd = torch.from_numpy(x_np).cuda().requires_grad_(True)
    assert q._one_call_step(xd) is not None
    z, loss, memo = q(xd, {})
    c = br.VqCase(f'cvq_module_{mix}', N, K, D, mix=mix, scal=(None, None, 1.0), seed=940)
    gz = br.upstream(mix, 941, N, D)
    outs, grads = [loss], [torch.ones((), device='cuda')]
    if gz is not None:
        outs.append(z)
        grads.append(torch.from_numpy(gz).cuda())
    torch.autograd.backward(outs, grads)
    inp = dict(x=torch.from_numpy(x_np), w=q.embedding.weight.detach().cpu(), idx=memo['quant'].cpu(),      # decoded from the UPDATED codebook
               g_zste=None if gz is None else torch.from_numpy(gz), g_xn=None)
    gx_ref, gw_ref = br.vq_value(c, inp)
    tx, tw = br.vq_tolerance(c, inp)
    _report(f'{c.name} grad_x', xd.grad, gx_ref, tx)
    _report(f'{c.name} grad_w', q.embedding.weight.grad, gw_ref, tw)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('mix', ['loss', 'commensurate'])
def test_tokenization_quantize_on_an_nchw_map(dtype, mix):
    from vector_quantization_amd import tokenization as T
    B, D, H, W, K = 3, 64, 16, 16, 128
    N = B * H * W
    x_np, w_np = synth.make_inputs('normal', 950, N, K, D)
    q = _build(_vq_cfg(K, D), w_np)
    c = br.VqCase(f'quantize_map_{dtype}_{mix}', N, K, D, dtype, mix=mix, scal=(None, None, 1.0), form='map', hw=H * W,
                  out_dtype=dtype, seed=950)
    x0 = br.to_dtype(x_np, dtype)
    x_map = br.to_map(x0, c).reshape(B, D, H, W).cuda().requires_grad_(True)
    z, loss, memo = T.quantize(q, x_map, {})
    gz = br.upstream(mix, 951, N, D)
    outs, grads = [loss], [torch.ones((), device='cuda')]
    if gz is not None:
        gz = torch.from_numpy(gz).to(z.dtype)                   # the upstream gradient arrives in the map's dtype: exact from here on
        outs.append(z)
        grads.append(br.to_map(gz, c).reshape(B, D, H, W).cuda())
    torch.autograd.backward(outs, grads)
    inp = dict(x=x0, w=torch.from_numpy(w_np), idx=memo['quantizer']['quant'].reshape(-1).cpu(),
               g_zste=None if gz is None else gz.float(), g_xn=None)
    gx_ref, gw_ref = br.vq_value(c, inp)
    tx, tw = br.vq_tolerance(c, inp)
    _report(f'{c.name} grad_map', x_map.grad.reshape(B, D, H * W), br.to_map(gx_ref, c), br.map_tolerance(c, gx_ref, tx))
    _report(f'{c.name} grad_w', q.embedding.weight.grad, gw_ref, tw)
