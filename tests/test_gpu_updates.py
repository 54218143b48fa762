"""Every codebook-update kernel against the float64 reference, under the derived bounds of tests/update_ref.py, off the defaults.

The kernels are called directly (``ops.*``) so that every form, stage and route is reached at the shapes where a wave-per-code
kernel can go wrong (D tails, K that is no multiple of a block's codes, the three paths of ``cvq_rows_kernel``) and at values
the fixtures never hold (g and eps off their defaults, empty and overfull codes, counts above 2^24, zero sums and rows, p in
{0, subnormal, threshold, 1, NaN}, rows at 2^60 and 2^-60).  The case table, the references, the tolerances and ``compare`` are
those tests/test_update_reference_cpu.py proves on the CPU.  Each case prints its worst err / tol (run with ``-s``);
profiles/update_parity.txt keeps one run's record.
"""
import numpy as np
import pytest
import torch

import update_ref as ur
from oracle import synth

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _report(name, got, ref, tol):
    v = ur.compare(got, ref, tol)
    print('\n' + v.line(name), end='')
    assert v.ok, v.line(name)
    return v


def _check_cvq(name, inp, got_w, got_p, ref, tol, nan_w=True):
    """p' and w' under their bounds; a NaN p gives a NaN p' and (where the codebook stage ran) a NaN row, and no other row."""
    nan = ur.nan_codes(inp['p'])
    gw, gp = got_w.detach().cpu().clone(), got_p.detach().cpu().clone()
    if bool(nan.any()):
        assert bool(torch.isnan(gp[nan]).all()), f'{name}: a NaN p must stay NaN'
        gp[nan] = ref['p'][nan].float()
        if nan_w:
            assert bool(torch.isnan(gw[nan]).all()), f'{name}: a NaN p must give a NaN row'
            gw[nan] = ref['w'][nan].float()
    _report(f'{name} p', gp, ref['p'], tol['p'])
    _report(f'{name} w', gw, ref['w'], tol['w'])


# ------------------------------------------------------------------------------------------------------------------
# vqkd_update_kernel
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', ur.KD_CASES, ids=lambda c: c.name)
def test_vqkd_update(c):
    from vector_quantization_amd import ops
    inp = ur.kd_inputs(c)
    hist, sums = inp['hist'].cuda(), inp['sums'].cuda()
    for mode in ('full', 'centroid'):
        w = inp['w'].cuda().clone()
        ops.vqkd_update_(w, hist, sums, ur.f32(c.g), mode=mode)
        ref = ur.kd_reference(inp['w'], inp['hist'], inp['sums'], c.g, mode)
        _report(f'vqkd_update_ {c.name} {mode}', w, ref, ur.kd_tolerance(inp['w'], inp['hist'], inp['sums'], c.g, mode))
        if mode == 'centroid':                         # a code without a token keeps its row bit for bit
            empty = inp['hist'] == 0
            assert torch.equal(w.cpu()[empty], inp['w'][empty])


# ------------------------------------------------------------------------------------------------------------------
# cvq_update_kernel (stages, numel as an int and on the device), cvq_decay_kernel
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', ur.CVQ_CASES, ids=lambda c: c.name)
def test_cvq_update_stages_and_decay(c):
    from vector_quantization_amd import ops
    inp = ur.cvq_inputs(c)
    r0 = inp['ranks'][0]
    anchors = r0['x'][r0['col']].contiguous()
    col = torch.arange(c.K)
    g, eps = ur.f32(c.g), ur.f32(c.eps)
    hist = inp['hist'].cuda()
    for stage in (1, 2, 3):
        ref = ur.cvq_reference(inp['w'], inp['p'], inp['hist'], inp['numel'], anchors, col, c.g, c.eps, stage=stage)
        tol = ur.cvq_tolerance(inp['w'], inp['p'], inp['hist'], inp['numel'], anchors.double().abs(), c.g, c.eps, stage=stage)
        for on_device in (False, True):
            w, p = inp['w'].cuda().clone(), inp['p'].cuda().clone()
            numel = torch.tensor(inp['numel'], dtype=torch.int64, device='cuda') if on_device else inp['numel']
            ops.cvq_update_(w, p, hist if stage & 1 else None, numel if stage & 1 else None, anchors.cuda() if stage & 2 else None,
                            g, eps, stage=stage)
            _check_cvq(f'cvq_update_ {c.name} stage={stage} numel_dev={on_device}', inp, w, p, ref, tol, nan_w=bool(stage & 2))
            if stage == 1:
                assert torch.equal(w.cpu(), inp['w'])
            if stage == 2:
                assert torch.equal(torch.nan_to_num(p.cpu(), nan=-1.0), torch.nan_to_num(inp['p'], nan=-1.0))
    ref2 = ur.cvq_reference(inp['w'], inp['p'], inp['hist'], inp['numel'], anchors, col, c.g, c.eps, stage=2)
    tol2 = ur.cvq_tolerance(inp['w'], inp['p'], inp['hist'], inp['numel'], anchors.double().abs(), c.g, c.eps, stage=2)
    decay = ops.cvq_decay(inp['p'].cuda(), c.K, g, eps).cpu()
    nan = ur.nan_codes(inp['p'])
    assert bool(torch.isnan(decay[nan]).all())
    decay[nan] = ref2['decay'][nan].float()
    _report(f'cvq_decay {c.name}', decay, ref2['decay'], tol2['decay'])


# ------------------------------------------------------------------------------------------------------------------
# cvq_step_kernel<DT>
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', ur.CVQ_CASES, ids=lambda c: c.name)
def test_cvq_step(c):
    from vector_quantization_amd import ops
    inp = ur.cvq_inputs(c)
    r0 = inp['ranks'][0]
    hist64 = r0['hist32'].to(torch.int64)
    g, eps = ur.f32(c.g), ur.f32(c.eps)
    for bf16 in (False, True):
        x = r0['x'].bfloat16() if bf16 else r0['x']
        xf = x.float()
        ref = ur.cvq_reference(inp['w'], inp['p'], hist64, c.N, xf, r0['col'], c.g, c.eps)
        tol = ur.cvq_tolerance(inp['w'], inp['p'], hist64, c.N, xf[r0['col']].double().abs(), c.g, c.eps)
        for aliased in (False, True):
            w_in, p_in = inp['w'].cuda().clone(), inp['p'].cuda().clone()
            w_out = w_in if aliased else torch.full_like(w_in, 7.0)
            p_out = p_in if aliased else torch.full_like(p_in, 7.0)
            ops.cvq_step(w_in, w_out, p_in, p_out, r0['hist32'].cuda(), c.N, x.cuda(), r0['col'].cuda(), g, eps)
            _check_cvq(f'cvq_step {c.name} bf16={bf16} aliased={aliased}', inp, w_out, p_out, ref, tol)
            if not aliased:
                assert torch.equal(w_in.cpu(), inp['w'])


# ------------------------------------------------------------------------------------------------------------------
# cvq_update_rows_kernel: listed rows, out-of-range rows among them
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', ur.CVQ_CASES, ids=lambda c: c.name)
def test_cvq_update_rows_drops_rows_out_of_range(c):
    from vector_quantization_amd import ops
    inp = ur.cvq_inputs(c)
    K, D = c.K, c.D
    valid = torch.arange(0, K, 2) if K > 1 else torch.zeros(1, dtype=torch.int64)
    rows = torch.cat([torch.tensor([-1, K]), valid, torch.tensor([K + 5, -7, 2 ** 40])])
    perm = torch.from_numpy(synth.rng(c.seed + 9).permutation(rows.numel()))
    rows = rows[perm]
    sub = torch.from_numpy(synth.rng(c.seed + 10).standard_normal((rows.numel(), D), dtype=np.float32))
    w = inp['w'].cuda().clone()
    ops.cvq_update_rows_(w, inp['p'].cuda(), rows.cuda(), sub.cuda(), ur.f32(c.g), ur.f32(c.eps))
    ok = (rows >= 0) & (rows < K)
    col = torch.zeros(K, dtype=torch.int64)
    col[rows[ok]] = torch.nonzero(ok).reshape(-1)
    ref = ur.cvq_reference(inp['w'], inp['p'], inp['hist'], inp['numel'], sub, col, c.g, c.eps, stage=2)
    tol = ur.cvq_tolerance(inp['w'], inp['p'], inp['hist'], inp['numel'], sub[col].double().abs(), c.g, c.eps, stage=2)
    touched = torch.zeros(K, dtype=torch.bool)
    touched[rows[ok]] = True
    got = w.cpu()
    assert torch.equal(got[~touched], inp['w'][~touched]), 'a code that is not listed, or a row out of range, changed the codebook'
    nan = ur.nan_codes(inp['p']) & touched
    assert bool(torch.isnan(got[nan]).all())
    keep = touched & ~nan
    _report(f'cvq_update_rows_ {c.name}', got[keep], ref['w'][keep], tol['w'][keep])


# ------------------------------------------------------------------------------------------------------------------
# cvq_apply_kernel<DT, PACKED>, cvq_pack_kernel, pack_counts / unpack_counts
# ------------------------------------------------------------------------------------------------------------------

def _slots(K, seed):
    """Two codes in three are listed: slot[k] = position in the list or -1."""
    listed = torch.from_numpy(synth.rng(seed).random(K) < 0.67) if K > 1 else torch.ones(1, dtype=torch.bool)
    slot = torch.full((K,), -1, dtype=torch.int32)
    slot[listed] = torch.arange(int(listed.sum()), dtype=torch.int32)
    return slot, int(listed.sum())


def _caps(M, K):
    """A capacity above the list length and one below it."""
    return sorted({min(K, M + 3), M // 2})


def _apply_reference(c, inp, slot, cap, payload, hist, numel, world):
    """``payload`` [cap, D]: the anchor (sum) of every slot below the capacity; other codes blend with nothing (w * decay)."""
    ext = torch.cat([payload.float(), torch.zeros(1, c.D)])
    s = slot.to(torch.int64)
    col = torch.where((s >= 0) & (s < cap), s, torch.full_like(s, cap))
    ref = ur.cvq_reference(inp['w'], inp['p'], hist, numel, ext, col, c.g, c.eps, world)
    tol = ur.cvq_tolerance(inp['w'], inp['p'], hist, numel, ext[col].double().abs() / world, c.g, c.eps, c_anchor=int(world > 1))
    return ref, tol


@pytest.mark.parametrize('c', ur.CVQ_CASES, ids=lambda c: c.name)
def test_cvq_apply_one_rank(c):
    from vector_quantization_amd import ops
    inp = ur.cvq_inputs(c)
    r0 = inp['ranks'][0]
    slot, M = _slots(c.K, c.seed + 20)
    hist64 = r0['hist32'].to(torch.int64)
    for cap in _caps(M, c.K):
        col_list = r0['col'][:max(cap, 1)].contiguous()                  # col_list[s]: the latent row of slot s
        for bf16 in (False, True):
            x = r0['x'].bfloat16() if bf16 else r0['x']
            payload = x.float()[col_list][:cap]
            ref, tol = _apply_reference(c, inp, slot, cap, payload, hist64, c.N, 1)
            for aliased in (False, True):
                w_in, p_in = inp['w'].cuda().clone(), inp['p'].cuda().clone()
                w_out = w_in if aliased else torch.full_like(w_in, 7.0)
                p_out = p_in if aliased else torch.full_like(p_in, 7.0)
                ops.cvq_apply(w_in, w_out, p_in, p_out, slot.cuda(), ur.f32(c.g), ur.f32(c.eps), hist32=r0['hist32'].cuda(), numel=c.N,
                              x=x.cuda(), col_idx=col_list.cuda(), cap=cap)
                _check_cvq(f'cvq_apply {c.name} cap={cap}/{M} bf16={bf16} aliased={aliased}', inp, w_out, p_out, ref, tol)


@pytest.mark.parametrize('world', [1, 3])
@pytest.mark.parametrize('c', ur.CVQ_CASES, ids=lambda c: c.name)
def test_cvq_apply_packed(c, world):
    """world = 3: three ``ops.cvq_pack`` buffers from three latent sets, summed as the all-reduce would; world = 1: the header
    from ``ops.pack_counts`` on the int64 histogram (counts of 2^24 + 1 and 2^40 included) next to rank 0's anchors.  The summed
    header comes back exactly through ``ops.unpack_counts``."""
    from vector_quantization_amd import ops
    inp = ur.cvq_inputs(c)
    K, D = c.K, c.D
    slot, M = _slots(K, c.seed + 20)
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    for cap in _caps(M, K):
        if world == 1:
            hist, numel = inp['hist'], inp['numel']
            r0 = inp['ranks'][0]
            packed = torch.zeros(ops.pack_floats(K, cap, D), dtype=torch.float32, device='cuda')
            assert packed.numel() == 2 * K + 4 + cap * D
            ops.pack_counts(hist.cuda(), numel, packed)
            rows = r0['x'][r0['col'][:cap]].clone()
            rows[M:] = 0.0
            packed[2 * K + 4:] = rows.reshape(-1).cuda()
        else:
            hist = sum(r['hist32'].to(torch.int64) for r in inp['ranks'])
            numel = 3 * c.N
            bufs = [ops.cvq_pack(r['hist32'].cuda(), c.N, r['x'].cuda(), r['col'][:max(cap, 1)].contiguous().cuda(), count, cap, K)
                    for r in inp['ranks']]
            packed = (bufs[0] + bufs[1]) + bufs[2]
        assert packed.numel() == 2 * K + 4 + cap * D
        back = ops.unpack_counts(packed, K).cpu()
        assert torch.equal(back[:K], hist) and int(back[K]) == numel
        assert torch.equal(back, ur.unpack_header(packed.cpu(), K))
        payload = packed[2 * K + 4:].reshape(cap, D).cpu()
        assert not payload[M:].any(), 'payload rows past the count must be zero'
        ref, tol = _apply_reference(c, inp, slot, cap, payload, hist, numel, world)
        for aliased in (False, True):
            w_in, p_in = inp['w'].cuda().clone(), inp['p'].cuda().clone()
            w_out = w_in if aliased else torch.full_like(w_in, 7.0)
            p_out = p_in if aliased else torch.full_like(p_in, 7.0)
            ops.cvq_apply(w_in, w_out, p_in, p_out, slot.cuda(), ur.f32(c.g), ur.f32(c.eps), packed=packed, world=world, cap=cap)
            _check_cvq(f'cvq_apply packed {c.name} world={world} cap={cap}/{M} aliased={aliased}', inp, w_out, p_out, ref, tol)


def test_pack_counts_header_is_the_restated_one():
    from vector_quantization_amd import ops
    hist = torch.tensor([0, 1, 65535, 65536, ur.BIG_A, ur.BIG_B, 3], dtype=torch.int64)
    numel = 2 ** 41 + 5
    packed = torch.full((2 * 7 + 4,), 9.0, device='cuda')
    ops.pack_counts(hist.cuda(), numel, packed)
    assert torch.equal(packed.cpu(), ur.pack_header(hist, numel))
    h32 = torch.tensor([0, 1, 65535, 65536, 2 ** 31 - 1], dtype=torch.int32)
    packed = torch.full((2 * 5 + 4,), 9.0, device='cuda')
    ops.pack_counts(h32.cuda(), 70001, packed)
    assert torch.equal(packed.cpu(), ur.pack_header(h32, 70001))
    assert torch.equal(ops.unpack_counts(packed, 5).cpu(), torch.cat([h32.to(torch.int64), torch.tensor([70001])]))


# ------------------------------------------------------------------------------------------------------------------
# cvq_rows_kernel: the listed set
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K,g,eps', ur.ROWS_SETTINGS)
def test_cvq_rows_listed_set(K, g, eps):
    from vector_quantization_amd import ops
    p = ur.rows_p(K, g, eps)
    pd = p.cuda()
    gf, ef = ur.f32(g), ur.f32(eps)
    rows, slot, count = ops.cvq_rows(pd, K, gf, ef)
    cnt = int(count.item())
    rows, slot = rows.cpu()[:cnt].to(torch.int64), slot.cpu().to(torch.int64)
    # structure
    assert 0 <= cnt <= K and bool((rows >= 0).all()) and bool((rows < K).all())
    assert bool((rows[1:] > rows[:-1]).all()), 'rows[:count] must be ascending'
    want = torch.full((K,), -1, dtype=torch.int64)
    want[rows] = torch.arange(cnt)
    assert torch.equal(slot, want) and cnt == int((slot >= 0).sum())
    is_listed = slot >= 0
    # soundness: whatever the histogram adds, an unlisted code ends with decay == 1.0f exactly (the update's own kernels)
    N = ur.ROWS_N
    w = torch.zeros(K, 1, device='cuda')
    p_freq0 = None
    for name, h in (('0', 0), ('1/N', 1), ('1', N)):
        p2 = pd.clone()
        ops.cvq_update_(w, p2, torch.full((K,), h, dtype=torch.int64, device='cuda'), N, None, gf, ef, stage=1)
        decay = ops.cvq_decay(p2, K, gf, ef).cpu()
        assert bool((decay[~is_listed] == 1.0).all()), f'freq={name}: an unlisted code has decay != 1'
        if h == 0:
            p_freq0 = p2.cpu()
    # NaN / negative p listed, agreement with the float64 predicate outside the band, the margin to 2^-25
    print('\n' + ur.check_listed_set(p, K, g, eps, is_listed, p_freq0), end='')


# ------------------------------------------------------------------------------------------------------------------
# module level, off the defaults: the shipped configs with ema.decay = 0.9 and eps = 1e-2 on every eager route
# ------------------------------------------------------------------------------------------------------------------

EMB = 'torch_nn_modules_sparse_Embedding'
MOD_K, MOD_D, MOD_N, MOD_G, MOD_EPS = 512, 32, 1500, 0.9, 1e-2


def _build(cfg, w):
    from vector_quantization_amd import Config, build_quantizer
    q = build_quantizer(cfg)
    q.train(True)
    q.init_weights(Config(type='vqgan') if cfg['type'] == 'VQGANQuantizer' else Config())
    q = q.cuda()
    q._forward_pre_hooks.clear()
    with torch.no_grad():
        q.embedding.weight.copy_(torch.from_numpy(w))
    for p in q.parameters():
        p.requires_grad_(False)
    return q


def _module_batches(w0, seed):
    g = synth.rng(seed)
    return [torch.from_numpy(g.standard_normal((MOD_N, MOD_D), dtype=np.float32) * np.float32(0.3)
                             + w0[g.integers(0, MOD_K // 8, MOD_N)]).cuda() for _ in range(3)]


@pytest.mark.parametrize('dist', ['L2', 'Cosine'])
def test_cvq_module_off_the_defaults_on_every_eager_route(dist):
    w0 = synth.unit_rows(synth.rng(51).standard_normal((MOD_K, MOD_D), dtype=np.float32))
    xs = _module_batches(w0, 52)
    routes = {(True, None): 'one_call_cvq', (False, None): 'fused_tail', (False, False): 'fused_tail', (True, False): 'fused_tail'}
    states = []
    for (one_call, sparse), route in routes.items():
        cfg = dict(type='VQGANQuantizer', embedding=dict(type=EMB, num_embeddings=MOD_K, embedding_dim=MOD_D),
                   distance=dict(type=f'{dist}Distance'), losses=dict(vqgan_loss=dict(type='VQGANLoss')),
                   callbacks=[dict(type='CVQVAECallback', ema=dict(decay=MOD_G), eps=MOD_EPS, sparse_anchors=sparse,
                                   anchor=dict(type='NearestAnchor'))])
        q = _build(cfg, w0)
        q.one_call_steps = one_call
        rec = []
        for step, x in enumerate(xs):
            w_old, p_old = q.embedding.weight.detach().cpu().clone(), q.get_buffer('_probability').cpu().clone()
            with torch.no_grad():
                _, _, memo = q(x, {})
            assert q.last_route.name == route, q.last_route
            if sparse is False:
                assert 'sparse_anchors=False' in q.last_route.why or not one_call, q.last_route
            quant = memo['quant'].reshape(-1).cpu()
            col = memo['encode']['distance'].argmin(0).cpu()             # the kernel's own column argmin of this step
            hist = torch.bincount(quant, minlength=MOD_K)
            xc = x.cpu()
            ref = ur.cvq_reference(w_old, p_old, hist, MOD_N, xc, col, MOD_G, MOD_EPS)
            tol = ur.cvq_tolerance(w_old, p_old, hist, MOD_N, xc[col].double().abs(), MOD_G, MOD_EPS)
            w_new, p_new = q.embedding.weight.detach().cpu().clone(), q.get_buffer('_probability').cpu().clone()
            name = f'CVQ module {dist} one_call={one_call} sparse_anchors={sparse} step {step}'
            _report(f'{name} p', p_new, ref['p'], tol['p'])
            _report(f'{name} w', w_new, ref['w'], tol['w'])
            assert bool((ref['decay'] < 0.999).any()) and ur.not_vacuous(ref['w'], tol['w'])
            rec.append((quant, w_new, p_new))
        states.append(rec)
    for other in states[1:]:                                             # the routes stay bit-identical, as at the defaults
        for (qa, wa, pa), (qb, wb, pb) in zip(states[0], other):
            assert torch.equal(qa, qb) and torch.equal(wa, wb) and torch.equal(pa, pb)


def test_vqkd_module_off_the_defaults_on_both_eager_routes():
    import torch.nn.functional as F
    w0 = synth.unit_rows(synth.rng(53).standard_normal((MOD_K, MOD_D), dtype=np.float32))
    xs = _module_batches(w0, 54)
    tokens = []
    for one_call, route in ((True, 'one_call_vqkd'), (False, 'hooks')):
        cfg = dict(type='VQKDQuantizer', embedding=dict(type=EMB, num_embeddings=MOD_K, embedding_dim=MOD_D),
                   distance=dict(type='CosineDistance'), callbacks=[dict(type='VQKDCallback', ema=dict(decay=MOD_G))],
                   losses=dict(commitment_loss=dict(type='CommitmentLoss', mse=dict(norm=True))))
        q = _build(cfg, w0)
        q.one_call_steps = one_call
        for step, x in enumerate(xs):
            with torch.no_grad():
                _, _, memo = q(x, {})
            assert q.last_route.name == route, q.last_route
            quant = memo['quant'].reshape(-1).cpu()
            xn = memo['x'].detach().cpu()                                # the rows the encode saw (normalised once, fp32)
            e0 = memo['encode']['distance'].operands[1].detach().cpu()   # the codebook the encode ran against: the update's input
            hist = torch.bincount(quant, minlength=MOD_K)
            x2 = F.normalize(xn.double())                                # callbacks.py:124 normalises the rows again
            sums = torch.zeros(MOD_K, MOD_D, dtype=F64).index_add_(0, quant, x2)
            a_sums = torch.zeros(MOD_K, MOD_D, dtype=F64).index_add_(0, quant, x2.abs())
            # the kernel's sums: fp32 rows out of normalize_rows (tree/2 + 2), at most m additions in any order
            tol_sums = (hist.double().reshape(-1, 1) + ur.tree(MOD_D) / 2 + 2) * ur.U * a_sums
            ref = ur.kd_reference(e0, hist, sums, MOD_G)
            tol = ur.kd_tolerance(e0, hist, sums, MOD_G, tol_sums=tol_sums)
            _report(f'VQ-KD module one_call={one_call} step {step}', q.embedding.weight.detach(), ref, tol)
            if step == 0:
                tokens.append(quant)
    # tokens only: below 32 768 tokens the centroid sums are fp32 atomics, so the two routes' codebooks are not bit-identical at the
    # defaults either (tests/test_gpu_one_call.py asks exact codebooks from N >= 32768); each route is held to the bound above
    assert torch.equal(tokens[0], tokens[1])
