"""Index exactness and the proposal bound on the hostile families of oracle/hostile.py (tests/test_hostile_cpu.py proves on
the CPU that a library without a working margin gets 15-100 % of their rows wrong).

Every index comparison is assert_array_equal / torch.equal on ALL rows: no row is excluded, no tolerance appears.

(a) test_indices_*: N = 1024, K = 2048 against the C oracle — ops.argmin on a prepared codebook, ops.encode (the fused front:
    its own statistics and image code), ops.argmin_exact, and for a subset ops.col_argmin (the role-swapped pipeline scales
    the LATENTS as its codebook).  Routes: L2, Cosine, L2 on NormalizeCallback-normalised inputs (the constant-norm form of
    the image: no bias term), CosineBF16.
(b) test_production_forms_*: the kernel forms small shapes never launch, against ops.argmin_exact on every row and the C
    oracle on a row sample.
(c) test_bound_holds: for EVERY (row, code) the proposal score is within margin/2 of the float64 score, and the rows
    without a bound (margin <= 0) are exactly the rows the restated rule predicts and show up in the last-resort counter.
(d) test_one_call_forwards: the one-call training forwards on channel_offset.

What the cross product was pruned to, and why (each listed combination runs every entry point above):
* L2 / fp32 rows: every case at D = 8, 32, 256, 768 (the dims whose mutation shares the CPU file proves: the group-record
  family, the padded-32 form, the headline instantiation, one tile per stage); D = 16, 64, 520, 1024 add only another
  instantiation of the same kernel, so they run the SUBSET (channel_offset, code_outliers_s28, row_scales, mixed — one per
  mechanism: fp16 rounding, codebook flush, token overflow / flush, all at once).
* L2 / bf16 rows: a second load path and, at D = 256, the XD = 1 prologue's own flush — every case at D = 32 and 256, the
  subset at D = 8, 520, 768.
* Cosine and the constant-norm L2 form normalise row and code scales away (test_hostile_cpu.py asserts it), so families
  3-7 add nothing there beyond their normalisation edge cases (all-zero and overflowing norms): every case at D = 8 and
  256 fp32, the subset at 32, 768, 1024 fp32 and 32, 256 bf16.
* CosineBF16: every case at D = 32 (the VQ-KD shape that ships with autocast), the subset at 8 and 256.
* col_argmin materialises the oracle's N x K matrix on the CPU: the subset plus huge_rows and tiny_rows (the latents are
  its codebook: these hit cb_scale from the other side), L2 and Cosine, D = 32 and 256, fp32 and (L2) bf16.
* argmin_exact's register form (D % 4 != 0; bf16 rows with D % 8 != 0): the subset at D = 6, 30, 250 fp32 and 12, 252 bf16.
* (c): families of kind codebook_scale are left out of the score comparison — |e|^2 or the fp16 residual sums overflow or
  underflow fp32 there, the statistics are exact zeros or inf and a float64 score is not something fp32 arithmetic could
  be within a bound of (the fp32 DEFINITION degenerates first: every distance ties and the oracle returns index 0); which
  rows have no bound is still checked for them, and their indices in (a).  bf16 rows at D = 32 and 256 only.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle as co, hostile, synth

pytestmark = pytest.mark.gpu

N, K = 1024, 2048
SEED = 20261016                      # the seed of tests/test_hostile_cpu.py: the same arrays its sha constants pin
CASES = list(hostile.CASES)
SUBSET = ['channel_offset', 'code_outliers_s28', 'row_scales', 'mixed']
LEANS_ON_MARGIN = {'code_outliers_s28', 'channel_scale', 'channel_scale_two', 'channel_offset', 'channel_offset_2p28', 'ulp_pairs'}
F32_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope='module')
def ops():
    from vector_quantization_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


@functools.lru_cache(maxsize=4)
def _make(case, D, n=N, k=K):
    return hostile.make(case, SEED, n, k, D)


def inputs(case, D, bf16, n=N, k=K):
    x, w = _make(case, D, n, k)
    return (synth.bf16_round(x) if bf16 else x), w


def _grid(all_dims, subset_dims):
    return [(c, D) for c in CASES for D in all_dims] + [(c, D) for c in SUBSET for D in subset_dims]


def _ids(grid):
    return [f'{c}-D{D}' for c, D in grid]


def _paths(tag, st, n):
    print(f'{tag}: rescan={int(st[0])} multi={int(st[1])} exact={int(st[2])} of {n}')


def no_bound_rows(x, w, metric):
    """Rows for which row_margin() can form no bound, restated from DESIGN.md §4.1: a non-finite token image (an entry above
    fp16's range), non-finite codebook statistics (|e|^2 overflows fp32: every row), or a magnitude |x|^2 + max|e|^2 +
    2 |x| max|e| of 1e30 or more (L2).  x, w: the operands as the kernel gets them (normalised rows for cosine)."""
    xi = hostile.f16_image(x)
    bad = ~np.isfinite(xi).all(1)
    e2 = (w.astype(np.float64) ** 2).sum(1)
    if not (e2.max() < F32_MAX):
        return np.ones(len(x), bool)
    if metric == 'L2':
        xn = np.sqrt((np.where(np.isfinite(xi), xi, 0.0) ** 2).sum(1)) + np.sqrt(((x - np.where(np.isfinite(xi), xi, 0.0)) ** 2).sum(1))
        mag = xn * xn + e2.max() + 2.0 * xn * np.sqrt(e2.max())
        assert not ((mag > 0.25e30) & (mag < 4e30)).any(), 'a row sits on the guard itself: the restated rule cannot call it'
        bad |= mag >= 1e30
    return bad


def check_route(ops, case, D, route, bf16, stats=True):
    """One (case, D, route, dtype): argmin on a prepared codebook, encode, argmin_exact — all rows against the C oracle."""
    x, w = inputs(case, D, bf16)
    dt = torch.bfloat16 if bf16 else None
    tag = f'{case}/{route}/D={D}/{"bf16" if bf16 else "fp32"}'
    if route == 'L2norm':                        # NormalizeCallback in front of an L2 quantizer: both sides unit rows
        x, w = co.normalize_rows(x), co.normalize_rows(w)
        dt = None
    if route in ('L2', 'L2norm'):
        ref = co.l2_argmin(x, w)
        xd, wd = dev(x, dt), dev(w)
        idx, st = ops.argmin(xd, ops.prepare_codebook(wd, 'L2'), return_stats=True)
        _paths(tag, st, N)
        np.testing.assert_array_equal(idx.cpu().numpy(), ref, err_msg=tag + ' argmin')
        np.testing.assert_array_equal(ops.encode(xd, wd, 'L2')[0].cpu().numpy(), ref, err_msg=tag + ' encode')
        np.testing.assert_array_equal(ops.argmin_exact(xd, wd, 'L2').cpu().numpy(), ref, err_msg=tag + ' argmin_exact')
        if stats and D % 8 == 0:
            inf_rows = int(no_bound_rows(x, w, 'L2').sum())
            assert int(st[2]) >= inf_rows, f'{tag}: {inf_rows} rows have no bound, the last-resort pass saw {int(st[2])}'
            if route == 'L2' and case in LEANS_ON_MARGIN:
                assert int(st[0]) + int(st[1]) + int(st[2]) >= 1, f'{tag}: no row left the fast path'
        return
    xd, wd = dev(x, dt), dev(w)
    if route == 'Cosine':
        ref = co.cos_argmin(x, w)
        xq, wq = dev(co.normalize_rows(x)), dev(co.normalize_rows(w))
    else:
        ref = co.cos_bf16_argmin(x, w)
        xq, wq = ops.normalize_rows(xd).bfloat16().float(), ops.normalize_rows(wd).bfloat16().float()
    idx, st = ops.argmin(xq, ops.prepare_codebook(wd, route), return_stats=True)
    _paths(tag, st, N)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref, err_msg=tag + ' argmin')
    got, _, xn = ops.encode(xd, wd, route)
    np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=tag + ' encode')
    if route == 'Cosine' and not bf16:           # the fused front's own normalisation is the oracle's, bit for bit
        np.testing.assert_array_equal(xn.cpu().numpy(), co.normalize_rows(x), err_msg=tag + ' normalised rows')
    np.testing.assert_array_equal(ops.argmin_exact(xq, wq, route).cpu().numpy(), ref, err_msg=tag + ' argmin_exact')


# ---- (a) indices against the C oracle ----------------------------------------------------------------------------

G_L2_F32 = _grid([8, 32, 256, 768], [16, 64, 520, 1024])
G_L2_BF16 = _grid([32, 256], [8, 520, 768])
G_NORM_F32 = _grid([8, 256], [32, 768, 1024])
G_NORM_BF16 = _grid([], [32, 256])
G_COSBF16 = _grid([32], [8, 256])


@pytest.mark.parametrize('case,D', G_L2_F32, ids=_ids(G_L2_F32))
def test_indices_l2(ops, case, D):
    check_route(ops, case, D, 'L2', False)


@pytest.mark.parametrize('case,D', G_L2_BF16, ids=_ids(G_L2_BF16))
def test_indices_l2_bf16_rows(ops, case, D):
    check_route(ops, case, D, 'L2', True)


@pytest.mark.parametrize('case,D', G_NORM_F32, ids=_ids(G_NORM_F32))
def test_indices_cosine(ops, case, D):
    check_route(ops, case, D, 'Cosine', False)


@pytest.mark.parametrize('case,D', G_NORM_BF16, ids=_ids(G_NORM_BF16))
def test_indices_cosine_bf16_rows(ops, case, D):
    check_route(ops, case, D, 'Cosine', True)


@pytest.mark.parametrize('case,D', G_NORM_F32, ids=_ids(G_NORM_F32))
def test_indices_l2_constant_norm_codebook(ops, case, D):
    check_route(ops, case, D, 'L2norm', False)


@pytest.mark.parametrize('case,D', G_COSBF16, ids=_ids(G_COSBF16))
def test_indices_cosine_bf16_autocast(ops, case, D):
    check_route(ops, case, D, 'CosineBF16', False)


@pytest.mark.parametrize('D,bf16', [(6, False), (30, False), (250, False), (12, True), (252, True)])
@pytest.mark.parametrize('case', SUBSET)
def test_indices_exact_route_register_form(ops, case, D, bf16):
    """D % 8 != 0: every entry point takes the all-fp32 route; D % 4 != 0 (and bf16 rows with D % 8 != 0) its register form."""
    check_route(ops, case, D, 'L2', bf16, stats=False)
    check_route(ops, case, D, 'Cosine', bf16, stats=False)


@pytest.mark.parametrize('metric,bf16', [('L2', False), ('L2', True), ('Cosine', False)])      # (cosine takes normalised fp32 rows)
@pytest.mark.parametrize('D', [32, 256])
@pytest.mark.parametrize('case', SUBSET + ['huge_rows', 'tiny_rows'])
def test_col_argmin(ops, case, D, metric, bf16):
    """NearestAnchor's column argmin: the role-swapped pipeline prepares the LATENTS as its codebook image — row_scales and
    huge_rows put the scale's edges (flushed and overflowing rows under one common scale) on that side.  Against
    d.argmin(0) of the oracle's materialised matrix."""
    x, w = inputs(case, D, bf16)
    if metric == 'Cosine':
        xo, wo = co.normalize_rows(x), co.normalize_rows(w)
        col = ops.col_argmin(dev(xo), dev(wo), metric)
        ref = co.col_argmin(co.cos_dist(x, w))
    else:
        col = ops.col_argmin(dev(x, torch.bfloat16 if bf16 else None), dev(w), metric)
        ref = co.col_argmin(co.l2_dist(x, w))
    np.testing.assert_array_equal(col.cpu().numpy(), ref)


# ---- (b) the production kernel forms ---------------------------------------------------------------------------------

FORM_FAMILIES = ['channel_offset', 'code_outliers_s28', 'mixed']


def check_against_exact(ops, x, w, metric, dt=None, sample=400, tag=''):
    xd, wd = dev(x, dt), dev(w)
    if metric == 'Cosine':
        xq, wq = ops.normalize_rows(xd), ops.normalize_rows(wd)
    else:
        xq, wq = xd, wd
    ref = ops.argmin_exact(xq, wq, metric)
    got, st = ops.argmin(xq, ops.prepare_codebook(wd, metric), return_stats=True)
    _paths(tag, st, len(x))
    assert torch.equal(got, ref), f'{tag}: {int((got != ref).sum())} rows differ from the all-fp32 route'
    enc = ops.encode(xd, wd, metric)[0]
    assert torch.equal(enc, ref), f'{tag}: encode: {int((enc != ref).sum())} rows differ from the all-fp32 route'
    rows = np.arange(0, len(x), max(1, len(x) // sample))
    xs = xd[torch.from_numpy(rows).cuda()].float().cpu().numpy()
    oracle = (co.cos_argmin if metric == 'Cosine' else co.l2_argmin)(xs, w)
    np.testing.assert_array_equal(ref.cpu().numpy()[rows], oracle, err_msg=tag + ' (oracle, row sample)')
    return xq, wq, ref


@pytest.mark.parametrize('metric', ['L2', 'Cosine'])
@pytest.mark.parametrize('D', [8, 16, 32])
@pytest.mark.parametrize('case', FORM_FAMILIES)
def test_production_forms_group_records(ops, case, D, metric):
    """D <= 32 at >= 16 384 tokens: coarse32_kernel's group records with identify32_kernel behind them."""
    n = 20000
    x, w = inputs(case, D, False, n, K)
    check_against_exact(ops, x, w, metric, tag=f'group records {case}/{metric}/D={D}')


@pytest.mark.parametrize('case', FORM_FAMILIES)
def test_production_forms_xdirect_prologue(ops, case):
    """coarse_kernel<..., XD = 1>: D = 256, bf16 rows, more than 16 384 of them — the proposal kernel makes its token fragments
    itself (v_cvt_pk_f16_f32 and its own flush) and slice 0 writes the row statistics.  Default slice count, then two and
    four forced slices (tuning key 2)."""
    from vector_quantization_amd import _lib
    L = _lib.lib()
    n, k = 20000, 4096
    x, w = inputs(case, 256, True, n, k)
    xq, wq, ref = check_against_exact(ops, x, w, 'L2', torch.bfloat16, tag=f'XD=1 {case}')
    cb = ops.prepare_codebook(wq, 'L2')
    try:
        for ns in (2, 4):
            assert L.vqhip_set_tuning(2, ns) == 0
            got = ops.argmin(xq, cb)
            assert torch.equal(got, ref), (case, ns, int((got != ref).sum()))
    finally:
        L.vqhip_set_tuning(2, 0)


@pytest.mark.parametrize('case', FORM_FAMILIES)
def test_production_forms_d1024_one_wave_per_simd(ops, case):
    n, k = 24576, 1024
    x, w = inputs(case, 1024, False, n, k)
    check_against_exact(ops, x, w, 'L2', sample=60, tag=f'D=1024 four-wave form {case}')


@pytest.mark.parametrize('case', FORM_FAMILIES)
def test_production_forms_nchw_map_route(ops, case):
    """tokenization.encode_to_quant on an NCHW-contiguous map (the transpose folded into the encode's first launch) equals the
    token-major call and the all-fp32 route."""
    from vector_quantization_amd import Config, build_quantizer, tokenization
    B, H, W, D, k = 16, 16, 16, 256, 2048
    x, w = inputs(case, D, False, B * H * W, k)
    q = build_quantizer(dict(type='VQGANQuantizer', embedding=dict(type='torch_nn_modules_sparse_Embedding', num_embeddings=k, embedding_dim=D),
                             distance=dict(type='L2Distance'), losses=dict(vqgan_loss=dict(type='VQGANLoss'))))
    q.init_weights(Config(type='vqgan'))
    q = q.cuda().eval()
    q._forward_pre_hooks.clear()
    with torch.no_grad():
        q.embedding.weight.copy_(dev(w))
        tokens = dev(x).reshape(B, H, W, D)
        nchw = tokens.permute(0, 3, 1, 2).contiguous()
        nhwc = tokens.permute(0, 3, 1, 2)                       # channels-last: the token-major call
        assert not tokenization.is_token_major(nchw) and tokenization.is_token_major(nhwc)
        qa, _ = tokenization.encode_to_quant(q, nchw, {})
        qb, _ = tokenization.encode_to_quant(q, nhwc, {})
    ref = ops.argmin_exact(dev(x), dev(w), 'L2')
    assert torch.equal(qa.reshape(-1), ref) and torch.equal(qb.reshape(-1), ref)
    np.testing.assert_array_equal(ref.cpu().numpy(), co.l2_argmin(x, w))


# ---- (c) the bound itself ----------------------------------------------------------------------------------------

BOUND_CASES = [c for c in CASES if hostile.CASES[c][0] != 'codebook_scale']
NB = 512        # rows per case (the first 512 of the same arrays: every row pattern of `mixed` and the strided families)


def _bound_case(ops, case, route, D, bf16):
    x, w = inputs(case, D, bf16)
    x = x[:NB]
    if route == 'L2':
        xe, we, metric = x, w, 'L2'
    elif route == 'L2norm':
        xe, we, metric = co.normalize_rows(x), co.normalize_rows(w), 'L2'
    else:
        xe, we, metric = co.normalize_rows(x), co.normalize_rows(w), 'Cosine'
    cb = ops.prepare_codebook(dev(w if route == 'Cosine' else we), metric)
    xq = dev(xe, torch.bfloat16 if (bf16 and route == 'L2') else None)
    scores, margin, se = ops.debug_proposal_scores(xq, cb)
    scores, margin, se = scores.cpu().numpy().astype(np.float64), margin.cpu().numpy().astype(np.float64), float(se.item())
    _, st = ops.argmin(xq, cb, return_stats=True)
    return xe, we, metric, scores, margin, se, st


def exact_scores(xe, we, metric, se):
    """The real-number score the margin is about, in float64.  L2: se (x.e_k - |e_k|^2 / 2).  L2 on a constant-norm codebook
    (cb_image_kernel: max |e|^2 - min |e|^2 <= 2^-16 max |e|^2 over the fp32 sums, aux = 0): the proposal scores carry NO
    bias term, the comparable score is se (x.e_k - (|e_k|^2 - min_j |e_j|^2) / 2) — the common -min/2 shifts every code
    alike — and the margin carries `en_spread` for what is left.  Cosine: se x.e_k on the normalised rows."""
    dot = xe.astype(np.float64) @ we.astype(np.float64).T
    if metric != 'L2':
        return se * dot, False
    en32 = co.row_sqnorm(we)
    const_norm = bool(np.isfinite(en32).all() and en32.max() > 0 and (en32.max() - en32.min()) <= en32.max() * 2.0 ** -16)
    en = (we.astype(np.float64) ** 2).sum(1)
    if const_norm:
        en = en - en.min()
    return se * (dot - 0.5 * en[None, :]), const_norm


BOUND_GRID = [(r, D, False) for r in ('L2', 'L2norm', 'Cosine') for D in (8, 32, 256, 768, 1024)] + [('L2', 32, True), ('L2', 256, True)]


@pytest.mark.parametrize('route,D,bf16', BOUND_GRID, ids=[f'{r}-D{D}-{"bf16" if b else "fp32"}' for r, D, b in BOUND_GRID])
@pytest.mark.parametrize('case', BOUND_CASES)
def test_bound_holds(ops, case, route, D, bf16):
    """test_margin_holds (tests/test_gpu_parity.py) on the hostile families: |proposal score - float64 score| <= margin / 2
    for every (row, code) of every row that HAS a margin; the rows without one are exactly those the restated rule names,
    and a plain argmin sends at least that many through the whole-codebook fp32 pass."""
    xe, we, metric, scores, margin, se, st = _bound_case(ops, case, route, D, bf16)
    predicted = no_bound_rows(xe, we, metric)
    np.testing.assert_array_equal(~(margin > 0), predicted, err_msg='rows without a bound are not the rows the rule predicts')
    assert int(st[2]) >= int(predicted.sum()), (st.tolist(), int(predicted.sum()))
    ok = margin > 0
    if route == 'L2norm':
        assert exact_scores(xe, we, metric, se)[1] or not np.isfinite(co.row_sqnorm(we)).all() or co.row_sqnorm(we).max() == 0
    if not ok.any():
        print(f'{case}/{route}/D={D}/{"bf16" if bf16 else "fp32"}: no row has a bound ({len(ok)} rows to the fp32 pass)')
        return
    exact, _ = exact_scores(xe[ok], we, metric, se)
    err = np.abs(scores[ok] - exact).max(1)
    ratio = err / (0.5 * margin[ok])
    print(f'{case}/{route}/D={D}/{"bf16" if bf16 else "fp32"}: max |score error| / (margin/2) = {ratio.max():.4f} '
          f'(median {np.median(ratio):.4f}), {int((~ok).sum())} rows without a bound')
    assert np.isfinite(scores[ok]).all()
    assert ratio.max() <= 1.0, f'error exceeds the bound: max ratio {ratio.max():.3f}'


@pytest.mark.parametrize('case', [c for c in CASES if hostile.CASES[c][0] == 'codebook_scale'])
def test_rows_without_a_bound_codebook_scale(ops, case):
    """The codebook_scale cases of (c): which rows have no bound (see the module docstring for why no scores are compared)."""
    for D in (8, 256):
        xe, we, metric, _, margin, _, st = _bound_case(ops, case, 'L2', D, False)
        predicted = no_bound_rows(xe, we, metric)
        np.testing.assert_array_equal(~(margin > 0), predicted)
        assert int(st[2]) >= int(predicted.sum())
        _paths(f'{case}/L2/D={D}', st, NB)


# ---- (d) the one-call training forwards --------------------------------------------------------------------------

def _quantizer(cfg, w, train=True):
    from vector_quantization_amd import Config, build_quantizer
    q = build_quantizer(cfg)
    q.train(train)
    q.init_weights(Config(type='vqgan'))
    q = q.cuda()
    q._forward_pre_hooks.clear()
    with torch.no_grad():
        q.embedding.weight.copy_(dev(w))
    return q


EMB = 'torch_nn_modules_sparse_Embedding'


def _vqgan_cfg(k, D, callbacks):
    return dict(type='VQGANQuantizer', embedding=dict(type=EMB, num_embeddings=k, embedding_dim=D), distance=dict(type='L2Distance'),
                losses=dict(vqgan_loss=dict(type='VQGANLoss')), callbacks=callbacks)


def _vqkd_cfg(k, D):
    return dict(type='VQKDQuantizer', embedding=dict(type=EMB, num_embeddings=k, embedding_dim=D), distance=dict(type='CosineDistance'),
                callbacks=[dict(type='VQKDCallback', ema=dict())], losses=dict(commitment_loss=dict(type='CommitmentLoss', mse=dict(norm=True))))


@pytest.mark.parametrize('name,n,k,D,bf16', [
    ('vq_forward', 16384, 16384, 256, True),        # VQGAN, the headline's per-image-batch shape
    ('cvq_forward', 3072, 16384, 256, False),       # the CVQ-VAE step
    ('vqkd_forward', 12544, 8192, 32, False),       # VQ-KD: 64 images of 14 x 14 tokens
])
def test_one_call_forwards(ops, name, n, k, D, bf16):
    """vqhip_vq_forward, vqhip_cvq_forward and vqhip_vqkd_forward once each on channel_offset at their shipped shapes:
    memo['quant'] is the all-fp32 route's argmin on the operands the step's encode used (L2: the latents and the codebook the
    step started from; VQ-KD: the normalised rows memo['encode'] keeps for its distance matrix)."""
    x, w = inputs('channel_offset', D, bf16, n, k)
    if name == 'vqkd_forward':
        cfg = _vqkd_cfg(k, D)
    else:
        cfg = _vqgan_cfg(k, D, [dict(type='CVQVAECallback', ema=dict(), anchor=dict(type='NearestAnchor'))] if name == 'cvq_forward' else [])
    q = _quantizer(cfg, w)
    if name == 'vqkd_forward':
        for p in q.parameters():
            p.requires_grad_(False)
    q.one_call_steps = True
    xd = dev(x, torch.bfloat16 if bf16 else None)
    assert q._one_call_step(xd) is not None, 'the one-call route does not take this configuration'
    w0 = dev(w)
    _, _, memo = q(xd.clone().requires_grad_(True), {})
    quant = memo['quant'].reshape(-1)
    if name == 'vqkd_forward':
        d = memo['encode']['distance']
        ref = ops.argmin_exact(d._xq, d._eq.clone(), 'Cosine')
    else:
        ref = ops.argmin_exact(xd, w0, 'L2')
    assert torch.equal(quant, ref), f'{name}: {int((quant != ref).sum())} rows differ'
