"""Pooled code features on the MI355X: tokens [B, *] -> [B, D] mean of the decoded rows in one launch, held bit for bit to the
numpy restatement of the contract (tests/pooled_ref.py), to the float64 mean within the derived bound, and — through the
modules — to `decode` + mean, whose [B*HW, D] matrix it must not allocate."""
import gc

import numpy as np
import pytest
import torch

import pooled_ref as PR

pytestmark = pytest.mark.gpu

EMB = 'torch_nn_modules_sparse_Embedding'
DTYPES = (torch.int64, torch.int32)
_codebooks = {}


def codebook(K, D):
    """One seeded fp32 codebook per (K, D), made once: (numpy [K, D], the same on the device)."""
    if (K, D) not in _codebooks:
        e = np.random.default_rng(K * 4099 + D).standard_normal((K, D)).astype(np.float32)
        _codebooks[(K, D)] = (e, torch.from_numpy(e).cuda())
    return _codebooks[(K, D)]


def same_bits(got, want) -> bool:
    """Equal as fp32 values with NaN == NaN, and the same sign on every zero."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got, want, equal_nan=True):
        return False
    finite = ~np.isnan(want)
    return np.array_equal(np.signbit(got[finite]), np.signbit(want[finite]))


def token_sets(rng, B, HW, K):
    """Uniform tokens, every token equal, and 0 .. HW-1 in order (modulo K)."""
    yield 'uniform', rng.integers(0, K, size=(B, HW))
    yield 'equal', np.full((B, HW), int(rng.integers(0, K)))
    yield 'ordered', np.broadcast_to(np.arange(HW) % K, (B, HW)).copy()


@pytest.mark.parametrize('HW', PR.HW_CASES)
@pytest.mark.parametrize('K,D', PR.KD_CASES)
def test_bit_exact_and_within_the_float64_bound(K, D, HW):
    from vector_quantization_amd import functional as VF, ops
    e, ed = codebook(K, D)
    rng = np.random.default_rng(HW * 131 + D)
    for B in (1, 3):
        for name, quant in token_sets(rng, B, HW, K):
            want = PR.pooled_tokens(e, quant)
            v = e[quant]
            ref64, bound = PR.mean64(v), PR.bound(v)
            for dtype in DTYPES:
                qd = torch.from_numpy(quant).to(dtype).cuda()
                got = ops.decode_pool(ed, qd)
                assert got.shape == (B, D) and got.dtype == torch.float32
                got = got.cpu().numpy()
                assert same_bits(got, want), (B, name, dtype, float(np.abs(got - want).max()))
            assert (np.abs(got.astype(np.float64) - ref64) <= bound).all(), (B, name)
            # the reference's definition on the device, in float64: decode, then the mean over the positions
            dev64 = VF.embedding(ed, torch.from_numpy(quant).cuda()).double().mean(dim=1).cpu().numpy()
            assert (np.abs(got.astype(np.float64) - dev64) <= bound).all(), (B, name)


def test_hostile_codebook_values():
    """+-inf, NaN, -0.0 and 1e38 rows among ordinary ones: the same bits as the restatement, whichever partial they meet in."""
    from vector_quantization_amd import ops
    K, D = 64, 32
    e = codebook(K, D)[0].copy()
    e[1], e[2], e[3], e[4], e[5], e[6] = np.inf, -np.inf, np.nan, -0.0, 1e38, -1e38
    e[7, ::2] = np.inf
    ed = torch.from_numpy(e).cuda()
    rng = np.random.default_rng(5)
    for HW in (1, 9, 196):
        quant = rng.integers(0, K, size=(12, HW))
        quant[0] = 4                                    # only -0.0 rows: the sum is +0.0
        quant[1] = rng.choice([4, 5, 6], size=HW)       # 1e38 - 1e38 and overflow
        quant[2] = rng.choice([1, 7, 9], size=HW)       # +inf alone
        quant[3] = rng.choice([1, 2, 9], size=HW)       # inf - inf
        quant[4] = rng.integers(8, K, size=HW)          # nothing special
        want = PR.pooled_tokens(e, quant)
        for dtype in DTYPES:
            got = ops.decode_pool(ed, torch.from_numpy(quant).to(dtype).cuda()).cpu().numpy()
            assert same_bits(got, want), (HW, dtype)
    assert not np.signbit(want[0]).any() and np.isfinite(want[4]).all()


@pytest.mark.parametrize('K,D,HW', [(64, 6, 9), (512, 32, 196), (16384, 256, 256), (64, 1028, 7)])
def test_out_of_range_tokens_make_their_image_nan_and_nothing_faults(K, D, HW):
    from vector_quantization_amd import ops
    e, ed = codebook(K, D)
    quant = np.random.default_rng(HW).integers(0, K, size=(3, HW))
    quant[1, 0], quant[1, HW - 1] = -1, K
    if HW > 2:
        quant[1, HW // 2] = np.iinfo(np.int32).max
    want = PR.pooled_tokens(e, quant)
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()
    for dtype in DTYPES:
        got = ops.decode_pool(ed, torch.from_numpy(quant).to(dtype).cuda())
        torch.cuda.synchronize()
        assert same_bits(got.cpu().numpy(), want), dtype
    far = quant.copy()
    far[1, 0] = -(1 << 40)                              # int64 only: a row 2^40 * D floats in front of the codebook
    got = ops.decode_pool(ed, torch.from_numpy(far).cuda())
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy(), want)


@pytest.mark.parametrize('levels', [[3, 3, 3], [8, 8, 5, 5, 5], [8, 8, 8, 5, 5, 5]])
def test_fsq_pool_is_the_contract_on_fsq_decodes_own_values(levels):
    from vector_quantization_amd import ops
    q = ops.fsq_constants(levels)
    K = int(np.prod(levels))
    rng = np.random.default_rng(K)
    for HW in (1, 9, 256):
        for B in (1, 3):
            quant = rng.integers(0, K, size=(B, HW))
            quant[0, 0] = -7
            quant[-1, HW - 1] = K + 11
            if HW > 2:
                quant[0, 1], quant[0, 2] = -(K * 3), np.iinfo(np.int32).min
            for dtype in DTYPES:
                qd = torch.from_numpy(quant).to(dtype).cuda()
                rows = ops.fsq_decode(qd, q)
                assert rows.shape == (B, HW, len(levels))
                want = PR.pooled(rows.cpu().numpy())
                got = ops.fsq_decode_pool(qd, q)
                assert got.shape == (B, len(levels))
                assert same_bits(got.cpu().numpy(), want), (levels, HW, B, dtype)
    big = torch.tensor([[1 << 40, -(1 << 40) - 3, 5]], dtype=torch.int64).cuda()
    assert same_bits(ops.fsq_decode_pool(big, q).cpu().numpy(), PR.pooled(ops.fsq_decode(big, q).cpu().numpy()))


@pytest.mark.parametrize('B,HW,K,D', [(3, 9, 16, 8), (2, 256, 64, 256), (4, 196, 8192, 32)])
def test_backward_against_float64_autograd(B, HW, K, D):
    from vector_quantization_amd import functional as VF
    rng = np.random.default_rng(B * HW)
    w = rng.standard_normal((K, D)).astype(np.float32)
    quant = rng.integers(0, K, size=(B, HW))
    quant[quant == 5] = 6                                # a code that no token names, also in the small codebooks
    r = rng.standard_normal((B, D)).astype(np.float32)
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    f64 = torch.nn.functional.embedding(torch.from_numpy(quant), w64).mean(dim=1)
    (want,) = torch.autograd.grad((f64 * torch.from_numpy(r).double()).sum(), w64)
    want = want.numpy()
    bound = PR.grad_bound(quant, r, K)
    unnamed = np.setdiff1d(np.arange(K), quant.reshape(-1))
    assert unnamed.size > 0
    for dtype in DTYPES:
        wd = torch.from_numpy(w).cuda().requires_grad_(True)
        qd = torch.from_numpy(quant).to(dtype).cuda()
        f = VF.decode_pool(wd, qd)
        assert same_bits(f.detach().cpu().numpy(), PR.pooled_tokens(w, quant))
        (got,) = torch.autograd.grad((f * torch.from_numpy(r).cuda()).sum(), wd)
        got = got.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), (dtype, float((err - bound).max()))
        assert not got[unnamed].any()                    # exactly zero


def test_backward_skips_out_of_range_tokens():
    from vector_quantization_amd import functional as VF, ops
    B, HW, K, D = 3, 9, 16, 8
    rng = np.random.default_rng(2)
    w = rng.standard_normal((K, D)).astype(np.float32)
    quant = rng.integers(0, K, size=(B, HW))
    quant[1, 2], quant[1, 3], quant[2, 8] = -1, K, 1 << 20
    r = rng.standard_normal((B, D)).astype(np.float32)
    want = np.zeros((K, D))
    for b in range(B):
        for p in range(HW):
            if 0 <= quant[b, p] < K:
                want[quant[b, p]] += r[b].astype(np.float64) / HW
    bound = PR.grad_bound(quant, r, K)
    for dtype in DTYPES:
        qd = torch.from_numpy(quant).to(dtype).cuda()
        got = ops.decode_pool_bwd(torch.from_numpy(r).cuda(), qd, K).cpu().numpy()
        assert (np.abs(got - want) <= bound).all(), dtype
        wd = torch.from_numpy(w).cuda().requires_grad_(True)
        (g2,) = torch.autograd.grad((VF.decode_pool(wd, qd) * torch.from_numpy(r).cuda()).sum(), wd)
        assert (np.abs(g2.cpu().numpy() - want) <= bound).all() and np.isfinite(g2.cpu().numpy()).all()


# ---- through the modules ----------------------------------------------------------------------------------------------------

def _build(cfg, weight=None):
    from vector_quantization_amd import Config, build_quantizer
    q = build_quantizer(cfg)
    q.train(False)
    q.init_weights(Config())
    q = q.cuda()
    q._forward_pre_hooks.clear()
    if weight is not None:
        with torch.no_grad():
            q.embedding.weight.copy_(weight)
    return q


def _vq_cfg(K, D, qtype='VQGANQuantizer', distance='L2', callbacks=(), losses=None):
    return dict(type=qtype, embedding=dict(type=EMB, num_embeddings=K, embedding_dim=D), distance=dict(type=f'{distance}Distance'),
                callbacks=[dict(c) for c in callbacks], losses=losses or dict(vqgan_loss=dict(type='VQGANLoss')))


def _module_cases():
    g = torch.Generator().manual_seed(17)
    yield 'vqgan_small', _build(_vq_cfg(64, 8), torch.randn(64, 8, generator=g)), torch.randn(3, 8, 2, 2, generator=g)
    yield 'vqgan_d256', _build(_vq_cfg(1024, 256), torch.randn(1024, 256, generator=g)), torch.randn(2, 256, 16, 16, generator=g)
    unit = torch.nn.functional.normalize(torch.randn(512, 32, generator=g))
    yield 'vqkd_cos_normalize', _build(_vq_cfg(512, 32, 'VQKDQuantizer', 'Cosine', [dict(type='NormalizeCallback')],
                                               dict(commitment_loss=dict(type='CommitmentLoss', mse=dict(norm=True)))), unit), \
        torch.randn(2, 32, 14, 14, generator=g)
    yield 'fsq', _build(dict(type='FiniteScalarQuantizer', num_scalars_per_channel=[8, 5, 5, 5])), torch.randn(2, 4, 16, 16, generator=g)


def test_pooled_features_through_the_modules():
    from vector_quantization_amd import ops, tokenization as T
    from vector_quantization_amd.quantizers import FiniteScalarQuantizer
    for name, q, x in _module_cases():
        for fmt in (torch.contiguous_format, torch.channels_last):
            xd = x.cuda().contiguous(memory_format=fmt)
            with torch.no_grad():
                T.encode_to_quant(q, xd, {})             # (NormalizeCallback re-normalises the codebook on every encode: settle it)
                tokens, _ = T.encode_to_quant(q, xd, {})
                features, quant, memo = T.pooled_features(q, xd, {})
                assert q.last_route.name == 'pooled' and q.last_route.why == '', (name, q.last_route)
                assert torch.equal(quant, tokens) and quant.shape == (x.shape[0], x.shape[2], x.shape[3]), name
                again, memo2 = T.pool_from_quant(q, tokens, {})
            assert features.shape == (x.shape[0], q.embedding_dim) and features.dtype == torch.float32
            assert same_bits(features.cpu().numpy(), again.cpu().numpy()), name
            assert 'encode' in memo['quantizer'] and 'decode' in memo['quantizer'], (name, list(memo['quantizer']))
            assert 'quant' in memo['quantizer'] and 'decode' in memo2['quantizer']
            # and they are the contract on the module's own decode
            if isinstance(q, FiniteScalarQuantizer):
                rows = ops.fsq_decode(tokens, q.constants)
            else:
                rows = q.embedding.weight.detach()[tokens]
            assert same_bits(features.cpu().numpy(), PR.pooled(rows.reshape(x.shape[0], -1, q.embedding_dim).cpu().numpy())), name


def test_the_rows_route_gives_the_same_features_within_the_bound():
    from vector_quantization_amd import tokenization as T
    g = torch.Generator().manual_seed(23)
    w = torch.randn(1024, 256, generator=g)
    q = _build(_vq_cfg(1024, 256), w)
    rows_q = _build(_vq_cfg(1024, 256), w)
    cls = type(rows_q)

    class SubDecode(cls):
        def _decode(self, quant, memo):
            return cls._decode(self, quant, memo)
    rows_q.__class__ = SubDecode
    tokens = torch.randint(0, 1024, (2, 16, 16), generator=g).cuda()
    with torch.no_grad():
        fused, _ = T.pool_from_quant(q, tokens, {})
        composed, memo = T.pool_from_quant(rows_q, tokens, {})
    assert q.last_route.name == 'pooled' and rows_q.last_route.name == 'rows' and '_decode' in rows_q.last_route.why
    assert 'decode' in memo['quantizer'] and composed.shape == fused.shape
    v = w.numpy()[tokens.cpu().numpy().reshape(2, -1)]
    ref64, bound = PR.mean64(v), PR.bound(v)
    assert (np.abs(fused.cpu().numpy().astype(np.float64) - ref64) <= bound).all()
    assert (np.abs(composed.cpu().numpy().astype(np.float64) - ref64) <= bound).all()
    # with autograd on, the fused route carries the codebook's gradient as decode + mean does
    r = torch.randn(2, 256, generator=g).cuda()
    (ga,) = torch.autograd.grad((T.pool_from_quant(q, tokens, {})[0] * r).sum(), q.embedding.weight)
    (gb,) = torch.autograd.grad((T.pool_from_quant(rows_q, tokens, {})[0] * r).sum(), rows_q.embedding.weight)
    gbound = 2 * PR.grad_bound(tokens.cpu().numpy(), r.cpu().numpy(), 1024)        # both sides are fp32 sums
    assert (np.abs(ga.cpu().numpy().astype(np.float64) - gb.cpu().numpy()) <= gbound).all()


def test_the_decoded_matrix_is_never_allocated():
    """B = 64, HW = 256, D = 256: the peak of device memory across pool_from_quant, over what was held before the call, stays
    below the B*HW*D*4 bytes of the decoded rows — which the composed route (decode, then mean) cannot do."""
    from vector_quantization_amd import tokenization as T
    B, HW, K, D = 64, 256, 1024, 256
    g = torch.Generator().manual_seed(29)
    q = _build(_vq_cfg(K, D), torch.randn(K, D, generator=g))
    tokens = torch.randint(0, K, (B, 16, 16), generator=g).cuda()
    matrix = B * HW * D * 4

    def peak_over_baseline(fn):
        gc.collect()                 # garbage of earlier tests freed DURING fn would lower the peak over the baseline
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    with torch.no_grad():
        T.pool_from_quant(q, tokens, {})                                   # (first call: code objects loaded)
    fused_peak, (fused, _) = peak_over_baseline(lambda: T.pool_from_quant(q, tokens, {}))
    assert q.last_route.name == 'pooled'

    def composed_route():
        z, _ = q.decode(tokens, {})
        return z.mean(dim=(1, 2))
    composed_peak, composed = peak_over_baseline(composed_route)
    print(f'peak over baseline: fused {fused_peak} B, composed {composed_peak} B, the matrix {matrix} B')
    assert fused_peak < matrix, (fused_peak, matrix)
    assert composed_peak >= matrix, (composed_peak, matrix)
    assert torch.allclose(fused, composed, rtol=0, atol=1e-5)


def test_reproducible_from_run_to_run_and_from_batch_to_batch():
    from vector_quantization_amd import ops
    for (K, D), HW in (((16384, 256), 256), ((512, 32), 196), ((512, 8), 9), ((300, 100), 7)):
        e, ed = codebook(K, D)
        quant = torch.from_numpy(np.random.default_rng(D).integers(0, K, size=(3, HW))).cuda()
        a, b = ops.decode_pool(ed, quant), ops.decode_pool(ed, quant)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        alone = ops.decode_pool(ed, quant[2:3].contiguous())
        assert torch.equal(alone.view(torch.int32)[0], a.view(torch.int32)[2]), (K, D, HW)
        assert torch.equal(ops.decode_pool(ed, quant.int()).view(torch.int32), a.view(torch.int32))
    q = ops.fsq_constants([8, 8, 8, 5, 5, 5])
    quant = torch.randint(0, 64000, (3, 256), generator=torch.Generator().manual_seed(1)).cuda()
    a = ops.fsq_decode_pool(quant, q)
    assert torch.equal(a.view(torch.int32), ops.fsq_decode_pool(quant, q).view(torch.int32))
    assert torch.equal(ops.fsq_decode_pool(quant[2:3].contiguous(), q).view(torch.int32)[0], a.view(torch.int32)[2])
