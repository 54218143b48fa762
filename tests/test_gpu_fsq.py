"""FiniteScalarQuantizer on the MI355X against the reference's own outputs (tests/golden/fsq, tools/make_golden_fsq.py).

Correctness bar ("FiniteScalarQuantizer"): tokens equal the reference's except for a digit whose pre-round value t,
recomputed here in fp32 from x, lies within 2^-19 of a half-integer (the tanh envelope: the device's tanhf and the CPU's may
differ by an ulp or two); z is bit-identical wherever the digit agrees; decode is bit-identical for every token; the gradient
differs by at most what a 2-ulp difference of tanh explains (fp32), or 1 bf16 ulp (bf16).
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fsq')
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, 'l*.npz')))
ENVELOPE = 2.0 ** -19
INT32_MIN = -(1 << 31)


def _quantizer(levels, eps=1e-3):
    from vector_quantization_amd import build_quantizer
    return build_quantizer(dict(type='FiniteScalarQuantizer', num_scalars_per_channel=list(levels), eps=eps)).cuda()


def _t(x: torch.Tensor, levels, eps) -> torch.Tensor:
    """The reference's pre-round value t = (tanh(x + c) * M - odd) / 2, in fp32, on x's device."""
    L = torch.tensor(levels, dtype=torch.int)
    M = (L - 1) * (1 - eps)
    odd = (L - 1) % 2
    c = torch.atanh(odd / M)
    dev = x.device
    return (torch.tanh(x.float() + c.to(dev)) * M.to(dev) - odd.to(dev)) / 2


def _digits(quant: np.ndarray, levels) -> np.ndarray:
    q = quant.astype(np.int64)[:, None]
    cum = np.cumprod([1] + list(levels[:-1])).astype(np.int64)
    return (q // cum) % np.array(levels, dtype=np.int64)


def _near_boundary(t: np.ndarray) -> np.ndarray:
    return np.abs(t - (np.floor(t) + 0.5)) <= ENVELOPE


def _check_tokens(quant, quant_ref, z, z_ref, t, levels):
    """Per digit: equal, or inside the envelope; z bit-identical where the digit agrees.  Returns (envelope digits,
    envelope digits that differ)."""
    nan_rows = quant_ref == INT32_MIN
    np.testing.assert_array_equal(quant[nan_rows], quant_ref[nan_rows])
    near = _near_boundary(t) & ~nan_rows[:, None]
    d, d_ref = _digits(quant, levels), _digits(quant_ref, levels)
    differ = (d != d_ref) & ~nan_rows[:, None]
    assert not (differ & ~near).any(), f'{int((differ & ~near).sum())} digits differ outside the tanh envelope'
    rows_ok = ~differ.any(1)
    np.testing.assert_array_equal(quant[rows_ok], quant_ref[rows_ok])
    same = ~differ
    zb, zrb = z.view(np.uint32), z_ref.view(np.uint32)
    bad = same & (zb != zrb) & ~(np.isnan(z) & np.isnan(z_ref))
    assert not bad.any(), f'z differs where the digit agrees: {np.argwhere(bad)[:5]}'
    return int(near.sum()), int(differ.sum())


def _check_grad(gx, gref, g, levels, eps, bf16):
    """fp32: |d| <= 2^-20 |g M / (2h)| + 1e-5 |ref| (a 2-ulp difference of y = tanh); bf16: 1 bf16 ulp of the reference."""
    L = np.array(levels, dtype=np.float32)
    M = ((L - 1) * np.float32(1 - eps)).astype(np.float32)
    h = np.floor(L / 2)
    nan = np.isnan(gref)
    np.testing.assert_array_equal(np.isnan(gx), nan)
    ok = ~nan
    ref = np.where(nan, 0, gref).astype(np.float64)
    if bf16:
        tol = np.where(ref == 0, 2.0 ** -126, np.ldexp(1.0, np.frexp(np.abs(ref))[1] - 8))
    else:
        tol = 2.0 ** -20 * np.abs(g * M / (2 * h)) + 1e-5 * np.abs(ref)
    err = np.abs(np.where(nan, 0, gx).astype(np.float64) - ref)
    assert (err[ok] <= tol[ok]).all(), f'gradient off by {err.max()} (tol there {tol.flat[err.argmax()]})'


@pytest.mark.parametrize('case', CASES)
def test_fixture_case_matches_the_reference(case):
    z = np.load(os.path.join(GOLD, case + '.npz'))
    spec = json.loads(str(z['spec']))
    levels, eps = spec['levels'], spec['eps']
    q = _quantizer(levels, eps)
    report = []
    for tag, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
        x = torch.from_numpy(z[f'{tag}_x']).to(dtype).cuda().requires_grad_(True)
        zq, loss, memo = q(x, {})
        assert memo['quant'].dtype == torch.int32 and zq.dtype == torch.float32 and zq.shape == x.shape
        assert memo['decode']['z'] is memo['encode']['z'] is zq
        assert float(loss) == 0.0
        zq.backward(torch.from_numpy(z['g']).cuda())
        assert x.grad.dtype == dtype
        t = _t(torch.from_numpy(z[f'{tag}_x']), levels, eps).numpy()
        n_env, n_diff = _check_tokens(memo['quant'].cpu().numpy(), z[f'{tag}_quant'], zq.detach().cpu().numpy(), z[f'{tag}_z'],
                                      t, levels)
        _check_grad(x.grad.float().cpu().numpy(), z[f'{tag}_grad'], z['g'], levels, eps, dtype == torch.bfloat16)
        report.append(f'{tag}: {n_env} envelope digits, {n_diff} differ')
        # the planted rows put digits inside the envelope: the bar is exercised, not vacuous
        if tag == 'f32':
            assert n_env > 0
        assert n_diff <= n_env
    tokens = torch.from_numpy(z['decode_tokens']).cuda()
    zd, _ = q.decode(tokens, {})
    assert zd.cpu().numpy().tobytes() == z['decode_z'].tobytes()
    fits = (z['decode_tokens'] >= INT32_MIN) & (z['decode_tokens'] < (1 << 31))
    zd32, _ = q.decode(tokens[torch.from_numpy(fits).cuda()].int(), {})
    assert zd32.cpu().numpy().tobytes() == z['decode_z'][fits].tobytes()
    print(case, '; '.join(report))


def test_nan_latent_gives_int32_min_and_nan_z():
    from vector_quantization_amd import ops
    q = _quantizer([8, 8, 5, 5, 5])
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.zeros(300, 5, dtype=dtype, device='cuda')
        x[7, 2] = float('nan')
        x[299, 0] = float('nan')
        x[8] = float('inf')
        x[9] = -float('inf')
        quant, zz, _ = ops.fsq_encode(x, q.constants)
        quant = quant.cpu()
        assert quant[7] == INT32_MIN and quant[299] == INT32_MIN
        assert 0 <= int(quant[8]) < q.codebook_size and 0 <= int(quant[9]) < q.codebook_size
        assert torch.isnan(zz[7, 2]) and not torch.isnan(zz[7, :2]).any() and not torch.isnan(zz[8]).any()


def _map_vs_tokens(q, B, H, W, dtype, seed):
    from vector_quantization_amd import tokenization as T
    C = q.embedding_dim
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x_map = (torch.randn(B, C, H, W, device='cuda', generator=gen) * 1.5).to(dtype)
    g_map = torch.randn(B, C, H, W, device='cuda', generator=gen)
    assert q.map_fusable(x_map) and q._fusable()
    xm = x_map.clone().requires_grad_(True)
    z_map, loss, memo = T.quantize(q, xm, {})
    assert memo['quantizer']['encode']['z'] is z_map                      # the map route ran: z straight from the encode
    assert z_map.is_contiguous() and z_map.dtype == torch.float32
    z_map.backward(g_map)
    xt = x_map.permute(0, 2, 3, 1).reshape(-1, C).clone().requires_grad_(True)
    z_tok, _, memo_t = q(xt, {})
    z_tok.backward(g_map.permute(0, 2, 3, 1).reshape(-1, C))
    assert torch.equal(memo['quantizer']['quant'], memo_t['quant'])
    to_map = lambda t: t.reshape(B, H, W, C).permute(0, 3, 1, 2)           # noqa: E731
    assert torch.equal(z_map, to_map(z_tok))
    assert torch.equal(xm.grad, to_map(xt.grad))
    # encode_to_quant: the tokens, the token rows (memo x) and the encode's z of the token route
    quant, memo_e = T.encode_to_quant(q, x_map, {})
    assert quant.shape == (B, H, W) and quant.dtype == torch.int32
    assert torch.equal(quant.reshape(-1), memo_t['quant'])
    assert torch.equal(memo_e['quantizer']['x'], x_map.permute(0, 2, 3, 1).reshape(-1, C))
    assert torch.equal(memo_e['quantizer']['encode']['z'], memo_t['encode']['z'].detach())
    # decode_from_quant of the tokens (int64 and int32) straight into the map == the token decode, rearranged
    for tok in (quant.long(), quant):
        z_dec, _ = T.decode_from_quant(q, tok, {})
        want, _ = q.decode(tok.reshape(-1), {})
        assert z_dec.is_contiguous() and torch.equal(z_dec, to_map(want))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_map_route_is_the_token_route(dtype):
    q = _quantizer([8, 8, 5, 5, 5])
    _map_vs_tokens(q, 3, 7, 7, dtype, 1)           # 147 tokens: one partial tile, tiles straddle images
    _map_vs_tokens(q, 4, 16, 16, dtype, 2)
    _map_vs_tokens(_quantizer([7, 5, 5, 5, 3, 3]), 5, 9, 13, dtype, 3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_tokenization_batch_matches_torch_restatement(dtype):
    """524 288 x 6: the kernels against the reference's ATen chain restated on the same GPU, under the same envelope rule."""
    from vector_quantization_amd import ops
    levels, eps = [8, 8, 8, 5, 5, 5], 1e-3
    q = _quantizer(levels, eps)
    N = 524288
    gen = torch.Generator(device='cuda').manual_seed(11)
    x = (torch.randn(N, 6, device='cuda', generator=gen) * 1.5).to(dtype)
    g = torch.randn(N, 6, device='cuda', generator=gen)
    L = torch.tensor(levels, dtype=torch.int)
    M = (L - 1) * (1 - eps)
    odd = (L - 1) % 2
    c = torch.atanh(odd / M).cuda()                # the constants on the host, as the module evaluates them
    L, M, odd = L.cuda(), M.cuda(), odd.cuda()
    h = L // 2
    cum = torch.tensor([1] + levels[:-1], device='cuda').cumprod(0)
    xr = x.clone().requires_grad_(True)
    t = (torch.tanh(xr + c) * M - odd) / 2
    zst = t + (t.round() - t).detach()
    z_ref = zst / h
    quant_ref = ((zst + h) * cum).sum(-1).to(torch.int)
    z_ref.backward(g)
    quant, zz, _ = ops.fsq_encode(x, q.constants)
    gx = ops.fsq_backward(x, g, q.constants)
    n_env, n_diff = _check_tokens(quant.cpu().numpy(), quant_ref.cpu().numpy(), zz.cpu().numpy(), z_ref.detach().cpu().numpy(),
                                  t.detach().cpu().numpy(), levels)
    assert n_diff <= n_env
    _check_grad(gx.float().cpu().numpy(), xr.grad.float().cpu().numpy(), g.cpu().numpy(), levels, eps, dtype == torch.bfloat16)
    # decode: bit-identical to the embeddings rows (digits / h - 1)
    zd = ops.fsq_decode(quant, q.constants)
    assert torch.equal(zd, q.embeddings[quant.long()])
    print(f'524288x6 {dtype}: {n_env} envelope digits, {n_diff} differ')


@pytest.mark.parametrize('levels', [[8, 8, 5, 5, 5], [8, 8, 8, 5, 5, 5]])
def test_codebook_counts_of_int32_tokens(levels):
    import types
    from vector_quantization_amd import ops, runners as R, tokenization as T
    q = _quantizer(levels)
    K = q.codebook_size
    for N in (3072, 65536):                        # global-atomic and (K <= 32768) LDS forms of vqhip_hist_i32
        x = torch.randn(N, len(levels), device='cuda') * 2
        x[5, 1] = float('nan')                     # an INT32_MIN token: skipped, like any token outside [0, K)
        hist = torch.zeros(K, dtype=torch.int32, device='cuda')
        quant, _, _ = ops.fsq_encode(x, q.constants, need_z=False, hist=hist)
        assert quant.dtype == torch.int32 and int(quant[5]) == INT32_MIN
        want = torch.bincount(quant[quant >= 0].long(), minlength=K)
        assert torch.equal(hist.long(), want)                               # the encode's own histogram
        counts = T.CodebookCounts(K)
        counts.update(quant)
        assert torch.equal(counts.reduced(), want)
        extra = torch.tensor([K, K + 5, -1, INT32_MIN, 0], dtype=torch.int32, device='cuda')
        assert torch.equal(ops.hist(extra, K).long(), torch.bincount(torch.tensor([0], device='cuda'), minlength=K))
        runner = types.SimpleNamespace(strategy=types.SimpleNamespace(module=types.SimpleNamespace(quantizer=q)))
        usage = R.CodebookUsageMetric(quant='["quantizer"]["quant"]')
        usage.bind(runner)
        usage.forward({}, dict(quantizer=dict(quant=quant)))
        assert torch.equal(usage._counts, want)
        assert usage.summary({}) == int((want > 0).sum()) / K


def test_token_files_keep_int32(tmp_path):
    from vector_quantization_amd import tokenization as T
    q = _quantizer([8, 8, 5, 5, 5])
    x = torch.randn(10, 5, 4, 4, device='cuda')
    quant, memo = T.encode_to_quant(q, x, {})
    assert quant.dtype == torch.int32
    path = T.save_tokens(tmp_path, 1, [str(i) for i in range(10)], torch.arange(10), quant, x.shape, rank=0)
    assert T.load_tokens(path)['tokens'].dtype == torch.int32
    codes, _ = T.save_llamagen(tmp_path, 256, 1, quant, torch.arange(10), rank=0, world_size=1)
    arr = np.load(codes)
    assert arr.dtype == np.int32 and arr.shape == (1, 10, 16)
    assert np.array_equal(arr.reshape(-1), quant.cpu().numpy().reshape(-1))
