"""CPU checks of the sampler: the numpy restatement against a torch composition of the reference's own steps, the registry, the
route decision, the torch route on CPU logits, the ABI limits, and the input conditions the GPU cases rely on."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sampler_ref as ref
from vector_quantization_amd import _lib, samplers
from vector_quantization_amd.quantizers import routes
from vector_quantization_amd.registries import VQSMSamplerRegistry


def _reference_steps(logits: torch.Tensor, top_k: int, top_p: float) -> torch.Tensor:
    """The reference's steps on float64 rows: topk, compare, stable ascending sort, softmax, cumsum, <= 1 - p, keep last, scatter.
    Returns the kept mask."""
    x = logits.clone()
    if top_k > 0:
        kth = torch.topk(x, min(top_k, x.shape[-1]))[0][..., -1, None]
        x = x.masked_fill(x < kth, -float('inf'))
    if 0 <= top_p <= 1:
        s, idx = torch.sort(x, descending=False, stable=True)
        c = s.softmax(-1).cumsum(-1)
        remove = c <= 1 - top_p
        remove[..., -1:] = False
        remove = remove.scatter(-1, idx, remove)
        x = x.masked_fill(remove, -float('inf'))
    return x > -float('inf')


@pytest.mark.parametrize('V,top_k,top_p', [(64, 0, 2.0), (257, 50, 0.92), (1024, 600, 0.5), (1024, 0, 0.92), (65, 2, 0.0),
                                           (4099, 600, 1.0), (63, 70, 0.92)])
def test_restatement_equals_the_reference_steps_on_tie_free_rows(V, top_k, top_p):
    """``ref.RowCut`` itself — the class the GPU tests hold the kernel to — on float64 rows against the torch composition.  The
    contract's threshold is 1 - (double)(float)top_p, so the composition gets the same fp32-rounded p."""
    g = np.random.default_rng(V + top_k)
    x = g.normal(0, 2, size=(4, V))
    assert all(len(np.unique(r)) == V for r in x)
    p32 = float(np.float32(top_p))
    want = _reference_steps(torch.from_numpy(x), top_k, p32).numpy()
    for r in range(4):
        rc = ref.RowCut(x[r], top_k, top_p, 1e-12)
        # softmax's own rounding can move a share across the threshold only if it sits within 1e-12 of it
        assert rc.ambiguous == 0
        assert np.array_equal(rc.surv, ref.topk_set(x[r], top_k))
        assert np.array_equal(rc.kept, want[r]), (r, rc.kept.sum(), want[r].sum())
        # the kept set is an upper set of the order (a, -index): the highest-ranked rc.kept.sum() tokens
        assert np.array_equal(np.sort(ref.ascending(x[r])[V - int(rc.kept.sum()):]), np.nonzero(rc.kept)[0])


def test_keys_are_fp32_operation_by_operation():
    g = np.random.default_rng(5)
    x = g.normal(0, 3, size=(6, 100)).astype(np.float32)
    a = ref.keys(x, cfg_alpha=1.75, temperature=0.7)
    t = torch.from_numpy(x)
    w0, w1 = torch.tensor(np.float32(1.0 - 1.75)), torch.tensor(np.float32(1.75))
    want = ((w0 * t[:3]) + (w1 * t[3:])) / torch.tensor(np.float32(0.7))
    assert np.array_equal(a, want.numpy())
    assert np.array_equal(ref.keys(x), x)
    z = ref.keys(np.array([[-0.0, 1.0]], dtype=np.float32))
    assert not np.signbit(z[0, 0])


def test_registry_builds_the_reference_configs():
    s = VQSMSamplerRegistry.build(dict(type='TopKTopPSampler'))                    # configs/ar/x2i.py:19
    assert type(s) is samplers.TopKTopPSampler and (s._temperature, s._top_k, s._top_p) == (1.0, 600, 0.92)
    s = VQSMSamplerRegistry.build(dict(type='TopKTopPSampler', cfg=1.75))           # the same under configs/ar/cfg.py
    assert type(s) is samplers.CFGSampler and s._alpha == 1.75 and type(s._sampler) is samplers.TopKTopPSampler
    s = VQSMSamplerRegistry.build(dict(type='CFGSampler', sampler=dict(type='BaseSampler'), alpha=2.0))
    assert type(s) is samplers.CFGSampler and type(s._sampler) is samplers.BaseSampler
    assert type(VQSMSamplerRegistry.build(dict(type='BaseSampler'))) is samplers.BaseSampler     # configs/llamagen/ar.py:17
    assert s.fused_arguments() == dict(temperature=1.0, top_k=0, top_p=2.0, cfg_alpha=2.0)
    from vector_quantization_amd import integration
    assert integration.REPLACED_SAMPLERS == {'VQSMSamplerRegistry': ('BaseSampler', 'TopKTopPSampler', 'CFGSampler')}
    for n in integration.REPLACED_SAMPLERS['VQSMSamplerRegistry']:
        assert VQSMSamplerRegistry.resolve(n) is getattr(samplers, n)


def test_route_reasons():
    s = samplers.TopKTopPSampler()
    x = torch.zeros(4, 32)
    r = routes.sampler_why(s, x)
    assert r.name == 'torch' and 'cpu' in r.why
    meta = torch.zeros(4, 32, device='meta')

    class Fake:
        """A tensor as the route decision sees it (no GPU here)."""
        def __init__(self, t, cuda=True):
            self.t, self.is_cuda = t, cuda
        def __getattr__(self, n):
            return getattr(self.t, n)

    assert routes.sampler_why(s, Fake(meta)) == routes.Route('fused')
    assert 'stride 1' in routes.sampler_why(s, Fake(meta.t())).why
    assert 'float64' in routes.sampler_why(s, Fake(torch.zeros(4, 32, dtype=torch.float64, device='meta'))).why
    assert '2^20' in routes.sampler_why(s, Fake(torch.zeros(1, (1 << 20) + 1, device='meta'))).why
    assert routes.sampler_why(s, Fake(torch.zeros(1, (1 << 20) + 1, device='meta')), 1, (1 << 20) + 1).name == 'fused'

    class Mine(samplers.TopKTopPSampler):
        def sample(self, logits, memo):
            return super().sample(logits * 2, memo)

    assert 'overrides sample' in routes.sampler_why(Mine(), Fake(meta)).why
    assert 'inner' in routes.sampler_why(samplers.CFGSampler(sampler=Mine(), alpha=1.5), Fake(meta)).why
    nested = samplers.CFGSampler(sampler=samplers.CFGSampler(sampler=s, alpha=1.0), alpha=1.5)
    assert 'inner' in routes.sampler_why(nested, Fake(meta)).why
    assert routes.sampler_why(samplers.CFGSampler(sampler=s, alpha=1.5), Fake(meta)).name == 'fused'

    # what the op would refuse takes the torch route with a reason instead
    assert 'overlap' in routes.sampler_why(s, Fake(meta[:1].expand(4, 32))).why
    assert 'slice' in routes.sampler_why(s, Fake(meta), 0, 33).why and 'slice' in routes.sampler_why(s, Fake(meta), 5, 5).why
    assert 'slice' in routes.sampler_why(s, Fake(meta[:, :16]), 0, 20).why
    for t in (0.0, -1.0, float('inf'), float('nan')):
        assert 'temperature' in routes.sampler_why(samplers.TopKTopPSampler(temperature=t), Fake(meta)).why
    assert 'temperature' in routes.sampler_why(samplers.CFGSampler(sampler=samplers.TopKTopPSampler(temperature=0.0), alpha=1.5), Fake(meta)).why
    cube = torch.zeros(2, 3, 32, device='meta')
    assert routes.sampler_why(s, Fake(cube)).name == 'fused'
    assert 'flatten' in routes.sampler_why(s, Fake(cube.transpose(0, 1))).why

    class Quiet(samplers.BaseSampler):                                             # a subclass that keeps sample() stays fused
        pass

    assert routes.sampler_why(Quiet(), Fake(meta)).name == 'fused'


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_cpu_logits_take_the_torch_route(dtype):
    torch.manual_seed(0)
    x = torch.randn(2, 3, 200).to(dtype)
    for s in (samplers.BaseSampler(), samplers.TopKTopPSampler(top_k=20), samplers.CFGSampler(sampler=samplers.TopKTopPSampler(top_k=20), alpha=1.75)):
        tokens, memo = s(x, 50, 150, {})
        assert s.last_route.name == 'torch' and tokens.shape == (2, 3) and tokens.dtype == torch.int64
        assert bool(((tokens >= 50) & (tokens < 150)).all())
        if isinstance(s, samplers.CFGSampler):
            flat = tokens.reshape(-1)
            assert torch.equal(flat[:3], flat[3:])
    # memo['u']: the inverse CDF in index order; u = 0 is the first kept token
    s = samplers.TopKTopPSampler(top_k=5, top_p=2.0)
    xs = torch.randn(4, 100)
    tokens, _ = s(xs, 0, 100, {'u': torch.zeros(4)})
    top5 = xs.topk(5).indices.sort(-1).values
    assert torch.equal(tokens, top5[:, 0])


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libvqhip.so is not built')
    return _lib.lib()


def test_abi_limits_are_refused_without_a_gpu(lib):
    fake = ctypes.c_void_p(0x1000)

    def call(logits=fake, dtype=0, R=4, stride=100, start=0, end=100, alpha=1.5, cfg=0, t=1.0, k=0, p=2.0, u=fake, tokens=fake):
        return lib.vqhip_sample_tokens(logits, dtype, R, stride, start, end, alpha, cfg, t, k, p, u, tokens, None, None)

    for kw in (dict(logits=None), dict(u=None), dict(tokens=None), dict(dtype=2), dict(dtype=9), dict(R=0), dict(R=1 << 31),
               dict(R=3, cfg=1), dict(start=-1), dict(start=100), dict(start=50, end=50), dict(end=101),
               dict(stride=(1 << 20) + 10, end=(1 << 20) + 1), dict(t=0.0), dict(t=-1.0), dict(t=float('inf')), dict(t=float('nan')),
               dict(cfg=1, alpha=float('inf')), dict(cfg=1, alpha=float('nan'))):
        assert call(**kw) == -22, kw
        assert b'vqhip_sample_tokens' in lib.vqhip_last_error()
    assert ctypes.sizeof(_lib.SampleCut) == 24
    assert _lib.sample_delta(16384) == ref.delta(16384) == 2.0 ** -18 + 16384 * 2.0 ** -39


def test_cpu_tensors_are_refused_by_the_op():
    from vector_quantization_amd import ops
    with pytest.raises(_lib.VqhipError):
        ops.sample_tokens(torch.zeros(2, 8), 0, 8, u=torch.zeros(2))


def test_the_reference_slice_clamps_on_the_torch_route():
    """end beyond the last dimension: the reference's slice clamps, and so does the torch route the decision falls back to."""
    s = samplers.TopKTopPSampler(top_k=4)
    tokens, _ = s(torch.randn(3, 20), 5, 50, {})
    assert s.last_route.name == 'torch' and bool(((tokens >= 5) & (tokens < 20)).all())


@pytest.mark.parametrize('V', ref.VS + ref.BIG_VS)
def test_gpu_cases_have_few_ambiguous_tokens(V):
    """The GPU top-p checks accept a cut anywhere inside the ambiguous run; that is a meaningful check only while the run is
    short: at most 16 tokens per row and 1 % of the tokens of a case, at the header's delta."""
    for (v, start, R, dtype, seed) in ref.cases():
        if v != V:
            continue
        a = ref.keys(ref.make_logits(v, start, R, dtype, seed)[:, start:start + v])
        for top_k in ref.TOP_P_KS:
            for top_p in ref.TOP_PS:
                n = 0
                for r in range(R):
                    rc = ref.RowCut(a[r], top_k, top_p, ref.delta(v))
                    assert rc.ambiguous <= 16, (v, start, dtype, top_k, top_p, r, rc.ambiguous)
                    n += rc.ambiguous
                assert n <= 0.01 * R * v, (v, start, dtype, top_k, top_p, n)
