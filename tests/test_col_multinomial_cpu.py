"""CPU checks of the fused MultinomialAnchor: the numpy restatement (col_multinomial_ref.py) against the float64 softmax of the
torch reference, its frequencies, mutations the acceptance rule must refuse, the route decision, the module on CPU tensors, the
argument errors of ``ops.col_multinomial`` and the ABI limits."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import col_multinomial_ref as ref
from oracle import synth, torch_ref
from vector_quantization_amd import _lib, ops
from vector_quantization_amd import quantizers as Q
from vector_quantization_amd.quantizers import routes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _golden_distances():
    g = np.load(os.path.join(GOLDEN, 'anchors_alt.npz'))
    spec = json.loads(str(g['spec']))
    N, K, D = spec['N'], spec['K'], spec['D']
    x, w = synth.make_inputs('normal', spec['seed'], N, K, D)
    w = synth.unit_rows(w)
    assert synth.sha(x) == str(g['x_sha']) and synth.sha(w) == str(g['w_sha'])
    d = torch_ref.l2_distance(torch.from_numpy(x), torch.from_numpy(w)).numpy().astype(np.float32)
    return d, g['multinomial_probs']


def test_delta_is_the_headers_macro():
    text = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'vqhip.h')).read()
    assert '#define VQHIP_SAMPLE_DELTA(V) (3.814697265625e-06 + (double)(V) * 1.8189894035458565e-12)' in text
    for N in (1, 257, 3000, 1 << 20):
        assert ref.delta(N) == 3.814697265625e-06 + N * 1.8189894035458565e-12 == _lib.sample_delta(N)
    assert _lib.COL_MULTINOMIAL_MAX_N == 1 << 20 and '#define VQHIP_COL_MULTINOMIAL_MAX_N (1ll << 20)' in text


def test_reference_against_torch_on_the_golden():
    """``pick`` draws from the distribution the reference's ``d.t().softmax(1)`` is: the recorded fp32 shares of the golden equal
    the float64 shares, and for every u of a grid the picked row is the inverse CDF of the float64 shares — exactly where u is
    further than delta from every boundary, within delta everywhere."""
    d, probs = _golden_distances()
    N, K = d.shape
    sh = ref.shares64(d)                                                         # [K, N]
    np.testing.assert_allclose(sh, probs, rtol=2e-5, atol=1e-8)
    t = torch.from_numpy(d).double().t().softmax(1).numpy()
    np.testing.assert_allclose(sh, t, rtol=1e-12, atol=0)
    cum = np.cumsum(sh, axis=1)
    dlt = ref.delta(N)
    decided = 0
    for i, u0 in enumerate(np.linspace(0.0, 1.0, 41, endpoint=False)):
        u = np.full(K, u0, dtype=np.float32) if i % 2 == 0 else ref.uniforms(K, i)
        idx = ref.pick(d, u)
        assert ref.check_pick(d, u, idx, dlt).ok.all()
        want = np.array([np.searchsorted(cum[k], float(u[k]), side='right') for k in range(K)])
        clear = np.abs(cum - u.astype(np.float64)[:, None]).min(1) > dlt
        assert np.array_equal(idx[clear], want[clear])
        decided += int(clear.sum())
    assert decided > 0.99 * 41 * K


def test_frequencies_reproduce_the_shares():
    """Over an even grid of G uniforms a row is picked (its share) G times, to within the two grid points at its ends and delta."""
    g = np.random.default_rng(5)
    N, K, G = 37, 6, 4096
    d = g.normal(0, 2, size=(N, K)).astype(np.float32)
    sh = ref.shares64(d)
    counts = np.zeros((K, N))
    for u0 in (np.arange(G, dtype=np.float64) + 0.5) / G:
        idx = ref.pick(d, np.full(K, u0, dtype=np.float32))
        counts[np.arange(K), idx] += 1
    assert np.abs(counts / G - sh).max() <= 2.0 / G + 2 * ref.delta(N)
    assert (counts.sum(1) == G).all()


def _mutation_case():
    g = np.random.default_rng(11)
    N, K = 257, 130
    # flat columns (no row holds more than a few percent of a column) on top of a ramp along the rows: the cumulative shares
    # of another distribution then differ from the right ones systematically, by far more than one row's interval everywhere
    # but at the two ends, and a wrong draw lands inside the right row's interval only there or by chance
    d = (g.normal(0, 0.5, size=(N, K)) + np.linspace(-1, 1, N)[:, None]).astype(np.float32)
    assert ref.shares64(d).max() < 0.08
    return d, ref.uniforms(K, 12), N, K


def test_the_definition_passes_its_own_rule():
    d, u, N, K = _mutation_case()
    c = ref.check_pick(d, u, ref.pick(d, u), ref.delta(N))
    assert c.ok.all() and c.worst <= 1.0


@pytest.mark.parametrize('mutation', ['softmax_of_minus_d', 'rows_and_columns_swapped', 'off_by_one_row', 'max_per_row'])
def test_mutations_fail_the_rule_in_nearly_all_columns(mutation):
    d, u, N, K = _mutation_case()
    if mutation == 'softmax_of_minus_d':
        idx = ref.pick(-d, u)
    elif mutation == 'rows_and_columns_swapped':                                  # the draw along the rows of a [K, K] corner
        idx = ref.pick(np.ascontiguousarray(d[:K, :K].T), u)
    elif mutation == 'off_by_one_row':
        idx = (ref.pick(d, u) + 1) % N
    else:                                                                         # masses exp(d - max of the ROW): shares off by exp(-rowmax[n])
        idx = ref.pick((d - d.max(1, keepdims=True)).astype(np.float32), u)
    ok = ref.check_pick(d, u, idx, ref.delta(N)).ok
    assert ok.mean() < 0.1, (mutation, ok.mean())


def test_bad_columns_need_minus_one_and_nothing_else_does():
    d, u, N, K = _mutation_case()
    d[5, 3] = np.nan
    d[9, 7] = np.inf
    d[1, 11] = -np.inf                                                            # an ordinary row of mass 0
    idx = ref.pick(d, u)
    assert idx[3] == -1 and idx[7] == -1 and idx[11] >= 0 and (idx >= 0).sum() == K - 2
    assert ref.check_pick(d, u, idx, ref.delta(N)).ok.all()
    wrong = idx.copy()
    wrong[3] = 0
    wrong[20] = -1
    ok = ref.check_pick(d, u, wrong, ref.delta(N)).ok
    assert not ok[3] and not ok[20] and ok.sum() == K - 2


def test_planted_uniforms_and_a_dominant_row():
    g = np.random.default_rng(2)
    N, K = 63, 7
    d = g.normal(0, 1, size=(N, K)).astype(np.float32)
    d[:3] -= 100.0                                                                # the first three rows have no mass
    d[-2:] -= 100.0                                                               # nor the last two
    assert (ref.pick(d, np.zeros(K, dtype=np.float32)) == 3).all()
    assert (ref.pick(d, np.full(K, np.nextafter(np.float32(1), np.float32(0)))) == N - 3).all()
    d[17] += 40.0                                                                 # farther than every other row by more than 28
    for u0 in (0.0, 0.3, 0.999999):
        assert (ref.pick(d, np.full(K, u0, dtype=np.float32)) == 17).all()


# ---- the route ---------------------------------------------------------------------------------------------------------------

class _StubDistance(Q.BaseDistance):
    """A distance with a CPU matrix: the handle's tensor behaviour and the route clauses need no device."""
    metric = 'L2'
    FUSED_ENTROPY_METRICS = ('L2',)

    def forward(self, x, e):
        return torch.cdist(x.float(), e.float())

    def argmin(self, x, e, hist=None, prepared=None):
        return torch.cdist(x.detach(), e.detach()).argmin(-1)


class _Meta:
    """What the route reads of a device tensor, without a device."""

    def __init__(self, shape, dtype=torch.float32, cuda=True):
        self.shape, self.dtype, self.is_cuda, self.device = tuple(shape), dtype, cuda, 'cuda:0' if cuda else 'cpu'

    def dim(self):
        return len(self.shape)


class _Handle(Q.LazyDistance):
    """A LazyDistance that reports a GPU: the clauses behind the device check, evaluated on this machine."""
    is_cuda = True


def _gpu_handle(N=10, K=6, metric='L2', dist=None):
    dist = dist or _StubDistance()
    return _Handle(dist, torch.randn(N, 4), torch.randn(K, 4), metric=metric)


def test_routing_gives_the_stated_route_and_reason():
    a = Q.MultinomialAnchor()
    x = _Meta((10, 4))
    assert routes.multinomial_anchor_why(a, _gpu_handle(), x) == routes.Route('fused', '')
    # CPU tensors
    xc, ec = torch.randn(10, 4), torch.randn(6, 4)
    r = routes.multinomial_anchor_why(a, Q.LazyDistance(_StubDistance(), xc, ec), xc)
    assert r.name == 'matrix' and 'not on a GPU' in r.why
    # a plain tensor: the caller already paid for the matrix
    r = routes.multinomial_anchor_why(a, torch.cdist(xc, ec), x)
    assert r.name == 'matrix' and 'is a matrix' in r.why and 'paid for' in r.why
    # a materialised handle likewise
    d = _gpu_handle()
    d.materialize()
    r = routes.multinomial_anchor_why(a, d, x)
    assert r.name == 'matrix' and 'materialised' in r.why
    # the bf16-autocast cosine: the reference's matrix is bf16 there
    cos = Q.CosineDistance(autocast='bf16')
    assert cos.metric == 'CosineBF16'
    r = routes.multinomial_anchor_why(a, _gpu_handle(dist=cos, metric='CosineBF16'), x)
    assert r.name == 'matrix' and 'CosineBF16' in r.why and 'fp32 definition' in r.why
    assert routes.multinomial_anchor_why(a, _gpu_handle(dist=Q.CosineDistance(autocast=None), metric='Cosine'), x).name == 'fused'
    # float64
    r = routes.multinomial_anchor_why(a, _gpu_handle(), _Meta((10, 4), torch.float64))
    assert r.name == 'matrix' and 'float64' in r.why
    # N > 2^20 (the handle carries the shape; nothing of that size is allocated)
    big = (1 << 20) + 1
    d = _Handle(_StubDistance(), torch.empty(big, 0), torch.randn(6, 0))
    r = routes.multinomial_anchor_why(a, d, _Meta((big, 0)))
    assert r.name == 'matrix' and '2^20' in r.why
    assert routes.multinomial_anchor_why(a, _Handle(_StubDistance(), torch.empty(1 << 20, 0), torch.randn(6, 0)),
                                         _Meta((1 << 20, 0))).name == 'fused'

    # a subclass that overrides _anchors or probabilities
    class Mine(Q.MultinomialAnchor):
        @staticmethod
        def probabilities(d):
            return Q.MultinomialAnchor.probabilities(d) ** 2

    class Other(Q.MultinomialAnchor):
        def _anchors(self, x, e, d, quant, p, memo):
            return super()._anchors(x, e, d, quant, p, memo)

    for cls, name in ((Mine, 'probabilities'), (Other, '_anchors')):
        r = routes.multinomial_anchor_why(cls(), _gpu_handle(), x)
        assert r.name == 'matrix' and r.why == f'{cls.__name__} overrides {name}'
    # fused=False
    r = routes.multinomial_anchor_why(Q.MultinomialAnchor(fused=False), _gpu_handle(), x)
    assert r == routes.Route('matrix', 'fused=False')
    # a distance that names no metric for the fused column passes
    class Plain(_StubDistance):
        FUSED_ENTROPY_METRICS = ()
    r = routes.multinomial_anchor_why(a, _gpu_handle(dist=Plain()), x)
    assert r.name == 'matrix' and 'no fused column draw' in r.why
    with pytest.raises(ValueError):
        Q.MultinomialAnchor(fused=True)


# ---- the module on CPU tensors ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fused', [None, False])
def test_module_on_cpu_takes_the_matrix_route_and_draws_as_before(fused, monkeypatch):
    """On CPU tensors the module takes 'matrix' and does exactly what it did: the same draw from the same generator state, then
    ``ops.gather_rows`` — which has no CPU path and says so (no quiet fall-back).  With the gather stubbed the anchors are the
    rows the seeded ``d.t().softmax(1).multinomial(1)`` picks."""
    g = torch.Generator().manual_seed(3)
    x, e = torch.randn(50, 4, generator=g), torch.randn(9, 4, generator=g)
    dist = _StubDistance()
    ma = Q.MultinomialAnchor(fused=fused)
    assert ma.last_route is None
    torch.manual_seed(7)
    with pytest.raises(_lib.VqhipError):
        ma(x, e, Q.LazyDistance(dist, x, e), None, torch.zeros(9))
    assert ma.last_route.name == 'matrix'
    assert ma.last_route.why == 'fused=False' if fused is False else 'not on a GPU' in ma.last_route.why
    monkeypatch.setattr(ops, 'gather_rows', lambda rows, idx: rows.float()[idx.reshape(-1)])
    for d in (Q.LazyDistance(dist, x, e), torch.cdist(x, e)):
        torch.manual_seed(7)
        a, _ = ma(x, e, d, None, torch.zeros(9))
        torch.manual_seed(7)
        want = torch.cdist(x, e).t().softmax(1).multinomial(1).reshape(-1)
        assert torch.equal(a, x[want]) and ma.last_route.name == 'matrix'


# ---- argument errors and ABI limits --------------------------------------------------------------------------------------------

def test_ops_col_multinomial_refuses_wrong_arguments():
    x, e = torch.zeros(12, 8), torch.zeros(5, 8)
    for u in (torch.zeros(4), torch.zeros(5, 1), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.bfloat16), [0.0] * 5):
        with pytest.raises(ValueError, match='u must be float32'):
            ops.col_multinomial(x, e, 'L2', u=u)
    with pytest.raises(ValueError, match='2\\^20'):
        ops.col_multinomial(torch.zeros((1 << 20) + 1, 1), torch.zeros(5, 1), 'L2', u=torch.zeros(5))
    with pytest.raises(ValueError, match='metric'):
        ops.col_multinomial(x, e, 'CosineBF16', u=torch.zeros(5))
    with pytest.raises(ValueError, match='block_rows'):
        ops.col_multinomial(x, e, 'L2', u=torch.zeros(5), block_rows=0)
    with pytest.raises(ValueError, match='latent dim'):
        ops.col_multinomial(x, torch.zeros(5, 4), 'L2', u=torch.zeros(5))
    with pytest.raises(_lib.VqhipError):                                          # everything right but the device: no CPU path
        ops.col_multinomial(x, e, 'L2', u=torch.zeros(5))


def test_abi_limits_are_checked_before_any_hip_call():
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    N, K, R = 3000, 130, 64
    need = L.vqhip_col_multinomial_workspace_bytes(N, K, R)
    blocks = -(-N // R)
    assert 16 * K + 8 * blocks * K <= need <= 16 * K + 8 * blocks * K + 4 * 256
    assert L.vqhip_col_multinomial_workspace_bytes(N, K, N) < L.vqhip_col_multinomial_workspace_bytes(N, K, 1)
    for bad in ((0, K, 1), ((1 << 20) + 1, K, R), (N, 0, R), (N, 1 << 31, R), (N, K, 0), (N, K, N + 1)):
        assert L.vqhip_col_multinomial_workspace_bytes(*bad) == 0
    calls = {
        'max': lambda tile, r0, n, k, r, ws, b: L.vqhip_col_multinomial_max(tile, r0, n, k, r, ws, b, None),
        'mass': lambda tile, r0, n, k, r, ws, b: L.vqhip_col_multinomial_mass(tile, r0, n, k, r, ws, b, None),
        'resolve': lambda tile, r0, n, k, r, ws, b: L.vqhip_col_multinomial_resolve(tile, r0, n, k, r, ws, b, fake, None),
    }
    for name, call in calls.items():
        for args in ((None, 0, N, K, R, fake, need), (fake, 0, N, K, R, None, need), (fake, 0, N, K, R, fake, need - 1),
                     (fake, 1, N, K, R, fake, need), (fake, R * blocks, N, K, R, fake, need), (fake, -R, N, K, R, fake, need),
                     (fake, 0, (1 << 20) + 1, K, R, fake, 1 << 40), (fake, 0, N, 1 << 31, R, fake, 1 << 50), (fake, 0, N, K, 0, fake, need)):
            assert call(*args) == -22, (name, args)
            assert f'vqhip_col_multinomial_{name}'.encode() in L.vqhip_last_error()
    assert L.vqhip_col_multinomial_resolve(fake, 0, N, K, R, fake, need, None, None) == -22
    for args in ((None, N, K, R, fake, need, fake), (fake, N, K, R, None, need, fake), (fake, N, K, R, fake, need, None),
                 (fake, N, K, R, fake, need - 1, fake), (fake, 0, K, R, fake, need, fake)):
        assert L.vqhip_col_multinomial_pick(*args, None) == -22
        assert b'vqhip_col_multinomial_pick' in L.vqhip_last_error()
    assert L.vqhip_col_multinomial_pick(fake, N, K, R, fake, need - 1, fake, None) == -22 and b'needed' in L.vqhip_last_error()
