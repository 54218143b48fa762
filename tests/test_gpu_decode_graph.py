"""The replayed decode step on the GPU: ``decode_attention_at`` bit for bit against the by-value kernel, its guard on the position,
one capture replayed over many positions, ``decode_advance``, and ``LlamaTransformer.generate`` with ``graph=True`` against the eager
decode route - tokens in fp32, the float64 yardstick of tests/test_gpu_llama_static_cache.py under bf16 autocast, reuse of the
captured graph, and a bad draw raised as ``ValueError``.

Every cache, output and sequence the kernels write is a view into a larger allocation with a sentinel on both sides: a store
outside the view lands in memory the test owns and shows as a changed sentinel."""
import contextlib
import copy
from types import SimpleNamespace

import pytest
import torch

from vector_quantization_amd import functional, samplers
from vector_quantization_amd.decode_graph import DecodeGraph
from vector_quantization_amd.kv_cache import StaticKVCache
from vector_quantization_amd.quantizers import routes

from llama_models import build_tiny, exact64

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
INT_OF = {8: torch.int64, 4: torch.int32, 2: torch.int16}
SENTINEL = 777.0
CAP = 300
# the edges of a wave's 8 positions and of a 32-position sweep: the PP = 8 geometry's (Dh = 64 in 16 bits, Dh = 24 in fp32), which
# the test below does not run - every geometry's own edges are in tests/test_gpu_decode_attention_geometry.py
SEENS = (0, 1, 7, 8, 255, 256, 299)
CODEBOOK = SimpleNamespace(start=8, end=48)
_BASE = {}


def bits(t):
    return t.contiguous().view(INT_OF[t.element_size()])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def tables(cap, Dh, theta=10000.0):
    """cos, sin fp32 [cap, Dh] as LlamaRotaryEmbedding computes them"""
    inv = 1.0 / (theta ** (torch.arange(0, Dh, 2, dtype=torch.float32) / Dh))
    f = torch.arange(cap, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((f, f), -1)
    return emb.cos().cuda(), emb.sin().cuda()


def framed(shape, dtype, fill=None, seed=0):
    """(the whole allocation [3, *shape], its middle): sentinels in front and behind, ``fill`` or random values inside"""
    whole = torch.full((3,) + tuple(shape), SENTINEL, dtype=dtype, device='cuda')
    if fill is None:
        whole[1] = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()
    else:
        whole[1] = fill
    return whole, whole[1]


def cache_in(whole):
    """A one-layer StaticKVCache whose K and V are the middle of ``whole`` [3, 2, B, Hkv, cap, Dh]"""
    cache = StaticKVCache(1, 1, 1, 1, 16, whole.dtype, 'cuda')
    cache._store = whole[1:2]
    assert cache._store.data_ptr() == whole[1].data_ptr() and cache.capacity == whole.shape[4]
    return cache


def rows(B, Hq, Hkv, Dh, dtype, seed):
    """q, k, v as views into packed rows whose stride is above (Hq + 2 Hkv) Dh"""
    nq, nk = Hq * Dh, Hkv * Dh
    r = torch.randn(B, nq + 2 * nk + 8, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()
    return r[:, :nq], r[:, nq:nq + nk], r[:, nq + nk:nq + 2 * nk]


@pytest.mark.parametrize('Dh', [16, 128])
@pytest.mark.parametrize('G', [1, 2, 8])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_every_byte_is_the_by_value_kernels(dtype, G, Dh):
    B, Hkv = 2, 2
    Hq, scale = G * Hkv, Dh ** -0.5
    cos, sin = tables(CAP, Dh)
    whole_at, _ = framed((2, B, Hkv, CAP, Dh), dtype, seed=1)
    whole_by = whole_at.clone()
    at, by_value = cache_in(whole_at), cache_in(whole_by)
    for seen in SEENS:
        q, k, v = rows(B, Hq, Hkv, Dh, dtype, seen)
        by_value._seen = seen
        want = functional.decode_attention(q, k, v, cos[seen], sin[seen], by_value, 0, scale=scale, strict=True)
        at.position.fill_(seen)
        out_whole, out = framed((B, Hq * Dh), dtype, fill=SENTINEL)
        got = functional.decode_attention_at(q, k, v, cos, sin, at, 0, scale=scale, strict=True, out=out)
        assert got.data_ptr() == out.data_ptr() and same(got, want), seen
        assert same(whole_at, whole_by), seen                                    # both caches whole, margins included
        assert bool((out_whole[0] == SENTINEL).all()) and bool((out_whole[2] == SENTINEL).all())
        assert int(at.position) == seen and at.get_seq_length() == 0             # the op reads the position and counts nothing
        assert same(functional.decode_attention_at(q, k, v, cos, sin, at, 0, scale=scale, strict=True), want)   # and allocates like its sibling


@pytest.mark.parametrize('pos', [CAP, -1, 2 ** 31 - 1])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_position_outside_the_cache_writes_nothing(dtype, pos):
    B, Hkv, G, Dh = 2, 2, 2, 16
    cos, sin = tables(CAP, Dh)
    whole, _ = framed((2, B, Hkv, CAP, Dh), dtype, seed=2)
    before = whole.clone()
    cache = cache_in(whole)
    cache.position.fill_(pos)
    q, k, v = rows(B, G * Hkv, Hkv, Dh, dtype, 3)
    out_whole, out = framed((B, G * Hkv * Dh), dtype, fill=SENTINEL)
    functional.decode_attention_at(q, k, v, cos, sin, cache, 0, scale=0.25, strict=True, out=out)
    torch.cuda.synchronize()
    assert same(whole, before) and bool((out_whole == SENTINEL).all()) and int(cache.position) == pos


def test_one_capture_serves_every_position():
    B, Hkv, G, Dh, cap, dtype = 2, 2, 2, 16, 16, torch.float32
    Hq = G * Hkv
    cos, sin = tables(cap, Dh)
    whole, _ = framed((2, B, Hkv, cap, Dh), dtype, seed=4)
    whole_by = whole.clone()
    by_value, cache = cache_in(whole_by), cache_in(whole)
    pristine = whole.clone()
    static = torch.zeros(B, (Hq + 2 * Hkv) * Dh + 8, dtype=dtype, device='cuda')
    nq, nk = Hq * Dh, Hkv * Dh
    q, k, v = static[:, :nq], static[:, nq:nq + nk], static[:, nq + nk:nq + 2 * nk]
    out_whole, out = framed((B, nq), dtype, fill=SENTINEL)
    seq_whole, sequence = framed((B, cap), torch.int64, fill=int(SENTINEL))
    token = torch.zeros(B, dtype=torch.int64, device='cuda')
    nxt = torch.zeros(B, dtype=torch.int64, device='cuda')

    def step():
        functional.decode_attention_at(q, k, v, cos, sin, cache, 0, scale=0.25, strict=True, out=out)
        functional.decode_advance(token, nxt, sequence, cache.position, strict=True)

    cache.position.fill_(6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                   # the warm-up torch asks for; undone below
    torch.cuda.current_stream().wait_stream(side)
    whole.copy_(pristine)
    sequence.fill_(int(SENTINEL))
    cache.position.fill_(6)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert int(cache.position) == 6 and same(whole, pristine)                    # the capture executed nothing
    for seen in range(6, 12):                                                    # across the slot edge at 8
        fresh = rows(B, Hq, Hkv, Dh, dtype, 50 + seen)
        for dst, src in zip((q, k, v), fresh):
            dst.copy_(src)
        token.copy_(torch.tensor([seen, -seen], device='cuda'))
        graph.replay()
        by_value._seen = seen
        want = functional.decode_attention(*fresh, cos[seen], sin[seen], by_value, 0, scale=0.25, strict=True)
        assert same(out, want), seen
        assert same(whole, whole_by), seen                                       # the caches whole, margins included
        assert sequence[:, seen + 1].tolist() == [seen, -seen] and nxt.tolist() == [seen, 0] and int(cache.position) == seen + 1
    assert int(cache.position) == 12
    assert bool((out_whole[0] == SENTINEL).all()) and bool((out_whole[2] == SENTINEL).all())
    assert bool((seq_whole[0] == int(SENTINEL)).all()) and bool((seq_whole[2] == int(SENTINEL)).all())
    assert same(whole[0], pristine[0]) and same(whole[2], pristine[2])


@pytest.mark.parametrize('R', [1, 5, 1000])
def test_decode_advance(R):
    length = 9
    seq_whole, sequence = framed((R, length), torch.int64, fill=int(SENTINEL))
    next_whole, nxt = framed((R,), torch.int64, fill=int(SENTINEL))
    token = torch.randint(8, 48, (R,), generator=torch.Generator().manual_seed(R)).cuda()
    token[R // 2] = -1
    pos = torch.tensor([3], dtype=torch.int32, device='cuda')
    functional.decode_advance(token, nxt, sequence, pos, strict=True)
    want = torch.full((R, length), int(SENTINEL), device='cuda')
    want[:, 4] = token
    assert torch.equal(sequence, want) and torch.equal(nxt, token.clamp(min=0)) and int(nxt[R // 2]) == 0 and int(pos) == 4
    for s in (length - 1, length, -1, 2 ** 31 - 1):                              # the last column, and outside: nothing is written
        pos.fill_(s)
        before = nxt.clone()
        functional.decode_advance(token + 1, nxt, sequence, pos, strict=True)
        assert torch.equal(sequence, want) and torch.equal(nxt, before) and int(pos) == s
    for whole in (seq_whole, next_whole):
        assert bool((whole[0] == int(SENTINEL)).all()) and bool((whole[2] == int(SENTINEL)).all())


# ---- generate ----------------------------------------------------------------------------------------------------------------

def base(kv_heads):
    if kv_heads not in _BASE:
        _BASE[kv_heads] = build_tiny(num_key_value_heads=kv_heads)
    return _BASE[kv_heads]


def sampler_of(kind):
    inner = samplers.TopKTopPSampler(temperature=1.0, top_k=20, top_p=0.95)
    return inner if kind == 'topk' else samplers.CFGSampler(sampler=inner, alpha=1.5)


def pair(kv_heads, kind='topk'):
    """(the model with graph=True, the same model on the eager decode route)"""
    graphed = copy.deepcopy(base(kv_heads)).cuda().eval()
    graphed._sampler = sampler_of(kind)
    graphed.static_cache = True
    eager = copy.deepcopy(graphed)
    graphed.graph = True
    return graphed, eager


def uniforms(n, seed=6):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)).cuda()


def count_calls(monkeypatch, owner, name):
    calls, inner = [], getattr(owner, name)

    def spy(self, *a, **k):
        calls.append(self)
        return inner(self, *a, **k)
    monkeypatch.setattr(owner, name, spy)
    return calls


PROMPTS = {1: torch.tensor([[1], [2], [3], [1]]), 3: torch.tensor([[1, 9, 30], [2, 40, 8], [3, 17, 17], [1, 9, 31]])}


@pytest.mark.parametrize('kind', ['topk', 'cfg'])
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('kv_heads', [4, 2], ids=['mha', 'gqa'])
def test_generate_replays_the_tokens_of_the_eager_decode_route(kv_heads, P, kind, monkeypatch):
    graphed, eager = pair(kv_heads, kind)
    prompt, length = PROMPTS[P].cuda(), 9
    u = uniforms(2 if kind == 'cfg' else 4)
    replays = count_calls(monkeypatch, torch.cuda.CUDAGraph, 'replay')
    want, _ = eager.generate(prompt, length, CODEBOOK, {'sampler': {'u': u}})
    assert eager.last_route == routes.Route('decode') and eager.graph_route is None and not replays
    got, memo = graphed.generate(prompt, length, CODEBOOK, {'sampler': {'u': u}})
    assert graphed.graph_route == graphed.last_route == routes.Route('graph') and graphed._packed is None
    assert got.shape == (4, length) and torch.equal(got, want) and 8 <= int(got[:, P:].min()) and int(got.max()) < 48
    assert len(replays) == length - P - 2                                        # the first step behind the prompt ran eagerly
    graph = graphed._decode_graph
    assert got.data_ptr() != graph.sequence.data_ptr() and torch.equal(got, graph.sequence) and graph.captures == 1
    assert graph.cache.get_seq_length() == int(graph.cache.position) == length - 1
    assert memo['sampler']['u'] is u


@pytest.mark.parametrize('kv_heads', [4, 2], ids=['mha', 'gqa'])
def test_generate_under_bf16_autocast_is_as_close_to_float64_as_the_torch_route(kv_heads):
    graphed, _ = pair(kv_heads)
    plain = copy.deepcopy(base(kv_heads)).cuda().eval()
    plain.fused = False
    prompt, length = PROMPTS[1].cuda(), 9
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        tokens, _ = graphed.generate(prompt, length, CODEBOOK, {'sampler': {'u': uniforms(4)}})
        torch_logits = plain._transformer(tokens)['logits']
    assert graphed.last_route == routes.Route('graph') and plain.last_route is None
    assert tokens.shape == (4, length) and torch.equal(tokens[:, :1], prompt) and 8 <= int(tokens[:, 1:].min()) and int(tokens.max()) < 48
    graph = graphed._decode_graph
    assert graph.logits.dtype == torch.bfloat16 and graph.cache.dtype == torch.bfloat16 and ('o', 0) in graph.weights.held
    with torch.no_grad():
        full = exact64(base(kv_heads))._transformer(tokens.cpu())['logits']
    # the last step read the token at length - 2 and predicted the one at length - 1
    e_graph = float((graph.logits.cpu().double() - full[:, length - 2]).abs().max())
    e_torch = float((torch_logits.cpu().double() - full).abs().max())
    print(f'last-step logits (autocast, {kv_heads} kv heads): graph {e_graph:.3e}, torch route over the same tokens {e_torch:.3e}')
    assert e_graph <= 2 * e_torch


def test_the_graph_is_reused_refreshed_and_dropped(monkeypatch):
    graphed, _ = pair(2)
    captures = count_calls(monkeypatch, DecodeGraph, 'capture')
    length = 9

    def both(prompt, u):
        eager = copy.deepcopy(graphed)
        eager.graph = False
        assert eager._decode_graph is None and eager.static_cache
        want, _ = eager.generate(prompt, length, CODEBOOK, {'sampler': {'u': u}})
        got, _ = graphed.generate(prompt, length, CODEBOOK, {'sampler': {'u': u}})
        assert eager.last_route == routes.Route('decode') and graphed.last_route == routes.Route('graph')
        assert torch.equal(got, want)
        return got

    first = both(PROMPTS[1].cuda(), uniforms(4))
    graph = graphed._decode_graph
    assert len(captures) == 1
    second = both(PROMPTS[1].flip(0).cuda() + 3, uniforms(4, seed=7))            # another prompt, other uniforms: nothing new is captured
    assert len(captures) == 1 and graphed._decode_graph is graph and not torch.equal(first, second)
    lm = graphed._transformer
    with torch.no_grad():                                                        # trained in place: packed, read in place, and the head
        lm.model.layers[0].self_attn.q_proj.weight.mul_(1.5)
        lm.model.layers[1].mlp.down_proj.weight.add_(0.05)
        lm.lm_head.weight.mul_(-1.0)
    third = both(PROMPTS[1].cuda(), uniforms(4))
    assert len(captures) == 1 and graphed._decode_graph is graph and not torch.equal(first, third)
    both(PROMPTS[1][:2].cuda(), uniforms(2))                                     # another batch size: a new capture
    assert len(captures) == 2 and graphed._decode_graph is not graph
    graphed.graph = False
    assert graphed._decode_graph is None
    tokens, _ = graphed.generate(PROMPTS[1].cuda(), length, CODEBOOK, {'sampler': {'u': uniforms(4)}})
    assert graphed.last_route == routes.Route('decode') and graphed._decode_graph is None and torch.equal(tokens, third)


def test_a_bad_draw_inside_a_replay_is_a_value_error():
    """The embedding row of a token that one sequence draws at column c >= 3 (and nobody earlier) is set to inf: every input up to
    there is finite and every draw up to there is the eager route's; the step that reads the token gives that row NaN logits, the
    sampler's -1 lands at column c + 1 from inside a replay, is clamped on the device, and the remaining replays run to the end."""
    graphed, eager = pair(4)
    prompt, length, u = PROMPTS[1].cuda(), 9, uniforms(4, seed=11)
    want, _ = eager.generate(prompt, length, CODEBOOK, {'sampler': {'u': u}})
    want = want.cpu()
    found = None
    for c in range(3, length - 1):
        for r in range(want.shape[0]):
            t = int(want[r, c])
            if found is None and not bool((want[:, :c] == t).any()) and int((want[:, c] == t).sum()) == 1:
                found = (r, c, t)
    assert found is not None, f'no token is drawn first at one place of columns 3 .. {length - 2}:\n{want}'
    r, c, t = found
    with torch.no_grad():
        graphed._transformer.model.embed_tokens.weight[t] = float('inf')
    with pytest.raises(ValueError, match=f'row {r} at column {c + 1} '):
        graphed.generate(prompt, length, CODEBOOK, {'sampler': {'u': u}})
    torch.cuda.synchronize()                                                     # no device assert fired
    sequence = graphed._decode_graph.sequence.cpu()
    assert torch.equal(sequence[:, :c + 1], want[:, :c + 1]) and int(sequence[r, c + 1]) == -1
    assert int(graphed._decode_graph.cache.position) == length - 1               # the steps behind it ran to the end
    assert int(torch.ones(3, device='cuda').sum()) == 3


@contextlib.contextmanager
def _capturing():
    one = torch.ones(4, device='cuda')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one + one                                                                # (a capture that is not empty)
        yield


def test_a_capturing_stream_is_a_clause_of_llama_graph_why():
    graphed, _ = pair(4)
    tokens = PROMPTS[3].cuda()
    assert routes.llama_graph_why(graphed, tokens, 9) == routes.Route('graph')
    seen = []
    with _capturing():
        seen.append(routes.llama_graph_why(graphed, tokens, 9))
    assert seen == [routes.Route('decode', 'the stream is already capturing')]
