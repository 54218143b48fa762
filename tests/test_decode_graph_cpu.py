"""The replayed decode step without a GPU: the two prototypes in the header-derived binding, every new VQHIP_EINVAL clause refused
before any HIP call, ``functional.decode_attention_at_torch`` / ``decode_advance_torch`` against their by-value siblings and their
definition, the step callable of ``DecodeGraph`` run eagerly against ``_walk_static`` in float64, every clause of
``routes.llama_graph_why``, and that ``graph`` is off by default and changes nothing on the CPU."""
import copy
import ctypes
from types import SimpleNamespace

import pytest
import torch

from vector_quantization_amd import _lib, functional, samplers
from vector_quantization_amd.decode_graph import DecodeGraph
from vector_quantization_amd.kv_cache import StaticKVCache
from vector_quantization_amd.llama_weights import LlamaWeights
from vector_quantization_amd.quantizers import routes
from vector_quantization_amd.transformers import LlamaTransformer

from vector_quantization_amd.registries import VQSMTransformerRegistry

from llama_models import TINY, VOCABULARY, build_tiny, exact64
from test_decode_attention_cpu import _Tokens

F64 = torch.float64
EINVAL = -22
CODEBOOK = SimpleNamespace(start=8, end=48)


@pytest.fixture(scope='module')
def lib():
    if not _lib.os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_the_prototypes_are_bound_from_the_header():
    res, args = _lib.SIGNATURES['vqhip_decode_attention_at']
    by_value = _lib.SIGNATURES['vqhip_decode_attention'][1]
    assert res is _lib._i32 and len(args) == 20 and args[11] is _lib._vp and by_value[11] is _lib._i64       # pos in place of seen
    assert args[:11] == by_value[:11] and args[12:] == by_value[12:]
    assert _lib.SIGNATURES['vqhip_decode_advance'] == (_lib._i32, [_lib._vp] * 3 + [_lib._i64] * 2 + [_lib._vp] * 2)


def _at(lib, pos=0x2000, cap=9, cos=0x1000, q=0x1000):
    p = ctypes.c_void_p
    return lib.vqhip_decode_attention_at(p(q), 64, p(0x1000), 32, p(0x1000), 32, _lib.DTYPE_F32, p(cos), p(0x1000), p(0x1000), p(0x1000),
                                         p(pos) if pos else None, cap, 0.25, 2, 4, 2, 16, p(0x1000), None)


def test_every_new_clause_is_refused_before_any_hip_call(lib):
    assert _at(lib, pos=0) == EINVAL and b'vqhip_decode_attention_at: pos is required' in lib.vqhip_last_error()
    for off in (1, 2, 3):
        assert _at(lib, pos=0x2000 + off) == EINVAL and b'pos must be 4-byte aligned' in lib.vqhip_last_error()
    # the clauses it shares with the by-value form, under its own name
    assert _at(lib, cap=0) == EINVAL and b'vqhip_decode_attention_at: cap must be in 1' in lib.vqhip_last_error()
    assert _at(lib, cap=_lib.ATTN_MAX_LEN + 1) == EINVAL and b'cap must be in 1' in lib.vqhip_last_error()
    assert _at(lib, cos=0) == EINVAL and b'are required' in lib.vqhip_last_error()
    assert _at(lib, q=0x1002) == EINVAL and b'alignment of their element type' in lib.vqhip_last_error()

    p = ctypes.c_void_p

    def advance(token=0x1000, nxt=0x1000, sequence=0x1000, R=4, length=9, pos=0x2000):
        return lib.vqhip_decode_advance(*(p(a) if a else None for a in (token, nxt, sequence)), R, length, p(pos) if pos else None, None)
    for name in ('token', 'nxt', 'sequence', 'pos'):
        assert advance(**{name: 0}) == EINVAL and b'vqhip_decode_advance: token, next, sequence and pos are required' in lib.vqhip_last_error()
    assert advance(length=1) == EINVAL and b'length must be in 2 .. VQHIP_ATTN_MAX_LEN' in lib.vqhip_last_error()
    assert advance(length=_lib.ATTN_MAX_LEN + 1) == EINVAL and b'length must be in 2' in lib.vqhip_last_error()
    assert advance(R=0) == EINVAL and b'R must be in 1' in lib.vqhip_last_error()
    assert advance(R=1 << 31) == EINVAL and b'R must be in 1' in lib.vqhip_last_error()
    assert advance(pos=0x2001) == EINVAL and b'pos 4-byte aligned' in lib.vqhip_last_error()
    assert advance(sequence=0x1004) == EINVAL and b'8-byte aligned' in lib.vqhip_last_error()


def _tables(cap, Dh):
    pos = torch.arange(cap, dtype=torch.float32)[:, None] * (1e4 ** (-torch.arange(0, Dh, 2) / Dh))[None]
    return torch.cat((pos, pos), -1).cos(), torch.cat((pos, pos), -1).sin()


@pytest.mark.parametrize('dtype', [F64, torch.float32], ids=['f64', 'f32'])
@torch.no_grad()
def test_the_restatement_at_a_device_position_is_the_by_value_one(dtype):
    B, Hq, Hkv, Dh, cap = 3, 4, 2, 16, 9
    gen = torch.Generator().manual_seed(5)
    cos, sin = _tables(cap, Dh)
    at, by_value = StaticKVCache(1, B, Hkv, cap, Dh, dtype, 'cpu'), StaticKVCache(1, B, Hkv, cap, Dh, dtype, 'cpu')
    assert at._position is None and at.position.dtype == torch.int32 and at.position.shape == (1,) and int(at.position) == 0
    for t in range(cap):
        q, k, v = (torch.randn(B, H * Dh, generator=gen).to(dtype) for H in (Hq, Hkv, Hkv))
        got = functional.decode_attention_at(q, k, v, cos, sin, at, 0)                       # a CPU tensor: the restatement
        want = functional.decode_attention_torch(q, k, v, cos[t], sin[t], by_value, 0)
        assert got.dtype == dtype and torch.equal(got, want) and torch.equal(at._store, by_value._store)
        by_value.advance(1)
        at.position.add_(1)                                                                  # (the host count is not read)
    assert int(at.position) == cap and at.get_seq_length() == 0
    before = at._store.clone()
    out = functional.decode_attention_at(q, k, v, cos, sin, at, 0)                           # pos = cap: nothing is written
    assert torch.equal(at._store, before) and not out.any()
    at.position.fill_(-1)
    functional.decode_attention_at_torch(q, k, v, cos, sin, at, 0)
    assert torch.equal(at._store, before)
    with pytest.raises(ValueError, match='not on a GPU'):
        functional.decode_attention_at(q, k, v, cos, sin, at, 0, strict=True)


def test_the_position_follows_the_host_count_only_when_asked():
    cache = StaticKVCache(1, 2, 1, 6, 16)
    cache.advance(3)
    assert cache._position is None                                               # a cache that never asks has none
    assert int(cache.position) == 3
    cache.advance(2)
    assert int(cache.position) == 3 and int(cache.sync_position()) == 5 and cache.position is cache.sync_position()
    cache.reset()
    assert int(cache.position) == 0 and cache.get_seq_length() == 0


def test_decode_advance_in_torch():
    length = 5
    sequence = torch.full((3, length), 7)
    nxt, pos = torch.zeros(3, 1, dtype=torch.int64), torch.tensor([1], dtype=torch.int32)
    functional.decode_advance(torch.tensor([11, -1, 13]), nxt, sequence, pos)                # CPU tensors: the restatement
    assert sequence.tolist() == [[7, 7, 11, 7, 7], [7, 7, -1, 7, 7], [7, 7, 13, 7, 7]]       # the -1 stays visible
    assert nxt.tolist() == [[11], [0], [13]] and int(pos) == 2                               # and is clamped for the next step
    functional.decode_advance(torch.tensor([1, 2, 3]), nxt, sequence, pos)
    assert sequence[:, 3].tolist() == [1, 2, 3] and int(pos) == 3
    functional.decode_advance(torch.tensor([4, 5, 6]), nxt, sequence, pos)
    assert sequence[:, 4].tolist() == [4, 5, 6] and int(pos) == length - 1
    before = sequence.clone()
    for s in (length - 1, length, -1):                                           # saturated, or outside: nothing is written
        pos.fill_(s)
        functional.decode_advance(torch.tensor([9, 9, 9]), nxt, sequence, pos)
        assert torch.equal(sequence, before) and nxt.tolist() == [[4], [5], [6]] and int(pos) == s
    with pytest.raises(ValueError, match='not on a GPU'):
        functional.decode_advance(torch.tensor([9, 9, 9]), nxt, sequence, pos, strict=True)


@pytest.mark.parametrize('kv_heads', [4, 2], ids=['mha', 'gqa'])
@torch.no_grad()
def test_the_step_of_the_graph_is_the_walk_behind_a_static_cache(kv_heads):
    m = exact64(build_tiny(num_key_value_heads=kv_heads))
    B, length = 3, 9
    tokens = torch.randint(0, 48, (B, length), generator=torch.Generator().manual_seed(2))
    graph = DecodeGraph(m, B, length, CODEBOOK, device='cpu', cache_dtype=F64)
    graph.begin(tokens[:, :1])
    assert graph.cos.dtype == torch.float32 and graph.cos.shape == (length, 16) and graph.weights('qkv', 0).dtype == F64
    cache = StaticKVCache.for_model(m._transformer.config, B, length, F64, 'cpu')
    for t in range(length):
        graph.token.copy_(tokens[:, t:t + 1])                                    # the fixed sequence in place of the step's own draw
        graph.step(torch_ops=True)
        want = m._walk_static(tokens[:, t:t + 1], cache, torch_ops=True)
        assert torch.equal(graph.logits, want[:, 0]), t
        assert int(graph.cache.position) == min(t + 1, length - 1)               # counted on the device, saturating
        if t + 1 < length:
            assert torch.equal(graph.sequence[:, t + 1:t + 2].clamp(min=0), graph.token) and int(graph.token.min()) >= 8
    assert torch.equal(graph.cache._store, cache._store)
    assert copy.deepcopy(graph) is None


@torch.no_grad()
def test_the_graph_form_of_the_weight_set_is_the_eager_one_and_follows_the_parameters_in_place():
    m = exact64(build_tiny(num_key_value_heads=2))
    eager = LlamaWeights(m).pack()
    graph = LlamaWeights(m).allocate('cpu')
    graph.refresh()
    keys = graph.entries()
    assert keys == eager.entries() == [(name, i) for i in range(2) for name in ('qkv', 'gate_up', 'o', 'down')] + [('lm_head', None)]
    assert all(graph(*key).dtype == F64 and torch.equal(graph(*key), eager(*key)) for key in keys)
    attn = m._transformer.model.layers[1].self_attn
    assert eager('o', 1) is attn.o_proj.weight and graph('o', 1) is attn.o_proj.weight       # not cast: the module's own parameter
    assert eager('qkv', 1).shape == (64 + 2 * 32, 64) and torch.equal(eager('qkv', 1)[64:96], attn.k_proj.weight)
    cast = LlamaWeights(m, torch.float32).allocate('cpu')                        # under a dtype the single projections are held too
    cast.refresh()
    assert set(cast.held) == set(keys) and all(torch.equal(cast(*key), eager(*key).float()) for key in keys)
    before = {key: cast(*key).data_ptr() for key in keys}
    stale = cast('qkv', 1).clone()
    attn.k_proj.weight.mul_(1.5)                                                 # trained in place between two generate calls
    assert torch.equal(cast('qkv', 1), stale)
    for form in (graph, cast):
        form.refresh()
    now = LlamaWeights(m).pack()
    assert {key: cast(*key).data_ptr() for key in keys} == before and not torch.equal(cast('qkv', 1), stale)
    assert all(torch.equal(graph(*key), now(*key)) and torch.equal(cast(*key), now(*key).float()) for key in keys)
    assert torch.equal(graph('qkv', 1)[64:96], attn.k_proj.weight) and torch.equal(graph('qkv', 1)[:64], eager('qkv', 1)[:64])


def test_every_clause_of_llama_graph_why():
    m = build_tiny()
    m.static_cache = m.graph = True
    tokens = _Tokens((2, 3))
    assert routes.llama_graph_why(m, tokens, 9) == routes.Route('graph')
    assert routes.llama_graph_why(m, tokens, 6) == routes.Route('graph')        # two steps behind the prompt's draw
    reasons = []

    def refused(module, length=9, tok=tokens):
        r = routes.llama_graph_why(module, tok, length)
        assert r.name == 'decode' and r.why
        reasons.append(r.why)
        return r.why

    off = copy.copy(m)
    off._graph = False
    assert refused(off) == 'graph=False'
    dynamic = copy.copy(m)
    dynamic.static_cache = False
    assert refused(dynamic) == 'static_cache=False'
    for name in ('sample', '_generate'):
        own = copy.copy(m)
        own.__class__ = type('Own', (LlamaTransformer,), {name: lambda self, *a, **k: getattr(LlamaTransformer, name)(self, *a, **k)})
        assert refused(own) == f'Own overrides {name}'
    class Hot(samplers.BaseSampler):
        def sample(self, logits, memo):
            return super().sample(logits, memo)
    for sampler, clause in ((Hot(), 'Hot overrides sample'), (samplers.TopKTopPSampler(temperature=0.0), 'temperature=0.0')):
        cold = copy.copy(m)
        cold._modules = dict(m._modules, _sampler=sampler)
        why = refused(cold)
        assert why.startswith('the sampler takes its torch route: ') and clause in why
    assert 'nothing to replay' in refused(m, 5) and 'nothing to replay' in refused(m, 4)
    assert len(set(reasons)) == len(reasons) == 8

    # what llama_decode_why refuses comes back as it is: an overridden _walk_static, CPU tokens
    walk = copy.copy(m)
    walk.__class__ = type('Own', (LlamaTransformer,), {'_walk_static': lambda self, *a, **k: None})
    assert routes.llama_graph_why(walk, tokens, 9) == routes.Route('walk', 'Own overrides _walk_static')
    cpu = torch.zeros(2, 3, dtype=torch.long)
    assert routes.llama_graph_why(m, cpu, 9) == routes.llama_why(m, cpu) and 'not on a GPU' in routes.llama_why(m, cpu).why


def test_graph_is_off_by_default_and_changes_nothing_on_the_cpu():
    m = build_tiny()
    assert m.graph is False and m.graph_route is None and m._decode_graph is None
    prompt, u = torch.tensor([[1], [2]]), torch.tensor([0.3, 0.8])
    want, _ = m.generate(prompt, 6, CODEBOOK, {'sampler': {'u': u}})
    assert m.graph_route is None
    torch.manual_seed(0)
    on = VQSMTransformerRegistry.build(dict(type='LlamaTransformer', transformer=dict(TINY), vocabulary_size=VOCABULARY,
                                            sampler=dict(type='BaseSampler'), static_cache=True, graph=True)).eval()
    on.load_state_dict(m.state_dict())
    assert on.graph is True and on.static_cache is True
    got, _ = on.generate(prompt, 6, CODEBOOK, {'sampler': {'u': u}})
    assert torch.equal(got, want) and on.graph_route.name == 'torch' and 'not on a GPU' in on.graph_route.why
    assert on.last_route.name == 'torch' and on._decode_graph is None
    on.graph = False
    assert on.graph is False
