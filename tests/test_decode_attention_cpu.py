"""The static KV cache and the decode-attention step without a GPU: the float64 restatement of tests/decode_attention_ref.py against
transformers' own ``LlamaAttention.forward`` behind a ``DynamicCache``, ``functional.*_torch`` against the restatement, the
bookkeeping of ``StaticKVCache``, every clause of ``routes.llama_decode_why``, the walk behind a ``StaticKVCache`` against HF's cached
forward in float64, and that ``static_cache=False`` leaves today's route and cache type alone."""
import copy
from types import SimpleNamespace

import pytest
import torch

from vector_quantization_amd import _lib, functional, ops
from vector_quantization_amd.kv_cache import StaticKVCache
from vector_quantization_amd.quantizers import routes
from vector_quantization_amd.transformers import LlamaTransformer

import decode_attention_ref as ref
from llama_models import build_tiny, exact64

F64 = torch.float64
B, PREFILL, STEPS = 3, 5, 4
_MODELS = {}


def tiny64(kv_heads):
    if kv_heads not in _MODELS:
        _MODELS[kv_heads] = exact64(build_tiny(num_key_value_heads=kv_heads))
    return _MODELS[kv_heads]


def _projections(attn, h):
    """rows [B L, H Dh] of q, k, v for hidden states h [B, L, hidden]"""
    rows = h.reshape(-1, h.shape[-1])
    return attn.q_proj(rows), attn.k_proj(rows), attn.v_proj(rows)


@pytest.mark.parametrize('kv_heads', [4, 2], ids=['mha', 'gqa'])
@torch.no_grad()
def test_the_restatement_is_transformers_attention_with_a_dynamic_cache(kv_heads):
    from transformers import DynamicCache
    m = tiny64(kv_heads)
    model = m._transformer.model
    attn = model.layers[0].self_attn
    Dh, total = attn.head_dim, PREFILL + STEPS
    h = torch.randn(B, total, model.config.hidden_size, dtype=F64, generator=torch.Generator().manual_seed(3))
    cos, sin = model.rotary_emb(h, position_ids=torch.arange(total).unsqueeze(0))
    hf_cache = DynamicCache(config=model.config)
    kc = torch.zeros(B, kv_heads, total, Dh, dtype=F64)
    vc = torch.zeros_like(kc)
    for lo, hi in [(0, PREFILL)] + [(t, t + 1) for t in range(PREFILL, total)]:
        want, _ = attn(hidden_states=h[:, lo:hi], position_embeddings=(cos[:, lo:hi], sin[:, lo:hi]), attention_mask=None,
                       past_key_values=hf_cache)
        q, k, v = _projections(attn, h[:, lo:hi])
        if hi - lo == 1:
            got = ref.decode64(q, k, v, cos[0, lo], sin[0, lo], kc, vc, lo, attn.scaling).reshape(B, 1, -1)
        else:
            q_rot = ref.append64(q, k, v, cos[0, lo:hi], sin[0, lo:hi], kc, vc, lo)
            got = torch.stack([ref.attend64(q_rot[:, :, t], kc[:, :, :t + 1], vc[:, :, :t + 1], attn.scaling)[0].reshape(B, -1)
                               for t in range(hi - lo)], 1)
        assert float((attn.o_proj(got) - want).abs().max()) <= 1e-12
    assert float((hf_cache.layers[0].keys - kc).abs().max()) <= 1e-12
    assert torch.equal(hf_cache.layers[0].values, vc)


@pytest.mark.parametrize('dtype', [F64, torch.float32, torch.bfloat16], ids=['f64', 'f32', 'bf16'])
@torch.no_grad()
def test_the_torch_restatements_are_the_definition(dtype):
    Hq, Hkv, Dh, cap = 4, 2, 16, 9
    gen = torch.Generator().manual_seed(5)
    pos = torch.arange(cap, dtype=torch.float32)[:, None] * (1e4 ** (-torch.arange(0, Dh, 2) / Dh))[None]
    cos, sin = torch.cat((pos, pos), -1).cos(), torch.cat((pos, pos), -1).sin()
    cache = StaticKVCache(1, B, Hkv, cap, Dh, dtype, 'cpu')
    kc64, vc64 = torch.zeros(B, Hkv, cap, Dh, dtype=F64), torch.zeros(B, Hkv, cap, Dh, dtype=F64)
    tol = {F64: 1e-14, torch.float32: 2e-6, torch.bfloat16: 2e-2}[dtype]

    def rows(n, H):
        return torch.randn(n, H * Dh, generator=gen).to(dtype)

    q, k, v = rows(B * PREFILL, Hq), rows(B * PREFILL, Hkv), rows(B * PREFILL, Hkv)
    got = functional.rope_append(q, k, v, cos[:PREFILL], sin[:PREFILL], cache, 0)           # a CPU tensor: the restatement
    want = ref.append64(q, k, v, cos[:PREFILL], sin[:PREFILL], kc64, vc64, 0)
    assert got.shape == (B, Hq, PREFILL, Dh) and got.dtype == dtype and float((got.to(F64) - want).abs().max()) <= tol
    cache.advance(PREFILL)
    for t in range(PREFILL, cap):
        q, k, v = rows(B, Hq), rows(B, Hkv), rows(B, Hkv)
        got = functional.decode_attention(q, k, v, cos[t], sin[t], cache, 0)
        want = ref.decode64(q, k, v, cos[t], sin[t], kc64, vc64, t, Dh ** -0.5)
        assert got.shape == (B, Hq * Dh) and got.dtype == dtype and float((got.to(F64) - want).abs().max()) <= tol
        cache.advance(1)
    kc, vc, seen = cache.layer(0)
    assert seen == cap and float((kc.to(F64) - kc64).abs().max()) <= tol and torch.equal(vc.to(F64), vc64)
    with pytest.raises(ValueError, match='not on a GPU'):
        functional.decode_attention(q, k, v, cos[0], sin[0], StaticKVCache(1, B, Hkv, cap, Dh, dtype, 'cpu'), 0, strict=True)


def test_ops_that_have_no_backward_refuse_inputs_that_require_grad():
    cache = StaticKVCache(1, 1, 1, 2, 16)
    q = torch.randn(1, 16, requires_grad=True)
    k, v, cos, sin = torch.randn(1, 16), torch.randn(1, 16), torch.ones(16), torch.zeros(16)
    with pytest.raises(ValueError, match='requires grad'):
        functional.decode_attention(q, k, v, cos, sin, cache, 0)
    with pytest.raises(ValueError, match='requires grad'):
        functional.rope_append(q, k, v, cos, sin, cache, 0)
    with torch.no_grad():
        assert functional.decode_attention(q, k, v, cos, sin, cache, 0).shape == (1, 16)


def test_static_kv_cache_counts_on_the_host_and_refuses_overflow():
    cache = StaticKVCache(2, 3, 2, 6, 16, torch.bfloat16)
    assert (cache.layers, cache.batch, cache.kv_heads, cache.capacity, cache.head_dim) == (2, 3, 2, 6, 16)
    assert cache.get_seq_length() == 0 and cache.dtype == torch.bfloat16
    k, v, seen = cache.layer(1)
    assert k.shape == v.shape == (3, 2, 6, 16) and seen == 0 and k.is_contiguous() and k.data_ptr() != v.data_ptr()
    assert cache.advance(5) == 5 and cache.layer(0)[2] == 5 and cache.get_seq_length() == 5
    with pytest.raises(ValueError, match='2 tokens behind 5 do not fit a capacity of 6'):
        cache.require_room(2)
    with pytest.raises(ValueError, match='do not fit'):
        cache.advance(2)
    assert cache.advance(1) == 6
    with pytest.raises(ValueError, match='do not fit'):
        cache.require_room(1)
    cache.reset()
    assert cache.get_seq_length() == 0
    with pytest.raises(ValueError, match='>= 1'):
        StaticKVCache(1, 1, 1, 0, 16)


def test_overflow_raises_before_the_walk_writes_anything():
    m = tiny64(4)
    cache = StaticKVCache.for_model(m._transformer.config, 1, 3, F64, 'cpu')
    with torch.no_grad():
        m._walk_static(torch.tensor([[1, 2, 3]]), cache, torch_ops=True)
        before = cache._store.clone()
        with pytest.raises(ValueError, match='do not fit'):
            m._walk_static(torch.tensor([[4]]), cache, torch_ops=True)
    assert torch.equal(before, cache._store) and cache.get_seq_length() == 3


class _Tokens:
    """What ``llama_decode_why`` reads of the tokens, claiming a GPU: the clauses are host logic and need none."""

    def __init__(self, shape, device='cuda:0'):
        self.shape, self.is_cuda, self.device = torch.Size(shape), True, torch.device(device)

    def dim(self):
        return len(self.shape)


class _OnGpu(StaticKVCache):
    """A cache without memory (meta) that reports the tokens' GPU as its device."""
    device = torch.device('cuda:0')


def _cache_for(m, batch=2, capacity=8, dtype=torch.float32, device='meta', cls=StaticKVCache):
    return cls.for_model(m._transformer.config, batch, capacity, dtype, device)


def test_every_clause_of_llama_decode_why():
    m = build_tiny()
    tokens, one = _Tokens((2, 3)), _Tokens((2, 1))
    assert routes.llama_decode_why(m, tokens, None) == routes.Route('decode')
    good = _cache_for(m, cls=_OnGpu)
    assert routes.llama_decode_why(m, tokens, good) == routes.Route('decode')
    # everything llama_why refuses comes back as it is
    assert routes.llama_decode_why(m, torch.zeros(2, 3, dtype=torch.long), None) == routes.llama_why(m, torch.zeros(2, 3, dtype=torch.long))
    plain = build_tiny(fused=False)
    assert routes.llama_decode_why(plain, tokens, None) == routes.Route('torch', 'fused=False')
    good.advance(2)
    r = routes.llama_decode_why(m, tokens, good)
    assert r.name == 'torch' and '3 tokens behind a cache of 2' in r.why
    assert routes.llama_decode_why(m, one, good) == routes.Route('decode')

    class Own(LlamaTransformer):
        def _walk_static(self, *a, **k):
            return super()._walk_static(*a, **k)
    own = copy.copy(m)
    own.__class__ = Own
    assert routes.llama_decode_why(own, tokens, None) == routes.Route('walk', 'Own overrides _walk_static')

    scaled = copy.deepcopy(m)
    scaled._transformer.model.rotary_emb.rope_type = 'linear'
    r = routes.llama_decode_why(scaled, tokens, None)
    assert r.name == 'walk' and 'rope_type' in r.why
    scaled._transformer.model.rotary_emb.rope_type = 'default'
    scaled._transformer.model.rotary_emb.attention_scaling = 0.5
    r = routes.llama_decode_why(scaled, tokens, None)
    assert r.name == 'walk' and 'attention_scaling' in r.why

    sliding = copy.deepcopy(m)
    sliding._transformer.config.sliding_window = 4
    assert routes.llama_decode_why(sliding, tokens, None) == routes.Route('walk', 'a sliding window is configured')

    wide = build_tiny(hidden_size=64, num_attention_heads=2, num_key_value_heads=2, head_dim=256)
    r = routes.llama_decode_why(wide, tokens, None)
    assert r.name == 'walk' and 'head dimension of 256' in r.why
    small = build_tiny(num_attention_heads=8)                                     # 64 / 8 = 8 < 16
    assert 'head dimension of 8' in routes.llama_decode_why(small, tokens, None).why
    grouped = build_tiny(hidden_size=256, num_attention_heads=16, num_key_value_heads=1)
    r = routes.llama_decode_why(grouped, tokens, None)
    assert r.name == 'walk' and '16 query heads per key-value head are beyond 8' in r.why

    r = routes.llama_decode_why(m, _Tokens((3, 1)), good)
    assert r.name == 'walk' and 'the cache holds' in r.why
    long = _cache_for(m, capacity=_lib.ATTN_MAX_LEN + 1, cls=_OnGpu)
    assert 'capacity of 4097 is beyond 4096' in routes.llama_decode_why(m, one, long).why
    r = routes.llama_decode_why(m, one, _cache_for(m))                            # still on meta
    assert r.name == 'walk' and 'the cache is on device meta' in r.why
    half = _cache_for(m, dtype=torch.bfloat16, cls=_OnGpu)
    r = routes.llama_decode_why(m, one, half)
    assert r.name == 'walk' and 'the cache is torch.bfloat16, the projections produce torch.float32' in r.why


def test_a_static_cache_behind_a_refused_route_raises_with_the_reason():
    m = build_tiny(fused=False)
    with pytest.raises(ValueError, match='decode route is refused: fused=False'):
        m.inference(torch.tensor([[1]]), _cache_for(m, 1, 4, device='cpu'), {})
    assert m.last_route == routes.Route('torch', 'fused=False')


@pytest.mark.parametrize('kv_heads', [4, 2], ids=['mha', 'gqa'])
@torch.no_grad()
def test_the_walk_behind_a_static_cache_is_hfs_cached_forward_in_float64(kv_heads):
    m = tiny64(kv_heads)
    tokens = torch.randint(0, 48, (B, PREFILL + STEPS), generator=torch.Generator().manual_seed(2))
    cache = StaticKVCache.for_model(m._transformer.config, B, PREFILL + STEPS, F64, 'cpu')
    hf_cache = None
    for lo, hi in [(0, PREFILL)] + [(t, t + 1) for t in range(PREFILL, PREFILL + STEPS)]:
        out = m._transformer(tokens[:, lo:hi], past_key_values=hf_cache)
        hf_cache = out['past_key_values']
        got = m._walk_static(tokens[:, lo:hi], cache, torch_ops=True)
        assert cache.get_seq_length() == hi == hf_cache.get_seq_length()
        assert float((got - out['logits']).abs().max()) <= 1e-12
    # nine single steps from an empty cache: the decode step alone fills it
    cache.reset()
    full = m._transformer(tokens)['logits']
    for t in range(PREFILL + STEPS):
        got = m._walk_static(tokens[:, t:t + 1], cache, torch_ops=True)
        assert float((got - full[:, t:t + 1]).abs().max()) <= 1e-12


def test_static_cache_off_leaves_todays_route_and_cache_type():
    from transformers import DynamicCache
    m = build_tiny()
    assert m.static_cache is False and m._packed is None
    logits, cache, _ = m.inference(torch.tensor([[1, 2]]), None, {})
    assert m.last_route.name == 'torch' and 'not on a GPU' in m.last_route.why and m.decode_route is None
    assert isinstance(cache, DynamicCache) and not isinstance(cache, StaticKVCache)
    on = build_tiny()
    on.static_cache = True
    tokens, _ = on.generate(torch.tensor([[1], [2]]), 4, SimpleNamespace(start=8, end=48), {})      # CPU: the decode route is refused
    assert tokens.shape == (2, 4) and on.decode_route.name == 'torch' and on.last_route.name == 'torch' and on._packed is None


def test_the_prototypes_are_bound_from_the_header():
    for name in ('vqhip_decode_attention', 'vqhip_rope_append'):
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i32 and len(args) == 20 and args[-1] is _lib._vp and args[0] is _lib._vp
    assert _lib.SIGNATURES['vqhip_decode_attention'][1][13] is _lib._f32         # scale
    assert (_lib.ATTN_MAX_HEAD_DIM, _lib.ATTN_MAX_GROUP, _lib.ATTN_MAX_LEN) == (128, 8, 4096)
    assert ops.attention_shape_refusal(16, 2, 64) == '' and 'multiple of 8' in ops.attention_shape_refusal(4, 4, 20)


def test_the_contract_entries_reach_both_entry_points():
    """tests/contract_cases.py finds entry points by a parameter called ``stream``; these two name theirs ``hip_stream``, and
    their placement, side-stream and capture properties are held by tests/test_gpu_decode_attention_contracts.py instead."""
    import test_gpu_decode_attention_contracts as contracts
    assert {'vqhip_decode_attention', 'vqhip_rope_append'} <= {n for c in contracts.CASES for n in c.abi}
