"""LlamaTransformer with ``static_cache=True`` on the GPU: generation behind a ``StaticKVCache`` on the decode route - one packed
q/k/v GEMM, ``functional.decode_attention``, ``o_proj`` per layer - on the tiny model of tests/llama_models.py, in fp32 and under bf16
autocast, with 4 and with 2 key-value heads.

The yardstick is tests/test_gpu_llama_transformer.py's: the float64 model's uncached pass on the CPU, and the ``fused=False`` model's
error against it on the same tokens.  The decode route and the torch route evaluate the same network in the same precision and
differ in rounding order only, so the decode route's worst error may be at most twice the torch route's."""
import contextlib
import copy
from types import SimpleNamespace

import pytest
import torch

from vector_quantization_amd.kv_cache import StaticKVCache
from vector_quantization_amd.quantizers import routes

from llama_models import build_tiny, exact64

pytestmark = pytest.mark.gpu

TOKENS = torch.randint(0, 48, (3, 9), generator=torch.Generator().manual_seed(2))
PREFILL_THEN_STEPS = ((0, 5), (5, 6), (6, 7), (7, 8), (8, 9))
SINGLE_STEPS = tuple((t, t + 1) for t in range(9))
_REFERENCE = {}


def reference(kv_heads):
    """(the fp32 model on the CPU, the float64 logits of the uncached pass): computed once per model, shared, left unchanged."""
    if kv_heads not in _REFERENCE:
        t = build_tiny(num_key_value_heads=kv_heads)
        with torch.no_grad():
            _REFERENCE[kv_heads] = (t, exact64(t)._transformer(TOKENS)['logits'])
    return _REFERENCE[kv_heads]


def autocast(on):
    return torch.autocast('cuda', dtype=torch.bfloat16) if on else contextlib.nullcontext()


def worst(a, b):
    return float((a.double() - b).abs().max())


def cached_error(model, cache, pieces, full, on):
    worst_e, seen_routes = 0.0, []
    with autocast(on):
        for lo, hi in pieces:
            logits, cache, _ = model.inference(TOKENS[:, lo:hi].cuda(), cache, {})
            worst_e = max(worst_e, worst(logits.cpu(), full[:, lo:hi]))
            seen_routes.append(model.last_route)
    return worst_e, seen_routes, cache


@pytest.mark.parametrize('pieces', [PREFILL_THEN_STEPS, SINGLE_STEPS], ids=['prefill5-then-steps', 'nine-single-steps'])
@pytest.mark.parametrize('kv_heads', [4, 2], ids=['mha', 'gqa'])
@pytest.mark.parametrize('on', [False, True], ids=['fp32', 'bf16-autocast'])
def test_cached_logits_are_as_close_to_float64_as_the_torch_route(on, kv_heads, pieces):
    base, full = reference(kv_heads)
    decode = copy.deepcopy(base).cuda().eval()
    plain = copy.deepcopy(base).cuda().eval()
    plain.fused = False
    dtype = torch.bfloat16 if on else torch.float32
    cache = StaticKVCache.for_model(decode._transformer.config, 3, 9, dtype, 'cuda')
    e_decode, seen_routes, cache = cached_error(decode, cache, pieces, full, on)
    assert all(r == routes.Route('decode') for r in seen_routes) and cache.get_seq_length() == 9 and decode._packed is None
    e_torch, seen_routes, _ = cached_error(plain, None, pieces, full, on)
    assert all(r.name == 'torch' for r in seen_routes)
    print(f'cached logits ({"autocast" if on else "fp32"}, {kv_heads} kv heads, {len(pieces)} calls): decode {e_decode:.3e}, torch {e_torch:.3e}')
    assert e_decode <= 2 * e_torch


@pytest.mark.parametrize('kv_heads', [4, 2], ids=['mha', 'gqa'])
@pytest.mark.parametrize('on', [False, True], ids=['fp32', 'bf16-autocast'])
def test_generate_runs_the_decode_route_at_every_step(on, kv_heads, monkeypatch):
    model = copy.deepcopy(reference(kv_heads)[0]).cuda().eval()
    model.static_cache = True
    seen_routes, caches = [], []
    inner = model._inference

    def spy(tokens, kv_cache, memo, attention_mask=None):
        out = inner(tokens, kv_cache, memo, attention_mask)
        seen_routes.append(model.last_route)
        caches.append(out[1])
        return out
    monkeypatch.setattr(model, '_inference', spy)
    codebook = SimpleNamespace(start=8, end=48)
    prompt = torch.tensor([[1], [2], [3], [1]]).cuda()
    u = torch.rand(4, generator=torch.Generator().manual_seed(6)).cuda()
    with autocast(on):
        tokens, _ = model.generate(prompt, 9, codebook, {'sampler': {'u': u}})
    assert tokens.shape == (4, 9) and torch.equal(tokens[:, :1], prompt) and 8 <= int(tokens[:, 1:].min()) and int(tokens.max()) < 48
    assert len(seen_routes) == 8 and all(r == routes.Route('decode') for r in seen_routes)
    assert all(c is caches[0] for c in caches) and isinstance(caches[0], StaticKVCache)
    assert caches[0].capacity == 9 and caches[0].get_seq_length() == 8 and caches[0].dtype == (torch.bfloat16 if on else torch.float32)
    assert model.decode_route == routes.Route('decode') and model._packed is None
    if not on:                                                                   # fp32: the tokens of today's loop under the same uniforms
        today = copy.deepcopy(reference(kv_heads)[0]).cuda().eval()
        want, _ = today.generate(prompt, 9, codebook, {'sampler': {'u': u}})
        assert today.last_route == routes.Route('fused') and torch.equal(tokens, want)


def test_static_cache_off_is_todays_route_and_cache():
    from transformers import DynamicCache
    model = copy.deepcopy(reference(4)[0]).cuda().eval()
    assert model.static_cache is False
    logits, cache, _ = model.inference(TOKENS[:, :5].cuda(), None, {})
    assert model.last_route == routes.Route('fused') and isinstance(cache, DynamicCache) and model.decode_route is None
    tokens, _ = model.generate(torch.tensor([[1], [2]]).cuda(), 5, SimpleNamespace(start=8, end=48), {})
    assert tokens.shape == (2, 5) and model.last_route == routes.Route('fused') and model.decode_route is None


def test_a_cache_of_another_dtype_is_refused_with_the_reason():
    model = copy.deepcopy(reference(4)[0]).cuda().eval()
    cache = StaticKVCache.for_model(model._transformer.config, 3, 9, torch.bfloat16, 'cuda')
    with pytest.raises(ValueError, match='the cache is torch.bfloat16, the projections produce torch.float32'):
        model.inference(TOKENS[:, :1].cuda(), cache, {})
    assert model.last_route.name == 'walk'
