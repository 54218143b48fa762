"""LlamaTransformer and the two row modes under it, without a GPU: every new VQHIP_EINVAL clause before any launch, the float64
restatements of tests/llama_ops_ref.py against torch.autograd, the class as the reference builds it (config dict, state-dict keys,
init_weights, registry), the route reasons, and the walk over transformers' submodules - with the ``_torch`` restatements in place
of the kernels - against ``LlamaForCausalLM``'s own forward, with and without a KV cache.

transformers' ``LlamaRMSNorm`` computes in fp32 whatever the input dtype (``hidden_states.to(torch.float32)``), so a ``.double()``
copy of the model still rounds every norm to fp32.  The float64 model the fp32 evaluations are compared with is therefore the
``.double()`` copy with each ``LlamaRMSNorm`` replaced by ``RMSNorm64`` below: the same lines without the cast (llama_models.py)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import vector_quantization_amd as vqa
from vector_quantization_amd import _lib, functional
from vector_quantization_amd.quantizers import routes
from vector_quantization_amd.registries import VQSMTransformerRegistry

import llama_ops_ref as ref
from llama_models import TINY, RMSNorm64, build_tiny, exact64

MEDIUM = dict(num_hidden_layers=24, num_attention_heads=16, hidden_size=1024, intermediate_size=2816, rms_norm_eps=1e-5)


def test_abi_refuses_the_new_clauses_before_a_launch():
    """beta (fwd) and dbeta (bwd) may be NULL, nothing else; act 3 takes no bias, dbias or ws and holds R 2 F below 2^31; act 2
    stays refused.  Every call below is refused: a pointer of 0x1000 would fault if anything were launched.  No entry point sees
    both beta and dbeta (they are arguments of different calls), so 'one NULL and the other set' is no clause of the C ABI: the
    pairing is held by ops.add_rms_norm / ops.add_rms_norm_backward, which tests/test_gpu_llama_ops.py runs as a pair."""
    L = _lib.lib()
    F32 = _lib.DTYPE_F32
    fake = ctypes.c_void_p(0x1000)

    def ln_fwd(x=fake, gamma=fake, beta=None, y=fake, stats=fake, yd=F32, R=4, D=8):
        return L.vqhip_add_layer_norm_fwd(x, F32, None, F32, R, D, gamma, beta, 1e-5, None, y, yd, stats, None)

    def ln_bwd(g=fake, s=fake, gamma=fake, stats=fake, gx=fake, dgamma=fake, dbeta=None, ws=fake, ws_bytes=1 << 20, R=4, D=8):
        return L.vqhip_add_layer_norm_bwd(g, F32, s, F32, None, R, D, gamma, stats, gx, dgamma, dbeta, ws, ws_bytes, None)

    def act_fwd(R, D, x=fake, bias=None, y=fake, act=3):
        return L.vqhip_row_bias_act_fwd(x, F32, R, D, bias, act, y, None)

    def act_bwd(R, D, g=fake, x=fake, bias=None, gx=fake, dbias=None, ws=None, ws_bytes=0, act=3):
        return L.vqhip_row_bias_act_bwd(g, x, F32, R, D, bias, act, gx, dbias, ws, ws_bytes, None)

    # RMS mode: every other pointer stays required, the sizes and dtypes are refused as before
    for name in ('x', 'gamma', 'y', 'stats'):
        assert ln_fwd(**{name: None}) == -22 and b'required' in L.vqhip_last_error(), name
    for name in ('g', 's', 'gamma', 'stats', 'gx', 'dgamma', 'ws'):
        assert ln_bwd(**{name: None}) == -22 and b'required' in L.vqhip_last_error(), name
    assert ln_fwd(yd=3) == -22 and b'dtype' in L.vqhip_last_error()
    assert ln_fwd(D=8193) == -22 and ln_bwd(D=8193) == -22 and ln_fwd(R=0) == -22
    assert ln_bwd(R=33, D=768, ws_bytes=2 * 3 * 768 * 4 - 1) == -22 and b'ws too small' in L.vqhip_last_error()
    # SwiGLU: no bias, no dbias, no ws
    assert act_fwd(4, 8, bias=fake) == -22 and b'no bias' in L.vqhip_last_error()
    assert act_bwd(4, 8, bias=fake) == -22 and b'no bias' in L.vqhip_last_error()
    assert act_bwd(4, 8, dbias=fake) == -22 and b'no bias' in L.vqhip_last_error()
    assert act_bwd(4, 8, ws=fake, ws_bytes=1 << 20) == -22 and b'no bias' in L.vqhip_last_error()
    assert act_bwd(4, 8, dbias=fake, ws=fake, ws_bytes=1 << 20) == -22 and b'no bias' in L.vqhip_last_error()
    # R 2 F >= 2^31 where R F < 2^31 (the other activations take these sizes)
    for R, D in (((1 << 30) // 768 + 1, 768), (1 << 18, 4096), ((1 << 31) // 5632 + 1, 2816)):
        assert R * D < (1 << 31) <= R * 2 * D
        assert act_fwd(R, D) == -22 and b'R * 2 D' in L.vqhip_last_error(), (R, D)
        assert act_bwd(R, D) == -22 and b'R * 2 D' in L.vqhip_last_error(), (R, D)
    for bad in ((0, 8), (4, 0), (4, 8193), ((1 << 24) + 1, 8)):
        assert act_fwd(*bad) == -22 and act_bwd(*bad) == -22, bad
    assert act_fwd(4, 8, x=None) == -22 and b'required' in L.vqhip_last_error()
    assert act_fwd(4, 8, y=None) == -22 and b'required' in L.vqhip_last_error()
    for name in ('g', 'x', 'gx'):
        assert act_bwd(4, 8, **{name: None}) == -22 and b'required' in L.vqhip_last_error(), name
    assert act_fwd(4, 8, act=2) == -22 and act_bwd(4, 8, act=2) == -22 and act_fwd(4, 8, act=4) == -22
    assert _lib.ROW_ACT_SWIGLU == 3 and '#define VQHIP_ROW_ACT_SWIGLU 3' in open(_lib.HEADER_PATH).read()


def test_restatements_equal_autograd_of_the_modules_in_float64():
    gen = torch.Generator().manual_seed(3)
    R, D = 7, 24
    x = torch.randn(R, D, generator=gen, dtype=torch.float64, requires_grad=True)
    g, skip = torch.randn(R, D, generator=gen, dtype=torch.float64), torch.randn(R, D, generator=gen, dtype=torch.float64)
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    hf = LlamaRMSNorm(D, 1e-5).double()
    hf.weight.data = torch.randn(D, generator=gen, dtype=torch.float64)
    exact = RMSNorm64(hf)
    y, stats, _ = ref.rms_forward(x.detach(), hf.weight.detach(), 1e-5)
    gx, dg, _ = ref.rms_backward(g, x.detach(), hf.weight.detach(), 1e-5, skip)
    assert not stats[:, 0].any() and stats.shape == (R, 2)
    # LlamaRMSNorm rounds to fp32 inside: 2^-22 relative.  The same lines without the cast: float64 rounding only.
    for module, tol in ((hf, 2.0 ** -22), (exact, 1e-13)):
        w = module.weight
        out = module(x)
        wgx, wdg = torch.autograd.grad(out, (x, w), g)
        want = out.detach()
        scale = float(want.abs().max())
        assert float((y - want).abs().max()) <= tol * scale
        assert float((gx - skip - wgx).abs().max()) <= tol * float(wgx.abs().max()) * 4
        assert float((dg - wdg).abs().max()) <= tol * float(wdg.abs().max()) * 4
    # functional's torch restatement: float64 stays float64, (s, y) with and without the branch
    s, yy = functional.add_rms_norm(x.detach(), skip, hf.weight.detach(), 1e-5)
    assert torch.equal(s, x.detach() + skip) and float((yy - ref.rms_forward(s, hf.weight.detach(), 1e-5)[0]).abs().max()) <= 1e-13
    s, yy = functional.add_rms_norm(x.detach(), None, hf.weight.detach(), 1e-5)
    assert s.data_ptr() == x.data_ptr() and float((yy - y).abs().max()) <= 1e-13
    # SwiGLU against F.silu(a) * b
    h = torch.randn(R, 2 * D, generator=gen, dtype=torch.float64, requires_grad=True)
    a, b = h.chunk(2, dim=1)
    want = F.silu(a) * b
    wgh, = torch.autograd.grad(want, h, g)
    y, _ = ref.swiglu_forward(h.detach())
    gh, _ = ref.swiglu_backward(g, h.detach())
    assert float((y - want).abs().max()) <= 1e-14 and float((gh - wgh).abs().max()) <= 1e-14
    assert torch.equal(functional.swiglu(h.detach()), functional.swiglu_torch(h.detach()))
    assert float((functional.swiglu(h.detach()) - y).abs().max()) <= 1e-14
    # strict: a refusal raises with the reason instead of computing in torch
    with pytest.raises(ValueError, match='not on a GPU'):
        functional.add_rms_norm(x.detach(), None, hf.weight.detach(), strict=True)
    with pytest.raises(ValueError, match='not on a GPU'):
        functional.swiglu(h.detach(), strict=True)


def test_builds_from_the_reference_config_with_its_keys_and_init():
    config = dict(type='LlamaTransformer', transformer=dict(MEDIUM, num_hidden_layers=2), vocabulary_size=1000 + 16384,
                  sampler=dict(type='TopKTopPSampler', top_k=100))
    with torch.device('meta'):                                                  # the medium widths without their memory
        m = VQSMTransformerRegistry.build(config)
    assert type(m) is vqa.LlamaTransformer and isinstance(m, vqa.HFTransformer) and isinstance(m, vqa.BaseTransformer)
    assert m.vocabulary_size == 17384 and type(m.sampler).__name__ == 'TopKTopPSampler'
    c = m._transformer.config
    assert (c.num_hidden_layers, c.num_attention_heads, c.hidden_size, c.intermediate_size, c.rms_norm_eps) == (2, 16, 1024, 2816, 1e-5)
    assert m._transformer.lm_head.weight.shape == (17384, 1024) and m._transformer.model.embed_tokens.weight.shape == (17384, 1024)
    for name in ('BaseTransformer', 'HFTransformer', 'LlamaTransformer', 'VQSMTransformerRegistry'):
        assert name in vqa.__all__ and hasattr(vqa, name)
    # the reference's state-dict keys: '_transformer.' + those of a bare LlamaForCausalLM
    from transformers import LlamaConfig, LlamaForCausalLM
    t = build_tiny()
    bare = LlamaForCausalLM(LlamaConfig(**TINY))
    bare.resize_token_embeddings(48)
    assert list(t.state_dict()) == ['_transformer.' + k for k in bare.state_dict()]
    assert {k: v.shape for k, v in t._transformer.state_dict().items()} == {k: v.shape for k, v in bare.state_dict().items()}
    # init_weights: normal(0, 0.02) for Linear and Embedding, lm_head zero, the norms' weights left at one
    torch.manual_seed(0)
    assert float(t._transformer.lm_head.weight.abs().max()) > 0 and t.init_weights(None) is False
    lm = t._transformer
    assert not lm.lm_head.weight.any()
    for mod in lm.model.modules():
        if isinstance(mod, (nn.Linear, nn.Embedding)):
            assert 0.015 < float(mod.weight.std()) < 0.025 and abs(float(mod.weight.mean())) < 0.005, mod
        elif type(mod).__name__ == 'LlamaRMSNorm':
            assert float(mod.weight.min()) == 1.0 == float(mod.weight.max())


def test_route_reasons():
    t = build_tiny()
    tokens = torch.randint(0, 48, (3, 9), generator=torch.Generator().manual_seed(1))
    loss, memo = t(SimpleNamespace(tokens=tokens), {})
    assert t.last_route == routes.Route('torch', 'the tokens are on device cpu, not on a GPU') and memo['logits'].shape == (3, 9, 48)
    loss2, memo2 = t(tokens, {})                                                # the token tensor itself
    assert torch.equal(loss, loss2) and torch.equal(memo['logits'], memo2['logits'])
    out = t._transformer(tokens, labels=tokens)
    assert torch.equal(loss, out['loss']) and torch.equal(memo['logits'], out['logits'])
    assert routes.llama_why(build_tiny(fused=False), tokens).why == 'fused=False'
    assert 'attention_mask' in routes.llama_why(t, tokens, None, torch.ones(3, 9)).why
    t(tokens, {}, attention_mask=torch.ones(3, 9, dtype=torch.long))
    assert 'attention_mask' in t.last_route.why and t.last_route.name == 'torch'
    for extra, word in ((dict(mlp_bias=True), 'mlp_bias'), (dict(attention_bias=True), 'attention_bias'),
                        (dict(hidden_act='gelu'), 'hidden_act'), (dict(tie_word_embeddings=True), 'tied'),
                        (dict(intermediate_size=8200), 'beyond 8192')):
        assert word in routes.llama_why(build_tiny(**extra), tokens).why, extra
    eager = build_tiny()
    eager._transformer.config._attn_implementation = 'eager'
    assert 'eager' in routes.llama_why(eager, tokens).why
    assert routes.llama_why(build_tiny().double(), tokens).why == 'the tokens are on device cpu, not on a GPU'

    class Mine(vqa.LlamaTransformer):
        def _walk(self, tokens, kv_cache=None, **kwargs):
            return super()._walk(tokens, kv_cache, **kwargs)
    mine = Mine(vocabulary_size=48, sampler=t.sampler, transformer=t._transformer)
    assert routes.llama_why(mine, tokens).why == 'Mine overrides _walk'
    # several tokens behind a cache that is not empty: transformers builds a mask for them
    _, cache, _ = t.inference(tokens[:, :5], None, {})
    assert cache.get_seq_length() == 5 and 'behind a cache of 5' in routes.llama_why(t, tokens[:, 5:7], cache).why
    assert 'behind a cache' not in routes.llama_why(t, tokens[:, 5:6], cache).why


def worst(a, b):
    return float((a.double() - b).abs().max())


def test_the_walk_equals_hf_forward_to_summation_order():
    """Both are fp32 evaluations of the same network that differ only in summation order (one GEMM for gate and up, the norm's
    reduction): against the float64 model the walk's worst logit error may be at most twice the HF route's."""
    t = build_tiny()
    tokens = torch.randint(0, 48, (3, 9), generator=torch.Generator().manual_seed(2))
    want = exact64(t)._transformer(tokens)['logits']
    with torch.no_grad():
        hf = t._transformer(tokens)['logits']
        walk = t._walk(tokens, torch_ops=True)
    e_hf, e_walk = worst(hf, want), worst(walk, want)
    print(f'logits: HF fp32 {e_hf:.3e}, walk fp32 {e_walk:.3e}, scale {float(want.abs().max()):.3e}')
    assert walk.shape == (3, 9, 48) and 0 < e_hf < 1e-5 * float(want.abs().max()) and e_walk <= 2 * e_hf


def test_the_walk_with_a_kv_cache_equals_hf():
    """A prefill of 5 tokens, then 4 single-token steps, each route on its own cache."""
    from transformers import DynamicCache
    t = build_tiny()
    t64 = exact64(t)
    tokens = torch.randint(0, 48, (3, 9), generator=torch.Generator().manual_seed(4))
    full = t64._transformer(tokens)['logits']
    c_hf, c_walk, c64 = None, DynamicCache(config=t._transformer.config), None
    e_hf = e_walk = 0.0
    with torch.no_grad():
        for lo, hi in ((0, 5), (5, 6), (6, 7), (7, 8), (8, 9)):
            out = t64._transformer(tokens[:, lo:hi], past_key_values=c64)
            want, c64 = out['logits'], out['past_key_values']
            assert worst(want, full[:, lo:hi]) < 1e-12                         # (the float64 model's cache is consistent with itself)
            out = t._transformer(tokens[:, lo:hi], past_key_values=c_hf)
            c_hf = out['past_key_values']
            walk = t._walk(tokens[:, lo:hi], c_walk, torch_ops=True)
            e_hf, e_walk = max(e_hf, worst(out['logits'], want)), max(e_walk, worst(walk, want))
            assert c_walk.get_seq_length() == hi == c_hf.get_seq_length()
    print(f'cached logits: HF fp32 {e_hf:.3e}, walk fp32 {e_walk:.3e}')
    assert 0 < e_hf and e_walk <= 2 * e_hf


def test_generate_runs_the_kv_cache_loop_through_the_sampler():
    t = build_tiny()
    codebook = SimpleNamespace(start=8, end=48)
    prompt = torch.tensor([[1], [2], [3], [1]])
    u = torch.rand(4, generator=torch.Generator().manual_seed(6))
    tokens, memo = t.generate(prompt, 7, codebook, {'sampler': {'u': u}})
    assert tokens.shape == (4, 7) and torch.equal(tokens[:, :1], prompt) and int(tokens[:, 1:].min()) >= 8 and int(tokens.max()) < 48
    again, _ = t.generate(prompt, 7, codebook, {'sampler': {'u': u}})
    assert torch.equal(tokens, again) and not tokens.requires_grad
    # the loop's logits are those of one uncached pass over what it generated
    with torch.no_grad():
        logits = t._transformer(tokens)['logits']
        step, _, _ = t.inference(tokens, None, {})
    assert float((logits - step).abs().max()) == 0.0
