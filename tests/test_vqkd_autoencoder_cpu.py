"""CPU checks of VQKDEncoder / VQKDDecoder and of the row ops under them: the float64 restatement of tests/vit_ops_ref.py against
torch.autograd, the state-dict keys against tests/golden/vqkd_autoencoder_keys.json (names and shapes of the reference's classes),
the two shipped config dicts through the registries, shapes, the bicubic position-embedding branch, the route reported for CPU
tensors, fused=True against fused=False, init_weights, and every VQHIP_EINVAL clause of the new ABI calls (no GPU is touched)."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import vector_quantization_amd as vqa
from vector_quantization_amd import _lib, functional, registries, tokenization, vqkd_autoencoders
from vector_quantization_amd.quantizers import routes

import vit_ops_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vqkd_autoencoder_keys.json')
SHAPES = [(1, 8), (5, 24), (7, 100), (3, 768)]
SMALL_ENCODER = dict(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, out_chans=8)
SMALL_DECODER = dict(img_size=2, in_chans=8, embed_dim=64, depth=1, num_heads=2, out_chans=16)
EPS = 1e-6


def close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('R,D', SHAPES, ids=str)
def test_restatement_equals_autograd_in_float64(R, D):
    gen = torch.Generator().manual_seed(R * 1000 + D)
    x, res, g, g_skip = (torch.randn(R, D, generator=gen, dtype=torch.float64) for _ in range(4))
    gamma, beta = torch.randn(D, generator=gen, dtype=torch.float64), torch.randn(D, generator=gen, dtype=torch.float64)
    xa, ra, wa, ba = (t.clone().requires_grad_() for t in (x, res, gamma, beta))
    s = xa + ra
    y = F.layer_norm(s, (D,), wa, ba, EPS)
    gx, gr, gw, gb = torch.autograd.grad((y * g).sum() + (s * g_skip).sum(), (xa, ra, wa, ba))
    sr = ref.rounded_sum(x, res)
    wy, stats, _ = ref.ln_forward(sr, gamma, beta, EPS)
    wgx, wdg, wdb, _ = ref.ln_backward(g, sr, gamma, beta, EPS, g_skip)
    assert torch.equal(sr, s.detach()) and close(wy, y.detach()) and close(wgx, gx) and close(wgx, gr) and close(wdg, gw) and close(wdb, gb)
    assert close(stats[:, 0], sr.mean(1)) and close(stats[:, 1], 1.0 / torch.sqrt(sr.var(1, unbiased=False) + EPS))
    for act, fn in (('gelu', F.gelu), ('tanh', torch.tanh)):
        xa, ba = x.clone().requires_grad_(), beta.clone().requires_grad_()
        y = fn(xa + ba)
        gx, gb = torch.autograd.grad(y, (xa, ba), g)
        wy, _ = ref.act_forward(x, beta, act)
        wgx, wdb, _ = ref.act_backward(g, x, beta, act)
        assert close(wy, y.detach()) and close(wgx, gx) and close(wdb, gb), act


def test_bound_helpers_are_the_header_macros():
    u = 2.0 ** -24 * (1.0 + 2.0 ** -9)
    assert _lib.row_act_bound(_lib.ROW_ACT_GELU, 2.0, 1.5) == ((3.0 + 3.02) * 2.0 + 2.0 * 1.5) * u + 2.0 ** -148
    assert _lib.row_act_bound(_lib.ROW_ACT_TANH, 2.0, 0.5) == (1.0 + 2.0 * 2.82) * u * 0.5 + 2.0 ** -148
    assert _lib.row_act_grad_bound(_lib.ROW_ACT_GELU, 0.0, 0.0) == (5.0 + 3.02 + 1.79 / 2.0) * u
    assert _lib.row_act_grad_bound(_lib.ROW_ACT_TANH, 0.5, 0.75) == ((3.0 + 4.0 * 2.82) * 0.25 + 0.75) * u
    assert _lib.ln_gx_bound(1.0, 2.0) == 1.0 + 2.0 * u
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'include', 'vqhip.h')).read()
    for line in ('#define VQHIP_VIT_ERF_ULPS 3.02', '#define VQHIP_VIT_TANH_ULPS 2.82', '#define VQHIP_VIT_EXP_ULPS 1.79',
                 '#define VQHIP_VIT_MAX_D 8192', '#define VQHIP_VERSION 600'):
        assert line in header, line


def test_state_dict_names_and_shapes_equal_the_fixture():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == ['decoder_default', 'decoder_depth1', 'decoder_pixels', 'decoder_small', 'encoder_default', 'encoder_small']
    for name, case in golden.items():
        with torch.device('meta'):
            m = getattr(vqkd_autoencoders, case['cls'])(**case['kwargs'])
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == case["keys"], name
        with torch.device('meta'):
            plain = getattr(vqkd_autoencoders, case['cls'])(**case['kwargs'], fused=False)
        assert list(plain.state_dict()) == list(m.state_dict()), name


def test_registries_and_config_dicts_build():
    """configs/vqkd/model.py:18,28 and configs/decoder/vqkd.py."""
    with torch.device('meta'):
        e = registries.VQEncoderRegistry.build(dict(type='VQKDEncoder'))
        d = registries.VQDecoderRegistry.build(dict(type='VQKDDecoder', depth=1))
        p = registries.VQDecoderRegistry.build(dict(type='VQKDDecoder', out_chans=3, out_patch_size=16))
    assert type(e) is vqa.VQKDEncoder and type(d) is vqa.VQKDDecoder and e.fused and d.fused
    assert e.out_channels == 32 and d.in_channels == 32 and len(e.blocks) == 12 and len(d.blocks) == 1
    assert d.last_parameter is d.task_layer[2].weight and tuple(d.last_parameter.shape) == (512, 768)
    assert tuple(p.last_parameter.shape) == (3 * 16 * 16, 768)
    assert e.blocks[0].norm1.eps == 1e-6 and e.fc_norm.eps == 1e-6 and isinstance(e.blocks[0].norm2, torch.nn.LayerNorm)


def _small_pair(**kw):
    torch.manual_seed(0)
    e, d = vqa.VQKDEncoder(**SMALL_ENCODER, **kw), vqa.VQKDDecoder(**SMALL_DECODER, **kw)
    e.init_weights()
    d.init_weights()
    return e, d


def test_small_encoder_and_decoder_shapes_and_cpu_route():
    e, d = _small_pair()
    memo = {}
    z, m = e(torch.randn(2, 3, 32, 32), memo)
    assert z.shape == (2, 8, 2, 2) and z.is_contiguous() and m is memo
    assert e.last_route == routes.Route('torch', 'the input is on device cpu, not on a GPU')
    out, _ = d(z, memo)
    assert out.shape == (2, 16, 2, 2) and d.last_route.name == 'torch'
    # the pixel decoder of configs/decoder/vqkd.py, small: out_patch_size spreads a token's values over a patch
    p = vqa.VQKDDecoder(img_size=2, in_chans=8, embed_dim=64, depth=1, num_heads=2, out_chans=3, out_patch_size=4)
    img, _ = p(z, memo)
    assert img.shape == (2, 3, 8, 8)
    tokens, _ = vqkd_autoencoders.VQKDMixin.forward(p, z, memo)
    assert torch.equal(img[1, 2, 4:8, 0:4], tokens[1, 2].reshape(4, 4, 3)[:, :, 2])        # token (h=1, w=0), channel 2
    # the distillation loss takes the decoder's map as it is
    loss = vqa.CosineEmbeddingLoss()
    target = torch.randn(2, 4, 16)
    assert torch.allclose(tokenization.distill_loss(loss, out, target), loss(out.flatten(2).transpose(1, 2), target))


def test_a_48_pixel_input_takes_the_bicubic_position_embedding():
    e, _ = _small_pair()
    x = torch.randn(1, 3, 48, 48)
    tokens = e.patch_embed(x)
    pos = e.interpolate_pos_encoding(torch.cat((e.cls_token, tokens), 1), 48, 48)
    assert pos.shape == (1, 10, 64) and torch.equal(pos[:, 0], e.pos_embed[:, 0])
    want = F.interpolate(e.pos_embed[:, 1:].reshape(1, 2, 2, 64).permute(0, 3, 1, 2), scale_factor=(3.1 / 2, 3.1 / 2), mode='bicubic')
    assert torch.equal(pos[:, 1:], want.permute(0, 2, 3, 1).reshape(1, 9, 64))
    assert e.interpolate_pos_encoding(torch.zeros(1, 5, 64), 32, 32) is e.pos_embed
    z, _ = e(x, {})
    assert z.shape == (1, 8, 3, 3)


def test_fused_true_and_false_agree_on_cpu_and_route_reasons():
    e, d = _small_pair()
    pe, pd = _small_pair(fused=False)
    pe.load_state_dict(e.state_dict(), strict=True)
    pd.load_state_dict(d.state_dict(), strict=True)
    x = torch.randn(2, 3, 32, 32)
    z, _ = e(x, {})
    pz, _ = pe(x, {})
    assert torch.equal(z, pz) and torch.equal(d(z, {})[0], pd(z, {})[0])
    assert pe.last_route == routes.Route('torch', 'fused=False')
    assert routes.vit_why(None, x.double()).why == 'the input is on device cpu, not on a GPU'

    class Mine(vqa.VQKDEncoder):
        def _forward_fused(self, x):
            return super()._forward_fused(x)

    class Embeds(vqa.VQKDEncoder):                                              # (the embedding is the same code on both routes)
        def _embed(self, x):
            return super()._embed(x)
    assert routes.vit_why(Mine(**SMALL_ENCODER), x).why == 'Mine overrides _forward_fused'
    assert routes.vit_why(Embeds(**SMALL_ENCODER), x).why == 'the input is on device cpu, not on a GPU'
    wide = vqa.VQKDEncoder(img_size=16, patch_size=16, embed_dim=64, depth=1, num_heads=2, mlp_ratio=200.0)
    assert wide.widest_row == 12800 and 'beyond 8192' in routes.vit_why(wide, x).why
    # the functional ops serve CPU and float64 tensors with the reference's lines
    t, r, w, b = torch.randn(3, 5, 8), torch.randn(3, 5, 8), torch.randn(8), torch.randn(8)
    s, y = functional.add_layer_norm(t, r, w, b, 1e-6)
    assert torch.equal(s, t + r) and torch.equal(y, F.layer_norm(t + r, (8,), w, b, 1e-6))
    s, y = functional.add_layer_norm(t, None, w, b)
    assert s is t and torch.equal(y, F.layer_norm(t, (8,), w, b, 1e-6))
    assert torch.equal(functional.row_bias_act(t, b), F.gelu(t + b)) and torch.equal(functional.row_bias_act(t, b, 'tanh'), torch.tanh(t + b))
    with pytest.raises(ValueError):
        functional.row_bias_act(t, b, 'relu')
    # strict (what a module on the fused route passes): a refusal raises with the reason instead of computing in torch
    with pytest.raises(ValueError, match='not on a GPU'):
        functional.add_layer_norm(t, r, w, b, strict=True)
    with pytest.raises(ValueError, match='not on a GPU'):
        functional.row_bias_act(t, b, strict=True)


def test_init_weights_rescales_block_i():
    torch.manual_seed(1)
    e = vqa.VQKDEncoder(img_size=32, patch_size=16, embed_dim=64, depth=3, num_heads=2)
    seen = {}
    keep = torch.nn.init.trunc_normal_

    def record(t, *a, **k):
        out = keep(t, *a, **k)
        seen[t.data_ptr()] = t.detach().clone()
        return out
    torch.nn.init.trunc_normal_ = record
    try:
        e.init_weights(None)
    finally:
        torch.nn.init.trunc_normal_ = keep
    for i, blk in enumerate(e.blocks):
        for w in (blk.attn.proj.weight, blk.mlp.fc2.weight):
            assert torch.equal(w, seen[w.data_ptr()] / (2 * (i + 1)) ** 0.5), i
        assert torch.equal(blk.attn.qkv.weight, seen[blk.attn.qkv.weight.data_ptr()])
        assert float(blk.norm1.weight.min()) == 1.0 and float(blk.mlp.fc1.bias.abs().max()) == 0.0
    assert float(e.pos_embed.abs().max()) > 0 and float(e.cls_token.abs().max()) > 0 and float(e.task_layer[0].weight.std()) < 0.03


def test_abi_refuses_before_a_launch():
    """Every VQHIP_EINVAL clause of the four calls: sizes first (null pointers never matter), then dtypes, then the pointers."""
    L = _lib.lib()
    F32, BF16, F16 = _lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16
    fake = ctypes.c_void_p(0x1000)

    def ln_fwd(R, D, x=None, xd=F32, res=None, rd=F32, yd=F32, eps=1e-6, sum_out=None, rest=None):
        return L.vqhip_add_layer_norm_fwd(x, xd, res, rd, R, D, rest, rest, eps, sum_out, rest, yd, rest, None)

    def ln_bwd(R, D, p=None, gd=F32, sd=F32, ws=None, ws_bytes=0):
        return L.vqhip_add_layer_norm_bwd(p, gd, p, sd, None, R, D, p, p, p, p, p, ws, ws_bytes, None)

    def act_fwd(R, D, p=None, dtype=F32, act=0):
        return L.vqhip_row_bias_act_fwd(p, dtype, R, D, p, act, p, None)

    def act_bwd(R, D, p=None, dtype=F32, act=0, dbias=None, ws=None, ws_bytes=0):
        return L.vqhip_row_bias_act_bwd(p, p, dtype, R, D, p, act, p, dbias, ws, ws_bytes, None)

    for bad in ((0, 8), (-1, 8), (4, 0), (4, -8), (4, 8193), (1 << 40, 8), ((1 << 24) + 1, 8), (1 << 20, 2048), ((1 << 31) // 768 + 1, 768)):
        for name, call in (('vqhip_add_layer_norm_fwd', ln_fwd), ('vqhip_add_layer_norm_bwd', ln_bwd),
                           ('vqhip_row_bias_act_fwd', act_fwd), ('vqhip_row_bias_act_bwd', act_bwd)):
            assert call(*bad, fake) == -22 and name.encode() in L.vqhip_last_error(), (name, bad)
        assert L.vqhip_add_layer_norm_slabs(*bad) == -1 and L.vqhip_row_bias_act_slabs(*bad) == -1, bad
    assert L.vqhip_add_layer_norm_slabs(33, 8192) == 3 and L.vqhip_row_bias_act_slabs(257, 1) == 2
    # dtype combinations outside the table, with every pointer given
    for xd, yd in ((BF16, F32), (F16, F32), (BF16, F16), (F16, BF16), (2, F32), (F32, 3), (5, 5)):
        assert ln_fwd(4, 8, fake, xd, None, yd, yd, rest=fake) == -22 and b'dtype' in L.vqhip_last_error(), (xd, yd)
        assert ln_bwd(4, 8, fake, yd, xd, fake, 1 << 20) == -22 and b'dtype' in L.vqhip_last_error(), (xd, yd)
    assert ln_fwd(4, 8, fake, F32, fake, F32, BF16, sum_out=fake, rest=fake) == -22 and b"res must have y's dtype" in L.vqhip_last_error()
    assert ln_fwd(4, 8, fake, F32, fake, BF16, BF16, sum_out=None, rest=fake) == -22 and b'res needs sum_out' in L.vqhip_last_error()
    for eps in (-1.0, float('inf'), float('nan')):
        assert ln_fwd(4, 8, fake, rest=fake, eps=eps) == -22 and b'eps' in L.vqhip_last_error()
    for dtype in (2, 3, 5, 7):
        assert act_fwd(4, 8, fake, dtype) == -22 and act_bwd(4, 8, fake, dtype) == -22
    for act in (-1, 2):
        assert act_fwd(4, 8, fake, act=act) == -22 and b'act' in L.vqhip_last_error()
        assert act_bwd(4, 8, fake, act=act) == -22 and b'act' in L.vqhip_last_error()
    # null pointers at a good shape
    assert ln_fwd(4, 8) == -22 and b'required' in L.vqhip_last_error()
    assert ln_fwd(4, 8, fake) == -22 and b'required' in L.vqhip_last_error()
    assert ln_bwd(4, 8) == -22 and b'required' in L.vqhip_last_error()
    assert ln_bwd(4, 8, fake) == -22 and b'required' in L.vqhip_last_error()          # ws missing
    assert act_fwd(4, 8) == -22 and b'required' in L.vqhip_last_error()
    assert act_bwd(4, 8) == -22 and b'required' in L.vqhip_last_error()
    assert act_bwd(4, 8, fake, dbias=fake) == -22 and b'dbias needs the workspace' in L.vqhip_last_error()
    # the workspaces: 2 D floats per slab of 16 rows, D floats per slab of 256 rows
    assert ln_bwd(33, 768, fake, ws=fake, ws_bytes=2 * 3 * 768 * 4 - 1) == -22 and b'ws too small' in L.vqhip_last_error()
    assert act_bwd(257, 768, fake, dbias=fake, ws=fake, ws_bytes=2 * 768 * 4 - 1) == -22 and b'ws too small' in L.vqhip_last_error()
    assert ref.ln_slabs(33) == 3 and ref.act_slabs(257) == 2
