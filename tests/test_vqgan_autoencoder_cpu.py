"""CPU checks of VQGANEncoder / VQGANDecoder and of the GroupNorm (+ SiLU) contract: the float64 restatement of
tests/group_norm_ref.py against torch.autograd, the state-dict keys against tests/golden/vqgan_autoencoder_keys.json (names and
shapes only, written by instantiating the reference's two classes), the registries and config dicts, the shapes of a small
encoder and decoder, the route reported for CPU tensors, and the refusals of the C ABI."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import vector_quantization_amd as vqa
from vector_quantization_amd import _lib, autoencoders, functional, registries
from vector_quantization_amd.quantizers import routes

import group_norm_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vqgan_autoencoder_keys.json')
SMALL_ENCODER = dict(width=32, width_mults=(1, 2))                              # the smallest that keeps 32 groups
SMALL_DECODER = dict(width=32, width_mults=(2, 1))


@pytest.mark.parametrize('act', [None, 'silu'])
@pytest.mark.parametrize('shape,G', [((2, 32, 5, 7), 32), ((3, 96, 3, 3), 32), ((2, 12, 4, 5), 4), ((2, 64, 1, 1), 32)], ids=str)
def test_restatement_equals_autograd_in_float64(shape, G, act):
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(shape[1], generator=gen, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(shape[1], generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn(shape, generator=gen, dtype=torch.float64)
    want = F.group_norm(x, G, gamma, beta, 1e-6)
    want = F.silu(want) if act else want
    wgx, wdg, wdb = torch.autograd.grad(want, (x, gamma, beta), g)
    y, stats, _ = ref.forward(x.detach(), G, gamma.detach(), beta.detach(), 1e-6, act)
    gx, dg, db, _ = ref.backward(g, x.detach(), G, gamma.detach(), beta.detach(), 1e-6, act)
    assert stats.shape == (shape[0], G, 2)
    for got, exp in ((y, want.detach()), (gx, wgx), (dg, wdg), (db, wdb)):
        assert float((got - exp).abs().max()) <= 1e-11 * max(1.0, float(exp.abs().max()))
    # functional.group_norm on a CPU or float64 tensor is the same definition in torch
    assert torch.equal(functional.group_norm(x.detach(), G, gamma.detach(), beta.detach(), 1e-6, act), want.detach())


def _keys(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def test_state_dict_names_and_shapes_equal_the_fixture():
    want = json.load(open(GOLDEN))
    assert _keys(vqa.VQGANEncoder()) == want['encoder']['default']
    assert _keys(vqa.VQGANDecoder()) == want['decoder']['default']
    assert _keys(vqa.VQGANEncoder(**SMALL_ENCODER)) == want['encoder']['small']
    assert _keys(vqa.VQGANDecoder(**SMALL_DECODER)) == want['decoder']['small']
    assert want['small_kwargs'] == {'encoder': {k: list(v) if isinstance(v, tuple) else v for k, v in SMALL_ENCODER.items()},
                                    'decoder': {k: list(v) if isinstance(v, tuple) else v for k, v in SMALL_DECODER.items()}}
    # every norm is an nn.GroupNorm(32, C, 1e-6) child, on both routes
    for m in vqa.VQGANDecoder(**SMALL_DECODER, fused=False).modules():
        if isinstance(m, torch.nn.GroupNorm):
            assert m.num_groups == 32 and m.eps == 1e-6


def test_registries_and_config_dicts_build():
    assert issubclass(registries.VQEncoderRegistry, registries.VQModelRegistry)
    assert issubclass(registries.VQDecoderRegistry, registries.VQModelRegistry)
    e = registries.VQEncoderRegistry.build(dict(type='VQGANEncoder'))            # configs/vqgan/model.py:17
    d = registries.VQDecoderRegistry.build(dict(type='VQGANDecoder'))            # configs/vqgan/model.py:25, what configs/decoder/vqgan.py loads
    assert type(e) is vqa.VQGANEncoder and type(d) is vqa.VQGANDecoder and e.fused and d.fused
    assert isinstance(e, vqa.BaseEncoder) and isinstance(d, vqa.BaseDecoder)
    assert (e.in_channels, e.out_channels, d.in_channels, d.out_channels) == (3, 256, 256, 3)
    assert d.last_parameter is d._projector[-1].weight and e.num_layers == 5
    for name in ('BaseEncoder', 'BaseDecoder', 'VQGANEncoder', 'VQGANDecoder', 'VQEncoderRegistry', 'VQDecoderRegistry'):
        assert name in vqa.__all__ and hasattr(vqa, name)


def test_small_encoder_and_decoder_shapes_and_cpu_route():
    torch.manual_seed(0)
    e, d = vqa.VQGANEncoder(**SMALL_ENCODER), vqa.VQGANDecoder(**SMALL_DECODER)
    memo = {}
    z, out_memo = e(torch.randn(1, 3, 32, 32), memo)
    assert z.shape == (1, 256, 16, 16) and out_memo is memo
    assert e.last_route == routes.Route('torch', 'the input is on device cpu, not on a GPU')
    image, _ = d(z, {})
    assert image.shape == (1, 3, 32, 32) and d.last_route.name == 'torch'
    image.square().mean().backward()
    assert d.last_parameter.grad is not None and all(p.grad is not None for p in e.parameters())
    assert routes.group_norm_why(vqa.VQGANEncoder(**SMALL_ENCODER, fused=False), torch.zeros(1, 3, 32, 32)) == routes.Route('torch', 'fused=False')
    assert 'group_norm_why' in routes.__doc__


def test_route_reasons():
    meta = torch.zeros(2, 3, 32, 32, device='meta')

    class Fake:                                                                 # a GPU tensor as far as the decision reads it
        def __init__(self, t):
            self.t = t
        is_cuda = True
        def __getattr__(self, name):
            return getattr(self.t, name)

    e = vqa.VQGANEncoder(**SMALL_ENCODER)
    assert routes.group_norm_why(e, Fake(meta)) == routes.Route('fused')
    assert routes.group_norm_why(e, Fake(meta.contiguous(memory_format=torch.channels_last))).name == 'fused'
    assert 'float64' in routes.group_norm_why(e, Fake(meta.double())).why
    assert 'neither' in routes.group_norm_why(e, Fake(meta[:, :, ::2])).why

    class Mine(vqa.VQGANEncoder):
        def forward(self, x, memo):
            return super().forward(x, memo)

    assert routes.group_norm_why(Mine(**SMALL_ENCODER), Fake(meta)).why == 'Mine overrides forward'


def test_upsample_keeps_the_float_round_trip_and_downsample_pads_right_and_bottom():
    up = autoencoders.Upsample(num_channels=4).to(torch.bfloat16)
    assert up(torch.randn(1, 4, 3, 3).to(torch.bfloat16)).dtype == torch.bfloat16
    down = autoencoders.Downsample(num_channels=4)
    assert down(torch.randn(1, 4, 8, 8)).shape == (1, 4, 4, 4)


def test_abi_refuses_bad_shapes_without_a_gpu():
    """C % G != 0, non-positive extents and overflowing products are VQHIP_EINVAL before any HIP call: null pointers never matter."""
    L = _lib.lib()
    M, F32 = _lib.LAYOUT_MAP, _lib.DTYPE_F32

    def fwd(B, C, P, G, layout=M, dtype=F32):
        return L.vqhip_group_norm_fwd(None, dtype, layout, B, C, P, G, None, None, 1e-6, 1, None, None, None, 0, None)

    def bwd(B, C, P, G):
        return L.vqhip_group_norm_bwd(None, None, F32, M, B, C, P, G, None, None, None, 1, None, None, None, None, 0, None)

    for bad in ((2, 33, 16, 32), (0, 32, 16, 32), (2, 0, 16, 32), (2, 32, 0, 32), (2, 32, 16, 0), (-1, 32, 16, 32), (2, 32, -4, 32),
                (1 << 30, 1 << 30, 1 << 30, 1), (1, 32, 1 << 31, 32), (1, 1 << 20, 1 << 20, 1)):
        assert fwd(*bad) == -22 and b'vqhip_group_norm_fwd' in L.vqhip_last_error(), bad
        assert bwd(*bad) == -22 and b'vqhip_group_norm_bwd' in L.vqhip_last_error(), bad
        assert L.vqhip_group_norm_ws_bytes(M, *bad) == -1, bad
    assert fwd(2, 32, 16, 32, layout=7) == -22 and fwd(2, 32, 16, 32, dtype=2) == -22
    assert fwd(2, 32, 16, 32) == -22 and b'required' in L.vqhip_last_error()  # a good shape: the null pointers are what is refused
    # the workspace: 2 floats per chunk of a group, 2 C floats per slab (B times the chunks of a group)
    assert L.vqhip_group_norm_ws_bytes(M, 2, 64, 25, 32) == 4 * (2 * 2 * 32 + 2 * 2 * 64)
    assert L.vqhip_group_norm_ws_bytes(_lib.LAYOUT_ROWS, 1, 128, 4900, 32) == 4 * (2 * 32 * 3 + 2 * 3 * 128)
    fake = ctypes.c_void_p(0x1000)
    need = L.vqhip_group_norm_ws_bytes(M, 1, 128, 4900, 32)
    assert L.vqhip_group_norm_fwd(fake, F32, M, 1, 128, 4900, 32, fake, fake, 1e-6, 1, fake, fake, fake, need - 1, None) == -22
    assert b'ws too small' in L.vqhip_last_error()
    assert L.vqhip_group_norm_fwd(fake, F32, M, 1, 128, 4900, 32, fake, fake, 1e-6, 2, fake, fake, fake, need, None) == -22
    assert ref.slabs(1, 128, 4900, 32) == 3 and ref.slabs(2, 512, 16, 32) == 2
