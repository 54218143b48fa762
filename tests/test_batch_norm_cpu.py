"""CPU checks of the batch-statistics mode of vqhip_group_norm_* and of PatchGANDiscriminator on it: what the ABI accepts and
refuses without a GPU (fake pointers, as test_vqkd_autoencoder_cpu.py does), the float64 restatement of tests/batch_norm_ref.py
against torch.autograd of F.batch_norm + F.leaky_relu, the module on the CPU against its own plain Sequential (outputs, running
statistics, state-dict keys), every reason of routes.patchgan_why, and the branch precondition of the GPU cases.

The ABI values: batch statistics are G == VQHIP_GN_BATCH (-2) and LeakyReLU is act == VQHIP_GN_ACT_LEAKY (2) behind batch
statistics only.  G == 0, G == -1, and act == 2 with G >= 1 stay VQHIP_EINVAL: test_vqgan_autoencoder_cpu.py holds the library
to that."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import vector_quantization_amd as vqa
from vector_quantization_amd import _lib, functional, gan_losses, ops
from vector_quantization_amd.quantizers import routes

import batch_norm_ref as ref

EINVAL = -22
BATCH, LEAKY = _lib.GN_BATCH, _lib.GN_ACT_LEAKY
M, R, F32, BF16 = _lib.LAYOUT_MAP, _lib.LAYOUT_ROWS, _lib.DTYPE_F32, _lib.DTYPE_BF16


def test_abi_accepts_batch_statistics_and_leaky_relu():
    L = _lib.lib()
    for layout in (M, R):
        for B, C, P in ((2, 3, 1), (8, 128, 4096), (8, 512, 961), (3, 130, 961)):
            assert L.vqhip_group_norm_ws_bytes(layout, B, C, P, BATCH) >= 8 * C, (layout, B, C, P)
        assert L.vqhip_group_norm_ws_bytes(layout, 1, 64, 1, BATCH) == -1                   # one value per channel
        assert L.vqhip_group_norm_ws_bytes(layout, 1, 64, 2, BATCH) >= 8 * 64
    fake = ctypes.c_void_p(0x1000)
    need = L.vqhip_group_norm_ws_bytes(M, 8, 128, 4096, BATCH)
    # a good shape, G and act: the null x is what is refused
    assert L.vqhip_group_norm_fwd(None, BF16, M, 8, 128, 4096, BATCH, fake, fake, 1e-5, LEAKY, fake, fake, fake, need, None) == EINVAL
    assert b'required' in L.vqhip_last_error()
    assert L.vqhip_group_norm_bwd(fake, None, BF16, M, 8, 128, 4096, BATCH, fake, fake, fake, LEAKY, fake, fake, fake, fake, need,
                                  None) == EINVAL
    assert b'required' in L.vqhip_last_error()
    # the workspace is checked in batch mode too
    assert L.vqhip_group_norm_fwd(fake, BF16, M, 8, 128, 4096, BATCH, fake, fake, 1e-5, LEAKY, fake, fake, fake, need - 1, None) == EINVAL
    assert b'ws too small' in L.vqhip_last_error()
    assert L.vqhip_group_norm_fwd(fake, F32, M, 1, 64, 1, BATCH, fake, fake, 1e-5, LEAKY, fake, fake, fake, 1 << 20, None) == EINVAL
    assert b'more than one value' in L.vqhip_last_error()


def test_abi_still_refuses_what_it_refused():
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    big = 1 << 30
    for G, act, word in ((BATCH, 3, b'act'), (-1, 0, b'G'), (0, 0, b'G'), (-3, 0, b'G'), (32, LEAKY, b'act'), (BATCH, -1, b'act')):
        assert L.vqhip_group_norm_fwd(fake, F32, M, 2, 64, 25, G, fake, fake, 1e-5, act, fake, fake, fake, big, None) == EINVAL, (G, act)
        assert word in L.vqhip_last_error(), (G, act, L.vqhip_last_error())
        assert L.vqhip_group_norm_bwd(fake, fake, F32, M, 2, 64, 25, G, fake, fake, fake, act, fake, fake, fake, fake, big, None) == EINVAL
        assert word in L.vqhip_last_error(), (G, act, L.vqhip_last_error())
    for G in (-1, 0, -3):
        assert L.vqhip_group_norm_ws_bytes(M, 2, 64, 25, G) == -1
    assert L.vqhip_group_norm_ws_bytes(M, 1 << 20, 4, 1 << 20, BATCH) == -1                 # n = B P >= 2^31


def test_python_layer_names_and_refusals():
    assert ops.GROUP_NORM_ACTS['leaky_relu'] == LEAKY and _lib.GN_LEAKY_SLOPE == 0.2
    x = torch.zeros(2, 4, 3, 3)
    assert ops.group_norm_refusal(x, 0) == '' and ops.group_norm_refusal(x.contiguous(memory_format=torch.channels_last), 0) == ''
    assert 'one' in ops.group_norm_refusal(torch.zeros(1, 4, 1, 1), 0) or '2 ..' in ops.group_norm_refusal(torch.zeros(1, 4, 1, 1), 0)
    assert 'float64' in ops.group_norm_refusal(x.double(), 0)
    assert 'neither' in ops.group_norm_refusal(x[:, :, ::2], 0)
    with pytest.raises(ValueError):
        functional.batch_norm(x, None, None, None, None, True, 0.1, 1e-5, 'silu')
    with pytest.raises(ValueError):
        functional.group_norm(x, 2, torch.ones(4), torch.zeros(4), 1e-6, 'leaky_relu')       # fused behind batch statistics only


@pytest.mark.parametrize('act', [None, 'leaky_relu'])
def test_restatement_against_torch_autograd(act):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 4, 3, generator=gen, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(5, generator=gen, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(5, generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn(3, 5, 4, 3, generator=gen, dtype=torch.float64)
    rm, rv = torch.zeros(5, dtype=torch.float64), torch.ones(5, dtype=torch.float64)
    want = functional.batch_norm_torch(x, rm, rv, gamma, beta, True, 1.0, 1e-5, act)
    y, stats, p = ref.forward(x.detach(), gamma.detach(), beta.detach(), 1e-5, act)
    # (F.leaky_relu holds 0.2 in double, the definition its fp32 rounding: 2^-26 relative on the slope branch)
    assert float(((y - want.detach()).abs() - 2.0 ** -25 * y.abs()).max()) < 1e-12
    assert float((rm - p['mean'].reshape(-1)).abs().max()) < 1e-14 and float((rv - p['unbiased'].reshape(-1)).abs().max()) < 1e-13
    wx, wg, wb = torch.autograd.grad(want, (x, gamma, beta), g)
    gx, dg, db, _ = ref.backward(g, x.detach(), gamma.detach(), beta.detach(), 1e-5, act)
    for got, exp in ((gx, wx), (dg, wg), (db, wb)):
        assert float((got - exp).abs().max()) < (1e-11 if act is None else 1e-6)


def _image(seed=0, size=32):
    return torch.randn(3, 3, size, size, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_module_on_the_cpu_is_its_own_sequential(training):
    torch.manual_seed(4)
    d = vqa.PatchGANDiscriminator(width=8).train(training)
    plain = copy.deepcopy(d)
    image = _image()
    out = d(image)
    want = plain._discriminator(image)
    assert torch.equal(out, want)
    assert d.last_route.name == 'torch' and 'device cpu' in d.last_route.why
    for (k, a), (_, b) in zip(d.state_dict().items(), plain.state_dict().items()):
        assert torch.equal(a, b), k
    assert int(d._discriminator[3].num_batches_tracked) == (1 if training else 0)


def test_state_dict_keys_and_strict_round_trip():
    d = vqa.PatchGANDiscriminator()
    want = [f'_discriminator.{i}.weight' for i in (0, 2, 5, 8, 11)] + ['_discriminator.0.bias', '_discriminator.11.bias'] \
        + [f'_discriminator.{i}.{n}' for i in (3, 6, 9) for n in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')]
    assert sorted(d.state_dict()) == sorted(want)
    other = vqa.PatchGANDiscriminator(fused=False)
    assert other.load_state_dict(d.state_dict(), strict=True).missing_keys == []
    assert all(torch.equal(a, b) for a, b in zip(d.state_dict().values(), other.state_dict().values()))
    assert d.fused and not other.fused and [type(m).__name__ for m in d._discriminator] == [type(m).__name__ for m in other._discriminator]


class Fake:                                                                     # a GPU tensor as far as the decision reads it
    def __init__(self, t):
        self.t = t
    is_cuda = True
    def __getattr__(self, name):
        return getattr(self.t, name)


def test_patchgan_why_reasons():
    d = vqa.PatchGANDiscriminator(width=8)
    x = torch.zeros(4, 3, 32, 32)
    assert routes.patchgan_why(d, x) == routes.Route('torch', 'the input is on device cpu, not on a GPU')
    meta = torch.zeros(4, 3, 32, 32, device='meta')
    assert routes.patchgan_why(d, Fake(meta)) == routes.Route('fused')
    assert routes.patchgan_why(d, Fake(meta.contiguous(memory_format=torch.channels_last))).name == 'fused'
    assert routes.patchgan_why(d, Fake(meta.bfloat16())).name == 'fused'
    assert 'float64' in routes.patchgan_why(d, Fake(meta.double())).why
    assert 'neither' in routes.patchgan_why(d, Fake(meta[:, :, ::2])).why
    assert routes.patchgan_why(vqa.PatchGANDiscriminator(width=8, fused=False), Fake(meta)) == routes.Route('torch', 'fused=False')

    class Mine(vqa.PatchGANDiscriminator):
        def forward(self, image):
            return super().forward(image) * 2

    assert routes.patchgan_why(Mine(width=8), Fake(meta)).why == 'Mine overrides forward'
    assert 'patchgan_why' in routes.__doc__
    # one site
    act = Fake(torch.zeros(4, 16, 8, 8, device='meta'))
    bn = torch.nn.BatchNorm2d(16)
    assert routes.patchgan_why(bn, act) == routes.Route('fused')
    assert 'eval mode' in routes.patchgan_why(copy.deepcopy(bn).eval(), act).why
    assert 'momentum=None' in routes.patchgan_why(torch.nn.BatchNorm2d(16, momentum=None), act).why
    assert routes.patchgan_why(torch.nn.BatchNorm2d(16, track_running_stats=False), act).why == 'track_running_stats=False'
    assert routes.patchgan_why(torch.nn.BatchNorm2d(16, affine=False), act).why == 'affine=False'
    assert 'values over the batch' in routes.patchgan_why(bn, Fake(torch.zeros(1, 16, 1, 1, device='meta'))).why
    assert 'device cpu' in routes.patchgan_why(bn, torch.zeros(4, 16, 8, 8)).why
    assert 'float64' in routes.patchgan_why(bn, Fake(torch.zeros(4, 16, 8, 8, device='meta').double())).why


def test_r1_penalty_on_the_cpu_runs_in_eval_mode_through_torch():
    torch.manual_seed(2)
    d = vqa.PatchGANDiscriminator(width=8)
    penalty = gan_losses.R1GradientPenalty()(d, _image(1))
    assert torch.isfinite(penalty).all() and d.training
    penalty.sum().backward()
    assert d._discriminator[0].weight.grad is not None and int(d._discriminator[3].num_batches_tracked) == 0


def test_the_gpu_cases_have_a_determined_branch():
    """Each case of tests/test_gpu_batch_norm.py: no value of the float64 restatement has |u| <= E_u, so the branch the kernel takes
    is the definition's and E_d = 0 (include/vqhip.h, LEAKY RELU).  Checked here, without a GPU, on the very inputs."""
    import test_gpu_batch_norm as gpu_cases
    for shape in gpu_cases.SHAPES:
        for dtype in gpu_cases.DTYPES:
            x, g, gamma, beta = gpu_cases.inputs(shape, dtype)
            _, _, p = ref.forward(x, gamma, beta, gpu_cases.EPS, 'leaky_relu')
            margin = ref.branch_margin(gamma, p)
            assert margin > 1.0, (shape, dtype, margin)
