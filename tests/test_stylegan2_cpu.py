"""CPU checks of the discriminator side of the VQGAN configs: the three registries and the shipped config dicts, the state-dict
keys of StyleGAN2Discriminator against tests/golden/stylegan2_keys.json (names and shapes only, written from the reference's
stylegan2.py by reading it: the reference does not import without mmcv), the torch route in float64 against the restatement of
tests/stylegan2_ref.py, the losses against closed forms, and the reasons of routes.stylegan2_why."""
import json
import os

import pytest
import torch

import vector_quantization_amd as vqa
from vector_quantization_amd import discriminators, gan_losses, registries
from vector_quantization_amd.quantizers import routes

import stylegan2_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stylegan2_keys.json')


def test_registries_and_shipped_config_dicts_build():
    assert issubclass(registries.VQDiscriminatorRegistry, registries.VQModelRegistry)
    assert issubclass(registries.VQGeneratorLossRegistry, registries.VQLossRegistry)
    assert issubclass(registries.VQDiscriminatorLossRegistry, registries.VQLossRegistry)
    # configs/vqgan/model.py:26, :31, :32 unchanged
    d = registries.VQDiscriminatorRegistry.build(dict(type='PatchGANDiscriminator'))
    assert type(d) is vqa.PatchGANDiscriminator and d(torch.zeros(1, 3, 32, 32)).shape == (1, 1, 2, 2)
    assert [k for k in d.state_dict()][:2] == ['_discriminator.0.weight', '_discriminator.0.bias'] and '_discriminator.11.weight' in d.state_dict()
    assert type(registries.VQGeneratorLossRegistry.build(dict(type='VQGANGeneratorLoss'))) is vqa.VQGANGeneratorLoss
    assert type(registries.VQDiscriminatorLossRegistry.build(dict(type='VQGANDiscriminatorLoss'))) is vqa.VQGANDiscriminatorLoss
    assert type(registries.VQGeneratorLossRegistry.build(dict(type='NonSaturatingLoss'))) is vqa.NonSaturatingLoss
    # the two stylegan2 overrides
    s = registries.VQDiscriminatorRegistry.build(dict(type='StyleGAN2Discriminator', image_size=256))
    assert type(s) is vqa.StyleGAN2Discriminator and s.fused
    for name in ('BaseDiscriminator', 'PatchGANDiscriminator', 'StyleGAN2Discriminator', 'VQGANGeneratorLoss', 'NonSaturatingLoss',
                 'VQGANDiscriminatorLoss', 'R1GradientPenalty'):
        assert name in vqa.__all__ and hasattr(vqa, name)


@pytest.mark.parametrize('image_size', [16, 256])
def test_state_dict_keys_and_shapes_equal_the_fixture(image_size):
    want = json.load(open(GOLDEN))[str(image_size)]
    sd = vqa.StyleGAN2Discriminator(image_size=image_size).state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == want
    conv = vqa.StyleGAN2Discriminator(image_size=image_size)._layers[1]._shortcut
    assert 'weight' not in dict(conv.named_parameters()) and 'weight' not in dict(conv.named_buffers()) and torch.is_tensor(conv.weight)


@pytest.fixture(scope='module')
def small():
    torch.manual_seed(11)
    d = vqa.StyleGAN2Discriminator(image_size=16).double()
    d.init_weights({})
    return d, torch.randn(4, 3, 16, 16, dtype=torch.float64)


def test_torch_route_float64_against_the_restatement(small):
    d, image = small
    assert all(float(p.abs().max()) == 0 for n, p in d.named_parameters() if n.endswith('bias'))        # init_weights: zero biases
    assert abs(float(d._layers[4]._original_weight.std()) - 1) < 0.01
    with torch.no_grad():
        for n, p in d.named_parameters():
            if n.endswith('bias'):
                p.normal_(0, 0.3)
        out = d(image)
        want = ref.discriminator(d.state_dict(), image)
    assert out.shape == (4, 1) and d.last_route == routes.Route('torch', 'the input is on device cpu, not on a GPU')
    assert float((out - want).abs().max()) <= 1e-12 * float(want.abs().max())
    with torch.no_grad():
        for n, p in d.named_parameters():
            if n.endswith('bias'):
                p.zero_()


def test_std_grouping_on_a_hand_computed_case():
    """B = 8, bg = 4: sample n = g * 2 + i holds the constant v[n]; position i sees v[i], v[2 + i], v[4 + i], v[6 + i]."""
    v = torch.tensor([1., 2., 4., 8., 16., 32., 64., 128.], dtype=torch.float64)
    x = v.view(8, 1, 1, 1).expand(8, 3, 2, 2).contiguous()
    out = discriminators.Std()(x)
    assert out.shape == (8, 4, 2, 2) and torch.equal(out[:, :3], x)
    want = [(v[i::2].var(unbiased=False) + 1e-8).sqrt() for i in range(2)]      # i = 0: {1, 4, 16, 64}; i = 1: {2, 8, 32, 128}
    assert abs(float(want[0]) - (((1 - 21.25) ** 2 + (4 - 21.25) ** 2 + (16 - 21.25) ** 2 + (64 - 21.25) ** 2) / 4 + 1e-8) ** 0.5) < 1e-12
    for n in range(8):
        assert torch.allclose(out[n, 3], want[n % 2].expand(2, 2), rtol=1e-14, atol=0)
    assert torch.allclose(ref.std_channel(x), out, rtol=1e-14, atol=0)


def test_shortcut_rewrite_equals_blur_then_stride_two():
    torch.manual_seed(3)
    conv = discriminators.Conv2d(5, 7, 1, downsample=True, bias=False).double()
    x = torch.randn(2, 5, 16, 16, dtype=torch.float64)
    want = conv(x)                                                              # torch route: blur (pad 1), 1 x 1 convolution at stride 2
    blurred = discriminators.blur_torch(x, conv._blur.kernel, (1, 1), down=2)
    got = conv._conv(blurred, stride=1)
    assert got.shape == want.shape == (2, 7, 8, 8)
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    assert torch.allclose(discriminators.blur_torch(x, conv._blur.kernel, (1, 1)), ref.blur(x, (1, 1, 1, 1)), rtol=1e-14, atol=1e-15)
    assert torch.allclose(discriminators.bias_act_torch(x, torch.ones(5, dtype=torch.float64)), ref.bias_act(x, torch.ones(5)), rtol=1e-15, atol=0)


def test_r1_gradient_penalty_reaches_the_parameters(small):
    """A finite scalar with a gradient for every parameter the penalty depends on.  The bias of the last Linear is added behind
    everything the image passes through, so d logits / d image does not contain it in any implementation: autograd leaves its
    gradient unset."""
    d, image = small
    d.zero_grad()
    training = d.training
    penalty = gan_losses.R1GradientPenalty()(d, image)
    assert penalty.dim() == 0 and torch.isfinite(penalty) and penalty > 0 and d.training == training
    penalty.backward()
    for n, p in d.named_parameters():
        if n == '_projector.1.bias':
            assert p.grad is None or float(p.grad.abs().max()) == 0
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert all(float(p.grad.abs().max()) > 0 for n, p in d.named_parameters() if n.endswith('_original_weight'))


def test_losses_against_closed_forms():
    fake = torch.tensor([[-2.0], [-0.5], [0.25], [3.0]], dtype=torch.float64)
    real = torch.tensor([[2.0], [0.5], [-0.25], [-3.0]], dtype=torch.float64)
    hinge = gan_losses.VQGANDiscriminatorLoss()(fake, real)
    # relu(1 + fake) = 0, .5, 1.25, 4; relu(1 - real) = 0, .5, 1.25, 4; halves of the sums: 0, .5, 1.25, 4; mean
    assert abs(float(hinge) - (0 + 0.5 + 1.25 + 4) / 4) < 1e-15
    assert torch.equal(gan_losses.VQGANDiscriminatorLoss(reduction='none')(fake, real), torch.tensor([[0.], [0.5], [1.25], [4.]], dtype=torch.float64))
    assert abs(float(gan_losses.VQGANGeneratorLoss()(fake)) - (2 + 0.5 - 0.25 - 3) / 4) < 1e-15
    want = torch.log1p(torch.exp(-fake)).mean()                                 # BCE with ones: softplus(-logit)
    assert abs(float(gan_losses.NonSaturatingLoss()(fake)) - float(want)) < 1e-14
    assert abs(float(gan_losses.VQGANGeneratorLoss(weight=0.5, reduction='sum')(fake)) - 0.5 * (2 + 0.5 - 0.25 - 3)) < 1e-15


def test_stylegan2_why_reasons():
    d = vqa.StyleGAN2Discriminator(image_size=16)
    x = torch.zeros(4, 3, 16, 16)
    assert 'device cpu' in routes.stylegan2_why(d, x).why and routes.stylegan2_why(d, x).name == 'torch'
    meta = torch.zeros(4, 3, 16, 16, device='meta')

    class Fake:                                                                 # a GPU tensor as far as the decision reads it
        def __init__(self, t):
            self.t = t
        is_cuda = True
        def __getattr__(self, name):
            return getattr(self.t, name)

    assert routes.stylegan2_why(d, Fake(meta)) == routes.Route('fused')
    assert routes.stylegan2_why(d, Fake(meta.contiguous(memory_format=torch.channels_last))).name == 'fused'
    assert 'float64' in routes.stylegan2_why(d, Fake(meta.double())).why
    assert 'neither' in routes.stylegan2_why(d, Fake(meta[:, :, ::2])).why
    assert routes.stylegan2_why(vqa.StyleGAN2Discriminator(image_size=16, fused=False), Fake(meta)) == routes.Route('torch', 'fused=False')
    assert 'kernel_size=5' in routes.stylegan2_why(discriminators.Conv2d(4, 4, 5, downsample=True), Fake(meta)).why

    class Mine(vqa.StyleGAN2Discriminator):
        def forward(self, image):
            return super().forward(image)

    assert routes.stylegan2_why(Mine(image_size=16), Fake(meta)).why == 'Mine overrides forward'
    assert 'stylegan2_why' in routes.__doc__
