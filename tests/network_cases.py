"""The cases behind tests/golden/networks/*.npz, and the one way a case is run (a plain module: torch and numpy only).

The recipe (oracle/make_network_golden.py) runs ``run_case`` on the reference's own module, the tests run it on this package's
module of the same name: the same seeded state dict loaded with ``strict=True``, the same seeded input, the same scalar
``sum(out * g)`` with a seeded ``g``.  Whatever differs afterwards is the module.

Weights are not stored.  ``seeded_state_dict`` walks the keys of a state dict in sorted order and draws every tensor from ONE
``torch.Generator`` in float64:

- ``num_batches_tracked``: 0;
- ``running_var``: ``0.5 + rand``;
- a one-dimensional ``weight`` (GroupNorm, LayerNorm, BatchNorm): ``1 + 0.2 randn``;
- a ``weight`` / ``in_proj_weight`` of two or more dimensions: ``randn / fan_in**0.5`` (fan_in = the product of every dimension
  but the first), which keeps the activations of a deep stack of order one, so that no softmax saturates and no gradient
  vanishes for a reason that is not the module's;
- everything else (biases, running means, cls token, position embedding): ``0.5 randn``.

The draws are rounded to fp32 and only then cast to the dtype of the run, so float64, fp32 and bf16 runs see the same values.

What a fixture keeps of a tensor (``stored``): everything of an output, an input gradient, a running statistic and of a parameter
gradient of at most ``WHOLE`` elements; of a larger parameter gradient the ``WHOLE`` elements at positions drawn without
replacement by ``numpy.random.RandomState`` (whose stream numpy freezes) from the case's seed and the tensor's name.  Every
parameter keeps a gradient check; a committed file stays below the size the repository allows for a fixture.
"""
import contextlib
import zlib

import numpy as np
import torch

WHOLE = 512

# the SMALL_* kwargs of tests/test_vqkd_autoencoder_cpu.py
_VQKD_ENCODER = dict(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, out_chans=8)
_VQKD_DECODER = dict(img_size=2, in_chans=8, embed_dim=64, depth=1, num_heads=2, out_chans=16)
_PATCHGAN = dict(width=16, depth=3)

# name -> cls, kwargs, input shape, train mode, seed.  ``rows``: a ViT (contiguous rows), else a convolutional network (NCHW and
# channels-last inputs on the GPU).
CASES = {
    # two levels, 64 -> 128 channels (2 and 4 per group): a convolution shortcut, a Downsample, attention in the last level, refine
    'vqgan_encoder': dict(cls='VQGANEncoder', kwargs=dict(width=64, width_mults=(1, 2), depth_mult=1, out_channels=8),
                          input=(2, 3, 32, 32), train=True, seed=1101),
    # 128 -> 64 channels: refine and attention in the first level, an Upsample, a convolution shortcut
    'vqgan_decoder': dict(cls='VQGANDecoder', kwargs=dict(in_channels=8, width=64, width_mults=(2, 1), depth_mult=1),
                          input=(2, 8, 8, 8), train=True, seed=1102),
    'vqkd_encoder_32': dict(cls='VQKDEncoder', kwargs=_VQKD_ENCODER, input=(2, 3, 32, 32), train=True, seed=1103, rows=True),
    # 48 pixels: 3 x 3 patches against a 2 x 2 position embedding, interpolate_pos_encoding's bicubic branch
    'vqkd_encoder_48': dict(cls='VQKDEncoder', kwargs=_VQKD_ENCODER, input=(2, 3, 48, 48), train=True, seed=1104, rows=True),
    'vqkd_decoder_2': dict(cls='VQKDDecoder', kwargs=_VQKD_DECODER, input=(2, 8, 2, 2), train=True, seed=1105, rows=True),
    # depth 2, a 3 x 3 map against the 2 x 2 position embedding, and 2 x 2 output patches: the (p q c) rearrangement
    'vqkd_decoder_3': dict(cls='VQKDDecoder', kwargs=dict(_VQKD_DECODER, depth=2, out_chans=4, out_patch_size=2),
                           input=(2, 8, 3, 3), train=True, seed=1106, rows=True),
    'patchgan_train': dict(cls='PatchGANDiscriminator', kwargs=_PATCHGAN, input=(2, 3, 32, 32), train=True, seed=1107),
    'patchgan_eval': dict(cls='PatchGANDiscriminator', kwargs=_PATCHGAN, input=(2, 3, 32, 32), train=False, seed=1108),
}

# init_weights: the class, its kwargs, the seed in front of the constructor and the one in front of init_weights
INIT_CASES = {
    'vqkd_encoder': dict(cls='VQKDEncoder', kwargs=_VQKD_ENCODER, seeds=(11, 12)),
    'vqkd_decoder': dict(cls='VQKDDecoder', kwargs=dict(_VQKD_DECODER, depth=2), seeds=(13, 14)),
    'patchgan': dict(cls='PatchGANDiscriminator', kwargs=_PATCHGAN, seeds=(15, 16)),
}

# the GAN losses: logits of two shapes; every reduction, and a weight that is not 1
LOSS_SHAPES = ((2, 1, 2, 2), (3, 1, 5, 7))
LOSS_SETTINGS = (dict(reduction='none', weight=1.0), dict(reduction='mean', weight=1.0), dict(reduction='sum', weight=1.0),
                 dict(reduction='mean', weight=0.5), dict(reduction='sum', weight=0.25))
LOSS_CLASSES = ('VQGANGeneratorLoss', 'NonSaturatingLoss', 'VQGANDiscriminatorLoss')
R1_CASE = dict(kwargs=_PATCHGAN, input=(2, 3, 32, 32), seed=1109, train=True)
LOSS_SEED = 1110


def seeded_tensor(shape, seed: int) -> torch.Tensor:
    """``randn`` of ``shape`` in float64, rounded to fp32 (returned as float64)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64).float().double()


def seeded_state_dict(template: dict, seed: int) -> dict:
    """A state dict with the keys, shapes and integer dtypes of ``template`` (see the module docstring); floats as float64."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key in sorted(template):
        t = template[key]
        leaf = key.rsplit('.', 1)[-1]
        if leaf == 'num_batches_tracked':
            out[key] = torch.zeros_like(t)
            continue
        shape = tuple(t.shape)
        if leaf == 'running_var':
            v = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
        else:
            v = torch.randn(shape, generator=g, dtype=torch.float64)
            if leaf == 'weight' and t.dim() == 1:
                v = 1 + 0.2 * v
            elif leaf in ('weight', 'in_proj_weight') and t.dim() >= 2:
                v = v / float(np.prod(shape[1:])) ** 0.5
            else:
                v = 0.5 * v
        out[key] = v.float().double()
    return out


def load_seeded(module, seed: int, dtype: torch.dtype):
    module.to(dtype=dtype)
    sd = seeded_state_dict(module.state_dict(), seed)
    module.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    return module


def positions(name: str, numel: int, seed: int):
    """Where ``stored`` reads a parameter gradient ``name`` of ``numel`` elements: None for all of it."""
    if numel <= WHOLE:
        return None
    rs = np.random.RandomState((seed * 1000003 + zlib.crc32(name.encode())) % (2 ** 32))
    return np.sort(rs.choice(numel, WHOLE, replace=False))


def stored(name: str, t: torch.Tensor, seed: int) -> np.ndarray:
    a = t.detach().to('cpu', torch.float64).contiguous().numpy()
    if not name.startswith('grad/'):
        return a
    pos = positions(name, a.size, seed)
    return a if pos is None else a.reshape(-1)[pos]


def call(module, x: torch.Tensor) -> torch.Tensor:
    """Encoders and decoders take ``(x, memo)`` and return ``(x, memo)``; a discriminator takes the image."""
    out = module(x, {}) if type(module).__name__ != 'PatchGANDiscriminator' else module(x)
    return out[0] if isinstance(out, tuple) else out


def run_case(module, case: dict, *, device='cpu', dtype=torch.float64, channels_last=False, autocast=None) -> dict:
    """name -> tensor: ``out``, ``gin``, ``grad/<parameter>`` for every parameter (zeros where autograd reached none) and, for a
    module in train mode with running statistics, ``running_mean/<module>`` / ``running_var/<module>`` after the one forward."""
    seed = case['seed']
    load_seeded(module, seed, dtype).to(device)
    module.train(case['train'])
    x = seeded_tensor(case['input'], seed + 1).to(device, dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    ctx = torch.autocast(torch.device(device).type, dtype=autocast) if autocast is not None else contextlib.nullcontext()
    with ctx:
        out = call(module, x)
    g = seeded_tensor(out.shape, seed + 2).to(device, dtype)
    (out.to(dtype) * g).sum().backward()
    res = {'out': out.detach(), 'gin': x.grad}
    for n, p in module.named_parameters():
        res['grad/' + n] = torch.zeros_like(p) if p.grad is None else p.grad
    if case['train']:
        for n, b in module.named_buffers():
            leaf = n.rsplit('.', 1)
            if leaf[-1] in ('running_mean', 'running_var'):
                res[f'{leaf[-1]}/{leaf[0]}'] = b.detach()
    return res


def rel_err(got: np.ndarray, want: np.ndarray) -> float:
    """``max|got - want| / max|want|``, the figure every tolerance of these tests is stated in."""
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def init_statistics(module, seeds, config) -> dict:
    """``torch.manual_seed(seeds[1])``, ``init_weights(config)``; name -> (mean, std) of every parameter in float64.  The module was
    built after ``torch.manual_seed(seeds[0])`` by the caller."""
    torch.manual_seed(seeds[1])
    module.init_weights(config)
    return {n: np.array([p.detach().double().mean().item(), p.detach().double().std(unbiased=False).item()])
            for n, p in module.named_parameters()}


def run_losses(classes: dict, dtype=torch.float64) -> dict:
    """name -> tensor for the GAN losses built from ``classes`` (name -> class; ``PatchGANDiscriminator`` among them).  For
    every shape, setting and loss over logits: the value and, through ``sum(value * g)``, the gradient to each logit tensor.  For
    ``R1GradientPenalty`` on the seeded discriminator in train mode: the value and the gradient to every parameter per setting,
    ``r1/modes_restored`` (1 where every module has its mode back) and the running statistics afterwards (eval mode moves none)."""
    res = {}
    for si, shape in enumerate(LOSS_SHAPES):
        fake, real = seeded_tensor(shape, LOSS_SEED + 2 * si), seeded_tensor(shape, LOSS_SEED + 2 * si + 1)
        for ki, kw in enumerate(LOSS_SETTINGS):
            for cname in LOSS_CLASSES:
                f, r = fake.to(dtype).clone().requires_grad_(), real.to(dtype).clone().requires_grad_()      # fresh leaves
                value = classes[cname](**kw)(*((f, r) if cname == 'VQGANDiscriminatorLoss' else (f,)))
                g = seeded_tensor(value.shape, LOSS_SEED + 100 + ki).to(dtype)
                (value * g).sum().backward()
                key = f'{cname}/s{si}/k{ki}'
                res[key + '/value'], res[key + '/dfake'] = value.detach(), f.grad
                if r.grad is not None:
                    res[key + '/dreal'] = r.grad
    case = R1_CASE
    disc = load_seeded(classes['PatchGANDiscriminator'](**case['kwargs']), case['seed'], dtype).train(case['train'])
    image = seeded_tensor(case['input'], case['seed'] + 1).to(dtype)
    before = {m: m.training for m in disc.modules()}
    restored = True
    for ki, kw in enumerate(LOSS_SETTINGS):
        disc.zero_grad()
        value = classes['R1GradientPenalty'](**kw)(disc, image)
        restored = restored and all(m.training == mode for m, mode in before.items())
        g = seeded_tensor(value.shape, LOSS_SEED + 200 + ki).to(dtype)
        (value * g).sum().backward()
        res[f'r1/k{ki}/value'] = value.detach()
        for n, p in disc.named_parameters():
            res[f'grad/r1/k{ki}/{n}'] = torch.zeros_like(p) if p.grad is None else p.grad.clone()
    res['r1/modes_restored'] = torch.tensor(float(restored), dtype=torch.float64)
    for n, b in disc.named_buffers():
        res['r1/buffer/' + n] = b.detach().double()
    return res
