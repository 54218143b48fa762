"""Float64 restatement of the StyleGAN2 discriminator ops of include/vqhip.h (bias-activation, the 4-tap FIR blur, their gradients)
and of the reference's discriminator composition, for the CPU and GPU tests.  Plain torch; nothing here calls the library."""
import torch
import torch.nn.functional as F

SLOPE, SCALE = 0.2, 2.0 ** 0.5


def _per_channel(bias, x):
    return bias.double().view((1, -1) + (1,) * (x.dim() - 2))


def bias_act(x, bias):
    t = x.double() + _per_channel(bias, x)
    return torch.where(t > 0, t, t * SLOPE) * SCALE


def bias_act_grad(g, y):
    """(gx, gbias) from the saved output y: the slope branch wherever y > 0 is false (zeros and NaNs included)."""
    gx = g.double() * torch.where(y.double() > 0, SCALE, SCALE * SLOPE)
    dims = [d for d in range(g.dim()) if d != 1]
    return gx, gx.sum(dims)


def kernel():
    k = torch.tensor([1., 3., 3., 1.], dtype=torch.float64)
    return k[None, :] * k[:, None] / 64


def blur(x, pad, down=1):
    """pad = (py0, py1, px0, px1); F.pad plus a depthwise F.conv2d, strided slicing for down."""
    py0, py1, px0, px1 = pad
    C = x.shape[1]
    xp = F.pad(x.double(), (px0, px1, py0, py1))
    return F.conv2d(xp, kernel().expand(C, 1, 4, 4).to(x.device), groups=C)[:, :, ::down, ::down]


def blur_adjoint(g, size, pad, down=1):
    """The gradient of blur with respect to its input of plane ``size``, by autograd in float64."""
    x = torch.zeros(*g.shape[:2], *size, dtype=torch.float64, device=g.device, requires_grad=True)
    out = blur(x, pad, down)
    return torch.autograd.grad(out, x, g.double())[0]


def act_factor(x, bias):
    t = x.double() + _per_channel(bias, x)
    return torch.where(t > 0, SCALE, SCALE * SLOPE)


def std_channel(x, groups=4, eps=1e-8):
    """Std of the reference: '(bg b) c h w -> bg b c h w', variance over bg, mean over c h w, repeated '(bg b)'."""
    B = x.shape[0]
    bg = min(B, groups)
    y = x.reshape(bg, B // bg, *x.shape[1:])
    y = (y.var(0, unbiased=False) + eps).sqrt().mean(dim=(1, 2, 3))
    return torch.cat([x, y.repeat(bg).view(B, 1, 1, 1).expand(B, 1, *x.shape[2:])], 1)


def discriminator(sd, image):
    """The reference's composition from a state dict of StyleGAN2Discriminator, in float64: blur, THEN the stride-2 convolution."""
    sd = {k: v.double() for k, v in sd.items()}

    def conv(x, key, stride=1, padding=0):
        w = sd[key + '._original_weight']
        return F.conv2d(x, w / (w[0].numel() ** 0.5), None, stride, padding)

    def act(x, key):
        return bias_act(x, sd[key + '._activate.bias'])

    x = act(conv(image.double(), '_layers.0'), '_layers.0')
    n = 1
    while f'_layers.{n}._shortcut._original_weight' in sd:
        p = f'_layers.{n}'
        r = act(conv(x, p + '._residual.0', 1, 1), p + '._residual.0')
        r = act(conv(blur(r, (2, 2, 2, 2)), p + '._residual.1', 2), p + '._residual.1')
        s = conv(blur(x, (1, 1, 1, 1)), p + '._shortcut', 2)
        x = (s + r) / 2 ** 0.5
        n += 1
    x = std_channel(x)
    x = act(conv(x, f'_layers.{n + 1}', 1, 1), f'_layers.{n + 1}')
    x = x.flatten(1)
    w = sd['_projector.0._original_weight']
    x = bias_act(x @ (w / w.shape[1] ** 0.5).t(), sd['_projector.0._activate.bias'])
    w = sd['_projector.1._original_weight']
    return x @ (w / w.shape[1] ** 0.5).t() + sd['_projector.1.bias']
