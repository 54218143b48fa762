"""Float64 restatement of the two modes of include/vqhip.h that LlamaTransformer runs on - add + RMS norm (the add + layer norm
calls with beta / dbeta NULL) and SwiGLU (act 3 of the row bias-activation calls) - forward and analytic gradients, and the error
bounds of their ERROR BOUND paragraphs evaluated on the restatement's own quantities, for the CPU and GPU tests.  Plain torch apart
from the bound formulas, which are the ones vector_quantization_amd._lib exposes."""
import torch

from vector_quantization_amd import _lib

from vit_ops_ref import ln_slabs, rounded_sum                                   # noqa: F401  (s and the slabs are the layer norm's)


# ---- add + RMS norm ----------------------------------------------------------------------------------------------------------------
def rms_forward(s, gamma, eps=1e-5):
    """(y, stats [R, 2], parts) of the RMS norm of the rows s [R, D], in float64."""
    s = s.double()
    ms = (s * s).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(ms + eps)
    xh = s * rstd
    y = xh * gamma.double()
    return y, torch.cat([torch.zeros_like(rstd), rstd], 1), dict(xh=xh, rstd=rstd)


def rms_backward(g, s, gamma, eps=1e-5, g_skip=None):
    """(gx, dgamma, parts): gx includes g_skip; parts['gx_norm'] is the norm's own term."""
    _, _, p = rms_forward(s, gamma, eps)
    xh, g = p['xh'], g.double()
    t = g * gamma.double()
    m2 = (t * xh).mean(1, keepdim=True)
    gx = p['rstd'] * (t - xh * m2)
    p.update(t=t, m2=m2, gx_norm=gx)
    return (gx if g_skip is None else gx + g_skip.double()), (g * xh).sum(0), p


def rms_forward_bound(gamma, y, p):
    return _lib.rms_y_bound(y.shape[1], p['xh'].abs(), gamma.double().abs(), y.abs())


def rms_backward_bounds(g, gamma, gx, p, g_skip=None):
    """(E_gx' per element, E_dgamma [D])."""
    R, D = g.shape
    xh, t, g = p['xh'].abs(), p['t'].abs(), g.double().abs()
    e_xh = _lib.gn_xhat_bound(D, 0.0, xh)
    e_t = 2.0 * _lib.GN_U * t
    mean = lambda v: v.mean(1, keepdim=True)
    e_gx = _lib.rms_gx_bound(D, p['rstd'], xh, t, p['m2'].abs(), mean(t * xh), mean(e_t * xh + t * e_xh), p['gx_norm'].abs())
    e_dg = _lib.gn_param_bound(ln_slabs(R), 2.0, (g * xh).sum(0), (_lib.GN_U * g * xh + g * e_xh).sum(0))
    return (e_gx if g_skip is None else _lib.ln_gx_bound(e_gx, gx.abs())), e_dg


# ---- SwiGLU ------------------------------------------------------------------------------------------------------------------------
def swiglu_forward(x):
    """(y, parts) of y = silu(gate) up of x [R, 2 F] = (gate | up) in float64; the sigmoid without a cancelling subtraction."""
    a, up = x.double().chunk(2, dim=1)
    e = torch.exp(-a.abs())
    sg = torch.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    qc = torch.where(a >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    s = a * sg
    return s * up, dict(a=a, up=up, sg=sg, qc=qc, s=s)


def swiglu_backward(g, x):
    """(gx [R, 2 F], parts)."""
    y, p = swiglu_forward(x)
    g = g.double()
    d = p['sg'] * (1.0 + p['a'] * p['qc'])
    p.update(d=d, g=g)
    return torch.cat([g * p['up'] * d, g * p['s']], 1), p


def swiglu_forward_bound(y, p):
    return _lib.swiglu_bound(p['a'].abs(), p['up'].abs(), y.abs())


def swiglu_backward_bound(gx, p):
    """E_gx per element of [R, 2 F]."""
    F = gx.shape[1] // 2
    e_gate, e_up = _lib.swiglu_gx_bounds(p['a'].abs(), p['sg'], p['d'].abs(), p['s'].abs(), p['g'].abs(), p['up'].abs(),
                                         gx[:, :F].abs(), gx[:, F:].abs())
    return torch.cat([e_gate, e_up], 1)
