"""Float64 restatement of the GroupNorm (+ SiLU) definition of include/vqhip.h, forward and analytic gradients, and the error
bounds of its ERROR BOUND paragraph evaluated on the restatement's own quantities, for the CPU and GPU tests.  Plain torch apart
from the bound formulas, which are the ones vector_quantization_amd._lib exposes."""
import torch

from vector_quantization_amd import _lib


def _grouped(x, G):
    B, C = x.shape[:2]
    return x.double().reshape(B, G, -1)


def _per_channel(p, x):
    return p.double().view((1, -1) + (1,) * (x.dim() - 2))


def forward(x, G, gamma, beta, eps=1e-6, act=None):
    """(y, stats [B, G, 2], parts): every intermediate of the definition, in float64, shaped like x."""
    xg = _grouped(x, G)
    mean = xg.mean(2, keepdim=True)
    var = ((xg - mean) ** 2).mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = ((xg - mean) * rstd).reshape(x.shape)
    u = xh * _per_channel(gamma, x) + _per_channel(beta, x)
    s = torch.sigmoid(u)
    y = u * s if act == 'silu' else u
    parts = dict(xh=xh, u=u, s=s, mean=mean, rstd=rstd, mabs=xg.abs().mean(2, keepdim=True), n=xg.shape[2])
    return y, torch.cat([mean, rstd], 2), parts


def backward(g, x, G, gamma, beta, eps=1e-6, act=None):
    """(gx, dgamma, dbeta, parts) by the formulas of the definition."""
    _, _, p = forward(x, G, gamma, beta, eps, act)
    xh, u, s = p['xh'], p['u'], p['s']
    d = s * (1 + u * (1 - s)) if act == 'silu' else torch.ones_like(u)
    gu = g.double() * d
    t = gu * _per_channel(gamma, x)
    m1 = _grouped(t, G).mean(2, keepdim=True)
    m2 = _grouped(t * xh, G).mean(2, keepdim=True)
    gx = (p['rstd'] * (_grouped(t, G) - m1 - _grouped(xh, G) * m2)).reshape(x.shape)
    dims = [k for k in range(x.dim()) if k != 1]
    p.update(d=d, gu=gu, t=t, m1=m1, m2=m2)
    return gx, (gu * xh).sum(dims), gu.sum(dims), p


def _expand(v, x, G):
    """A per-group [B, G, 1] quantity shaped like x."""
    return v.expand(-1, -1, x.numel() // (x.shape[0] * G)).reshape(x.shape)


def forward_bound(x, G, gamma, beta, eps, act, y, parts):
    """E_y per element: the bound on |kernel - exact| in fp32, before the store."""
    n = parts['n']
    q = _expand(_lib.gn_q(n, parts['mabs'], parts['rstd']), x, G)
    return _lib.gn_y_bound(n, q, parts['xh'].abs(), _per_channel(gamma, x).abs(), parts['u'].abs(), y.abs(), 1 if act == 'silu' else 0)


def backward_bounds(g, x, G, gamma, beta, eps, act, gx, p, slabs):
    """(E_gx per element, E_dgamma [C], E_dbeta [C])."""
    n, a = p['n'], 1 if act == 'silu' else 0
    q = _expand(_lib.gn_q(n, p['mabs'], p['rstd']), x, G)
    gam = _per_channel(gamma, x).abs()
    xh, u = p['xh'].abs(), p['u'].abs()
    e_xh = _lib.gn_xhat_bound(n, q, xh)
    e_d = _lib.gn_d_bound(n, q, xh, gam, u, a)
    t = p['t'].abs()
    e_t = g.double().abs() * gam * e_d + 2.0 * _lib.GN_U * t
    mean = lambda v: _expand(_grouped(v, G).mean(2, keepdim=True), x, G)
    e_gx = _lib.gn_gx_bound(n, q, _expand(p['rstd'], x, G), xh, e_t, t, _expand(p['m1'].abs(), x, G), _expand(p['m2'].abs(), x, G),
                            mean(t), mean(t * xh), mean(e_t), mean(e_t * xh + t * e_xh), gx.abs())
    gu = p['gu'].abs()
    e_gu = g.double().abs() * e_d + _lib.GN_U * gu
    dims = [k for k in range(x.dim()) if k != 1]
    e_dg = _lib.gn_param_bound(slabs, 2.0, (gu * xh).sum(dims), (e_gu * xh + gu * e_xh).sum(dims))
    e_db = _lib.gn_param_bound(slabs, 0.0, gu.sum(dims), e_gu.sum(dims))
    return e_gx, e_dg, e_db


def slabs(B, C, P, G):
    """The slabs of the dgamma / dbeta first stage: B times the chunks of a group (include/vqhip.h, LAUNCH SHAPE)."""
    n = C // G * P
    return B * (1 if n <= _lib.GN_SMALL else -(-n // _lib.GN_CHUNK))
