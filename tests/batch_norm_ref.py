"""Float64 restatement of the batch-statistics mode of include/vqhip.h (G == VQHIP_GN_BATCH: BatchNorm2d in training mode with an
optional LeakyReLU(0.2)), forward, analytic gradients and the unbiased variance, on inputs converted from their storage dtype, and
the bounds of the header's ERROR BOUND / LEAKY RELU / BATCH STATISTICS paragraphs evaluated on the restatement's own quantities
with n = B P.  Plain torch apart from the bound formulas, which are the ``_lib.gn_*`` copies of the header's macros."""
import torch

from vector_quantization_amd import _lib

SLOPE = float(torch.tensor(_lib.GN_LEAKY_SLOPE, dtype=torch.float32))          # the kernels hold the fp32 rounding of the slope


def _channels(x):
    """[C, n] float64: channel c's values over all images and positions."""
    return x.double().transpose(0, 1).reshape(x.shape[1], -1)


def _back(v, x):
    """A [C, n] quantity shaped like x."""
    B, C = x.shape[:2]
    return v.reshape(C, B, *x.shape[2:]).transpose(0, 1)


def _col(p):
    return p.double().reshape(-1, 1)


def forward(x, gamma, beta, eps=1e-5, act=None):
    """(y shaped like x, stats [C, 2], parts): every intermediate of the definition in float64; the per-value parts are [C, n]."""
    xc = _channels(x)
    n = xc.shape[1]
    mean = xc.mean(1, keepdim=True)
    m2 = ((xc - mean) ** 2).sum(1, keepdim=True)
    var = m2 / n
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (xc - mean) * rstd
    u = xh * _col(gamma) + _col(beta)
    y = torch.where(u > 0, u, SLOPE * u) if act == 'leaky_relu' else u
    parts = dict(xh=xh, u=u, y=y, mean=mean, rstd=rstd, var=var, unbiased=m2 / (n - 1), mabs=xc.abs().mean(1, keepdim=True), n=n)
    return _back(y, x), torch.cat([mean, rstd], 1), parts


def backward(g, x, gamma, beta, eps=1e-5, act=None):
    """(gx shaped like x, dgamma [C], dbeta [C], parts) by the formulas of the definition."""
    _, _, p = forward(x, gamma, beta, eps, act)
    xh, u, n = p['xh'], p['u'], p['n']
    d = torch.where(u > 0, torch.ones_like(u), torch.full_like(u, SLOPE)) if act == 'leaky_relu' else torch.ones_like(u)
    gu = _channels(g) * d
    dbeta, dgamma = gu.sum(1, keepdim=True), (gu * xh).sum(1, keepdim=True)
    gx = _col(gamma) * p['rstd'] * (gu - dbeta / n - xh * dgamma / n)
    t = gu * _col(gamma)
    p.update(d=d, gu=gu, t=t, m1=t.mean(1, keepdim=True), m2=(t * xh).mean(1, keepdim=True), gx=gx)
    return _back(gx, x), dgamma.reshape(-1), dbeta.reshape(-1), p


def q_of(p):
    return _lib.gn_q(p['n'], p['mabs'], p['rstd'])


def u_bound(gamma, p):
    """E_u per value, [C, n]."""
    return _lib.gn_u_bound(p['n'], q_of(p), p['xh'].abs(), _col(gamma).abs(), p['u'].abs())


def branch_margin(gamma, p):
    """min over the values of |u| / E_u: above 1 the LeakyReLU branch of every value is determined (include/vqhip.h, LEAKY RELU).
    Channels with gamma == beta == 0 have u == 0 exactly in the kernel and in the definition (the slope branch) and are left out."""
    e = u_bound(gamma, p)
    live = (e > 0).expand_as(p['u']) & (p['u'] != 0)
    return float((p['u'].abs() / e.clamp_min(1e-300))[live].min()) if live.any() else float('inf')


def forward_bound(x, gamma, p, act):
    """E_y per element shaped like x: E_u, plus 2 u0 |y| behind the LeakyReLU."""
    e = u_bound(gamma, p)
    if act == 'leaky_relu':
        e = e + 2.0 * _lib.GN_U * p['y'].abs()
    return _back(e, x)


def mean_bound(p):
    """[C, 1]: N u0 mabs (stats and the block)."""
    return _lib.gn_chain(p['n']) * _lib.GN_U * p['mabs'] + 1e-45


def rstd_bound(p):
    return _lib.gn_rho(p['n'], q_of(p)) * p['rstd']


def unbiased_bound(p, eps):
    """[C, 1]: 2 rho (var + eps) n / (n - 1)."""
    n = p['n']
    return 2.0 * _lib.gn_rho(n, q_of(p)) * (p['var'] + eps) * n / (n - 1)


def backward_bounds(g, x, gamma, p):
    """(E_gx shaped like x, E_dgamma [C], E_dbeta [C]) where every branch is determined (E_d = 0)."""
    n = p['n']
    q, gam = q_of(p), _col(gamma).abs()
    xh = p['xh'].abs()
    e_xh = _lib.gn_xhat_bound(n, q, xh)
    t, gu = p['t'].abs(), p['gu'].abs()
    e_t = 2.0 * _lib.GN_U * t                                                   # E_d = 0
    mean = lambda v: v.mean(1, keepdim=True)
    e_gx = _lib.gn_gx_bound(n, q, p['rstd'], xh, e_t, t, p['m1'].abs(), p['m2'].abs(), mean(t), mean(t * xh), mean(e_t),
                            mean(e_t * xh + t * e_xh), p['gx'].abs())
    e_gu = _lib.GN_U * gu
    N = _lib.gn_chain(n)
    e_dg = (N + 2.0) * _lib.GN_U * (gu * xh).sum(1) + (e_gu * xh + gu * e_xh).sum(1)
    e_db = N * _lib.GN_U * gu.sum(1) + e_gu.sum(1)
    return _back(e_gx, x), e_dg, e_db
