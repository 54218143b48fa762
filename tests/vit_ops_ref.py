"""Float64 restatement of the row ops of include/vqhip.h (add + LayerNorm, bias + GELU / tanh), forward and analytic gradients, and
the error bounds of their ERROR BOUND paragraph evaluated on the restatement's own quantities, for the CPU and GPU tests.  Plain
torch apart from the bound formulas, which are the ones vector_quantization_amd._lib exposes.  A row of D is a group of n = D of
the group norm, so the norm's bounds are tests/group_norm_ref.py's on the [R, D, 1] view with one group."""
import math

import torch

from vector_quantization_amd import _lib

import group_norm_ref as gn

ACTS = {'gelu': _lib.ROW_ACT_GELU, 'tanh': _lib.ROW_ACT_TANH}


def rounded_sum(x, res):
    """s = round_to_x_dtype(x + res): what torch's ``x + branch`` leaves behind (the fp32 sum is exact in float64)."""
    return x if res is None else (x.double() + res.double()).to(x.dtype)


def ln_forward(s, gamma, beta, eps=1e-6):
    """(y, stats [R, 2], parts) of the norm of the rows s [R, D], in float64."""
    y, stats, parts = gn.forward(s.unsqueeze(2), 1, gamma, beta, eps, None)
    return y.squeeze(2), stats.squeeze(1), parts


def ln_backward(g, s, gamma, beta, eps=1e-6, g_skip=None):
    """(gx, dgamma, dbeta, parts): gx includes g_skip; parts['gx_norm'] is the norm's own term."""
    gx, dg, db, p = gn.backward(g.unsqueeze(2), s.unsqueeze(2), 1, gamma, beta, eps, None)
    gx = gx.squeeze(2)
    p['gx_norm'] = gx
    return (gx if g_skip is None else gx + g_skip.double()), dg, db, p


def ln_forward_bound(s, gamma, beta, eps, y, parts):
    return gn.forward_bound(s.unsqueeze(2), 1, gamma, beta, eps, None, y.unsqueeze(2), parts).squeeze(2)


def ln_slabs(R):
    return -(-R // _lib.LN_SLAB)


def ln_backward_bounds(g, s, gamma, beta, eps, gx, p, g_skip=None):
    """(E_gx' per element, E_dgamma [D], E_dbeta [D])."""
    e_gx, e_dg, e_db = gn.backward_bounds(g.unsqueeze(2), s.unsqueeze(2), 1, gamma, beta, eps, None, p['gx_norm'].unsqueeze(2), p,
                                          ln_slabs(s.shape[0]))
    e_gx = e_gx.squeeze(2)
    return (e_gx if g_skip is None else _lib.ln_gx_bound(e_gx, gx.abs())), e_dg, e_db


def act_forward(x, bias, act):
    """(y, parts) of y = act(x + bias) in float64."""
    t = x.double() + bias.double()
    if act == 'gelu':
        h = 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0)))
        y, d = t * h, h + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
    else:
        y = torch.tanh(t)
        d = 1.0 - y * y
    return y, dict(t=t, d=d)


def act_backward(g, x, bias, act):
    """(gx, dbias, parts)."""
    y, p = act_forward(x, bias, act)
    gx = g.double() * p['d']
    p['y'] = y
    return gx, gx.sum(0), p


def act_forward_bound(act, y, p):
    return _lib.row_act_bound(ACTS[act], p['t'].abs(), y.abs())


def act_slabs(R):
    return -(-R // _lib.ROW_ACT_SLAB)


def act_backward_bounds(act, g, gx, p):
    """(E_gx per element, E_dbias [D])."""
    e_gx = _lib.row_act_gx_bound(ACTS[act], g.double().abs(), p['y'].abs(), p['d'].abs(), gx.abs())
    return e_gx, _lib.gn_param_bound(act_slabs(g.shape[0]), 0.0, gx.abs().sum(0), e_gx.sum(0))
