"""ctypes binding of libvqhip.so (C ABI in include/vqhip.h).

The library is built in-tree by ``vector_quantization_amd/csrc/build.sh`` (hipcc, gfx950).  There is no
CPU or PyTorch fallback: if the shared object is missing or a call fails, an exception is raised.

The prototypes are not written down here: ``SIGNATURES`` is read from include/vqhip.h at import (``parse_header``), so a new
entry point is its declaration in the header and its caller.  What a regex cannot derive stays a copy in this file - the five
``Structure`` layouts, the numeric constants and the ``VQHIP_*_BOUND`` family as Python functions - and every such copy is
held to the header by tests/test_binding_header_cpu.py, which compiles a C probe against it.  ``ABI_VERSION`` is
hand-written on purpose.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VQHIP_LIB') or os.path.join(_HERE, 'libvqhip.so')   # VQHIP_LIB: experiment builds

ABI_VERSION = 600          # VQHIP_VERSION of include/vqhip.h this binding was written against
METRIC_L2, METRIC_COS, METRIC_COS_BF16 = 0, 1, 5
DTYPE_F32, DTYPE_BF16 = 0, 1
DTYPE_F16 = 4                              # sampler, token CE and the activation ops; not the quantizer core or FSQ (2, 3: below)
DTYPE_I32, DTYPE_I64 = 2, 3                # token dtypes of vqhip_fsq_decode
DTYPE_U8 = 5                               # images of vqhip_image_metrics only
IMAGE_NCHW, IMAGE_NHWC = 0, 1              # layouts of vqhip_image_metrics
IMAGE_METRICS_TILE = 32                    # VQHIP_IMAGE_METRICS_TILE: pixels per side of a workgroup's tile
IMAGE_SSIM_MAX_WINDOWS = 1 << 22           # VQHIP_IMAGE_SSIM_MAX_WINDOWS
IMAGE_SSIM_BOUND = 2.0 ** -40              # VQHIP_IMAGE_SSIM_BOUND: |kernel ssim - float64 ssim| (derivation in include/vqhip.h)
LAYOUT_ROWS, LAYOUT_MAP = 0, 1             # [N, C] token-major / NCHW-contiguous map [B, C, H*W]
FSQ_MAX_C = 16

_vp, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
_f64 = ctypes.c_double


class CvqForwardArgs(ctypes.Structure):
    """vqhip_cvq_forward_t of include/vqhip.h, field for field."""
    _fields_ = [('struct_bytes', _i64), ('N', _i64), ('K', _i64),
                ('D', _i32), ('x_dtype', _i32), ('metric', _i32), ('world', _i32),
                ('ema_decay', _f32), ('eps', _f32), ('beta', _f32),
                ('phases', _i32), ('exchange', _i32), ('list_ready', _i32), ('prefetch', _i32), ('anchor_sync', _i32), ('rank', _i32),
                ('cap', _i64),
                ('x', _vp), ('w_in', _vp), ('p_in', _vp), ('w_out', _vp), ('p_out', _vp),
                ('rows', _vp), ('slot', _vp), ('count', _vp), ('count_host', _vp), ('count_event', _vp), ('comm', _vp),
                ('cb', _vp), ('cb_bytes', _i64), ('idx', _vp), ('hist', _vp), ('xq', _vp),
                ('packed', _vp), ('packed_floats', _i64),
                ('z_ste', _vp), ('mse', _vp), ('scratch16', _vp),
                ('ws', _vp), ('ws_bytes', _i64),
                ('cap_used', _i64), ('exchange_floats', _i64),
                ('early_word_host', _vp), ('early_seq_dev', _vp), ('keys', _vp)]


class VqkdForwardArgs(ctypes.Structure):
    """vqhip_vqkd_forward_t of include/vqhip.h, field for field."""
    _fields_ = [('struct_bytes', _i64), ('N', _i64), ('K', _i64),
                ('D', _i32), ('x_dtype', _i32), ('metric', _i32), ('world', _i32),
                ('ema_decay', _f32),
                ('phases', _i32), ('exchange', _i32), ('ordered', _i32), ('tail', _i32), ('reserved0', _i32),
                ('x', _vp), ('w_in', _vp), ('w_mid', _vp), ('w_out', _vp), ('xn', _vp), ('xq', _vp), ('comm', _vp),
                ('cb', _vp), ('cb_bytes', _i64), ('idx', _vp), ('hist', _vp),
                ('packed', _vp), ('packed_floats', _i64),
                ('z_ste', _vp), ('mse', _vp), ('scratch16', _vp),
                ('ws', _vp), ('ws_bytes', _i64),
                ('exchange_floats', _i64)]


class VqForwardArgs(ctypes.Structure):
    """vqhip_vq_forward_t of include/vqhip.h, field for field."""
    _fields_ = [('struct_bytes', _i64), ('N', _i64), ('K', _i64),
                ('D', _i32), ('x_dtype', _i32), ('metric', _i32), ('normalize', _i32),
                ('beta', _f32), ('reserved0', _i32),
                ('x', _vp), ('w_in', _vp), ('w_out', _vp), ('xn', _vp),
                ('cb', _vp), ('cb_bytes', _i64), ('idx', _vp), ('hist', _vp), ('xq', _vp),
                ('z_ste', _vp), ('mse', _vp), ('scratch16', _vp),
                ('ws', _vp), ('ws_bytes', _i64)]


class FsqConstants(ctypes.Structure):
    """vqhip_fsq_t of include/vqhip.h, field for field."""
    _fields_ = [('struct_bytes', _i64), ('C', _i32), ('levels', _i32 * FSQ_MAX_C),
                ('shift', _f32 * FSQ_MAX_C), ('scale', _f32 * FSQ_MAX_C)]


class SampleCut(ctypes.Structure):
    """vqhip_sample_cut_t of include/vqhip.h, field for field (24 bytes per output row)."""
    _fields_ = [('kept', ctypes.c_int32), ('topk_kept', ctypes.c_int32), ('cut_value', _f32), ('cut_index', ctypes.c_int32),
                ('max', _f32), ('z', _f32)]


def sample_delta(V: int) -> float:
    """VQHIP_SAMPLE_DELTA(V) of include/vqhip.h: the bound on |kernel share - exact share| of vqhip_sample_tokens."""
    return 2.0 ** -18 + V * 2.0 ** -39


COL_MULTINOMIAL_MAX_N = 1 << 20            # VQHIP_COL_MULTINOMIAL_MAX_N: rows of vqhip_col_multinomial_* (keeps a column's mass below 2^61)


def token_ce_chain(n: int) -> float:
    """VQHIP_TOKEN_CE_CHAIN of include/vqhip.h: the longest chain of fp32 additions over n elements (a row) or n rows."""
    return float(n // 256 + 20)


def token_ce_lse_bound(V: int, amax: float) -> float:
    """VQHIP_TOKEN_CE_LSE_BOUND(V, amax) of include/vqhip.h: |kernel lse - exact lse| of vqhip_token_ce_fwd."""
    return (5.0 * amax + 44.0 + 4.0 * token_ce_chain(V)) * 2.0 ** -24 * (1.0 + 2.0 ** -9)


def token_ce_bound(V: int, amax: float) -> float:
    """VQHIP_TOKEN_CE_BOUND(V, amax): the bound that holds for lse and for the per-row loss, any label smoothing."""
    return token_ce_lse_bound(V, amax) + ((token_ce_chain(V) + 11.0) * amax + 70.0) * 2.0 ** -24


def token_ce_grad_bound(V: int, amax: float) -> float:
    """VQHIP_TOKEN_CE_GRAD_BOUND(V, amax): a gradient element in fp32, before the rounding to the output dtype, per unit |c_r|."""
    return token_ce_lse_bound(V, amax) + (2.0 * amax + 22.0) * 2.0 ** -24


COSINE_EMBED_MAX_C = 1 << 16               # VQHIP_COSINE_EMBED_MAX_C


def cosine_embed_chain(C: int) -> float:
    """VQHIP_COSINE_EMBED_CHAIN(C) of include/vqhip.h: the longest chain of fp32 additions of a row's sums, either layout."""
    return float(C // 32 + 16)


def cosine_embed_bound(C: int) -> float:
    """VQHIP_COSINE_EMBED_BOUND(C): |kernel - exact| of a row's cos and loss of vqhip_cosine_embed_fwd, absolute."""
    return (2.0 * cosine_embed_chain(C) + 6.0) * 2.0 ** -24 * (1.0 + 2.0 ** -9)


def cosine_embed_grad_bound(C: int, h: float) -> float:
    """VQHIP_COSINE_EMBED_GRAD_BOUND(C, h): a gradient element in fp32, before the rounding to the output dtype, per unit |c_r|;
    h = 1 / sqrt(|p|^2 + 1e-12)."""
    return (4.0 * cosine_embed_chain(C) + 21.0) * 2.0 ** -24 * (1.0 + 2.0 ** -9) * h


LPIPS_MAX_C = 1 << 16                      # VQHIP_LPIPS_MAX_C
LPIPS_EPS = 1e-10                          # VQHIP_LPIPS_EPS, as the fp32 constant the kernels and ATen's normalize compare against


def lpips_chain(C: int) -> float:
    """VQHIP_LPIPS_CHAIN(C) of include/vqhip.h: the longest chain of fp32 additions of a pixel's sums over channels, either layout."""
    return float(C // 4 + 12)


def lpips_bound(C: int, wabs: float) -> float:
    """VQHIP_LPIPS_BOUND(C, wabs): |kernel - exact| of a pixel's s and of one layer's share of an image's value of vqhip_lpips_fwd,
    absolute; wabs = max |w|.  With dropout, times 1 / (1 - p)."""
    return (8.0 * lpips_chain(C) + 56.0) * 2.0 ** -24 * (1.0 + 2.0 ** -9) * wabs


def lpips_grad_bound(C: int, wabs: float, h: float) -> float:
    """VQHIP_LPIPS_GRAD_BOUND(C, wabs, h): a gradient element in fp32, before the rounding to the output dtype, per unit of
    |g_out[b]| / P (and of 1 / (1 - p)); h = 1 / max(|f|, 1e-10)."""
    return (16.0 * lpips_chain(C) + 136.0) * 2.0 ** -24 * (1.0 + 2.0 ** -9) * wabs * h


SG2_MAX_C = 1 << 16                        # VQHIP_SG2_MAX_C
SG2_SLOPE, SG2_SCALE = 0.2, 2.0 ** 0.5     # VQHIP_SG2_SLOPE, VQHIP_SG2_SCALE: the definition's constants (the kernels hold their fp32 roundings)
SG2_U = 2.0 ** -24 * (1.0 + 2.0 ** -9)     # VQHIP_SG2_U


def bias_act_bound(y: float) -> float:
    """VQHIP_BIAS_ACT_BOUND(y) of include/vqhip.h: |kernel - exact| of an output (or a gx) of magnitude y, in fp32 before the store."""
    return 4.0 * SG2_U * y


def fir4_bound(a: float, fused: bool = False) -> float:
    """VQHIP_FIR4_BOUND(a), or VQHIP_FIR4_ACT_BOUND(a) for the fused forms: a blur (or adjoint) output whose sources' magnitudes blur to a."""
    return (12.0 if fused else 8.0) * SG2_U * a


def sg2_gbias_chain(slabs: int) -> float:
    """VQHIP_SG2_GBIAS_CHAIN(slabs): the additions one term of gbias passes through, both launches."""
    return float(slabs // 16 + 80)


def sg2_gbias_bound(slabs: int, e: float, sumabs: float) -> float:
    """VQHIP_SG2_GBIAS_BOUND(slabs, e, sumabs): a gbias element; e = 4 (bias-activation) or 12 (fused blur backward)."""
    return (sg2_gbias_chain(slabs) + e) * SG2_U * sumabs


def sg2_store_u(dtype: int) -> float:
    """VQHIP_SG2_STORE_U(dtype): half an ulp of the output dtype, relative (fp16 adds 2^-25 absolute)."""
    return {DTYPE_BF16: 2.0 ** -8, DTYPE_F16: 2.0 ** -11}.get(dtype, 0.0)


GN_U = SG2_U                               # VQHIP_GN_U
GN_SMALL, GN_CHUNK = 2048, 8192            # a wave per group up to GN_SMALL values; beyond GN_CHUNK a group is split over workgroups
GN_BATCH = -2                              # VQHIP_GN_BATCH: the G of batch statistics (one group per channel over all images)
GN_ACT_LEAKY, GN_LEAKY_SLOPE = 2, 0.2      # VQHIP_GN_ACT_LEAKY, VQHIP_GN_LEAKY_SLOPE (the kernels hold the slope's fp32 rounding)


def gn_chain(n: int) -> float:
    """VQHIP_GN_CHAIN(n) of include/vqhip.h: the roundings a value passes on the way into a sum over a group of n."""
    return float(n // 2097152 + 56)


def gn_q(n: int, mabs, rstd):
    """VQHIP_GN_Q(n, mabs, rstd): the error of the group's mean in units of the deviation; mabs = the group's mean of |x|."""
    return gn_chain(n) * GN_U * mabs * rstd


def gn_rho(n: int, q):
    """VQHIP_GN_RHO(n, q): the relative error of rstd (with the roundings of xh and u reserved)."""
    return (gn_chain(n) / 2.0 + 8.0) * GN_U + 2.0 * q + 2.0 * q * q


def gn_xhat_bound(n: int, q, xh):
    """E_xh of include/vqhip.h for a normalised value of magnitude xh."""
    return xh * gn_rho(n, q) + q


def gn_u_bound(n: int, q, xh, gamma, u):
    """E_u: the affine value u = xh gamma + beta, from the magnitudes of xh, gamma and u."""
    return gamma * gn_xhat_bound(n, q, xh) + 2.0 * GN_U * u


def gn_y_bound(n: int, q, xh, gamma, u, y, act: int):
    """|kernel y - exact y| in fp32, before the store: E_u, or 1.1 E_u + 8 u0 |y| behind the SiLU."""
    e = gn_u_bound(n, q, xh, gamma, u)
    return 1.1 * e + 8.0 * GN_U * y if act else e


def gn_d_bound(n: int, q, xh, gamma, u, act: int):
    """E_d: the derivative of the activation, 0 without one."""
    return 0.5 * gn_u_bound(n, q, xh, gamma, u) + 10.0 * GN_U if act else 0.0 * xh


def gn_gx_bound(n: int, q, rstd, xh, e_t, t, m1, m2, mean_t, mean_txh, mean_e_t, mean_e_txh, gx):
    """E_gx of include/vqhip.h.  e_t = g gamma E_d + 2 u0 t per value; mean_* are the group's means of t, t xh, e_t and of
    e_t xh + t E_xh; m1, m2 the magnitudes of the two group means of the definition."""
    N = gn_chain(n)
    e1 = N * GN_U * mean_t + mean_e_t
    e2 = (N + 1.0) * GN_U * mean_txh + mean_e_txh
    return rstd * (e_t + e1 + xh * e2 + m2 * gn_xhat_bound(n, q, xh) + 4.0 * GN_U * (t + m1 + xh * m2)) + gn_rho(n, q) * gx


def gn_param_bound(slabs: int, extra: float, sumabs, sum_err):
    """dgamma (extra = 2) or dbeta (extra = 0): (M + extra) u0 sum|terms| + the sum of the terms' own errors."""
    return (sg2_gbias_chain(slabs) + extra) * GN_U * sumabs + sum_err


VIT_MAX_D = 8192                           # VQHIP_VIT_MAX_D: the widest row of vqhip_add_layer_norm_* / vqhip_row_bias_act_*
VIT_MAX_R = 1 << 24                        # VQHIP_VIT_MAX_R: their most rows (no launch of more than 2^32 threads)
ROW_ACT_GRID_PIECES = 8192 * 256           # 16-byte pieces the row bias-activation forward covers with a thread each; beyond: grid-stride
LN_SLAB, ROW_ACT_SLAB = 16, 256            # rows per workgroup of the two backwards (the slabs of their column sums)
ROW_ACT_GELU, ROW_ACT_TANH = 0, 1          # VQHIP_ROW_ACT_*
ROW_ACT_SWIGLU = 3                         # VQHIP_ROW_ACT_SWIGLU: x = (gate | up) [R, 2 D]; 2 is not an activation
SWIGLU_CLAMP = 88.0                        # the exponential of the SwiGLU mode sees max(-|a|, -88)
# VQHIP_VIT_*_ULPS: twice the measured accuracy of the device erff / tanhf / expf (include/vqhip.h; profiles/vqkd_autoencoder.txt)
VIT_ERF_ULPS, VIT_TANH_ULPS, VIT_EXP_ULPS = 3.02, 2.82, 1.79
VIT_TINY = 2.0 ** -148                     # VQHIP_VIT_TINY


def ln_gx_bound(e_gx, gx_total):
    """E_gx' of include/vqhip.h: the group norm's E_gx (n = D, act 0) and the one rounding of the addition of g_skip."""
    return e_gx + GN_U * gx_total


def row_act_bound(act: int, t, y):
    """VQHIP_ROW_GELU_BOUND(t, y) / VQHIP_ROW_TANH_BOUND(y): |kernel y - exact y| in fp32, before the store; magnitudes."""
    if act == ROW_ACT_GELU:
        return ((3.0 + VIT_ERF_ULPS) * t + 2.0 * y) * GN_U + VIT_TINY
    return (1.0 + 2.0 * VIT_TANH_ULPS) * GN_U * y + VIT_TINY


def row_act_grad_bound(act: int, y, d):
    """VQHIP_ROW_GELU_GRAD_BOUND / VQHIP_ROW_TANH_GRAD_BOUND(y, d): the derivative d of the activation, absolute."""
    if act == ROW_ACT_GELU:
        return (5.0 + VIT_ERF_ULPS + VIT_EXP_ULPS / 2.0) * GN_U + 0.0 * d
    return ((3.0 + 4.0 * VIT_TANH_ULPS) * y * y + d) * GN_U


def row_act_gx_bound(act: int, g, y, d, gx):
    """gx = g d: |g| E_d + u0 |gx|."""
    return g * row_act_grad_bound(act, y, d) + GN_U * gx


def rms_y_bound(D: int, xh, gamma, y):
    """E_y of the RMS mode of include/vqhip.h: the group norm's E_u at q = 0 (no mean) and beta = 0."""
    return gn_u_bound(D, 0.0, xh, gamma, y)


def rms_gx_bound(D: int, rstd, xh, t, m2, mean_txh, mean_e_txh, gx):
    """E_gx of the RMS mode: the group norm's at q = 0 with every m1 term absent; E_t = 2 u0 |t|; mean_e_txh = the row's mean of
    E_t |xh| + |t| E_xh."""
    return gn_gx_bound(D, 0.0, rstd, xh, 2.0 * GN_U * t, t, 0.0, m2, 0.0, mean_txh, 0.0, mean_e_txh, gx)


def swiglu_floor(a, f):
    """The absolute terms of the SwiGLU bounds for a gate of magnitude a and a factor of magnitude f (up, g up or g): the
    subnormal results, and the exponential's argument held at -88."""
    held = 2.0 ** -126 * (1.0 + a) * f
    return VIT_TINY * (1.0 + (1.0 + a) * f) + held * (a > SWIGLU_CLAMP)


def swiglu_silu_bound(s):
    """E_s of include/vqhip.h: silu(a) of magnitude s, relative part."""
    return (3.0 * VIT_EXP_ULPS + 3.0) * GN_U * s


def swiglu_bound(a, up, y):
    """E_y of the SwiGLU mode: |kernel y - exact y| in fp32, before the store; magnitudes."""
    return (3.0 * VIT_EXP_ULPS + 4.0) * GN_U * y + swiglu_floor(a, up)


def swiglu_grad_bound(a, sg, d):
    """E_d: the factor d = sg (1 + a (1 - sg)) of the gate's gradient, absolute; magnitudes, sg = sigmoid of the signed gate."""
    return ((3.0 * VIT_EXP_ULPS + 3.0) * a * sg * (1.0 - sg) + (3.0 * VIT_EXP_ULPS + 4.0) * d) * GN_U


def swiglu_gx_bounds(a, sg, d, s, g, up, gx_gate, gx_up):
    """(E of gx[:, :F], E of gx[:, F:]) of the SwiGLU backward."""
    gu = g * up
    return (gu * swiglu_grad_bound(a, sg, d) + 2.0 * GN_U * gx_gate + swiglu_floor(a, gu),
            g * swiglu_silu_bound(s) + GN_U * gx_up + swiglu_floor(a, g))


ATTN_MAX_HEAD_DIM, ATTN_MAX_GROUP, ATTN_MAX_LEN = 128, 8, 4096      # VQHIP_ATTN_MAX_*: vqhip_decode_attention / vqhip_rope_append

STEP_BEFORE_EXCHANGE, STEP_AFTER_EXCHANGE, STEP_ALL, STEP_PACK_SYNC = 1, 2, 3, 4


class VqhipError(RuntimeError):
    pass


HEADER_PATH = os.path.join(_HERE, os.pardir, 'include', 'vqhip.h')
# the header's typedef names -> their ctypes layouts above (the only structs a prototype may point to)
STRUCTS = {'vqhip_cvq_forward_t': CvqForwardArgs, 'vqhip_vqkd_forward_t': VqkdForwardArgs, 'vqhip_vq_forward_t': VqForwardArgs,
           'vqhip_fsq_t': FsqConstants, 'vqhip_sample_cut_t': SampleCut}
_DEVICE_STRUCTS = {'vqhip_sample_cut_t'}   # an array the kernel writes on the DEVICE: callers pass its address, as for any buffer
_SCALARS = {'int': _i32, 'int32_t': _i32, 'int64_t': _i64, 'float': _f32, 'double': _f64}


def _ctype(c_type: str, fn: str):
    """The ctypes type of one parameter or return type of a prototype: the scalars above, ``const char *``, a pointer to one
    of STRUCTS, any other pointer as c_void_p.  Anything else is refused by name: at import, not at a launch."""
    t = re.sub(r'\bconst\b|\s+', '', c_type)
    if t in _SCALARS:
        return _SCALARS[t]
    if t == 'char*':
        return ctypes.c_char_p
    if t.endswith('*') and t[:-1] in STRUCTS:
        return _vp if t[:-1] in _DEVICE_STRUCTS else ctypes.POINTER(STRUCTS[t[:-1]])
    if t.endswith('*') and not re.fullmatch(r'vqhip_\w+_t\*', t):
        return _vp
    raise VqhipError(f'include/vqhip.h: {fn}: no ctypes rule for the type "{" ".join(c_type.split())}"')


def parse_header(text: str) -> dict:
    """name -> (restype, [argtypes]) of every ``ret vqhip_name(params);`` in the text of a C header."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text.replace('\\\n', ' '), flags=re.S)
    text = re.sub(r'(?m)^[ \t]*#.*$', '', text)
    out = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w\s*]*?)\b(vqhip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text):
        params = [] if params.strip() == 'void' else [p.strip() for p in params.split(',')]
        # a parameter is its type and then its name
        out[name] = (_ctype(ret, name), [_ctype(re.sub(r'(?<=[\s*])\w+$', '', p), name) for p in params])
    unread = set(re.findall(r'\b(vqhip_[a-z0-9_]+)\s*\(', text)) - set(out)
    if unread:
        raise VqhipError(f'include/vqhip.h: not read as prototypes: {sorted(unread)}')
    return out


# name -> (restype, [argtypes]): derived from the prototypes of include/vqhip.h, which is the only place they are written
with open(HEADER_PATH) as _f:
    SIGNATURES = parse_header(_f.read())

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libvqhip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    script = os.path.join(_HERE, 'csrc', 'build.sh')
    res = subprocess.run(['bash', script], capture_output=True, text=True)
    if res.returncode != 0:
        raise VqhipError(f'hipcc build of libvqhip.so failed:\n{res.stdout}\n{res.stderr}')
    if verbose:
        print(res.stdout.strip())
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Load libvqhip.so and declare every entry point of include/vqhip.h; raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VqhipError(
                f'{LIB_PATH} not found: build it with vector_quantization_amd/csrc/build.sh '
                '(or __graft_entry__.build()); there is no fallback path')
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)            # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.vqhip_version() != ABI_VERSION:
            raise VqhipError(f'{LIB_PATH} has ABI version {L.vqhip_version()}, this package binds {ABI_VERSION}: '
                             'rebuild it with vector_quantization_amd/csrc/build.sh')
        # VQHIP_TUNING="18=0,2=4": A/B knobs of vqhip_set_tuning applied at load (measurement and debugging; results never change)
        for kv in filter(None, os.environ.get('VQHIP_TUNING', '').split(',')):
            key, _, value = kv.partition('=')
            if L.vqhip_set_tuning(int(key), int(value)) != 0:
                raise VqhipError(f'VQHIP_TUNING: vqhip_set_tuning({key}, {value}) refused')
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().vqhip_last_error()
        raise VqhipError(f'{what} failed with code {rc}: {msg.decode() if msg else ""}')
