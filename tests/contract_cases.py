"""The table behind tests/test_op_contract_table_cpu.py and tests/test_gpu_op_contracts.py: one entry per (op family, direction,
dtype, launch shape) of the fused ops, with what the placement, side-stream and capture properties need to run it.

An entry (``Case``) gives
  abi       the entry points of include/vqhip.h it reaches;
  clause    words of the header it relies on, quoted (the CPU test holds the quotation to the header);
  make      seed -> dict of the tensor arguments on the GPU (the same shapes, dtypes and strides for every seed);
  call      that dict -> tuple of result tensors, through ``ops.*``.  A backward entry runs its forward first, so a capture of
            ``call`` holds both;
  free      the names of ``make`` the header frees from 16-byte alignment: the placement test rebuilds those at element offsets
            1 and 3 past a 16-byte boundary - the activations, the fp32 parameter vectors (as slices of a flat parameter would
            lie) and the small vectors (uniforms, targets, seeds, incoming gradients); what a backward takes over from its
            forward (lse, the weight sum, stats) goes through ``saved`` and is placed with them;
  outs      (with ``call_abi``) that dict -> [(shape, strides, dtype)] of the results of ``call``, in order;
  call_abi  (args, outs) -> None: the same launch through ``_lib.lib()`` with the outputs where the test put them.  For a
            backward entry only the backward's outputs are placed; its forward runs through ``ops``.

Entries without ``free`` belong to families whose pointers the header keeps at 16 bytes (LIMITS, ``alignment``): the host layer
copies (``ops._latents`` / ``ops._codebook``) or allocates them itself, and they take part in the stream and capture
properties only.

Shapes are the smallest of each family's own GPU test or *_ref.py per launch shape (cosine embedding, LPIPS and image metrics:
named where they are set; GroupNorm: a wave, a workgroup, a split group; the ViT
rows: (5, 24), (3, 2051), (3, 2052), (2, 8192); bias-act / FIR: C = 130 and C = 3; sampler and token CE: a vocabulary with a ragged
tail inside a longer row).  Nothing here is larger than the largest of those.

``EXEMPT`` names every other entry point with a ``stream`` parameter, with the reason it is not in the table.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from vector_quantization_amd import _lib, ops

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
NAME = {F32: 'f32', BF16: 'bf16', F16: 'f16', torch.int32: 'i32', torch.int64: 'i64', torch.uint8: 'u8'}
CODE = ops.FLOAT_DTYPES

# the header's words each family relies on (one line of include/vqhip.h each)
CLAUSE = {
    'sampler': 'The pointer and the slice start need only element alignment',
    'token_ce': 'element alignment only; columns [start, end) are read, V = end - start.',
    'token_ce_bits': 'not of the address or alignment of a row',
    'cosine': 'two may differ; element alignment only.',
    'cosine_bits': 'address or alignment of a row (a strided view and its copy give the same bits)',
    'lpips': 'Each in its own dtype, VQHIP_DTYPE_F32, _BF16 or _F16; element alignment',
    'sg2': 'VQHIP_DTYPE_F32, _BF16 or _F16, element alignment only; outputs in the same dtype and layout.',
    'group_norm': 'element alignment only; y and gx in the same dtype and layout.',
    'vit': 'Rows [R, D], dense (row stride D), element alignment only.',
    'image_metrics': 'channels-last dense); element alignment only.',
    'pool': '16-byte loads where D % 4 == 0 and e, out are 16-byte aligned, channel by channel otherwise',
    'small': 'the small vectors are read and written element by element',
    'outputs': 'an output tensor needs the alignment of its element type as an input does',
    'limits': 'every buffer pointer 16-byte aligned (hipMalloc / torch allocations are); rows dense, no padding',
    'entropy': 'All sums run in a fixed order (no atomics).',
}


@dataclass
class Case:
    id: str
    family: str
    abi: tuple
    clause: str
    make: Callable
    call: Callable
    free: tuple = ()
    outs: Optional[Callable] = None
    call_abi: Optional[Callable] = None


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


S = ops._stream


def like(t):
    return tuple(t.shape), tuple(t.stride()), t.dtype


def flat(shape, dtype):
    return tuple(shape), tuple(torch.empty(shape, device='meta').stride()), dtype


def _gen(seed):
    return torch.Generator().manual_seed(1000 + seed)


def _randn(gen, shape, dtype=F32, nhwc=False, scale=1.0):
    t = (scale * torch.randn(shape, generator=gen)).to(dtype).cuda()
    return t.contiguous(memory_format=torch.channels_last) if nhwc else t


def _lay(nhwc):
    return 'nhwc' if nhwc else 'nchw'


def _layout_code(t):
    return ops.LAYOUTS[ops.dense_layout(t)]


CASES: list = []

# element offset at which a backward entry hands the forward's saved vectors (lse, stats) on; the placement test sets it
INTERMEDIATE_OFFSET = 0


def saved(t):
    """``t`` itself, or (``INTERMEDIATE_OFFSET`` != 0) a device copy of it that many elements past a 16-byte boundary: how a
    backward entry passes on what its forward saved, so that those pointers are placed like the arguments of ``make``."""
    if not INTERMEDIATE_OFFSET:
        return t
    buf = torch.empty(t.numel() + INTERMEDIATE_OFFSET + 16, dtype=t.dtype, device=t.device)
    view = buf[INTERMEDIATE_OFFSET:INTERMEDIATE_OFFSET + t.numel()].view(t.shape)
    assert buf.data_ptr() % 16 == 0 and t.is_contiguous()
    view.copy_(t)
    return view


def add(**kw):
    CASES.append(Case(**kw))


# ---- sampler ---------------------------------------------------------------------------------------------------------------
SAMPLE_VT, SAMPLE_STRIDE, SAMPLE_START, SAMPLE_END, SAMPLE_R = 1037, 1048, 5, 1006, 6      # V = 1001 inside rows of 1048


def _logits(gen, R, dtype):
    """[R, Vt] logits as a view of rows of SAMPLE_STRIDE elements: the row stride is larger than the vocabulary."""
    full = (3.0 * torch.randn(R, SAMPLE_STRIDE, generator=gen)).to(dtype).cuda()
    return full[:, :SAMPLE_VT]


def _sampler(dtype, cfg):
    alpha = 1.5 if cfg else None
    Ro = SAMPLE_R // 2 if cfg else SAMPLE_R
    kw = dict(temperature=0.9, top_k=50, top_p=0.9)

    def make(seed):
        gen = _gen(seed)
        return dict(logits=_logits(gen, SAMPLE_R, dtype), u=torch.rand(Ro, generator=gen).cuda())

    def call(a):
        return ops.sample_tokens(a['logits'], SAMPLE_START, SAMPLE_END, u=a['u'], cfg_alpha=alpha, want_cut=True, **kw)

    def outs(a):
        return [flat((SAMPLE_R,), torch.int64), flat((Ro, 6), torch.int32)]

    def call_abi(a, o):
        lg = a['logits']
        _lib.check(_lib.lib().vqhip_sample_tokens(P(lg), CODE[dtype], SAMPLE_R, lg.stride(0), SAMPLE_START, SAMPLE_END,
                                                  float(alpha) if cfg else 0.0, int(cfg), kw['temperature'], kw['top_k'], kw['top_p'],
                                                  P(a['u']), P(o[0]), P(o[1]), S()), 'vqhip_sample_tokens')

    add(id=f'sample_tokens-{NAME[dtype]}-{"cfg" if cfg else "plain"}', family='sampler', abi=('vqhip_sample_tokens',),
        clause=CLAUSE['sampler'], make=make, call=call, free=('logits', 'u'), outs=outs, call_abi=call_abi)


for _dt in DTYPES:
    for _cfg in (False, True):
        _sampler(_dt, _cfg)


# ---- token cross-entropy -----------------------------------------------------------------------------------------------------
def _token_ce(dtype, tdtype, backward):
    R, kw = 5, dict(label_smoothing=0.1, ignore_index=-100)
    V = SAMPLE_END - SAMPLE_START

    def make(seed):
        gen = _gen(seed)
        t = torch.randint(SAMPLE_START, SAMPLE_END, (R,), generator=gen)
        t[seed % R] = -100
        a = dict(logits=_logits(gen, R, dtype), targets=t.to(tdtype).cuda(), weight=torch.rand(R, generator=gen).cuda() + 0.5)
        if backward:
            a['g'] = torch.randn(1, generator=gen).cuda()
        return a

    def forward(a):
        return ops.token_ce_forward(a['logits'], a['targets'], SAMPLE_START, SAMPLE_END, weight=a['weight'], **kw)

    def head(a):
        lg = a['logits']
        return (P(lg), CODE[dtype], R, lg.stride(0), SAMPLE_START, SAMPLE_END, P(a['targets']), ops.TOKEN_DTYPES[tdtype], 0,
                kw['ignore_index'], kw['label_smoothing'], P(a['weight']))

    if not backward:
        def call(a):
            f = forward(a)
            return f['loss'], f['lse'], f['hit'], f['out']

        def outs(a):
            return [flat((R,), F32), flat((R,), F32), flat((R,), torch.int32), flat((4,), F32)]

        def call_abi(a, o):
            _lib.check(_lib.lib().vqhip_token_ce_fwd(*head(a), P(o[0]), P(o[1]), P(o[2]), P(o[3]), S()), 'vqhip_token_ce_fwd')
        abi = ('vqhip_token_ce_fwd',)
    else:
        def call(a):
            f = forward(a)
            return (ops.token_ce_backward(a['logits'], a['targets'], saved(f['lse']), a['g'], SAMPLE_START, SAMPLE_END, weight=a['weight'],
                                          weight_sum=saved(f['out'][1:2]), **kw),)

        def outs(a):
            return [flat((R, SAMPLE_VT), dtype)]

        def call_abi(a, o):
            f = forward(a)
            _lib.check(_lib.lib().vqhip_token_ce_bwd(*head(a), P(saved(f['lse'])), P(a['g']), 0, P(saved(f['out'][1:2])), P(o[0]), SAMPLE_VT, SAMPLE_VT,
                                                     S()), 'vqhip_token_ce_bwd')
        abi = ('vqhip_token_ce_fwd', 'vqhip_token_ce_bwd')
    assert V == 1001
    add(id=f'token_ce_{"backward" if backward else "forward"}-{NAME[dtype]}-{NAME[tdtype]}', family='token_ce', abi=abi,
        clause=CLAUSE['token_ce_bits' if backward else 'token_ce'], make=make, call=call, free=('logits', 'weight', 'targets', 'g'), outs=outs,
        call_abi=call_abi)


for _dt in DTYPES:
    for _td in (torch.int32, torch.int64):
        _token_ce(_dt, _td, False)
        _token_ce(_dt, _td, True)


# ---- cosine embedding -------------------------------------------------------------------------------------------------------
COSINE_ROWS = ((5, 33), (5, 520))                  # (R, C) of cosine_embed_ref.CS x RS: a ragged tail, whole 16-byte pieces past a wave
COSINE_MAPS = ((3, 7, 49), (2, 33, 65))            # (B, C, P) of cosine_embed_ref.MAP_SHAPES: P either side of the 32 positions of a workgroup


def _cosine(shape, pdtype, tdtype, layout, backward):
    B, C, HW = shape if layout == 'map' else (shape[0], shape[1], 1)
    R = B * HW

    def make(seed):
        gen = _gen(seed)
        a = dict(pred=_randn(gen, (B, C, HW) if layout == 'map' else (R, C), pdtype),
                 target=_randn(gen, (B, HW, C) if layout == 'map' else (R, C), tdtype))
        if backward:
            a['g'] = torch.randn(R, generator=gen).cuda()
        return a

    def head(a):
        p, t = a['pred'], a['target'].view(R, C)
        return (P(p), CODE[pdtype], ops.LAYOUTS[layout], C if layout == 'rows' else 0, P(t), CODE[tdtype], C,
                R if layout == 'rows' else B, 1 if layout == 'rows' else HW, C)

    def forward(a):
        return ops.cosine_embedding_forward(a['pred'], a['target'], layout=layout)

    if not backward:
        def call(a):
            f = forward(a)
            return f['loss'], f['stats'], f['out']

        def outs(a):
            return [flat((R,), F32), flat((R, 3), F32), flat((2,), F32)]

        def call_abi(a, o):
            _lib.check(_lib.lib().vqhip_cosine_embed_fwd(*head(a), P(o[0]), P(o[1]), P(o[2]), S()), 'vqhip_cosine_embed_fwd')
        abi = ('vqhip_cosine_embed_fwd',)
    else:
        def call(a):
            f = forward(a)
            return (ops.cosine_embedding_backward(a['pred'], a['target'], saved(f['stats']), a['g'], layout=layout, mean=True),)

        def outs(a):
            return [like(a['pred'])]

        def call_abi(a, o):
            f = forward(a)
            _lib.check(_lib.lib().vqhip_cosine_embed_bwd(*head(a), P(saved(f['stats'])), P(a['g']), 1, 1, P(o[0]), C if layout == 'rows' else 0,
                                                         S()), 'vqhip_cosine_embed_bwd')
        abi = ('vqhip_cosine_embed_fwd', 'vqhip_cosine_embed_bwd')
    add(id=f'cosine_embedding_{"backward" if backward else "forward"}-{layout}-{"x".join(map(str, shape))}-{NAME[pdtype]}-{NAME[tdtype]}', family='cosine',
        abi=abi, clause=CLAUSE['cosine_bits' if backward else 'cosine'], make=make, call=call, free=('pred', 'target', 'g'), outs=outs,
        call_abi=call_abi)


for _lay_name, _shapes in (('rows', COSINE_ROWS), ('map', COSINE_MAPS)):
    for _shape in _shapes:
        for _pd, _td in ((F32, F32), (BF16, F32), (F16, F32), (BF16, BF16), (F16, F16)):
            _cosine(_shape, _pd, _td, _lay_name, False)
            _cosine(_shape, _pd, _td, _lay_name, True)


# ---- LPIPS tail -------------------------------------------------------------------------------------------------------------
LPIPS_P, LPIPS_LAYER = 0.5, 2


LPIPS_CS = (3, 64, 65)                             # lpips_ref.CS: single elements, whole 16-byte pieces per lane, pieces and a tail
LPIPS_BHW = (2, 5, 7)                              # lpips_ref.BPS


def _lpips(C, dtype, nhwc, backward):
    B, H, W = LPIPS_BHW
    Px = H * W

    def make(seed):
        gen = _gen(seed)
        a = dict(pred=_randn(gen, (B, C, H, W), dtype, nhwc), target=_randn(gen, (B, C, H, W), dtype, nhwc),
                 weight=torch.rand(1, C, 1, 1, generator=gen).cuda(),
                 seed=torch.randint(0, 2 ** 31 - 1, (2,), generator=gen).to(torch.int32).cuda())
        if backward:
            a['g'] = torch.randn(B, generator=gen).cuda()
        return a

    def head(a):
        return (P(a['pred']), CODE[dtype], P(a['target']), CODE[dtype], _layout_code(a['pred']), B, C, Px, P(a['weight']), P(a['seed']),
                LPIPS_P, LPIPS_LAYER)

    def forward(a):
        return ops.lpips_layer_forward(a['pred'], a['target'], a['weight'], seed=a['seed'], p=LPIPS_P, layer=LPIPS_LAYER)

    if not backward:
        def call(a):
            f = forward(a)
            return f['stats'], f['value']

        def outs(a):
            return [flat((B, Px, 4), F32), flat((B,), F32)]

        def call_abi(a, o):
            _lib.check(_lib.lib().vqhip_lpips_fwd(*head(a), P(o[0]), P(o[1]), 0, S()), 'vqhip_lpips_fwd')
        abi = ('vqhip_lpips_fwd',)
    else:
        def call(a):
            f = forward(a)
            return (ops.lpips_layer_backward(a['pred'], a['target'], a['weight'], saved(f['stats']), a['g'], seed=a['seed'], p=LPIPS_P,
                                             layer=LPIPS_LAYER),)

        def outs(a):
            return [like(a['pred'])]

        def call_abi(a, o):
            f = forward(a)
            _lib.check(_lib.lib().vqhip_lpips_bwd(*head(a), P(saved(f['stats'])), P(a['g']), P(o[0]), S()), 'vqhip_lpips_bwd')
        abi = ('vqhip_lpips_fwd', 'vqhip_lpips_bwd')
    add(id=f'lpips_layer_{"backward" if backward else "forward"}-C{C}-{_lay(nhwc)}-{NAME[dtype]}', family='lpips', abi=abi,
        clause=CLAUSE['lpips'], make=make, call=call, free=('pred', 'target', 'weight', 'seed', 'g'), outs=outs, call_abi=call_abi)


for _C in LPIPS_CS:
    for _dt in DTYPES:
        for _nhwc in (False, True):
            _lpips(_C, _dt, _nhwc, False)
            _lpips(_C, _dt, _nhwc, True)


def _lpips_mask():
    B, C, Px = 2, 65, 35

    def make(seed):
        return dict(seed=torch.randint(0, 2 ** 31 - 1, (2,), generator=_gen(seed)).to(torch.int32).cuda())

    def call(a):
        return (ops.lpips_keep_mask(a['seed'], LPIPS_P, LPIPS_LAYER, B, C, Px),)

    def call_abi(a, o):
        _lib.check(_lib.lib().vqhip_lpips_keep_mask(P(a['seed']), LPIPS_P, LPIPS_LAYER, B, C, Px, P(o[0]), S()), 'vqhip_lpips_keep_mask')

    add(id='lpips_keep_mask', family='lpips', abi=('vqhip_lpips_keep_mask',), clause=CLAUSE['lpips'], make=make, call=call,
        free=('seed',), outs=lambda a: [flat((B, C, Px), torch.uint8)], call_abi=call_abi)


_lpips_mask()


# ---- StyleGAN2: bias-activation and the FIR blur ------------------------------------------------------------------------------
SG2_SHAPES = ((2, 130, 6, 5), (2, 3, 9, 7))


def _bias_act(shape, dtype, nhwc, backward):
    B, C, H, W = shape

    def make(seed):
        gen = _gen(seed)
        a = dict(x=_randn(gen, shape, dtype, nhwc), bias=torch.randn(C, generator=gen).cuda())
        if backward:
            a['g'] = _randn(gen, shape, dtype, nhwc)
        return a

    if not backward:
        def call(a):
            return (ops.bias_act(a['x'], a['bias']),)

        def outs(a):
            return [like(a['x'])]

        def call_abi(a, o):
            x = a['x']
            _lib.check(_lib.lib().vqhip_bias_act_fwd(P(x), CODE[dtype], _layout_code(x), B, C, H * W, P(a['bias']), P(o[0]), S()),
                       'vqhip_bias_act_fwd')
        abi, free = ('vqhip_bias_act_fwd',), ('x', 'bias')
    else:
        def call(a):
            return ops.bias_act_backward(a['g'], ops.bias_act(a['x'], a['bias']))

        def outs(a):
            return [like(a['x']), flat((C,), F32)]

        def call_abi(a, o):
            y = ops.bias_act(a['x'], a['bias'])
            L, layout = _lib.lib(), _layout_code(y)
            ws = torch.empty(L.vqhip_bias_act_slabs(layout, B, C, H * W) * C, dtype=F32, device='cuda')
            _lib.check(L.vqhip_bias_act_bwd(P(a['g']), P(y), CODE[dtype], layout, B, C, H * W, P(o[0]), P(o[1]), P(ws), ws.numel() * 4, S()),
                       'vqhip_bias_act_bwd')
        abi, free = ('vqhip_bias_act_fwd', 'vqhip_bias_act_bwd'), ('x', 'bias', 'g')
    add(id=f'bias_act{"_backward" if backward else ""}-C{C}-{_lay(nhwc)}-{NAME[dtype]}', family='stylegan2', abi=abi, clause=CLAUSE['sg2'],
        make=make, call=call, free=free, outs=outs, call_abi=call_abi)


def _fir4(shape, dtype, nhwc, down, fused, backward):
    B, C, H, W = shape
    pad = (2, 2, 2, 2) if down == 1 else (1, 1, 1, 1)
    OH, OW = ops.fir4_out_size(H, W, pad, down)

    def make(seed):
        gen = _gen(seed)
        a = dict(x=_randn(gen, shape, dtype, nhwc))
        if fused:
            a['bias'] = torch.randn(C, generator=gen).cuda()
        if backward:
            a['g'] = _randn(gen, (B, C, OH, OW), dtype, nhwc)
        return a

    def out_like(a, size):
        return like(ops._empty_like(a['x'], size))

    if not backward:
        def call(a):
            return (ops.fir4(a['x'], pad, down, a.get('bias')),)

        def outs(a):
            return [out_like(a, (B, C, OH, OW))]

        def call_abi(a, o):
            x = a['x']
            _lib.check(_lib.lib().vqhip_fir4_fwd(P(x), CODE[dtype], _layout_code(x), B, C, H, W, down, *pad, P(a.get('bias')), P(o[0]),
                                                 S()), 'vqhip_fir4_fwd')
        abi = ('vqhip_fir4_fwd',)
        free = ('x', 'bias') if fused else ('x',)
    else:
        # the adjoint alone reads g only, so only g is freed (x serves its layout); the fused form reads the saved input and the
        # bias as well
        def call(a):
            if fused:
                return ops.fir4_backward(a['g'], (H, W), pad, down, a['x'], a['bias'])
            return (ops.fir4_backward(a['g'], (H, W), pad, down),)

        def outs(a):
            return [out_like(a, (B, C, H, W))] + ([flat((C,), F32)] if fused else [])

        def call_abi(a, o):
            L, g = _lib.lib(), a['g']
            layout = _layout_code(a['x'])
            ws = None
            if fused:
                ws = torch.empty(L.vqhip_fir4_slabs(layout, B, C, H, W) * C, dtype=F32, device='cuda')
            _lib.check(L.vqhip_fir4_bwd(P(g), CODE[dtype], layout, B, C, H, W, down, *pad, P(a['x']) if fused else None, P(a.get('bias')),
                                        P(o[0]), P(o[1]) if fused else None, P(ws), 0 if ws is None else ws.numel() * 4, S()),
                       'vqhip_fir4_bwd')
        abi = ('vqhip_fir4_bwd',)
        free = ('g', 'x', 'bias') if fused else ('g',)
    name = ('bias_act_blur' if fused else 'fir4') + ('_backward' if backward else '')
    add(id=f'{name}-down{down}-C{C}-{_lay(nhwc)}-{NAME[dtype]}', family='stylegan2', abi=abi, clause=CLAUSE['sg2'], make=make, call=call,
        free=free, outs=outs, call_abi=call_abi)


for _shape in SG2_SHAPES:
    for _dt in DTYPES:
        for _nhwc in (False, True):
            _bias_act(_shape, _dt, _nhwc, False)
            _bias_act(_shape, _dt, _nhwc, True)
            for _down in (1, 2):
                _fir4(_shape, _dt, _nhwc, _down, False, False)
                _fir4(_shape, _dt, _nhwc, _down, False, True)
            # the fused form, bias-activation on the way into the blur, both directions
            for _down in (1, 2):
                _fir4(_shape, _dt, _nhwc, _down, True, False)
                _fir4(_shape, _dt, _nhwc, _down, True, True)


# ---- GroupNorm (+ SiLU) --------------------------------------------------------------------------------------------------------
GN_SHAPES = ((2, 32, 5, 7), (1, 64, 40, 40), (1, 128, 70, 70))          # a wave per group, a workgroup per group, a split group
GN_G, GN_EPS = 32, 1e-6


def _group_norm(shape, dtype, nhwc, backward):
    B, C = shape[:2]
    Px = shape[2] * shape[3]

    def make(seed):
        gen = _gen(seed)
        a = dict(x=_randn(gen, shape, dtype, nhwc), gamma=torch.randn(C, generator=gen).cuda(), beta=torch.randn(C, generator=gen).cuda())
        if backward:
            a['g'] = _randn(gen, shape, dtype, nhwc)
        return a

    def ws_of(a):
        n = _lib.lib().vqhip_group_norm_ws_bytes(_layout_code(a['x']), B, C, Px, GN_G)
        return torch.empty(max(n // 4, 1), dtype=F32, device='cuda'), n

    if not backward:
        def call(a):
            return ops.group_norm(a['x'], GN_G, a['gamma'], a['beta'], GN_EPS, 'silu')

        def outs(a):
            return [like(a['x']), flat((B, GN_G, 2), F32)]

        def call_abi(a, o):
            x = a['x']
            ws, n = ws_of(a)
            _lib.check(_lib.lib().vqhip_group_norm_fwd(P(x), CODE[dtype], _layout_code(x), B, C, Px, GN_G, P(a['gamma']), P(a['beta']),
                                                       GN_EPS, 1, P(o[0]), P(o[1]), P(ws), n, S()), 'vqhip_group_norm_fwd')
        abi, free = ('vqhip_group_norm_fwd',), ('x', 'gamma', 'beta')
    else:
        def call(a):
            _, stats = ops.group_norm(a['x'], GN_G, a['gamma'], a['beta'], GN_EPS, 'silu')
            return ops.group_norm_backward(a['g'], a['x'], saved(stats), GN_G, a['gamma'], a['beta'], 'silu')

        def outs(a):
            return [like(a['x']), flat((C,), F32), flat((C,), F32)]

        def call_abi(a, o):
            x = a['x']
            _, stats = ops.group_norm(x, GN_G, a['gamma'], a['beta'], GN_EPS, 'silu')
            ws, n = ws_of(a)
            _lib.check(_lib.lib().vqhip_group_norm_bwd(P(a['g']), P(x), CODE[dtype], _layout_code(x), B, C, Px, GN_G, P(a['gamma']),
                                                       P(a['beta']), P(saved(stats)), 1, P(o[0]), P(o[1]), P(o[2]), P(ws), n, S()),
                       'vqhip_group_norm_bwd')
        abi, free = ('vqhip_group_norm_fwd', 'vqhip_group_norm_bwd'), ('x', 'gamma', 'beta', 'g')
    add(id=f'group_norm{"_backward" if backward else ""}-{"x".join(map(str, shape))}-{_lay(nhwc)}-{NAME[dtype]}', family='group_norm',
        abi=abi, clause=CLAUSE['group_norm'], make=make, call=call, free=free, outs=outs, call_abi=call_abi)


for _shape in GN_SHAPES:
    for _dt in DTYPES:
        for _nhwc in (False, True):
            _group_norm(_shape, _dt, _nhwc, False)
            _group_norm(_shape, _dt, _nhwc, True)


# ---- the ViT row ops ---------------------------------------------------------------------------------------------------------
VIT_SHAPES = ((5, 24), (3, 2051), (3, 2052), (2, 8192))
LN_PAIRS = ((F32, F32), (BF16, BF16), (F16, F16), (F32, BF16), (F32, F16))       # (x and s, res and y and g): the header's table
LN_EPS = 1e-6


def _add_layer_norm(shape, xd, yd, with_res, backward):
    R, D = shape

    def make(seed):
        gen = _gen(seed)
        a = dict(x=_randn(gen, shape, xd), gamma=torch.randn(D, generator=gen).cuda(), beta=torch.randn(D, generator=gen).cuda())
        if with_res:
            a['res'] = _randn(gen, shape, yd)
        if backward:
            a['g'] = _randn(gen, shape, yd)
            a['g_skip'] = _randn(gen, shape, xd)
        return a

    def forward(a):
        return ops.add_layer_norm(a['x'], a.get('res'), a['gamma'], a['beta'], LN_EPS, yd)

    if not backward:
        def call(a):
            s, y, stats = forward(a)
            return (s, y, stats) if with_res else (y, stats)

        def outs(a):
            return ([flat(shape, xd)] if with_res else []) + [flat(shape, yd), flat((R, 2), F32)]

        def call_abi(a, o):
            s = o[0] if with_res else None
            y, stats = o[-2], o[-1]
            _lib.check(_lib.lib().vqhip_add_layer_norm_fwd(P(a['x']), CODE[xd], P(a.get('res')), CODE[yd], R, D, P(a['gamma']), P(a['beta']),
                                                           LN_EPS, P(s), P(y), CODE[yd], P(stats), S()), 'vqhip_add_layer_norm_fwd')
        abi, free = ('vqhip_add_layer_norm_fwd',), ('x', 'res', 'gamma', 'beta')
    else:
        def call(a):
            s, _, stats = forward(a)
            return ops.add_layer_norm_backward(a['g'], s, saved(stats), a['gamma'], a['g_skip'])

        def outs(a):
            return [flat(shape, xd), flat((D,), F32), flat((D,), F32)]

        def call_abi(a, o):
            s, _, stats = forward(a)
            L = _lib.lib()
            ws = torch.empty(2 * L.vqhip_add_layer_norm_slabs(R, D) * D, dtype=F32, device='cuda')
            _lib.check(L.vqhip_add_layer_norm_bwd(P(a['g']), CODE[yd], P(s), CODE[xd], P(a['g_skip']), R, D, P(a['gamma']), P(saved(stats)), P(o[0]),
                                                  P(o[1]), P(o[2]), P(ws), ws.numel() * 4, S()), 'vqhip_add_layer_norm_bwd')
        abi, free = ('vqhip_add_layer_norm_fwd', 'vqhip_add_layer_norm_bwd'), ('x', 'res', 'gamma', 'beta', 'g', 'g_skip')
    add(id=f'add_layer_norm{"_backward" if backward else ""}-{R}x{D}-{NAME[xd]}-{NAME[yd]}-{"res" if with_res else "nores"}',
        family='vit_rows', abi=abi, clause=CLAUSE['vit'], make=make, call=call, free=tuple(n for n in free if with_res or n != 'res'),
        outs=outs, call_abi=call_abi)


def _row_bias_act(shape, dtype, act, backward):
    R, D = shape

    def make(seed):
        gen = _gen(seed)
        a = dict(x=_randn(gen, shape, dtype), bias=torch.randn(D, generator=gen).cuda())
        if backward:
            a['g'] = _randn(gen, shape, dtype)
        return a

    if not backward:
        def call(a):
            return (ops.row_bias_act(a['x'], a['bias'], act),)

        def outs(a):
            return [flat(shape, dtype)]

        def call_abi(a, o):
            _lib.check(_lib.lib().vqhip_row_bias_act_fwd(P(a['x']), CODE[dtype], R, D, P(a['bias']), ops.ROW_ACTS[act], P(o[0]), S()),
                       'vqhip_row_bias_act_fwd')
        abi, free = ('vqhip_row_bias_act_fwd',), ('x', 'bias')
    else:
        def call(a):
            return ops.row_bias_act_backward(a['g'], a['x'], a['bias'], act)

        def outs(a):
            return [flat(shape, dtype), flat((D,), F32)]

        def call_abi(a, o):
            L = _lib.lib()
            ws = torch.empty(L.vqhip_row_bias_act_slabs(R, D) * D, dtype=F32, device='cuda')
            _lib.check(L.vqhip_row_bias_act_bwd(P(a['g']), P(a['x']), CODE[dtype], R, D, P(a['bias']), ops.ROW_ACTS[act], P(o[0]), P(o[1]),
                                                P(ws), ws.numel() * 4, S()), 'vqhip_row_bias_act_bwd')
        abi, free = ('vqhip_row_bias_act_bwd',), ('x', 'bias', 'g')
    add(id=f'row_bias_act{"_backward" if backward else ""}-{R}x{D}-{act}-{NAME[dtype]}', family='vit_rows', abi=abi, clause=CLAUSE['vit'],
        make=make, call=call, free=free, outs=outs, call_abi=call_abi)


for _shape in VIT_SHAPES:
    for _xd, _yd in LN_PAIRS:
        # every shape with the branch to add; the widest and the narrowest also without it
        for _res in ((True, False) if _shape in ((5, 24), (2, 8192)) else (True,)):
            _add_layer_norm(_shape, _xd, _yd, _res, False)
            _add_layer_norm(_shape, _xd, _yd, _res, True)
    for _dt in DTYPES:
        for _act in ('gelu', 'tanh'):
            _row_bias_act(_shape, _dt, _act, False)
            _row_bias_act(_shape, _dt, _act, True)


# ---- image metrics -----------------------------------------------------------------------------------------------------------
def _image_metrics(pdtype, idtype, pnhwc, inhwc):
    B, C, H, W = 2, 3, 33, 65                                                   # image_metrics_ref.SHAPES: more than one tile each way

    def image(gen, dtype, nhwc):
        if dtype == torch.uint8:
            t = torch.randint(0, 256, (B, C, H, W), generator=gen).to(torch.uint8).cuda()
        else:
            t = (2.0 * torch.rand(B, C, H, W, generator=gen) - 1.0).to(dtype).cuda()
        return t.contiguous(memory_format=torch.channels_last) if nhwc else t

    def make(seed):
        gen = _gen(seed)
        return dict(pred=image(gen, pdtype, pnhwc), image=image(gen, idtype, inhwc))

    def call(a):
        m = ops.image_metrics(a['pred'], a['image'])
        return m['values64'], m['values32'], torch.stack((m['abs_sum'], m['sq_sum']), 1)

    def outs(a):
        return [flat((B, 4), torch.float64), flat((B, 4), F32), flat((B, 2), torch.int64)]

    def call_abi(a, o):
        L, p, im = _lib.lib(), a['pred'], a['image']
        n = L.vqhip_image_metrics_workspace_bytes(B, C, H, W)
        ws = torch.empty(max(n // 8, 1), dtype=torch.int64, device='cuda')
        _lib.check(L.vqhip_image_metrics(P(p), ops.IMAGE_DTYPES[pdtype], ops.IMAGE_LAYOUTS[ops.dense_layout(p)], P(im),
                                         ops.IMAGE_DTYPES[idtype], ops.IMAGE_LAYOUTS[ops.dense_layout(im)], B, C, H, W, 1, ops.SSIM_C1,
                                         ops.SSIM_C2, P(ws), n, P(o[0]), P(o[1]), P(o[2]), S()), 'vqhip_image_metrics')

    add(id=f'image_metrics-{NAME[pdtype]}-{_lay(pnhwc)}-{NAME[idtype]}-{_lay(inhwc)}', family='image_metrics', abi=('vqhip_image_metrics',),
        clause=CLAUSE['image_metrics'], make=make, call=call, free=('pred', 'image'), outs=outs, call_abi=call_abi)


for _pd, _id, _pn, _in in ((F32, F32, False, False), (BF16, F32, True, False), (F16, torch.uint8, False, True),
                           (torch.uint8, torch.uint8, True, True), (F32, BF16, True, True), (BF16, F16, False, False)):
    _image_metrics(_pd, _id, _pn, _in)


# ---- families the header keeps at 16 bytes: the stream and capture properties only ------------------------------------------
POOL_B, POOL_HW, POOL_K, POOL_D = 3, 37, 80, 20


def _pool():
    def tokens(gen, tdtype, K):
        return torch.randint(0, K, (POOL_B, POOL_HW), generator=gen).to(tdtype).cuda()

    for tdtype in (torch.int32, torch.int64):
        def make(seed, tdtype=tdtype):
            gen = _gen(seed)
            return dict(e=torch.randn(POOL_K, POOL_D, generator=gen).cuda(), quant=tokens(gen, tdtype, POOL_K))
        add(id=f'decode_pool-{NAME[tdtype]}', family='pooled', abi=('vqhip_decode_pool',), clause=CLAUSE['pool'], make=make,
            call=lambda a: (ops.decode_pool(a['e'], a['quant']),))

        def make_fsq(seed, tdtype=tdtype):
            return dict(quant=tokens(_gen(seed), tdtype, 8 * 5 * 5))
        add(id=f'fsq_decode_pool-{NAME[tdtype]}', family='pooled', abi=('vqhip_fsq_decode_pool',), clause=CLAUSE['pool'], make=make_fsq,
            call=lambda a: (ops.fsq_decode_pool(a['quant'], ops.fsq_constants((8, 5, 5))),))

    def make_bwd(seed):
        # float atomics: two addends per element at the most, so that their order cannot show (a + b == b + a exactly)
        gen = _gen(seed)
        quant = torch.cat([torch.randperm(POOL_K, generator=gen)[:POOL_HW] for _ in range(2)]).view(2, POOL_HW)
        return dict(g=torch.randn(2, POOL_D, generator=gen).cuda(), quant=quant.cuda())
    add(id='decode_pool_bwd', family='pooled', abi=('vqhip_decode_pool_bwd',), clause=CLAUSE['pool'], make=make_bwd,
        call=lambda a: (ops.decode_pool_bwd(a['g'], a['quant'], POOL_K),))


_pool()

FSQ_LEVELS = (8, 5, 5, 5)


def _fsq():
    q = ops.fsq_constants(FSQ_LEVELS)
    C = len(FSQ_LEVELS)
    for dtype in (F32, BF16):
        for shape in ((77, C), (2, C, 5, 7)):
            kind = 'map' if len(shape) == 4 else 'rows'

            def make(seed, dtype=dtype, shape=shape):
                gen = _gen(seed)
                return dict(x=_randn(gen, shape, dtype, scale=2.0), g=torch.randn(shape, generator=gen).cuda())

            def encode(a):
                quant, z, _ = ops.fsq_encode(a['x'], q)
                return quant, z

            def backward(a):
                return encode(a) + (ops.fsq_backward(a['x'], a['g'], q),)

            def decode(a, shape=shape):
                quant, _ = encode(a)
                return (ops.fsq_decode(quant, q, map_shape=(shape[0], shape[2], shape[3]) if len(shape) == 4 else None),)

            add(id=f'fsq_encode-{kind}-{NAME[dtype]}', family='fsq', abi=('vqhip_fsq_encode',), clause=CLAUSE['limits'], make=make, call=encode)
            add(id=f'fsq_backward-{kind}-{NAME[dtype]}', family='fsq', abi=('vqhip_fsq_encode', 'vqhip_fsq_backward'), clause=CLAUSE['limits'],
                make=make, call=backward)
            add(id=f'fsq_decode-{kind}-{NAME[dtype]}', family='fsq', abi=('vqhip_fsq_encode', 'vqhip_fsq_decode'), clause=CLAUSE['limits'],
                make=make, call=decode)


_fsq()

ENT_N, ENT_K, ENT_D, ENT_BLOCK = 150, 96, 16, 64                              # three row blocks, the last one ragged


def _entropy_and_anchor():
    for metric in ('L2', 'Cosine'):
        def make(seed, metric=metric):
            gen = _gen(seed)
            x, e = torch.randn(ENT_N, ENT_D, generator=gen).cuda(), torch.randn(ENT_K, ENT_D, generator=gen).cuda()
            if metric == 'Cosine':
                x, e = ops.normalize_rows(x), ops.normalize_rows(e)
            return dict(x=x, e=e, u=torch.rand(ENT_K, generator=gen).cuda(), upstream=torch.randn(1, generator=gen).cuda())

        def loss(a, metric=metric):
            value, saved = ops.entropy_loss(a['x'], a['e'], metric, 0.7, ENT_BLOCK)
            return value, saved['lse'], saved['spa'], saved['q'], saved['c']

        def grad(a, metric=metric):
            _, saved = ops.entropy_loss(a['x'], a['e'], metric, 0.7, ENT_BLOCK)
            return ops.entropy_loss_backward(a['x'], a['e'], metric, 0.7, saved, a['upstream'])

        add(id=f'entropy_loss-{metric}', family='entropy', abi=('vqhip_distance', 'vqhip_entropy_rows', 'vqhip_entropy_finish'),
            clause=CLAUSE['entropy'], make=make, call=loss)
        add(id=f'entropy_loss_backward-{metric}', family='entropy',
            abi=('vqhip_distance', 'vqhip_entropy_rows', 'vqhip_entropy_finish', 'vqhip_entropy_grad'), clause=CLAUSE['entropy'], make=make,
            call=grad)
        add(id=f'col_multinomial-{metric}', family='multinomial_anchor',
            abi=('vqhip_distance', 'vqhip_col_multinomial_max', 'vqhip_col_multinomial_mass', 'vqhip_col_multinomial_pick',
                 'vqhip_col_multinomial_resolve'), clause=CLAUSE['limits'], make=make,
            call=lambda a, metric=metric: (ops.col_multinomial(a['x'], a['e'], metric, u=a['u'], block_rows=ENT_BLOCK),))


_entropy_and_anchor()

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), 'two table entries share an id'
PLACED = [c for c in CASES if c.call_abi is not None]


# ---- what is not in the table, and why -----------------------------------------------------------------------------------------
_QUANTIZER = 'quantizer path: off the default stream and inside captures in test_gpu_parity (side stream, GraphedQuantizer); 16-byte LIMITS'
_ONE_CALL = 'one-call training forward: streams and captures in test_gpu_one_call; 16-byte LIMITS'
_UPDATE = 'codebook update path: held to float64 in test_gpu_updates, captured in the GraphedQuantizer tests; 16-byte LIMITS'
_EXCHANGE = 'rank exchange: needs a process group or an RCCL communicator (rccl_ws1_child, test_gpu_two_ranks)'
_BACKWARD = 'quantizer backward: test_gpu_backward; reached from the captured training steps of test_gpu_parity; 16-byte LIMITS'
_DEBUG = 'debug / statistics entry point read back on the host by definition'

EXEMPT = {
    **{n: _QUANTIZER for n in (
        'vqhip_encode', 'vqhip_encode_ex', 'vqhip_encode_map', 'vqhip_codebook_prepare', 'vqhip_argmin', 'vqhip_argmin_exact',
        'vqhip_col_argmin', 'vqhip_row_sqnorm', 'vqhip_normalize_rows', 'vqhip_gather_ste_loss', 'vqhip_gather_ste_mse',
        'vqhip_gather_ste_map', 'vqhip_hist', 'vqhip_hist_i32', 'vqhip_gather_rows', 'vqhip_diff', 'vqhip_ste', 'vqhip_transpose')},
    **{n: _ONE_CALL for n in ('vqhip_cvq_forward', 'vqhip_vqkd_forward', 'vqhip_vq_forward')},
    **{n: _UPDATE for n in (
        'vqhip_vqkd_update', 'vqhip_cvq_update', 'vqhip_cvq_step', 'vqhip_cvq_decay', 'vqhip_cvq_update_rows', 'vqhip_cvq_rows',
        'vqhip_col_argmin_rows', 'vqhip_cvq_apply', 'vqhip_token_order', 'vqhip_segsum_rows')},
    **{n: _EXCHANGE for n in (
        'vqhip_pack_counts', 'vqhip_unpack_counts', 'vqhip_allreduce_packed', 'vqhip_cvq_pack', 'vqhip_cvq_col_keys', 'vqhip_cvq_pack_sync',
        'vqhip_allreduce_min_i64')},
    **{n: _BACKWARD for n in (
        'vqhip_vqkd_backward', 'vqhip_vq_backward', 'vqhip_vq_backward_ex', 'vqhip_vq_backward_map', 'vqhip_normalize_rows_bwd',
        'vqhip_vq_backward_w_ordered')},
    'vqhip_scatter_add_rows': 'fp32 atomics: not bit-reproducible, so neither property can be stated as equal bits',
    'vqhip_codebook_metrics': 'its caller reads the result on the host (.tolist()): a host read by definition',
    'vqhip_argmin_stats': _DEBUG,
    'vqhip_debug_proposal_scores': _DEBUG,
}
# (ops.sample_cut_fields is a host reader of sample_tokens' cut records and has no entry point of its own.)
