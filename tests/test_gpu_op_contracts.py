"""Where the data lives and how the launch is issued, for every entry of tests/contract_cases.py: three properties, all of them
equal bits against a call on fresh, allocator-aligned tensors on the default stream (the summation orders of include/vqhip.h are
defined by element index, so there is no tolerance to choose).

(a) placement   every tensor the family's clause frees from alignment, the fp32 parameter vectors with them, is rebuilt as a view
                into a larger buffer at element offsets 1 and 3 past a 16-byte boundary (16-bit: addresses = 2 and 6 mod 16; fp32:
                4 and 12), and the op runs through ``ops`` on those.  Then the same launch goes through ``_lib.lib()`` with every
                output at the same offsets inside a buffer filled with a byte sentinel, 256 guard bytes on either side: the bits
                are those of the baseline and no guard byte has changed.
(b) side stream the call runs on a non-blocking side stream directly behind a device-side ``copy_`` of new contents into its inputs
                (and a short device sleep in front of the copy): a launch that escaped to stream 0 reads the old contents.
(c) capture     three warm-up calls on a side stream, one call captured, new contents copied into the static inputs, one replay:
                the bits of an eager call on the new contents.  A host read baked into the launch reproduces the old result; a
                host synchronisation or a launch on another stream ends the capture with HIP's message, which is the failure.

One forward of every family whose clause frees alignment is also held to the float64 restatement of its tests/*_ref.py at a
misaligned placement (element offset 3), within the derived bound of the family's own test, so that the misaligned result is not
only equal to itself."""
import pytest
import torch

from vector_quantization_amd import _lib, functional, ops, samplers

import numpy as np

import contract_cases as table
import cosine_embed_ref
import group_norm_ref
import image_metrics_ref
import lpips_ref
import sampler_ref
import stylegan2_ref
import test_gpu_sampler as sampler_checks
import token_ce_ref
import vit_ops_ref

pytestmark = pytest.mark.gpu

OFFSETS = (1, 3)
GUARD = 256
SENTINEL = 0xA5
SLEEP_CYCLES = 2_000_000                     # about a millisecond in front of the copy: far longer than a launch takes to start
INT_OF = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}


def same_bits(got, want, what):
    assert len(got) == len(want), f'{what}: {len(got)} results, {len(want)} expected'
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, f'{what}: result {i} is missing on one side'
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, f'{what}: result {i} is {a.dtype} {tuple(a.shape)}, expected {b.dtype} {tuple(b.shape)}'
        if a.is_floating_point():
            na, nb = torch.isnan(a), torch.isnan(b)
            assert torch.equal(na, nb), f'{what}: result {i} has its NaNs elsewhere'
            kind = INT_OF[a.element_size()]
            a, b = a[~na].view(kind), b[~nb].view(kind)
        differ = int((a != b).sum())
        assert differ == 0, f'{what}: result {i} differs in {differ} of {a.numel()} elements'


class Block:
    """A view of the given shape, strides and dtype whose first element lies ``off`` elements past a 16-byte boundary, inside a
    buffer of sentinel bytes with at least GUARD bytes in front of it and behind it."""

    def __init__(self, shape, stride, dtype, off, source=None):
        es = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        self.span = (sum((s - 1) * st for s, st in zip(shape, stride)) + 1) if numel else 0
        # an output is dense, so everything outside its span is guard; an input may be rows with padding (the logits), which
        # is checked as a whole buffer that must not change
        assert source is not None or self.span == numel, 'an output of the table is dense: its whole span belongs to it'
        self.lead = GUARD // es + off
        total = (self.lead + self.span) * es + GUARD + 16
        self.raw = torch.full((total - total % -16,), SENTINEL, dtype=torch.uint8, device='cuda')
        assert self.raw.data_ptr() % 16 == 0
        self.view = self.raw.view(dtype).as_strided(shape, stride, self.lead)
        assert self.view.data_ptr() % 16 == (off * es) % 16
        self.lo, self.hi = self.lead * es, (self.lead + self.span) * es
        if source is not None:
            self.view.copy_(source)
            self.snapshot = self.raw.clone()

    def guards_intact(self) -> bool:
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())

    def untouched(self) -> bool:
        return torch.equal(self.raw, self.snapshot)


def placed_arguments(case, args, off):
    blocks = {name: Block(args[name].shape, args[name].stride(), args[name].dtype, off, args[name]) for name in case.free if name in args}
    moved = dict(args)
    moved.update({name: blk.view for name, blk in blocks.items()})
    for name in blocks:                                                         # the strided views keep their strides
        assert moved[name].stride() == args[name].stride() and torch.equal(moved[name], args[name])
    return moved, blocks


@pytest.mark.parametrize('case', table.PLACED, ids=lambda c: c.id)
def test_placement(case):
    args = case.make(0)
    base = case.call(args)
    torch.cuda.synchronize()
    for off in OFFSETS:
        tag = f'{case.id} at element offset {off}'
        moved, blocks = placed_arguments(case, args, off)
        outs = [Block(shape, stride, dtype, off) for shape, stride, dtype in case.outs(moved)]
        table.INTERMEDIATE_OFFSET = off                                         # what a backward takes over from its forward, too
        try:
            same_bits(case.call(moved), base, tag + ', inputs placed')
            case.call_abi(moved, [o.view for o in outs])
            torch.cuda.synchronize()
        finally:
            table.INTERMEDIATE_OFFSET = 0
        same_bits([o.view for o in outs], base, tag + ', inputs and outputs placed')
        for i, o in enumerate(outs):
            assert o.guards_intact(), f'{tag}: a guard byte around output {i} has changed'
        for name, blk in blocks.items():
            assert blk.untouched(), f'{tag}: the input {name} or a guard byte around it has changed'


@pytest.mark.parametrize('case', table.CASES, ids=lambda c: c.id)
def test_side_stream(case):
    static, new = case.make(0), case.make(1)
    want = case.call(new)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        for name, t in static.items():
            t.copy_(new[name])
        got = case.call(static)
    side.synchronize()
    same_bits(got, want, f'{case.id} on a side stream')


def capture_and_replay(call, static, new):
    """``call(static)`` captured behind three warm-up calls on a side stream, replayed once on the contents of ``new``."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = call(static)
    for name, t in static.items():
        t.copy_(new[name])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    return graph, got


@pytest.mark.parametrize('case', table.CASES, ids=lambda c: c.id)
def test_capture_and_replay(case):
    static, new = case.make(0), case.make(1)
    want = case.call(new)
    torch.cuda.synchronize()
    _, got = capture_and_replay(case.call, static, new)
    same_bits(got, want, f'{case.id} replayed on new contents')


# ---- against the float64 restatement, misaligned -------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', table.DTYPES, ids=str)
def test_a_misaligned_group_norm_is_within_the_derived_bound(dtype):
    case = table.BY_ID[f'group_norm-1x64x40x40-nchw-{table.NAME[dtype]}']
    args, _ = placed_arguments(case, case.make(0), 3)
    x, gamma, beta = args['x'], args['gamma'], args['beta']
    y, _ = case.call(args)
    act = 'silu'
    want, _, parts = group_norm_ref.forward(x, table.GN_G, gamma, beta, table.GN_EPS, act)
    bound = group_norm_ref.forward_bound(x, table.GN_G, gamma, beta, table.GN_EPS, act, want, parts)
    bound = bound + _lib.sg2_store_u(table.CODE[dtype]) * (want.abs() + bound) + (2.0 ** -25 if dtype == torch.float16 else 0.0)
    err = (y.double() - want.double()).abs()
    assert torch.isfinite(err).all()
    worst = float((err / bound).max())
    print(f'group_norm misaligned {dtype}: worst error / bound = {worst:.3f}')
    assert worst <= 1.0


def _store(value, dtype):
    """Half an ulp of the output dtype on top of a bound for |value| (VQHIP_SG2_STORE_U; 2^-25 / 2^-134: its subnormals)."""
    return _lib.sg2_store_u(table.CODE[dtype]) * value + {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}.get(dtype, 0.0)


def _within(got, want, bound, what):
    err = (got.double() - want.double()).abs()
    assert torch.isfinite(err).all(), f'{what}: not finite'
    worst = float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())
    print(f'{what}: worst error / bound = {worst:.3f}')
    assert worst <= 1.0, f'{what}: error / bound = {worst}'


def _misaligned(case_id):
    case = table.BY_ID[case_id]
    args, _ = placed_arguments(case, case.make(0), 3)
    return case, args


@pytest.mark.parametrize('dtype', table.DTYPES, ids=str)
def test_a_misaligned_sampler_row_draws_as_the_restatement(dtype):
    """Top-k alone (a pure comparison: exact), the draw inside its interval and the kept mass within VQHIP_SAMPLE_DELTA."""
    _, args = _misaligned(f'sample_tokens-{table.NAME[dtype]}-plain')
    start, end, top_k = table.SAMPLE_START, table.SAMPLE_END, 50
    tokens, cut = ops.sample_tokens(args['logits'], start, end, u=args['u'], top_k=top_k, want_cut=True)
    tokens, cut, u = tokens.cpu().numpy(), ops.sample_cut_fields(cut), args['u'].cpu().numpy()
    a = sampler_ref.keys(args['logits'].float().cpu().numpy()[:, start:end])
    dlt = sampler_ref.delta(end - start)
    for r in range(table.SAMPLE_R):
        surv = sampler_ref.topk_set(a[r], top_k)
        assert cut['topk_kept'][r] == surv.sum() == cut['kept'][r]
        kept = sampler_ref.kept_from_cut(a[r], cut['cut_value'][r], cut['cut_index'][r])
        assert np.array_equal(kept, surv) and cut['max'][r] == a[r].max()
        sampler_checks.check_draw(a[r], kept, tokens[r], u[r], dlt, start)
        sampler_checks.check_z(a[r], kept, cut['z'][r], dlt)


@pytest.mark.parametrize('dtype', table.DTYPES, ids=str)
def test_a_misaligned_token_ce_forward_is_within_the_derived_bound(dtype):
    case, args = _misaligned(f'token_ce_forward-{table.NAME[dtype]}-i64')
    loss, lse, hit, _ = case.call(args)
    start, V = table.SAMPLE_START, table.SAMPLE_END - table.SAMPLE_START
    a = token_ce_ref.slice64(args['logits'].cpu(), start, V)
    e = token_ce_ref.reference(a, token_ce_ref.row_targets(args['targets'].cpu().numpy(), start, V), 0.1,
                               args['weight'].double().cpu().numpy())
    b = np.array([token_ce_ref.bound(V, am) for am in np.abs(a).max(-1)])
    assert not e['live'].all() and e['live'].any()
    for name, got in (('lse', lse), ('loss', loss)):
        err = np.abs(got.double().cpu().numpy() - e[name])
        print(f'token CE misaligned {dtype} {name}: worst error / bound = {(err / b).max():.3f}')
        assert (err <= b).all(), (name, err.max(), b)
    assert np.array_equal(hit.cpu().numpy(), e['hit'])


@pytest.mark.parametrize('dtype', table.DTYPES, ids=str)
def test_a_misaligned_cosine_embedding_forward_is_within_the_derived_bound(dtype):
    case, args = _misaligned(f'cosine_embedding_forward-rows-5x520-{table.NAME[dtype]}-f32')
    loss, stats, _ = case.call(args)
    e = cosine_embed_ref.reference(cosine_embed_ref.as64(args['pred'].cpu()), cosine_embed_ref.as64(args['target'].cpu()))
    b = cosine_embed_ref.bound(520)
    for name, got, want in (('loss', loss, e['loss']), ('cos', stats[:, 1], e['cos'])):
        err = np.abs(got.double().cpu().numpy() - want)
        print(f'cosine embedding misaligned {dtype} {name}: worst error / bound = {err.max() / b:.3f}')
        assert (err <= b).all(), (name, err.max(), b)


@pytest.mark.parametrize('dtype', table.DTYPES, ids=str)
def test_a_misaligned_lpips_layer_forward_is_within_the_derived_bound(dtype):
    case, args = _misaligned(f'lpips_layer_forward-C65-nhwc-{table.NAME[dtype]}')
    stats, value = case.call(args)
    B, C, Px = stats.shape[0], 65, stats.shape[1]
    mask = ops.lpips_keep_mask(args['seed'], table.LPIPS_P, table.LPIPS_LAYER, B, C, Px).cpu().numpy()
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(table.LPIPS_P)))
    w = args['weight'].reshape(-1).double().cpu().numpy()
    e = lpips_ref.reference(lpips_ref.as64(args['pred']), lpips_ref.as64(args['target']), w, mask, scale)
    fb = lpips_ref.bound(C, float(np.abs(w).max())) * scale
    for name, got, want in (('s', stats[..., 3], e['s']), ('value', value, e['value'])):
        err = np.abs(got.double().cpu().numpy() - want)
        print(f'LPIPS misaligned {dtype} {name}: worst error / bound = {err.max() / fb:.3f}')
        assert (err <= fb).all(), (name, err.max(), fb)


@pytest.mark.parametrize('dtype', table.DTYPES, ids=str)
def test_a_misaligned_bias_act_is_within_the_derived_bound(dtype):
    case, args = _misaligned(f'bias_act-C130-nhwc-{table.NAME[dtype]}')
    y, = case.call(args)
    want = stylegan2_ref.bias_act(args['x'], args['bias'])
    bound = _lib.bias_act_bound(1.0) * want.abs()
    _within(y, want, bound + _lib.sg2_store_u(table.CODE[dtype]) * (want.abs() + bound) + (2.0 ** -25 if dtype == torch.float16 else 0.0),
            f'bias_act misaligned {dtype}')


@pytest.mark.parametrize('xdt,ydt', table.LN_PAIRS, ids=str)
def test_a_misaligned_add_layer_norm_is_within_the_derived_bound(xdt, ydt):
    case, args = _misaligned(f'add_layer_norm-3x2051-{table.NAME[xdt]}-{table.NAME[ydt]}-res')
    s, y, _ = case.call(args)
    ws = vit_ops_ref.rounded_sum(args['x'], args['res'])
    assert torch.equal(s, ws)
    want, _, parts = vit_ops_ref.ln_forward(ws, args['gamma'], args['beta'], table.LN_EPS)
    bound = vit_ops_ref.ln_forward_bound(ws, args['gamma'], args['beta'], table.LN_EPS, want, parts)
    _within(y, want, bound + _store(want.abs() + bound, ydt), f'add_layer_norm misaligned {xdt} {ydt}')


@pytest.mark.parametrize('act', ['gelu', 'tanh'])
@pytest.mark.parametrize('dtype', table.DTYPES, ids=str)
def test_a_misaligned_row_bias_act_is_within_the_derived_bound(dtype, act):
    case, args = _misaligned(f'row_bias_act-3x2051-{act}-{table.NAME[dtype]}')
    y, = case.call(args)
    want, parts = vit_ops_ref.act_forward(args['x'], args['bias'], act)
    bound = vit_ops_ref.act_forward_bound(act, want, parts)
    _within(y, want, bound + _store(want.abs() + bound, dtype), f'row_bias_act misaligned {dtype} {act}')


@pytest.mark.parametrize('case_id', ['image_metrics-f32-nchw-f32-nchw', 'image_metrics-bf16-nhwc-f32-nchw', 'image_metrics-bf16-nchw-f16-nchw'])
def test_misaligned_image_metrics_are_the_restatement(case_id):
    """The integer sums, l1 and mse exactly, psnr within 2 double ulp, ssim within VQHIP_IMAGE_SSIM_BOUND: the family's own check."""
    case, args = _misaligned(case_id)
    values64, values32, sums = (t.cpu().numpy() for t in case.call(args))
    e = image_metrics_ref.metrics(image_metrics_ref.decode(args['pred'].cpu()).numpy(), image_metrics_ref.decode(args['image'].cpu()).numpy())
    assert np.array_equal(sums[:, 0], e['abs_sum']) and np.array_equal(sums[:, 1], e['sq_sum'])
    assert np.array_equal(values64[:, 0], e['l1']) and np.array_equal(values64[:, 1], e['mse'])
    assert (image_metrics_ref.ulps(values64[:, 2], e['psnr']) <= 2).all()
    err = np.abs(values64[:, 3] - e['ssim'])
    print(f'{case_id} misaligned: largest ssim error {err.max() / image_metrics_ref.SSIM_BOUND:.4f} of the bound')
    assert (err <= image_metrics_ref.SSIM_BOUND).all()
    assert np.array_equal(values32, values64.astype(np.float32), equal_nan=True)


# ---- the modules ---------------------------------------------------------------------------------------------------------------
def _cfg_sampler():
    return samplers.CFGSampler(sampler=samplers.TopKTopPSampler(temperature=0.9, top_k=50, top_p=0.9), alpha=1.5)


def _sampler_inputs(seed):
    gen = torch.Generator().manual_seed(50 + seed)
    return dict(logits=table._logits(gen, table.SAMPLE_R, torch.bfloat16), u=torch.rand(table.SAMPLE_R // 2, generator=gen).cuda())


def test_sampler_module_captured_with_static_uniforms():
    sampler = _cfg_sampler()

    def call(a):
        tokens, _ = sampler(a['logits'], table.SAMPLE_START, table.SAMPLE_END, {'u': a['u']})
        assert sampler.last_route.name == 'fused', sampler.last_route
        return (tokens,)

    static, new = _sampler_inputs(0), _sampler_inputs(1)
    want = call(new)
    torch.cuda.synchronize()
    _, got = capture_and_replay(call, static, new)
    same_bits(got, want, 'CFGSampler replayed on new logits and new memo[\'u\']')


def test_sampler_module_captured_without_uniforms_draws_anew_on_every_replay():
    """Flat logits over 1001 tokens, 3 output rows: two replays that agree in every token have drawn from the same uniforms
    (the chance otherwise is 1001^-3)."""
    sampler = samplers.CFGSampler(sampler=samplers.TopKTopPSampler(temperature=1.0, top_k=0, top_p=2.0), alpha=1.5)
    static = dict(logits=torch.zeros(table.SAMPLE_R, table.SAMPLE_VT, dtype=torch.float32, device='cuda'))

    def call(a):
        tokens, _ = sampler(a['logits'], table.SAMPLE_START, table.SAMPLE_END, {})
        assert sampler.last_route.name == 'fused', sampler.last_route
        return (tokens,)

    graph, got = capture_and_replay(call, static, static)
    first = got[0].clone()
    graph.replay()
    torch.cuda.synchronize()
    second = got[0].clone()
    for tokens in (first, second):
        assert int(tokens.min()) >= table.SAMPLE_START and int(tokens.max()) < table.SAMPLE_END
        assert torch.equal(tokens[:3], tokens[3:])                              # the CFG duplication
    assert not torch.equal(first, second), 'two replays drew the same tokens: the uniforms were baked into the capture'
    # and outside a capture the module's block still serves a seeded run
    sampler._u_block = None
    torch.manual_seed(11)
    a, _ = sampler(static['logits'], table.SAMPLE_START, table.SAMPLE_END, {})
    sampler._u_block = None
    torch.manual_seed(11)
    b, _ = sampler(static['logits'], table.SAMPLE_START, table.SAMPLE_END, {})
    assert torch.equal(a, b)


def test_lpips_module_captured_in_training_mode_masks_anew_on_every_replay():
    import vector_quantization_amd as vqa
    torch.manual_seed(3)
    loss = vqa.LPIPSLoss(reduction='none').cuda().train()
    seeds = []
    draw = loss._seed
    loss._seed = lambda device: seeds.append(draw(device)) or seeds[-1]

    def inputs(seed):
        gen = torch.Generator().manual_seed(60 + seed)
        image = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
        return dict(pred=(image + 0.3 * torch.randn(2, 3, 32, 32, generator=gen)).clamp(-1, 1).cuda(), image=image.cuda())

    taps = []
    extract = loss.extract_features
    loss.extract_features = lambda image: taps.append(extract(image)) or taps[-1]

    def call(a):
        """The value, the gradient the fused tail hands to the deepest feature map, the gradient at the image, and the ten feature
        maps themselves: the convolution library's features need not repeat their bits between an eager and a captured run, so
        the fused tail is held to equal bits on the features the replay itself produced."""
        del taps[:]
        x = a['pred'].detach().requires_grad_()
        out = loss(x, a['image'])
        assert loss.last_route.name == 'fused', loss.last_route
        at_image, at_tap = torch.autograd.grad(out.sum(), [x, taps[0][-1]])
        return (out, at_tap, at_image) + tuple(taps[0]) + tuple(t.detach() for t in taps[1])

    static, new = inputs(0), inputs(1)
    graph, got = capture_and_replay(call, static, new)
    seed = seeds[-1]                                                            # the capture's own: static, rewritten by every replay
    words = [seed.clone()]
    results = [[t.clone() for t in got]]
    graph.replay()
    torch.cuda.synchronize()
    words.append(seed.clone())
    results.append([t.clone() for t in got])
    assert not torch.equal(words[0], words[1]), 'two replays used the same seed words'
    B, C, Px = 2, ops.LPIPS_CHANNELS[0], 32 * 32
    masks = [ops.lpips_keep_mask(w, loss._dropout.p, 0, B, C, Px) for w in words]
    assert not torch.equal(masks[0], masks[1]), 'two replays used the same keep mask'
    assert all(0.45 < float(m.float().mean()) < 0.55 for m in masks)
    # each replay is the eager fused tail, value and gradient, on that replay's own feature maps under that replay's seed words
    weights = [conv.weight for conv in loss._convs]
    for w, replayed in zip(words, results):
        preds, targets = [t.clone().requires_grad_() for t in replayed[3:8]], replayed[8:13]
        value = loss._reduce(ops.lpips_distance(preds, targets, weights, w, loss._dropout.p).view(-1, 1, 1, 1))
        at_tap, = torch.autograd.grad(value.sum(), preds[-1])
        same_bits((value.detach(), at_tap), replayed[:2], 'LPIPSLoss replayed in training mode')
        for grad in replayed[1:3]:
            assert bool(torch.isfinite(grad).all()) and float(grad.abs().sum()) > 0
    assert not torch.equal(results[0][1], results[1][1]), 'two replays gave the same gradient: the mask did not change'


def test_functional_group_norm_and_add_layer_norm_through_autograd_in_one_capture():
    def inputs(seed):
        gen = torch.Generator().manual_seed(70 + seed)
        r = lambda *shape: torch.randn(*shape, generator=gen).cuda()
        return dict(x=r(2, 32, 5, 7), gw=r(32), gb=r(32), g=r(2, 32, 5, 7), rows=r(3, 2051), res=r(3, 2051), lw=r(2051), lb=r(2051),
                    gs=r(3, 2051), gy=r(3, 2051))

    def call(a):
        leaves = [a[k].detach().requires_grad_() for k in ('x', 'gw', 'gb', 'rows', 'res', 'lw', 'lb')]
        x, gw, gb, rows, res, lw, lb = leaves
        y = functional.group_norm(x, 32, gw, gb, 1e-6, 'silu')
        s, z = functional.add_layer_norm(rows, res, lw, lb, 1e-6)
        grads = torch.autograd.grad([y, s, z], leaves, [a['g'], a['gs'], a['gy']])
        return (y, s, z) + tuple(grads)

    static, new = inputs(0), inputs(1)
    want = call(new)
    torch.cuda.synchronize()
    _, got = capture_and_replay(call, static, new)
    same_bits(got, want, 'group_norm and add_layer_norm through autograd, replayed')
