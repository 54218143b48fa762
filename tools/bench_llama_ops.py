"""The row ops of LlamaTransformer: ``functional.add_rms_norm`` and ``functional.swiglu`` (one HIP launch forward, the recomputing
backwards) against the torch composition a ``LlamaDecoderLayer`` runs (``residual + hidden_states``, the lines of ``LlamaRMSNorm``;
``act_fn(gate) * up``), forward + backward, and one training step of the medium ``LlamaTransformer`` (configs/ar/transformers/llama.py:
24 layers, hidden 1024, 16 heads, intermediate 2816) on both routes - the torch route is transformers' own forward with
``labels=tokens``, what the class ran before the kernels - in the same process on the same GPU.

    python tools/bench_llama_ops.py [--batch 64] [--blocks 5] [--iters 1000] [--module-iters 5] [--skip-module] [--layers 24]
                                    [--generate-batch 32] [--generate-length 65] [--out profiles/llama_transformer.txt]
    python tools/bench_llama_ops.py --generate-only --generate-length 65,257 --out profiles/llama_decode.txt

Generation has a third route, ``decode``: the same model with ``static_cache=True`` (a ``StaticKVCache`` and one
``functional.decode_attention`` launch per layer and token), alternating block by block with the other two; its line also carries
the kernel launches of one single-token step per layer, counted with the profiler.  ``--generate-only`` times generation alone, at
every length of ``--generate-length`` (a comma-separated list).  A fourth route, ``graph``, is the decode route with ``graph=True``:
the single-token steps replayed from one captured HIP graph (``decode_graph.DecodeGraph``).  Its line carries two figures, both
against the eager decode route of the same run: ``first_call`` - one ``generate`` that has to capture, timed once, beside one decode
call timed at the same moment - and the alternating blocks, where the captured graph is reused.

Shapes: [B * 257, 1024] (the residual stream) and [B * 257, 2 * 2816] (the gate | up tensor) with B = ``--batch`` images of 256 tokens
and the class token.  configs/llamagen/ar.py trains with 256 images per rank; the default here is 64, so that the 24 layers' saved
activations of both routes fit one device side by side, and B is written into every line.  fp32 and bf16 autocast (fp32 stream,
bf16 branch and output).  Warm-up, then ``blocks`` blocks timed with device events, the routes alternating block by block: ``iters``
calls per block for an op (1000 calls of 130 - 480 us: windows of 0.13 - 0.5 s), ``module-iters`` training steps per block for the
model, one whole ``generate`` per block for generation (``generate-batch`` class tokens to ``generate-length`` tokens through the KV
cache and ``BaseSampler``, under no_grad, one token per step).  The figure is the median of the block means in microseconds, host
enqueue included, with the smallest and largest block; every line carries the iteration count it was timed with.  One JSON line
per case; ``--out`` appends the lines to a file.  Whatever is measured is written down as it is."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MEDIUM = dict(num_hidden_layers=24, num_attention_heads=16, hidden_size=1024, intermediate_size=2816, rms_norm_eps=1e-5)
VOCABULARY = 1000 + 16384                                                       # class tokens + the LlamaGen codebook


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fns, blocks, iters):
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(block_us(fn, iters))
    return {name: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for name, v in times.items()}


def norm_case(functional, R, D, autocast, args):
    torch.manual_seed(0)
    low = torch.bfloat16 if autocast else torch.float32
    x = torch.randn(R, D, device='cuda', requires_grad=True)
    r = torch.randn(R, D, device='cuda').to(low).requires_grad_()
    w = torch.randn(D, device='cuda', requires_grad=True)
    g, gs = torch.randn(R, D, device='cuda').to(low), torch.randn(R, D, device='cuda')

    def run(fn):
        x.grad = r.grad = w.grad = None
        s, y = fn()
        torch.autograd.backward((s, y), (gs, g))

    def torch_route():
        # as a decoder layer runs it: the add promotes to the stream's fp32, LlamaRMSNorm's five passes, the next linear casts
        with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
            s = x + r
            h = s.to(torch.float32)
            h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-5)
            return s, (w * h.to(s.dtype)).to(low)

    res = alternate({'fused': lambda: run(lambda: functional.add_rms_norm(x, r, w, 1e-5, low, strict=True)), 'torch': lambda: run(torch_route)},
                    args.blocks, args.iters)
    # forward reads x and res, writes s and y; backward reads g, s and g_skip, writes gx (and the cast of gx for res under autocast)
    nbytes = R * D * (4 + r.element_size() + 4 + r.element_size() + g.element_size() + 4 + 4 + 4)
    return dict(case='add_rms_norm_fwd_bwd', nbytes=nbytes, **res)


def swiglu_case(functional, R, width, autocast, args):
    torch.manual_seed(0)
    low = torch.bfloat16 if autocast else torch.float32
    h = torch.randn(R, 2 * width, device='cuda').to(low).requires_grad_()
    gate, up = (t.detach().clone().requires_grad_() for t in h.chunk(2, dim=1))  # what two GEMMs leave: two dense tensors
    g = torch.randn(R, width, device='cuda').to(low)

    def fused():
        h.grad = None
        functional.swiglu(h, strict=True).backward(g)

    def plain():
        gate.grad = up.grad = None
        (F.silu(gate) * up).backward(g)

    res = alternate({'fused': fused, 'torch': plain}, args.blocks, args.iters)
    nbytes = R * width * h.element_size() * 8                                   # forward 2 in, 1 out; backward 1 + 2 in, 2 out
    return dict(case='swiglu_fwd_bwd', nbytes=nbytes, **res)


def module_case(autocast, args):
    from vector_quantization_amd.registries import VQSMTransformerRegistry
    torch.manual_seed(0)
    config = dict(type='LlamaTransformer', transformer=dict(MEDIUM, num_hidden_layers=args.layers), vocabulary_size=VOCABULARY,
                  sampler=dict(type='BaseSampler'))
    nets = {name: VQSMTransformerRegistry.build(dict(config, fused=name == 'fused')).cuda() for name in ('fused', 'torch')}
    nets['fused'].init_weights(None)
    torch.nn.init.normal_(nets['fused']._transformer.lm_head.weight, std=0.02)   # (zero would make the loss's backward trivial)
    nets['torch'].load_state_dict(nets['fused'].state_dict(), strict=True)
    tokens = torch.randint(0, VOCABULARY, (args.batch, 257), device='cuda')
    losses = {}

    def step(name):
        net = nets[name]
        net.zero_grad(set_to_none=True)
        with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
            loss, _ = net(tokens, {})
        loss.backward()
        losses[name] = loss.detach()

    res = alternate({name: (lambda n=name: step(n)) for name in nets}, args.blocks, args.module_iters)
    assert nets['fused'].last_route.name == 'fused' and nets['torch'].last_route.name == 'torch', (nets['fused'].last_route, nets['torch'].last_route)
    peak = {}
    for name in nets:
        torch.cuda.reset_peak_memory_stats()
        step(name)
        torch.cuda.synchronize()
        peak[name + '_peak_mib'] = round(torch.cuda.max_memory_allocated() / 2 ** 20)
    line = dict(case=f'llama_medium_{args.layers}_layers_step', fused_loss=round(float(losses['fused']), 5),
                torch_loss=round(float(losses['torch']), 5), iters=args.module_iters, **res, **peak)
    for net in nets.values():
        net.zero_grad(set_to_none=True)
    return line, nets


def step_launches(net, autocast, batch, static):
    """Kernel launches of one single-token step behind a cache of 8 positions, counted with the profiler (None without one)."""
    from vector_quantization_amd.kv_cache import StaticKVCache
    try:
        from torch.profiler import ProfilerActivity, profile
        with torch.no_grad(), torch.autocast('cuda', torch.bfloat16, enabled=autocast):
            cache = StaticKVCache.for_model(net._transformer.config, batch, 16, torch.bfloat16 if autocast else torch.float32, 'cuda') if static else None
            token = torch.randint(0, 1000, (batch, 1), device='cuda')
            for _ in range(8):
                _, cache, _ = net.inference(token, cache, {})
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                net.inference(token, cache, {})
                torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower())
    except Exception as err:                                                    # no profiler on this build: the count is left out
        print(f'step_launches: {err!r}', file=sys.stderr)
        return None


def generate_case(nets, autocast, args, length=None):
    """Cached generation, one token per step: ``generate`` from a class token to ``length`` tokens, every route on the same
    uniforms; the figure is microseconds per generated token."""
    import copy
    from types import SimpleNamespace
    length = length or args.generate_length[0]
    if 'decode' not in nets:
        nets['decode'] = copy.deepcopy(nets['fused'])
        nets['decode'].static_cache = True
    if 'graph' not in nets:
        nets['graph'] = copy.deepcopy(nets['decode'])
        nets['graph'].graph = True
    codebook = SimpleNamespace(start=1000, end=VOCABULARY)
    prompt = torch.randint(0, 1000, (args.generate_batch, 1), device='cuda')
    u = torch.rand(args.generate_batch, device='cuda')
    new = length - 1
    tokens = {}

    def run(name):
        with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
            tokens[name], _ = nets[name].eval().generate(prompt, length, codebook, {'sampler': {'u': u}})

    # the first call of the graph route, capture included, beside a decode call at the same moment (decode warmed by two calls)
    nets['graph'].graph = False                                                 # (drops a graph an earlier case left)
    nets['graph'].graph = True
    run('decode'); run('decode')
    torch.cuda.synchronize()
    first = {name: round(block_us(lambda n=name: run(n), 1) / new, 1) for name in ('decode', 'graph')}
    assert nets['graph']._decode_graph.captures == 1
    res = alternate({name: (lambda n=name: run(n)) for name in nets}, args.blocks, 1)
    assert nets['fused'].last_route.name == 'fused' and nets['torch'].last_route.name == 'torch' and nets['decode'].last_route.name == 'decode' \
        and nets['graph'].last_route.name == 'graph' and nets['graph']._decode_graph.captures == 1, [n.last_route for n in nets.values()]
    res = {name: {k: round(v / new, 1) for k, v in r.items()} for name, r in res.items()}
    same = float((tokens['fused'] == tokens['torch']).float().mean())
    same_decode = float((tokens['fused'] == tokens['decode']).float().mean())
    same_graph = float((tokens['decode'] == tokens['graph']).float().mean())
    launches = {name: step_launches(nets[name], autocast, args.generate_batch, name == 'decode') for name in ('fused', 'decode')}
    per_layer = {f'{name}_launches_per_layer_step': None if n is None else round(n / args.layers, 2) for name, n in launches.items()}
    return dict(case=f'llama_medium_{args.layers}_layers_generate_us_per_token', new_tokens=new, iters=1, equal_token_share=round(same, 4),
                decode_equal_token_share=round(same_decode, 4), fused_over_decode=round(res['fused']['median_us'] / res['decode']['median_us'], 2),
                graph_equal_token_share_of_decode=round(same_graph, 4),
                decode_over_graph=round(res['decode']['median_us'] / res['graph']['median_us'], 2),
                first_call=dict(first, decode_over_graph=round(first['decode'] / first['graph'], 2)), **per_layer, **res)


def generate_nets(args):
    """The two models of ``module_case`` without its training steps."""
    from vector_quantization_amd.registries import VQSMTransformerRegistry
    torch.manual_seed(0)
    config = dict(type='LlamaTransformer', transformer=dict(MEDIUM, num_hidden_layers=args.layers), vocabulary_size=VOCABULARY,
                  sampler=dict(type='BaseSampler'))
    nets = {name: VQSMTransformerRegistry.build(dict(config, fused=name == 'fused')).cuda() for name in ('fused', 'torch')}
    nets['fused'].init_weights(None)
    torch.nn.init.normal_(nets['fused']._transformer.lm_head.weight, std=0.02)
    nets['torch'].load_state_dict(nets['fused'].state_dict(), strict=True)
    return nets


def main():
    from vector_quantization_amd import functional
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--module-iters', type=int, default=5)
    ap.add_argument('--generate-batch', type=int, default=32)
    ap.add_argument('--generate-length', type=lambda t: [int(v) for v in t.split(',')], default=[65])
    ap.add_argument('--generate-only', action='store_true')
    ap.add_argument('--layers', type=int, default=MEDIUM['num_hidden_layers'])
    ap.add_argument('--skip-module', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_llama_ops.py needs an MI355X'
    R = args.batch * 257
    lines = []

    def emit(line, shape, autocast, B=args.batch):
        nbytes = line.pop('nbytes', None)
        line.setdefault('iters', args.iters)
        line.update(shape=shape, B=B, dtype='bf16_autocast' if autocast else 'fp32',
                    torch_over_fused=round(line['torch']['median_us'] / line['fused']['median_us'], 2), blocks=args.blocks)
        if nbytes:
            line['fused_gbs'] = round(nbytes / line['fused']['median_us'] / 1e3, 1)
        print(json.dumps(line), flush=True)
        lines.append(line)

    if args.generate_only:
        nets = generate_nets(args)
        for length in args.generate_length:
            for autocast in (False, True):
                emit(generate_case(nets, autocast, args, length), [args.generate_batch, 1], autocast, B=args.generate_batch)
    else:
        for autocast in (False, True):
            emit(norm_case(functional, R, MEDIUM['hidden_size'], autocast, args), [R, MEDIUM['hidden_size']], autocast)
            emit(swiglu_case(functional, R, MEDIUM['intermediate_size'], autocast, args), [R, 2 * MEDIUM['intermediate_size']], autocast)
    if not args.skip_module and not args.generate_only:
        for autocast in (False, True):
            line, nets = module_case(autocast, args)
            emit(line, [args.batch, 257], autocast)
            for length in args.generate_length:
                emit(generate_case(nets, autocast, args, length), [args.generate_batch, 1], autocast, B=args.generate_batch)
            del nets
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
