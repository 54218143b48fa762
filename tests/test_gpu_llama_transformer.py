"""LlamaTransformer on the GPU: the fused walk (HIP add + RMS norm and SwiGLU between the framework's GEMMs and attention) against
the torch route - transformers' own forward, what the class ran before the kernels - on the tiny model of tests/llama_models.py,
in fp32 and under bf16 autocast: training forward + backward and cached generation through the sampler.

The yardstick is the float64 model on the CPU (llama_models.exact64).  Both routes are evaluations of the same network in the
same precision that differ in summation order (and, under autocast, in fewer bf16 roundings on the fused route), so the fused
route's worst error against the float64 values may be at most twice the torch route's, for the logits, the loss and every
parameter gradient."""
import copy
from types import SimpleNamespace

import pytest
import torch

from vector_quantization_amd.quantizers import routes

from llama_models import build_tiny, exact64

pytestmark = pytest.mark.gpu

TOKENS = torch.randint(0, 48, (3, 9), generator=torch.Generator().manual_seed(2))
_REFERENCE = {}


def reference():
    """(the fp32 model on the CPU, the float64 logits, loss and parameter gradients): computed once, shared, left unchanged."""
    if not _REFERENCE:
        t = build_tiny()
        t64 = exact64(t)
        loss, memo = t64(TOKENS, {})
        loss.backward()
        _REFERENCE.update(model=t, logits=memo['logits'].detach(), loss=loss.detach(),
                          grads={k: p.grad.clone() for k, p in t64.named_parameters()})
    return _REFERENCE


def step(model, autocast):
    """(logits, loss, {name: grad}) of one training step on the GPU."""
    model.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        loss, memo = model(SimpleNamespace(tokens=TOKENS.cuda()), {})
    loss.backward()
    torch.cuda.synchronize()
    return memo['logits'].detach().cpu(), loss.detach().cpu(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


def worst(a, b):
    return float((a.double() - b).abs().max())


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16-autocast'])
def test_training_step_is_as_close_to_float64_as_the_torch_route(autocast):
    want = reference()
    fused = copy.deepcopy(want['model']).cuda().train()
    plain = copy.deepcopy(want['model']).cuda().train()
    plain.fused = False
    lf, ff, gf = step(fused, autocast)
    lt, ft, gt = step(plain, autocast)
    assert fused.last_route == routes.Route('fused') and plain.last_route == routes.Route('torch', 'fused=False')
    assert fused._loss.last_route.name == 'fused'
    assert lf.dtype == (torch.bfloat16 if autocast else torch.float32) and lf.shape == (3, 9, 48)
    rows = [('logits', worst(lf, want['logits']), worst(lt, want['logits'])), ('loss', worst(ff, want['loss']), worst(ft, want['loss']))]
    assert set(gf) == set(gt) == set(want['grads'])
    rows += [(k, worst(gf[k], want['grads'][k]), worst(gt[k], want['grads'][k])) for k in want['grads']]
    failed = []
    for name, e_fused, e_torch in rows:
        print(f'{"autocast" if autocast else "fp32"} {name}: fused {e_fused:.3e}, torch {e_torch:.3e}')
        if not e_fused <= 2 * e_torch:
            failed.append((name, e_fused, e_torch))
    assert not failed, failed


def test_cached_generation_equals_the_torch_route_in_fp32():
    """Tokens generated under a fixed memo['u'] are equal on both routes; every step of the loop runs the fused walk."""
    want = reference()
    fused = copy.deepcopy(want['model']).cuda().eval()
    plain = copy.deepcopy(want['model']).cuda().eval()
    plain.fused = False
    codebook = SimpleNamespace(start=8, end=48)
    prompt = torch.tensor([[1], [2], [3], [1]]).cuda()
    u = torch.rand(4, generator=torch.Generator().manual_seed(6)).cuda()
    a, _ = fused.generate(prompt, 9, codebook, {'sampler': {'u': u}})
    assert fused.last_route == routes.Route('fused') and fused.sampler.last_route.name == 'fused'
    b, _ = plain.generate(prompt, 9, codebook, {'sampler': {'u': u}})
    assert plain.last_route.name == 'torch'
    assert a.shape == (4, 9) and torch.equal(a[:, :1], prompt) and int(a[:, 1:].min()) >= 8 and torch.equal(a, b)
    # the cached logits against the float64 model's uncached pass over the generated sequence
    t64 = exact64(want['model'])
    full = t64._transformer(a.cpu())['logits']
    e_fused = e_torch = 0.0
    for model in (fused, plain):
        cache, worst_e = None, 0.0
        for lo, hi in ((0, 5), (5, 6), (6, 7), (7, 8), (8, 9)):
            logits, cache, _ = model.inference(a[:, lo:hi], cache, {})
            worst_e = max(worst_e, worst(logits.cpu(), full[:, lo:hi]))
        if model is fused:
            e_fused = worst_e
            assert model.last_route == routes.Route('fused')
        else:
            e_torch = worst_e
    print(f'cached logits: fused {e_fused:.3e}, torch {e_torch:.3e}')
    assert e_fused <= 2 * e_torch


def test_cached_generation_under_autocast_runs_the_fused_route():
    fused = copy.deepcopy(reference()['model']).cuda().eval()
    codebook = SimpleNamespace(start=8, end=48)
    prompt = torch.tensor([[1], [2]]).cuda()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        tokens, _ = fused.generate(prompt, 6, codebook, {'sampler': {'u': torch.tensor([0.25, 0.75]).cuda()}})
    assert fused.last_route == routes.Route('fused') and tokens.shape == (2, 6) and int(tokens[:, 1:].min()) >= 8


def test_float64_parameters_take_the_torch_route_on_the_gpu():
    model = copy.deepcopy(reference()['model']).cuda().double()
    loss, memo = model(TOKENS.cuda(), {})
    assert model.last_route.name == 'torch' and 'float64' in model.last_route.why and 'parameters' in model.last_route.why
    assert memo['logits'].dtype == torch.float64 and torch.isfinite(loss)
    assert routes.llama_why(model, TOKENS.cuda()) == model.last_route
