"""GPU checks of VQKDEncoder / VQKDDecoder: the fused route (HIP add + LayerNorm and bias-activation, framework GEMMs and SDPA)
against the torch route (the reference's lines), on a small pair, in fp32 (TF32 off) and under bf16 autocast: outputs, the
``last_parameter`` gradient taken twice, and every parameter gradient.

The tolerance is not a fixed number.  The torch route in float64 is the yardstick; per tensor, the fused route's error against it
(largest difference over the yardstick's largest magnitude) may be at most 4 times the fp32 / bf16 torch route's own error against
it: the margin covers the different GEMM and SDPA algorithms the two routes select.  Only where the torch route reproduces the
yardstick exactly (error 0) does one ulp of the arithmetic's dtype (2^-23 for fp32, 2^-8 under bf16 autocast) stand in for it.
Both numbers are printed; profiles/vqkd_autoencoder.txt records a run."""
import copy
import io

import pytest
import torch

import vector_quantization_amd as vqa
from vector_quantization_amd import tokenization

pytestmark = pytest.mark.gpu

SMALL_ENCODER = dict(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, out_chans=8)
SMALL_DECODER = dict(img_size=2, in_chans=8, embed_dim=64, depth=1, num_heads=2, out_chans=16)


def _pair(fused):
    torch.manual_seed(5)
    pair = torch.nn.ModuleList([vqa.VQKDEncoder(**SMALL_ENCODER, fused=fused), vqa.VQKDDecoder(**SMALL_DECODER, fused=fused)])
    for m in pair:
        m.init_weights()
    with torch.no_grad():                                                       # init_weights leaves zeros and ones: give every parameter a value
        for m in pair.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
            if isinstance(m, torch.nn.Linear) and m.bias is not None:
                m.bias.normal_(0.0, 0.2)
            if isinstance(m, vqa.vqkd_autoencoders.Attention):
                m.q_bias.normal_(0.0, 0.2)
                m.v_bias.normal_(0.0, 0.2)
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(10.0)                                             # (std 0.2: branches of the size of the stream)
    return pair.cuda()


def _run(pair, image, autocast):
    pair.zero_grad()
    with torch.autocast('cuda', torch.bfloat16, enabled=autocast):
        z, _ = pair[0](image, {})
        out, _ = pair[1](z, {})
    loss = out.double().square().mean() + z.double().square().mean()
    last = pair[1].last_parameter
    g1, = torch.autograd.grad(loss, last, retain_graph=True)
    g2, = torch.autograd.grad(loss, last, retain_graph=True)
    loss.backward()
    got = {n: p.grad.detach().double().clone() for n, p in pair.named_parameters()}
    assert torch.equal(g1, g2)
    got.update(out=out.detach().double(), z=z.detach().double(), last_parameter=g1.double())
    return got


def _err(a, want):
    return float((a - want).abs().max() / want.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16_autocast'])
def test_fused_route_against_torch_route_with_float64_as_the_yardstick(autocast):
    keep = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    try:
        fused, plain = _pair(True), _pair(False)
        plain.load_state_dict(fused.state_dict(), strict=True)
        exact = copy.deepcopy(plain).double()
        image = torch.randn(3, 3, 32, 32, device='cuda')
        want = _run(exact, image.double(), False)
        assert exact[0].last_route.name == 'torch'
        base = _run(plain, image, autocast)
        assert plain[0].last_route.why == plain[1].last_route.why == 'fused=False'
        got = _run(fused, image, autocast)
        assert fused[0].last_route.name == 'fused' and fused[1].last_route.name == 'fused', (fused[0].last_route, fused[1].last_route)
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = keep
    floor = 2.0 ** -8 if autocast else 2.0 ** -23
    worst = (0.0, '')
    for name in want:
        assert torch.isfinite(got[name]).all(), name
        e_torch, e_fused = _err(base[name], want[name]), _err(got[name], want[name])
        ratio = e_fused / max(e_torch, floor)
        worst = max(worst, (ratio, name))
        print(f'autocast={autocast} {name}: torch route {e_torch:.3e}, fused route {e_fused:.3e} of the float64 yardstick, ratio {ratio:.2f}')
    print(f'autocast={autocast}: worst ratio {worst[0]:.2f} at {worst[1]}')
    for name in want:
        e_torch = _err(base[name], want[name])
        assert _err(got[name], want[name]) <= 4.0 * (e_torch if e_torch > 0.0 else floor), name


def test_checkpoints_cross_the_routes_and_the_distillation_loss_takes_the_map():
    fused, plain = _pair(True), _pair(False)
    for src, dst in ((fused, plain), (plain, fused)):
        with torch.no_grad():
            for p in src.parameters():
                p.add_(0.01)
        buf = io.BytesIO()
        torch.save(src.state_dict(), buf)
        buf.seek(0)
        assert dst.load_state_dict(torch.load(buf), strict=True).missing_keys == []
        assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))
    image = torch.randn(2, 3, 32, 32, device='cuda')
    z, _ = fused[0](image, {})
    out, _ = fused[1](z, {})
    assert z.shape == (2, 8, 2, 2) and out.shape == (2, 16, 2, 2) and fused[1].last_route.name == 'fused'
    loss = vqa.CosineEmbeddingLoss()
    target = torch.randn(2, 4, 16, device='cuda')
    value = tokenization.distill_loss(loss, out, target)
    want = torch.nn.functional.cosine_embedding_loss(out.flatten(2).transpose(1, 2).reshape(-1, 16).double(), target.reshape(-1, 16).double(),
                                                     torch.ones(8, device='cuda', dtype=torch.float64))
    assert abs(float(value) - float(want)) <= 1e-5
    value.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in fused.parameters())
    # a 48 x 48 image interpolates the position embedding on the fused route too
    z, _ = fused[0](torch.randn(1, 3, 48, 48, device='cuda'), {})
    assert z.shape == (1, 8, 3, 3) and fused[0].last_route.name == 'fused'
