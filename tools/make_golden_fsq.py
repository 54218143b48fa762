"""Fixtures of FiniteScalarQuantizer from the reference's own files: writes tests/golden/fsq/*.npz.

    python tools/make_golden_fsq.py [OUT_DIR]        (needs the reference checkout; re-runs itself under make_golden's pinned env)

``oracle.ref_import.load()`` puts the reference's quantizer path on ``sys.modules``; the two packages FSQ lives in
(``vq.algorithms.sq``, ``vq.algorithms.fsq``) are then added as bare package modules that do what their ``__init__.py`` does
(``from .quantizers import *``), so that vq/algorithms/sq/quantizers.py and vq/algorithms/fsq/quantizers.py run unchanged
and register into the reference's own ``VQITQuantizerRegistry``.  Every array below is what those classes return.

Cases: the levels of the two shipped configs (configs/fsq/model.py:13-16) and three others, one of them also with eps=1e-2;
fp32 and bf16 latents with rows planted within 2^-17 of a rounding boundary of t and rows of +-inf, NaN, +-0 and +-1e30; a
fixed upstream gradient and the reference's x.grad; the decode (no memo z) of an int64 token list with negative and >= K
tokens; the embeddings and state-dict keys of both shipped configs.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden, ref_import  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'fsq')
CITE = ['vq/algorithms/fsq/quantizers.py:17-150', 'vq/algorithms/sq/quantizers.py:1-12',
        'vq/tasks/image_tokenization/models/quantizers/base.py:120-182']
SHIPPED = {'fsq_8000': [8, 8, 5, 5, 5], 'fsq_64000': [8, 8, 8, 5, 5, 5]}          # configs/fsq/model.py:13-16
CASES = [('l88555', [8, 8, 5, 5, 5], 1e-3), ('l888555', [8, 8, 8, 5, 5, 5], 1e-3), ('l7555', [7, 5, 5, 5], 1e-3),
         ('l333', [3, 3, 3], 1e-3), ('l1694', [16, 9, 4], 1e-3), ('l7555_eps1e2', [7, 5, 5, 5], 1e-2)]
N_RANDOM, N_PLANTED = 192, 64
SPECIALS = [float('inf'), float('-inf'), float('nan'), 0.0, -0.0, 1e30, -1e30]


def load_fsq() -> types.SimpleNamespace:
    """The reference's ScalarQuantizer / FiniteScalarQuantizer, from their files, registered in its registry."""
    ref = ref_import.load()
    for pkg in ('vq.algorithms.sq', 'vq.algorithms.fsq'):               # sq/__init__.py:1, fsq/__init__.py:1
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, *pkg.split('.'))]
            sys.modules[pkg] = m
            sub = importlib.import_module(pkg + '.quantizers')
            m.__all__ = list(sub.__all__)
            for n in sub.__all__:
                setattr(m, n, getattr(sub, n))
            setattr(sys.modules['vq.algorithms'], pkg.rsplit('.', 1)[1], m)
    sq, fsq = sys.modules['vq.algorithms.sq'], sys.modules['vq.algorithms.fsq']
    files = {n: os.path.relpath(sys.modules[n + '.quantizers'].__file__, ref_import.REFERENCE_ROOT) for n in (sq.__name__, fsq.__name__)}
    return types.SimpleNamespace(ref=ref, ScalarQuantizer=sq.ScalarQuantizer, FiniteScalarQuantizer=fsq.FiniteScalarQuantizer,
                                 files=files)


def build(ns, levels, eps=None):
    cfg = dict(type='FiniteScalarQuantizer', num_scalars_per_channel=list(levels))
    if eps is not None:
        cfg['eps'] = eps
    return ns.ref.build_quantizer(cfg)


def planted_rows(levels, eps, n, gen) -> np.ndarray:
    """Latents whose t lies within 2^-17 of a half-integer (a rounding boundary), channel by channel (float64, then fp32)."""
    L = np.array(levels, dtype=np.float64)
    M = (L - 1) * (1 - eps)
    odd = (L - 1) % 2
    h = np.floor(L / 2)
    c = np.arctanh(odd / M)
    rows = np.empty((n, len(levels)), dtype=np.float64)
    for i in range(len(levels)):
        ks = [k for k in range(-int(h[i]), int(h[i])) if abs((2 * (k + 0.5) + odd[i]) / M[i]) < 1 - 1e-6]   # boundaries in t's range
        k = gen.choice(np.array(ks), size=n)
        t = k + 0.5 + gen.uniform(-2.0 ** -17, 2.0 ** -17, size=n)
        y = (2 * t + odd[i]) / M[i]
        rows[:, i] = np.arctanh(y) - c[i]
    return rows.astype(np.float32)


def latents(levels, eps, seed) -> np.ndarray:
    gen = np.random.default_rng(seed)
    C = len(levels)
    x = (gen.standard_normal((N_RANDOM, C)) * 1.5).astype(np.float32)
    special = np.array([[v] * C for v in SPECIALS], dtype=np.float32)
    special[:, 0] = 0.25                                                 # the other channels of a special row stay ordinary
    return np.concatenate([x, planted_rows(levels, eps, N_PLANTED, gen), special])


def run_case(ns, name, levels, eps, seed) -> dict:
    q = build(ns, levels, eps)
    x32 = latents(levels, eps, seed)
    g = np.random.default_rng(seed + 1).standard_normal(x32.shape).astype(np.float32)
    rec = {}
    for tag, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
        x = torch.from_numpy(x32).to(dtype).requires_grad_(True)
        z, loss, memo = q(x, {})
        z.backward(torch.from_numpy(g))
        quant = memo['quant']
        assert quant.dtype == torch.int32 and z.dtype == torch.float32
        rec[f'{tag}_x'] = x.detach().float().numpy()                     # bf16 values are exact in fp32
        rec[f'{tag}_quant'] = quant.numpy()
        rec[f'{tag}_z'] = z.detach().numpy()
        rec[f'{tag}_grad'] = x.grad.float().numpy()
        assert memo['decode']['z'] is memo['encode']['z'] is z                  # fsq/quantizers.py:148-149
    rec['g'] = g
    K = q.codebook_size
    tokens = torch.tensor([0, 1, K - 1, K, K + 1, 2 * K + 3, -1, -2, -K, -K - 1, 12345 % K, (1 << 31) - 1, -(1 << 31), (1 << 40) + 7],
                          dtype=torch.int64)
    z_dec, _ = q.decode(tokens, {})
    rec['decode_tokens'] = tokens.numpy()
    rec['decode_z'] = z_dec.numpy()
    rec['spec'] = json.dumps(dict(name=name, levels=list(levels), eps=eps, seed=seed, N=int(x32.shape[0]), n_random=N_RANDOM,
                                  n_planted=N_PLANTED, specials=[repr(v) for v in SPECIALS], K=K, source='reference-import',
                                  torch=torch.__version__, reference=CITE))
    return rec


def main(out_dir=None) -> None:
    if not ref_import.available():
        sys.exit('tools/make_golden_fsq.py needs the reference checkout')
    make_golden.check_pinned()
    out = out_dir or OUT
    os.makedirs(out, exist_ok=True)
    torch.set_num_threads(make_golden.FIXTURE_THREADS)
    ns = load_fsq()
    for seed, (name, levels, eps) in enumerate(CASES):
        np.savez_compressed(os.path.join(out, name + '.npz'), **run_case(ns, name, levels, eps, 100 + seed))
    for name, levels in SHIPPED.items():
        q = build(ns, levels)
        sd = q.state_dict()
        assert list(sd) == ['_embeddings'] and torch.equal(sd['_embeddings'], q.embeddings)
        np.savez_compressed(os.path.join(out, name + '.npz'), embeddings=q.embeddings.numpy(),
                            state_dict_keys=np.array(list(sd)), codebook_size=q.codebook_size, embedding_dim=q.embedding_dim,
                            spec=json.dumps(dict(name=name, levels=levels, source='reference-import', torch=torch.__version__,
                                                 reference=CITE[:1] + ['configs/fsq/model.py:13-16'])))


if __name__ == '__main__':
    if any(os.environ.get(k) != v for k, v in make_golden.PINNED_ENV.items()):      # a fresh process with the pinned numerics
        import subprocess
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=make_golden.pinned_env()).returncode)
    main(sys.argv[1] if len(sys.argv) > 1 else None)
