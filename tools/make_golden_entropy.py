"""Fixtures of the fused EntropyLoss from the reference's own files: writes tests/golden/entropy/*.npz.

    python tools/make_golden_entropy.py [OUT_DIR]     (needs the reference checkout; re-runs itself under make_golden's pinned env)

``oracle.ref_import.load()`` puts the reference's quantizer path on ``sys.modules``; every value below is what the reference's
``EntropyLoss`` (built through its loss registry, the way a config reaches it) returns on ``memo['distance']`` of its own
``L2Distance`` / ``CosineDistance``, and what torch autograd makes of it.  Arrays and a JSON spec only.

Cases: both metrics; temperatures 0.5, 0.01 and -1; a latent equal to a code (L2: d == 0, torch.cdist's zero subgradient) and an
all-zero latent (Cosine: F.normalize's clamp).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden, ref_import, synth  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'entropy')
CITE = ['vq/algorithms/vq/losses.py:130-153', 'vq/algorithms/vq/distances.py:28-46']
# name, metric, temperature, N, K, D, plant
CASES = [('l2_t05', 'L2', 0.5, 200, 96, 24, 'none'), ('cos_t001', 'Cosine', 0.01, 200, 96, 24, 'none'),
         ('l2_tm1_equal', 'L2', -1.0, 24, 20, 8, 'equal'), ('cos_tm1_zero', 'Cosine', -1.0, 130, 64, 32, 'zero'),
         ('l2_t001_k1000', 'L2', 0.01, 300, 1000, 30, 'none')]
PLANT_ROW, PLANT_CODE = 3, 2


def latents(seed, N, K, D, plant):
    x, w = synth.make_inputs('normal', seed, N, K, D)
    if plant == 'equal':
        v = synth.rng(seed + 5).integers(1, 4, D).astype(np.float32) * np.where(np.arange(D) % 2, 1.0, -1.0).astype(np.float32)
        x[PLANT_ROW] = v
        w[PLANT_CODE] = v
    if plant == 'zero':
        x[PLANT_ROW] = 0.0
    return x, w


def run_case(ref, name, metric, T, N, K, D, plant, seed) -> dict:
    x, w = latents(seed, N, K, D, plant)
    xt = torch.from_numpy(x).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    d = getattr(ref, f'{metric}Distance')()(xt, wt)
    entropy = ref.VQITQuantizerLossRegistry.build(dict(type='EntropyLoss', temperature=T))
    loss = entropy(None, xt, dict(distance=d))
    loss.backward()
    return dict(x=x, w=w, loss=np.float32(loss.item()), grad_x=xt.grad.numpy(), grad_w=wt.grad.numpy(),
                spec=json.dumps(dict(name=name, metric=metric, temperature=T, N=N, K=K, D=D, plant=plant, seed=seed,
                                     plant_row=PLANT_ROW, plant_code=PLANT_CODE, source='reference-import',
                                     torch=torch.__version__, reference=CITE)))


def main(out_dir=None) -> None:
    if not ref_import.available():
        sys.exit('tools/make_golden_entropy.py needs the reference checkout')
    make_golden.check_pinned()
    out = out_dir or OUT
    os.makedirs(out, exist_ok=True)
    torch.set_num_threads(make_golden.FIXTURE_THREADS)
    ref = ref_import.load()
    for i, (name, metric, T, N, K, D, plant) in enumerate(CASES):
        np.savez_compressed(os.path.join(out, name + '.npz'), **run_case(ref, name, metric, T, N, K, D, plant, 940 + i))


if __name__ == '__main__':
    if any(os.environ.get(k) != v for k, v in make_golden.PINNED_ENV.items()):      # a fresh process with the pinned numerics
        import subprocess
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=make_golden.pinned_env()).returncode)
    main(sys.argv[1] if len(sys.argv) > 1 else None)
