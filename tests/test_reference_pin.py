"""The oracle's pin to the reference ITSELF (CPU, build container only: /root/reference cannot travel).

``oracle/ref_import.py`` executes the reference's own quantizer-path source files behind a structure-only stand-in
for todd.  These tests (a) regenerate every fixture from those files and require the committed ``tests/golden/*.npz``
to be byte-identical, (b) thereby re-run make_golden's assertions that the restatement ``oracle/torch_ref.py`` is
byte-identical to the reference on every case (it is what runs on the GPU box), (c) check the stand-in supplies no
arithmetic beyond the three documented un-vendored todd definitions, and (d) drive the product's
``integration.register_into_reference()`` against the reference's real registries.
"""
import glob
import json
import os
import re

import numpy as np
import pytest

from oracle import ref_import

# the tests that execute the reference's own files need its checkout (ref_import.REFERENCE_ROOT, VQ_REFERENCE_ROOT)
needs_reference = pytest.mark.skipif(not ref_import.available(), reason='the reference checkout is not present on this machine')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@needs_reference
def test_reference_files_are_the_ones_executed():
    ref = ref_import.load()
    want = {'vq/algorithms/vq/distances.py', 'vq/algorithms/vq/quantizers.py', 'vq/algorithms/vq/losses.py',
            'vq/algorithms/vq/utils.py', 'vq/algorithms/vq/callbacks/normalize.py', 'vq/algorithms/vq/callbacks/update.py',
            'vq/algorithms/vqgan/quantizer.py', 'vq/algorithms/vqkd/quantizers/base.py',
            'vq/algorithms/vqkd/quantizers/callbacks.py', 'vq/algorithms/cvqvae/anchors.py',
            'vq/algorithms/cvqvae/quantizer_callback.py', 'vq/tasks/image_tokenization/models/quantizers/base.py',
            'vq/tasks/image_tokenization/models/quantizers/utils/ste.py',
            'vq/tasks/image_tokenization/models/quantizers/callbacks/composed.py'}
    assert want <= set(ref.files.values())
    for mod in ref.modules.values():                       # every loaded class lives in a file under the reference root
        for name, obj in vars(mod).items():
            if isinstance(obj, type) and obj.__module__.startswith('vq.'):
                import sys
                assert sys.modules[obj.__module__].__file__.startswith(ref_import.REFERENCE_ROOT), name


@needs_reference
def test_runner_level_classes_are_the_reference_files_too():
    """tests/golden/runner_files.npz comes from the reference's Tokenizer / TokenizeCallback / metrics / LlamaGen tool."""
    import sys
    rr = ref_import.load_runners()
    for f in rr.files:
        assert os.path.isfile(os.path.join(ref_import.REFERENCE_ROOT, f)), f
    for cls in (rr.Tokenizer, rr.TokenizeCallback, rr.CodebookUsageMetric, rr.CodebookPPLMetric, rr.LlamaGenTokenizeCallback):
        assert sys.modules[cls.__module__].__file__.startswith(ref_import.REFERENCE_ROOT), cls
    assert rr.VQITCallbackRegistry._resolve('TokenizeCallback') is rr.LlamaGenTokenizeCallback      # the tool registers with force=True
    assert rr.VQITMetricRegistry._resolve('CodebookPPLMetric') is rr.CodebookPPLMetric


def test_standin_supplies_no_arithmetic_but_the_documented_three():
    """No torch/numpy arithmetic call in the stand-in outside _ToddArithmetic (ema, EMA, MSELoss(norm))."""
    src = open(ref_import.__file__).read()
    body = src.split('def _install_todd()')[1].split('# 2. the reference')[0]
    for needle in ('torch.cdist', 'einsum', 'argmin', 'softmax', 'scatter_add', 'bincount', '.normalize(', 'mse_loss',
                   'torch.exp', 'torch.sqrt'):
        assert needle not in body, f'stand-in todd computes with {needle}'
    arith = src.split('class _ToddArithmetic')[1].split('def _install_todd()')[0]
    assert 'a * decay + b * (1 - decay)' in arith and 'F.mse_loss' in arith


@needs_reference
def test_committed_fixtures_are_the_reference_outputs(tmp_path):
    """Regenerate everything from /root/reference (incl. the two-process gloo run of the reference callbacks) and
    compare with the committed files key by key, byte by byte.  make_golden asserts torch_ref == reference inside.  The
    regeneration runs in a fresh process under make_golden.PINNED_ENV, the numerics the fixtures were written with."""
    import subprocess
    import sys
    from oracle import make_golden
    if not make_golden.host_has_avx512():
        pytest.skip('the fixtures were written with AVX-512 kernels; this processor has no AVX-512')
    root = os.path.dirname(os.path.dirname(GOLDEN))           # the repository: `oracle` importable from there
    res = subprocess.run([sys.executable, '-c', 'import sys; from oracle import make_golden; make_golden.main(out_dir=sys.argv[1], quiet=True)',
                          str(tmp_path)], env=make_golden.pinned_env(), cwd=root, capture_output=True, text=True, timeout=1800)
    assert res.returncode == 0, res.stderr[-3000:]
    fresh = sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(tmp_path), '*.npz')))
    committed = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, '*.npz')))
    assert fresh == committed
    for name in fresh:
        a, b = np.load(os.path.join(str(tmp_path), name)), np.load(os.path.join(GOLDEN, name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            if k == 'spec':
                sa, sb = json.loads(str(a[k])), json.loads(str(b[k]))
                assert sb['source'] == 'reference-import' and sb['reference'], name
                sa.pop('torch', None), sb.pop('torch', None)
                assert sa == sb, name
            else:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f'{name}:{k} drifted from the reference'


def test_every_fixture_cites_reference_lines():
    """Every fixture names the reference lines it comes from; where the reference checkout is present, the files exist."""
    paths = glob.glob(os.path.join(GOLDEN, '*.npz'))
    assert paths
    for p in paths:
        spec = json.loads(str(np.load(p)['spec']))
        assert spec['source'] == 'reference-import' and spec['reference'], p
        for cite in spec['reference']:
            m = re.match(r'((?:vq|tools)/[\w/]+\.py):[\d,\-]+$', cite)
            assert m, cite
            if ref_import.available():
                assert os.path.isfile(os.path.join(ref_import.REFERENCE_ROOT, m.group(1))), cite


@needs_reference
def test_register_into_reference_registries():
    """integration.register_into_reference() against the reference's real registry classes: afterwards the reference's
    own ``VQITQuantizerRegistry.build`` of the reference's config dict returns THIS package's quantizer."""
    ref = ref_import.load()
    from vector_quantization_amd import integration, quantizers as Q
    saved = {}
    regs = dict(VQITQuantizerRegistry=ref.VQITQuantizerRegistry, VQITQuantizerDistanceRegistry=ref.VQITQuantizerDistanceRegistry,
                VQITQuantizerLossRegistry=ref.VQITQuantizerLossRegistry,
                VQITQuantizerCallbackRegistry=ref.VQITQuantizerCallbackRegistry, AnchorRegistry=ref.AnchorRegistry)
    for n, r in regs.items():
        saved[n] = dict(r._table)
    try:
        done = integration.register_into_reference()
        assert 'VQGANQuantizer' in done['VQITQuantizerRegistry']
        assert ref.VQITQuantizerRegistry._resolve('VQGANQuantizer') is Q.VQGANQuantizer
        assert ref.VQITQuantizerCallbackRegistry._resolve('CVQVAECallback') is Q.CVQVAECallback
        assert ref.AnchorRegistry._resolve('NearestAnchor') is Q.NearestAnchor
    finally:
        for n, r in regs.items():
            r._table.clear()
            r._table.update(saved[n])
