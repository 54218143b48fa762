"""tests/golden/fsq/ pinned to the reference itself (CPU; needs the reference checkout and AVX-512, like
tests/test_reference_pin.py): the fixtures regenerate byte for byte from vq/algorithms/{sq,fsq}/quantizers.py, those classes
come from the reference's files, and register_into_reference() puts this package's FiniteScalarQuantizer in their place."""
import glob
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import make_golden, ref_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'fsq')
TOOL = os.path.join(ROOT, 'tools', 'make_golden_fsq.py')

pytestmark = pytest.mark.skipif(not ref_import.available(), reason='the reference checkout is not present on this machine')


def _in_fresh_process(body: str) -> None:
    """Run ``body`` in a child process: loading the reference puts its modules on sys.modules, which must not leak into the
    other tests of this session (tests/test_host_cpu.py expects the reference to be absent)."""
    prelude = ('import importlib.util, sys\n'
               f'spec = importlib.util.spec_from_file_location("make_golden_fsq", {TOOL!r})\n'
               'tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)\n'
               'ns = tool.load_fsq(); ref = ns.ref\n')
    res = subprocess.run([sys.executable, '-c', prelude + body], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]


def test_fsq_fixtures_are_the_reference_outputs(tmp_path):
    if not make_golden.host_has_avx512():
        pytest.skip('the fixtures were written with AVX-512 kernels; this processor has no AVX-512')
    res = subprocess.run([sys.executable, TOOL, str(tmp_path)], env=make_golden.pinned_env(), cwd=ROOT, capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    fresh = sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(tmp_path), '*.npz')))
    committed = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, '*.npz')))
    assert fresh == committed and len(committed) == 8
    for name in fresh:
        a, b = np.load(os.path.join(str(tmp_path), name)), np.load(os.path.join(GOLD, name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            if k == 'spec':
                sa, sb = json.loads(str(a[k])), json.loads(str(b[k]))
                assert sb['source'] == 'reference-import' and sb['reference'], name
                sa.pop('torch', None), sb.pop('torch', None)
                assert sa == sb, name
            else:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f'{name}:{k} drifted from the reference'


def test_fsq_classes_are_the_reference_files():
    _in_fresh_process(f"""
import glob, json, os
import numpy as np
from oracle import ref_import
assert ns.files == {{'vq.algorithms.sq': 'vq/algorithms/sq/quantizers.py', 'vq.algorithms.fsq': 'vq/algorithms/fsq/quantizers.py'}}, ns.files
for cls in (ns.ScalarQuantizer, ns.FiniteScalarQuantizer):
    assert sys.modules[cls.__module__].__file__.startswith(ref_import.REFERENCE_ROOT), cls
assert ref.VQITQuantizerRegistry._resolve('FiniteScalarQuantizer') is ns.FiniteScalarQuantizer
for p in glob.glob(os.path.join({GOLD!r}, '*.npz')):
    for cite in json.loads(str(np.load(p)['spec']))['reference']:
        assert os.path.isfile(os.path.join(ref_import.REFERENCE_ROOT, cite.split(':')[0])), cite
""")


def test_register_into_reference_replaces_fsq():
    _in_fresh_process("""
from vector_quantization_amd import integration, quantizers as Q
assert ref.VQITQuantizerRegistry._resolve('FiniteScalarQuantizer') is ns.FiniteScalarQuantizer
done = integration.register_into_reference()
assert {'ScalarQuantizer', 'FiniteScalarQuantizer'} <= set(done['VQITQuantizerRegistry'])
assert ref.VQITQuantizerRegistry._resolve('FiniteScalarQuantizer') is Q.FiniteScalarQuantizer
assert ref.VQITQuantizerRegistry._resolve('ScalarQuantizer') is Q.ScalarQuantizer
""")
