"""include/vqhip.h against its Python binding (vector_quantization_amd/_lib.py), without loading the library.

``_lib.SIGNATURES`` is read from the header's prototypes at import.  What stays a hand copy in _lib.py is held to the header
here by a C probe: a small program, generated below and compiled once with the host compiler against the header itself, prints
the layout of the five argument structs, the value of every numeric macro that has a Python twin, and every function-like
``VQHIP_*(...)`` macro (the error bounds the GPU tests assert) at sample points either side of each integer-division step.
A bound macro that is added to the header without a row in ``BOUNDS`` fails.  No compiler fails: nothing here skips.
"""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest

from vector_quantization_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')

# Both sides evaluate a bound in double arithmetic, fewer than twenty operations on positive terms with at most 2^-53 relative
# rounding each: copies that order the operations differently agree to well below 2^-48; a differing coefficient does not.
REL = 2.0 ** -48

# header macro whose Python twin carries another name (every other twin is the macro's name without VQHIP_)
TWINS = {'VERSION': 'ABI_VERSION'}

GELU, TANH = _lib.ROW_ACT_GELU, _lib.ROW_ACT_TANH
DTYPES = [(_lib.DTYPE_F32,), (_lib.DTYPE_BF16,), (_lib.DTYPE_I32,), (_lib.DTYPE_I64,), (_lib.DTYPE_F16,), (_lib.DTYPE_U8,)]
# (macro, its Python copy, sample arguments): sizes on both sides of each division step (255 / 256, 31 / 32, 3 / 4, 15 / 16,
# 2^21 - 1 / 2^21) and one large one; magnitudes are arbitrary positive numbers.  An empty sample is an object-like macro.
BOUNDS = [
    ('VQHIP_SAMPLE_DELTA', _lib.sample_delta, [(1,), (16384,), (1 << 20,)]),
    ('VQHIP_TOKEN_CE_CHAIN', _lib.token_ce_chain, [(255,), (256,), (1 << 20,)]),
    ('VQHIP_TOKEN_CE_LSE_BOUND', _lib.token_ce_lse_bound, [(255, 0.37), (256, 8.5), (1 << 20, 1000.0)]),
    ('VQHIP_TOKEN_CE_BOUND', _lib.token_ce_bound, [(255, 0.37), (256, 8.5), (1 << 20, 1000.0)]),
    ('VQHIP_TOKEN_CE_GRAD_BOUND', _lib.token_ce_grad_bound, [(255, 0.37), (256, 8.5), (1 << 20, 1000.0)]),
    ('VQHIP_COSINE_EMBED_CHAIN', _lib.cosine_embed_chain, [(31,), (32,), (1 << 16,)]),
    ('VQHIP_COSINE_EMBED_BOUND', _lib.cosine_embed_bound, [(31,), (32,), (1 << 16,)]),
    ('VQHIP_COSINE_EMBED_GRAD_BOUND', _lib.cosine_embed_grad_bound, [(31, 0.37), (32, 12.5), (1 << 16, 1e6)]),
    ('VQHIP_LPIPS_CHAIN', _lib.lpips_chain, [(3,), (4,), (512,)]),
    ('VQHIP_LPIPS_BOUND', _lib.lpips_bound, [(3, 0.37), (4, 2.25), (512, 17.0)]),
    ('VQHIP_LPIPS_GRAD_BOUND', _lib.lpips_grad_bound, [(3, 0.37, 1e10), (4, 2.25, 0.7), (512, 17.0, 31.0)]),
    ('VQHIP_BIAS_ACT_BOUND', _lib.bias_act_bound, [(0.37,), (1234.5,)]),
    ('VQHIP_FIR4_BOUND', _lib.fir4_bound, [(0.37,), (1234.5,)]),
    ('VQHIP_FIR4_ACT_BOUND', lambda a: _lib.fir4_bound(a, fused=True), [(0.37,), (1234.5,)]),
    ('VQHIP_SG2_GBIAS_CHAIN', _lib.sg2_gbias_chain, [(15,), (16,), (4097,)]),
    ('VQHIP_SG2_GBIAS_BOUND', _lib.sg2_gbias_bound, [(15, 4.0, 0.37), (16, 12.0, 99.5), (4097, 4.0, 1e5)]),
    ('VQHIP_SG2_STORE_U', _lib.sg2_store_u, DTYPES),
    ('VQHIP_GN_CHAIN', _lib.gn_chain, [(2097151,), (2097152,), (1 << 24,)]),
    ('VQHIP_GN_Q', _lib.gn_q, [(2097151, 0.37, 2.5), (2097152, 3.0, 1e3), (1 << 24, 0.01, 1e-2)]),
    ('VQHIP_GN_RHO', _lib.gn_rho, [(2097151, 1e-6), (2097152, 0.02), (1 << 24, 3e-4)]),
    ('VQHIP_ROW_GELU_BOUND', lambda t, y: _lib.row_act_bound(GELU, t, y), [(0.37, 0.2), (11.5, 11.5)]),
    ('VQHIP_ROW_GELU_GRAD_BOUND', lambda: _lib.row_act_grad_bound(GELU, 1.0, 1.0), [()]),
    ('VQHIP_ROW_TANH_BOUND', lambda y: _lib.row_act_bound(TANH, 1.0, y), [(0.37,), (0.999,)]),
    ('VQHIP_ROW_TANH_GRAD_BOUND', lambda y, d: _lib.row_act_grad_bound(TANH, y, d), [(0.37, 0.86), (0.999, 0.002)]),
]


def header_text() -> str:
    """The header without comments and with continuation lines joined (preprocessor lines kept)."""
    text = open(os.path.join(INCLUDE, 'vqhip.h')).read().replace('\\\n', ' ')
    return re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)


def object_macros() -> dict:
    """NAME -> body of every ``#define VQHIP_NAME body`` without parameters (the include guard has no body)."""
    return {n: b.strip() for n, b in re.findall(r'(?m)^[ \t]*#[ \t]*define[ \t]+VQHIP_(\w+)[ \t]+(\S.*)$', header_text())}


def function_macros() -> list:
    return re.findall(r'(?m)^[ \t]*#[ \t]*define[ \t]+(VQHIP_\w+)\(', header_text())


def twin(name: str):
    """The number _lib holds for the header's VQHIP_<name>, or None where it keeps no copy."""
    v = getattr(_lib, TWINS.get(name, name), None)
    return v if isinstance(v, (int, float)) and not isinstance(v, bool) else None


def c_literal(v) -> str:
    return repr(v) if isinstance(v, float) else str(int(v))     # repr round-trips a double; an int stays an integer expression


def probe_source() -> str:
    out = ['#include <stddef.h>', '#include <stdio.h>', '#include "vqhip.h"', 'int main(void) {']
    for typedef, cls in _lib.STRUCTS.items():
        out.append(f'    printf("sizeof {typedef} %zu\\n", sizeof({typedef}));')
        for field in cls._fields_:                              # a field the header lacks does not compile
            out.append(f'    printf("field {typedef}.{field[0]} %zu %zu\\n", offsetof({typedef}, {field[0]}), '
                       f'sizeof((({typedef} *)0)->{field[0]}));')
    for name in object_macros():
        if twin(name) is not None:
            out.append(f'    printf("const {name} %.17g\\n", (double)(VQHIP_{name}));')
    for macro, _, samples in BOUNDS:
        for i, args in enumerate(samples):
            call = f'{macro}({", ".join(map(c_literal, args))})' if args else macro
            out.append(f'    printf("bound {macro}.{i} %.17g\\n", (double)({call}));')
    return '\n'.join(out + ['    return 0;', '}', ''])


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    """key -> the numbers the compiled probe printed for it."""
    cc = shutil.which('cc') or shutil.which('clang') or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang')
    if not (os.path.isfile(cc) and os.access(cc, os.X_OK)):
        pytest.fail('no C compiler (cc, or clang of the ROCm tree): the header cannot be checked against its binding')
    d = tmp_path_factory.mktemp('binding_probe')
    src, exe = d / 'probe.c', d / 'probe'
    src.write_text(probe_source())
    res = subprocess.run([cc, '-std=c11', '-O0', '-ffp-contract=off', f'-I{INCLUDE}', str(src), '-o', str(exe)],
                         capture_output=True, text=True)
    assert res.returncode == 0, f'the probe does not compile against include/vqhip.h:\n{res.stderr}'
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    got = {}
    for line in res.stdout.splitlines():
        kind, key, *values = line.split()
        got[f'{kind} {key}'] = [float(v) for v in values]
    return got


def test_struct_layouts_are_the_headers(probe):
    typedefs = set(re.findall(r'\}\s*(vqhip_\w+_t)\s*;', header_text()))
    assert typedefs == set(_lib.STRUCTS) and len(typedefs) == 5
    classes = {v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    assert classes == set(_lib.STRUCTS.values())
    for typedef, cls in _lib.STRUCTS.items():
        assert probe[f'sizeof {typedef}'] == [ctypes.sizeof(cls)], typedef
        for field in cls._fields_:
            f = getattr(cls, field[0])
            assert probe[f'field {typedef}.{field[0]}'] == [f.offset, f.size], f'{typedef}.{field[0]}: (offset, size)'


def test_constants_equal_the_headers_macros(probe):
    checked = []
    for name, body in object_macros().items():
        want = twin(name)
        if want is None:
            continue                                            # no Python copy: listed in profiles/binding.txt
        if re.search(r'[\d.]f$', body, flags=re.I):            # a float constant: its twin is the number the fp32 holds
            want = struct.unpack('f', struct.pack('f', want))[0]
        assert probe[f'const {name}'] == [float(want)], f'VQHIP_{name} = {body}, _lib has {want!r}'
        checked.append(name)
    assert 'VERSION' in checked and {'METRIC_L2', 'METRIC_COS', 'METRIC_COS_BF16'} <= set(checked)
    assert len(checked) >= 39                                   # the twins at the time of writing: a renamed one is noticed


def test_every_bound_macro_has_a_row_and_equals_its_python_copy(probe):
    table = [macro for macro, _, _ in BOUNDS]
    assert len(table) == len(set(table))
    missing = set(function_macros()) - set(table)
    assert not missing, f'function-like macros of include/vqhip.h without a row in BOUNDS: {sorted(missing)}'
    for macro, fn, samples in BOUNDS:
        assert len(samples) >= 2 or samples == [()]
        for i, args in enumerate(samples):
            (c,), py = probe[f'bound {macro}.{i}'], float(fn(*args))
            assert c >= 0.0 and py >= 0.0
            assert abs(c - py) <= REL * max(c, py), f'{macro}{args}: header {c!r}, _lib {py!r}'
        values = [probe[f'bound {macro}.{i}'][0] for i in range(len(samples))]
        assert len(set(values)) > 1 or samples == [()], f'{macro}: the samples do not tell its arguments apart'


def declared_prototypes() -> dict:
    """name -> parameter strings, by a regex of this file's own (not _lib.parse_header)."""
    text = re.sub(r'(?m)^[ \t]*#.*$', '', header_text())
    return {n: [p.strip() for p in ps.split(',')] for n, ps in re.findall(r'\b(vqhip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)}


def test_derived_signatures_cover_the_declared_prototypes():
    protos = declared_prototypes()
    assert sorted(_lib.SIGNATURES) == sorted(protos) and len(protos) >= 108
    for name, params in protos.items():
        res, args = _lib.SIGNATURES[name]
        if params == ['void']:
            assert args == []
            continue
        assert len(args) == len(params), name
        for p, a in zip(params, args):
            pointer = a is ctypes.c_void_p or a is ctypes.c_char_p or hasattr(a, 'contents')
            assert ('*' in p) == pointer, (name, p)
            if not pointer:
                assert ctypes.sizeof(a) == (8 if p.split()[0] in ('int64_t', 'double') else 4), (name, p)
    assert _lib.SIGNATURES['vqhip_version'] == (ctypes.c_int, [])
    assert _lib.SIGNATURES['vqhip_last_error'] == (ctypes.c_char_p, [])
    assert _lib.SIGNATURES['vqhip_cvq_forward'][1] == [ctypes.POINTER(_lib.CvqForwardArgs), ctypes.c_void_p]
    assert _lib.SIGNATURES['vqhip_fsq_encode'][1][0] is ctypes.POINTER(_lib.FsqConstants)


def test_a_type_outside_the_rules_is_refused_by_name():
    with pytest.raises(_lib.VqhipError, match=r'vqhip_new.*unsigned long'):
        _lib.parse_header('int vqhip_new(const void *x, unsigned long x);')
    with pytest.raises(_lib.VqhipError, match=r'vqhip_new.*size_t'):
        _lib.parse_header('size_t vqhip_new(void);')
    with pytest.raises(_lib.VqhipError, match=r'vqhip_new.*vqhip_other_t'):
        _lib.parse_header('int vqhip_new(const vqhip_other_t *args);')
    with pytest.raises(_lib.VqhipError, match=r'not read as prototypes.*vqhip_new'):
        _lib.parse_header('int vqhip_new(int (*callback)(int));')
    assert _lib.parse_header('/* int vqhip_old(int); */ int64_t vqhip_new(int64_t n, const float *v, // int vqhip_old(int);\n float s);') \
        == {'vqhip_new': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_float])}
