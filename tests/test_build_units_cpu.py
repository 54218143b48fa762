"""The translation units of libvqhip, read from the sources alone (nothing is compiled).

csrc/Makefile's UNITS is the only list of sources; every unit is compiled on its own and the objects are linked into one
library.  What keeps that sound: the list and the directory agree, a kernel header that defines a non-template ``__global__``
kernel is compiled into one unit alone (twice would be two definitions of one symbol at link time), and every function the
public header declares is defined by one unit.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vector_quantization_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'vqhip.h')


def _read(path):
    with open(path, encoding='utf-8') as f:
        return f.read()


def _code(text):
    """the text without comments"""
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _units():
    m = re.search(r'^UNITS\s*:?=\s*(.*)$', _read(os.path.join(CSRC, 'Makefile')), flags=re.M)
    assert m, 'csrc/Makefile has no UNITS line'
    return m.group(1).split()


def _reachable(path, seen=None):
    """the files under csrc/ that `path` includes with #include "...", followed transitively"""
    seen = set() if seen is None else seen
    for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _read(path), flags=re.M):
        inc = os.path.join(CSRC, name)
        if name not in seen and os.path.isfile(inc):
            seen.add(name)
            _reachable(inc, seen)
    return seen


def _has_plain_kernel(text):
    """a __global__ definition that no template<> introduces"""
    code = _code(text)
    for m in re.finditer(r'__global__', code):
        head = code[:m.start()]
        start = max(head.rfind(';'), head.rfind('}'))       # the end of the item in front
        if not re.search(r'\btemplate\s*<', head[start + 1:]):
            return True
    return False


def test_every_unit_has_a_source():
    units = _units()
    assert len(units) == len(set(units)), 'a unit is listed twice'
    missing = [u for u in units if not os.path.isfile(os.path.join(CSRC, u + '.hip'))]
    assert not missing, f'UNITS without a .hip file: {missing}'


def test_every_source_is_a_unit():
    sources = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith('.hip'))
    unlisted = [s for s in sources if s not in _units()]
    assert not unlisted, f'.hip files that csrc/Makefile does not build: {unlisted}'


def test_plain_kernels_are_compiled_once():
    included = {u: _reachable(os.path.join(CSRC, u + '.hip')) for u in _units()}
    headers = sorted(f for f in os.listdir(CSRC) if re.fullmatch(r'vqhip_\w+_kernels\.h', f))
    assert headers, 'no kernel headers found'
    checked = 0
    for h in headers:
        if not _has_plain_kernel(_read(os.path.join(CSRC, h))):
            continue
        checked += 1
        owners = sorted(u for u, inc in included.items() if h in inc)
        assert len(owners) == 1, f'{h} defines a non-template __global__ kernel and is compiled into {owners or "no unit"}'
    assert checked, 'the search for non-template kernels found none: it no longer reads the sources as they are written'


def test_every_entry_point_is_defined_once():
    declared = re.findall(r'^(?:int|int64_t) (vqhip_\w+)\(', _code(_read(HEADER)), flags=re.M)
    assert len(declared) > 100 and len(declared) == len(set(declared)), 'the prototypes of include/vqhip.h'
    defined = {}
    for u in _units():
        # a definition: the parameter list closes in front of an opening brace (a prototype ends in a semicolon)
        for name in re.findall(r'^(?:int|int64_t) (vqhip_\w+)\([^;{]*\)\s*\{', _code(_read(os.path.join(CSRC, u + '.hip'))), flags=re.M):
            defined.setdefault(name, []).append(u)
    wrong = {n: defined.get(n, []) for n in declared if len(defined.get(n, [])) != 1}
    assert not wrong, f'entry points not defined by exactly one unit: {wrong}'
