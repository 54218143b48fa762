#!/usr/bin/env python3
"""Do two builds of libvqhip hold the same device code?  usage: isa_same.py <dirA> <dirB> [-v]

Each directory holds the gfx950 listings of one build (VQ_KEEP_TEMPS=1 bash vector_quantization_amd/csrc/build.sh -> build/asm/*gfx950.s,
one per translation unit).  For every device function found on either side — kernels and the few functions the compiler did not
inline — the tool reports whether both sides define it exactly once, whether the instruction text is the same, and for kernels
whether the .amdhsa_* resource lines (VGPRs, SGPRs, LDS, scratch, ...) and the compiler's .set <symbol>.<resource> lines are the
same.  Comments and debug directives are dropped and local labels are renumbered in order of appearance, so a function may move
between translation units, or inside one, without showing up.  The comparison is textual: it looks for no particular instruction.
Exit status 0 only if nothing differs, nothing is missing and nothing is defined twice."""
import glob, os, re, sys

SKIP = ('.loc', '.file', '.cfi_', '.section', '.text', '.ident', '.addrsig')
LABEL = re.compile(r'\.L[A-Za-z_]+\d+(?:_\d+)*')


def functions(directory):
    """name -> list of (instruction text, resource text, is_kernel), one entry per definition"""
    files = sorted(glob.glob(os.path.join(directory, '*gfx950.s')))
    if not files:
        sys.exit(f'isa_same: no *gfx950.s under {directory}')
    found = {}
    for path in files:
        lines = open(path).read().split('\n')
        declared = {m.group(1) for l in lines for m in [re.match(r'\s*\.type\s+(\S+),@function', l)] if m}
        sets = {}                                        # symbol -> its `.set symbol.field, value` lines
        for l in lines:
            m = re.match(r'\s*\.set\s+(\S+)\.(\w+),\s*(.*)', l)
            if m and m.group(1) in declared:
                sets.setdefault(m.group(1), []).append(f'{m.group(2)} = {m.group(3).strip()}')
        i = 0
        while i < len(lines):
            m = re.match(r'(\S+):', lines[i])
            if not (m and m.group(1) in declared):
                i += 1
                continue
            name, text, res, labels, in_desc, kernel = m.group(1), [], [], {}, False, False
            i += 1
            while i < len(lines) and not re.match(r'\.Lfunc_end\d+:', lines[i]):
                l = lines[i].split(';')[0].strip()
                i += 1
                if l.startswith('.amdhsa_kernel'):
                    in_desc = kernel = True
                elif l.startswith('.end_amdhsa_kernel'):
                    in_desc = False
                elif in_desc:
                    res.append(' '.join(l.split()))
                elif l and not l.startswith(SKIP):
                    text.append(LABEL.sub(lambda t: labels.setdefault(t.group(0), f'.L{len(labels)}'), ' '.join(l.split())))
            res += sets.get(name, [])
            found.setdefault(name, []).append(('\n'.join(text), '\n'.join(res), kernel))
    return found


def main():
    args = [a for a in sys.argv[1:] if a != '-v']
    verbose = '-v' in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = functions(args[0]), functions(args[1])
    bad = 0
    for name in sorted(set(a) | set(b)):
        da, db = a.get(name, []), b.get(name, [])
        kind = 'kernel' if any(d[2] for d in da + db) else 'function'
        notes = []
        if len(da) != 1 or len(db) != 1:
            notes.append(f'defined {len(da)} x in A, {len(db)} x in B')
        if da and db:
            if any(x[0] != y[0] for x in da for y in db):
                notes.append('instructions differ')
            if any(x[1] != y[1] for x in da for y in db):
                notes.append('resources differ')
        bad += bool(notes)
        if notes or verbose:
            print(f'{"DIFF" if notes else "same"} {kind:8s} {name[:140]}' + (': ' + '; '.join(notes) if notes else ''))
    nk = sum(1 for n in set(a) | set(b) if any(d[2] for d in a.get(n, []) + b.get(n, [])))
    print(f'isa_same: {len(set(a) | set(b))} device functions ({nk} kernels), {bad} with differences')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
