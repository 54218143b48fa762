"""The max3 / med3 top-2 network of csrc/vqhip_top2.h against the sequential per-score update, bit for bit, on the CPU.

A stand-alone C++ program is built around the header's host path (v_max3_f32 / v_med3_f32 for operands that are no NaN, as
MI355X computes them: the maximum orders -0 below +0, and so does the median in finding the largest of its three) and folds
the same pools both ways: the network (top2_fold8 / top2_fold4) and `b2 = med3(b1, b2, v); b1 = max(b1, v)` score by score.

Pools.  A pool is (b1 >= b2, eight — or four — scores); every finite value carries the tag of its position in the low four
mantissa bits as the kernel writes it (mask 0xFFFFFFF0, id e), b1 and b2 carry tags of earlier tiles.  -inf stands as it is at
any position (a tagged -inf would be a NaN, which is out of contract; the trackers start from the bare value).
  1. exhaustive: every position over {-inf, -2, -1, -0.0, +0.0, 1, 2}.  7^10 pools are too many, so for the 8-score form
     s1 runs over {-inf, -0.0, 2} and s4 over {-inf, +0.0, 1}; the 28 ordered (b1, b2) pairs and the other six scores run over
     all seven values, once with b1 and b2 at tag 0 (where the two zeros stay two bit patterns) and once with tags that
     change from pool to pool.  The 4-score form is exhaustive in all six positions and all 64 tag pairs of (b1, b2).
  2. random: 400 000 pools of random float32 values over the whole exponent range with planted duplicates (a score copied
     to other positions, b1 or b2 copied into the scores with its own tag kept, so that equal BITS meet), both forms.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vector_quantization_amd', 'csrc')

PROGRAM = r'''
#include <math.h>
#include <stdio.h>
#include "vqhip_top2.h"

static void seq(float &b1, float &b2, float v) { b2 = top2_med3(b1, b2, v); b1 = top2_max(b1, v); }
static bool same(float a, float b) { return top2_bits(a) == top2_bits(b); }
static void order(float &b1, float &b2) {      // b1 >= b2 in the maximum's order (+0 above -0)
    if (!same(top2_max(b1, b2), b1)) { const float x = b1; b1 = b2; b2 = x; }
}
static float tagged(float v, unsigned e) { return (isinf(v) && v < 0) ? v : top2_tag(v, e); }

static unsigned long long rs = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (unsigned)(rs >> 32); }
static float rnd_float() {                     // any finite float32, all exponents
    for (;;) {
        unsigned b = rnd();
        if (((b >> 23) & 0xFF) != 0xFF) { float f; memcpy(&f, &b, 4); return f; }
    }
}

static long long bad8 = 0, bad4 = 0, shown = 0;
static void check8(float b1, float b2, const float (&s)[8]) {
    float n1 = b1, n2 = b2, q1 = b1, q2 = b2;
    top2_fold8(n1, n2, s);
    for (int e = 0; e < 8; ++e) seq(q1, q2, s[e]);
    if (!same(n1, q1) || !same(n2, q2)) {
        ++bad8;
        if (shown++ < 5) {
            printf("mismatch8 b1 %08x b2 %08x s", top2_bits(b1), top2_bits(b2));
            for (int e = 0; e < 8; ++e) printf(" %08x", top2_bits(s[e]));
            printf(" network %08x %08x sequential %08x %08x\n", top2_bits(n1), top2_bits(n2), top2_bits(q1), top2_bits(q2));
        }
    }
}
static void check4(float b1, float b2, const float (&s)[4], unsigned e0) {
    float n1 = b1, n2 = b2, q1 = b1, q2 = b2;
    top2_fold4(n1, n2, s[0], s[1], s[2], s[3]);
    for (int e = 0; e < 4; ++e) seq(q1, q2, s[e]);
    if (!same(n1, q1) || !same(n2, q2)) {
        ++bad4;
        if (shown++ < 5)
            printf("mismatch4 (tags from %u) b1 %08x b2 %08x s %08x %08x %08x %08x network %08x %08x sequential %08x %08x\n", e0,
                   top2_bits(b1), top2_bits(b2), top2_bits(s[0]), top2_bits(s[1]), top2_bits(s[2]), top2_bits(s[3]),
                   top2_bits(n1), top2_bits(n2), top2_bits(q1), top2_bits(q2));
    }
}

int main() {
    const float V[7] = {-INFINITY, -2.0f, -1.0f, -0.0f, 0.0f, 1.0f, 2.0f};      // ascending in the maximum's order
    const float S1[3] = {-INFINITY, -0.0f, 2.0f}, S4[3] = {-INFINITY, 0.0f, 1.0f};
    long long n8 = 0, n4 = 0;
    // 1. exhaustive
    for (int pass = 0; pass < 2; ++pass)
        for (int i1 = 0; i1 < 7; ++i1)
            for (int i2 = 0; i2 <= i1; ++i2)
                for (int a1 = 0; a1 < 3; ++a1)
                    for (int a4 = 0; a4 < 3; ++a4)
                        for (int c = 0; c < 7 * 7 * 7 * 7 * 7 * 7; ++c) {
                            float s[8];
                            int r = c;
                            for (int e = 0; e < 8; ++e) {
                                float v;
                                if (e == 1) v = S1[a1]; else if (e == 4) v = S4[a4]; else { v = V[r % 7]; r /= 7; }
                                s[e] = tagged(v, (unsigned)e);
                            }
                            const unsigned t1 = pass ? (unsigned)(c % 8) : 0u, t2 = pass ? (unsigned)(c / 8 % 8) : 0u;
                            float b1 = tagged(V[i1], t1), b2 = tagged(V[i2], t2);
                            order(b1, b2);
                            check8(b1, b2, s);
                            ++n8;
                        }
    for (unsigned half = 0; half < 2; ++half)                         // tags 0..3 and 4..7: the two code halves
        for (unsigned tt = 0; tt < 64; ++tt)
            for (int i1 = 0; i1 < 7; ++i1)
                for (int i2 = 0; i2 <= i1; ++i2)
                    for (int c = 0; c < 7 * 7 * 7 * 7; ++c) {
                        float s[4];
                        int r = c;
                        for (int e = 0; e < 4; ++e) { s[e] = tagged(V[r % 7], 4 * half + (unsigned)e); r /= 7; }
                        float b1 = tagged(V[i1], tt % 8), b2 = tagged(V[i2], tt / 8);
                        order(b1, b2);
                        check4(b1, b2, s, 4 * half);
                        ++n4;
                    }
    printf("exhaustive fold8 %lld fold4 %lld\n", n8, n4);
    // 2. random with planted duplicates
    long long m8 = 0, m4 = 0;
    for (int i = 0; i < 400000; ++i) {
        float s[8], h[4];
        for (int e = 0; e < 8; ++e) s[e] = top2_tag(rnd_float(), (unsigned)e);
        float b1 = (rnd() % 16 == 0) ? -INFINITY : top2_tag(rnd_float(), rnd() % 8);
        float b2 = (rnd() % 8 == 0) ? -INFINITY : top2_tag(rnd_float(), rnd() % 8);
        const unsigned dup = rnd();
        if (dup & 1) s[rnd() % 8] = s[rnd() % 8];                                                            // a score at two positions, bits and all
        if (dup & 2) { const unsigned a = rnd() % 8, b = rnd() % 8; s[b] = top2_tag(s[a], b); }             // the same score under another tag
        if (dup & 4) s[rnd() % 8] = b1;                                                                     // a score equal to the best so far, bits and all
        if (dup & 8) s[rnd() % 8] = b2;
        if (dup & 16) b2 = b1;
        if (dup & 32) { const float v = s[rnd() % 8]; for (int k = 0; k < 3; ++k) s[rnd() % 8] = v; }
        order(b1, b2);
        check8(b1, b2, s); ++m8;
        for (int e = 0; e < 4; ++e) h[e] = s[(i & 1) * 4 + e];
        check4(b1, b2, h, (unsigned)(i & 1) * 4); ++m4;
    }
    printf("random fold8 %lld fold4 %lld\n", m8, m4);
    printf("mismatches fold8 %lld fold4 %lld\n", bad8, bad4);
    return 0;
}
'''


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    cxx = (shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
           or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang++'))
    if not (os.path.isfile(cxx) and os.access(cxx, os.X_OK)):
        pytest.fail('no C++ compiler (c++, g++, clang++ or the ROCm tree\'s): the host path of vqhip_top2.h cannot be built')
    d = tmp_path_factory.mktemp('top2_network')
    src, exe = d / 'top2.cpp', d / 'top2'
    src.write_text(PROGRAM)
    res = subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', f'-I{CSRC}', str(src), '-o', str(exe)],
                         capture_output=True, text=True)
    assert res.returncode == 0, f'the program does not compile against csrc/vqhip_top2.h:\n{res.stderr}'
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    print(res.stdout)
    out = {}
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] in ('exhaustive', 'random', 'mismatches'):
            out[w[0]] = {w[1]: int(w[2]), w[3]: int(w[4])}
    out['text'] = res.stdout
    return out


def test_pools_were_folded(report):
    assert report['exhaustive']['fold8'] == 2 * 28 * 9 * 7 ** 6
    assert report['exhaustive']['fold4'] == 2 * 64 * 28 * 7 ** 4
    assert report['random'] == {'fold8': 400000, 'fold4': 400000}


def test_eight_score_network_is_the_sequential_update(report):
    assert report['mismatches']['fold8'] == 0, report['text'][:2000]


def test_four_score_network_is_the_sequential_update(report):
    assert report['mismatches']['fold4'] == 0, report['text'][:2000]
