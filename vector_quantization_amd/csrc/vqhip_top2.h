// libvqhip: the proposal epilogue's top-2 fold as a network of three-input maximum / median instructions.
// Stands alone: device code reaches it through vqhip_proposal_kernels.h, and a plain C++ compiler takes the host path
// (tests/test_top2_network_cpu.py builds a program around it).
//
// A lane keeps, per token, the best tagged score b1 and the runner-up b2 (b1 >= b2).  The sequential update takes one score
// at a time, b2 = med3(b1, b2, v); b1 = max(b1, v): 2 instructions per score in one dependent chain.  All a lane needs after the
// eight scores s0..s7 of a (token tile, code tile) is the top two of the multiset {b1, b2, s0..s7}:
//     m1 = max3(s0,s1,s2)   r1 = med3(s0,s1,s2)
//     m2 = max3(s3,s4,s5)   r2 = med3(s3,s4,s5)
//     m3 = max3(s6,s7,b1)   r3 = med3(s6,s7,b1)        p = max3(r1,r2,r3)
//     b1' = max3(m1,m2,m3)  y  = med3(m1,m2,m3)        b2' = max3(y, p, b2)
// 10 instructions for 8 scores and a chain of 4.  b1' is the maximum of the same nine values; b2' is the second largest of the
// same multiset, duplicates included: it is y (the best of the two groups that lost) or the runner-up of some group or b2, and
// r_i <= m_i, b2 <= b1 keep every other value out.  The pair is therefore bitwise the sequential update's for finite and
// +-inf scores; NaN is out of contract (rows with non-finite statistics go to the whole-codebook fp32 pass whatever the
// record holds).  The four steps are separate functions so that the stream loop can spread one fold over four chunks of MFMAs.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VQ_TOP2_FN __host__ __device__ __forceinline__
#else
#define VQ_TOP2_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// single instructions (hipcc otherwise wraps fmaxf on values of unknown origin in canonicalising v_max pairs)
VQ_TOP2_FN float top2_max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
VQ_TOP2_FN float top2_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
VQ_TOP2_FN float top2_tag(float score, uint32_t e) { return __uint_as_float((__float_as_uint(score) & 0xFFFFFFF0u) | e); }
#else
// Host path: v_max_f32 / v_max3_f32 / v_med3_f32 for operands that are no NaN.  The maximum orders -0 below +0.  The median
// returns the maximum of the two operands that are not the maximum of the three, and it tells the two zeros apart in finding
// that one: measured on MI355X over all 343 triples of {-inf, -2, -1, -0, +0, 1, 2}, where a median that looks for the maximum
// with a floating-point == (to which the zeros are equal) differs from the device in 11 (profiles/top2_network.txt).
VQ_TOP2_FN uint32_t top2_bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
VQ_TOP2_FN float top2_max(float a, float b) {
    if (a == 0.0f && b == 0.0f) return (top2_bits(a) >> 31) ? b : a;
    return a >= b ? a : b;
}
VQ_TOP2_FN float top2_max3(float a, float b, float c) { return top2_max(top2_max(a, b), c); }
VQ_TOP2_FN float top2_med3(float a, float b, float c) {
    const uint32_t m = top2_bits(top2_max3(a, b, c));
    if (m == top2_bits(a)) return top2_max(b, c);
    if (m == top2_bits(b)) return top2_max(a, c);
    return top2_max(a, b);
}
VQ_TOP2_FN float top2_tag(float score, uint32_t e) {
    const uint32_t b = (top2_bits(score) & 0xFFFFFFF0u) | e;
    float r; memcpy(&r, &b, 4); return r;
}
#endif

struct Top2Net { float m1, r1, m2, r2, m3, p; };

VQ_TOP2_FN void top2_net_a(Top2Net &n, float s0, float s1, float s2) { n.m1 = top2_max3(s0, s1, s2); n.r1 = top2_med3(s0, s1, s2); }
VQ_TOP2_FN void top2_net_b(Top2Net &n, float s3, float s4, float s5) { n.m2 = top2_max3(s3, s4, s5); n.r2 = top2_med3(s3, s4, s5); }
VQ_TOP2_FN void top2_net_c(Top2Net &n, float s6, float s7, float b1) {
    n.m3 = top2_max3(s6, s7, b1);
    n.p = top2_max3(n.r1, n.r2, top2_med3(s6, s7, b1));
}
VQ_TOP2_FN void top2_net_d(const Top2Net &n, float &b1, float &b2) {
    b1 = top2_max3(n.m1, n.m2, n.m3);
    b2 = top2_max3(top2_med3(n.m1, n.m2, n.m3), n.p, b2);
}

// eight tagged scores at once
VQ_TOP2_FN void top2_fold8(float &b1, float &b2, const float (&s)[8]) {
    Top2Net n;
    top2_net_a(n, s[0], s[1], s[2]);
    top2_net_b(n, s[3], s[4], s[5]);
    top2_net_c(n, s[6], s[7], b1);
    top2_net_d(n, b1, b2);
}

// four tagged scores (the half tiles of the one-wave-per-SIMD forms): 5 instructions where the sequential update takes 8
VQ_TOP2_FN void top2_fold4(float &b1, float &b2, float a, float b, float c, float d) {
    const float m = top2_max3(a, b, c), s = top2_med3(a, b, c);
    const float x = top2_med3(b1, m, d);
    b1 = top2_max3(b1, m, d);
    b2 = top2_max3(b2, s, x);
}
