// Fused token sampler of stage-2 generation (vq/tasks/sequence_modeling/models/samplers.py): logits [R, >= end] -> one token per
// output row, in ONE launch: slice, CFG mix, temperature, top-k, top-p, inverse-CDF draw, + start, CFG duplication.
//
// Contract: include/vqhip.h (vqhip_sample_tokens), DESIGN.md §8.  One workgroup of VQ_SAMPLE_THREADS per output row.
//   pass 0   read the slice (16-byte loads where the row allows, element loads otherwise), a = mix / temperature in fp32, the
//            order-preserving 32-bit key of a; row maximum, minimum and the bad-row flag.  RESIDENT: the keys stay in LDS
//            (V <= VQ_SAMPLE_RESIDENT_MAX) and every later pass reads LDS; otherwise a pass re-reads the logits (L2) and
//            recomputes the same keys with the same instructions: both forms return the same bits.
//   top-k    radix select of the k-th largest key: 4 passes over 8 bits, LDS histograms of counts.
//   top-p    radix select, ascending, of the first token whose cumulative mass exceeds (1 - p) Z: 4 passes, LDS histograms of
//            MASSES.  A mass is exp(a - max) as a 64-bit fixed-point integer (40 fraction bits): integer sums are exact and
//            independent of the order the LDS atomics arrive in, so the decision is bit-reproducible.
//   ties     among tokens of the cut value the lower index ranks higher: the index of the last kept one (one pass; a radix
//            select over the index when only some of the tied tokens are kept).
//   draw     running mass in index order: a contiguous chunk per thread (streamed rows: the chunk sums come from one more
//            coalesced sweep into LDS), a workgroup scan of the chunk sums, and the one thread whose chunk holds the crossing
//            walks it.
// No sort, no global scratch, no float atomics.  Every LDS index is a histogram bin (& 255), a wave number or an element index
// below V.
// ------------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vqhip.h"
#include "vqhip_elem.h"                         // SampleElem: the exact conversion to fp32

#define VQ_SAMPLE_THREADS 512
#define VQ_SAMPLE_WAVES (VQ_SAMPLE_THREADS / 64)
#define VQ_SAMPLE_RESIDENT_MAX 32768            // keys of a row kept in LDS up to this V (128 KiB of the CU's 160)
#define VQ_SAMPLE_MAX_V (1 << 20)
#define VQ_SAMPLE_FRAC_BITS 40                  // a mass <= 1 is an integer <= 2^40; 2^20 of them sum below 2^61

typedef unsigned long long sample_u64;

struct VqSampleArgs {
    const void *logits;
    int64_t row_stride, start;
    int V;
    int Ro;
    int cfg;
    float w_uncond, w_cond;                     // (float)(1.0 - (double)alpha), alpha
    float temperature;
    int k;                                      // 0: top-k off; else min(top_k, V)
    int use_top_p;
    double one_minus_p;                         // 1.0 - (double)top_p
    const float *u;
    int64_t *tokens;
    vqhip_sample_cut_t *cut;
};

struct VqSampleShared {
    sample_u64 mass[256];
    unsigned int cnt[256];
    sample_u64 wave_tot[VQ_SAMPLE_WAVES];
    sample_u64 chunk_mass[VQ_SAMPLE_THREADS];  // streamed draw: the kept mass of each thread's chunk
    sample_u64 acc64, r_below_mass, r_eq_mass, r_total;
    unsigned int maxkey, minkey, bad, acc_max;
    unsigned int r_bin, r_kk, r_above, r_eq, r_below_cnt;
    int found, last_kept;
};

// a -> key with key order == (a) order for non-NaN a (-0 was folded into +0 before); and back
__device__ __forceinline__ unsigned int sample_key(float a) {
    const unsigned int b = __float_as_uint(a);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(unsigned int k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// the row as one workgroup sees it
template <int DT, bool RESIDENT>
struct SampleRow {
    typedef SampleElem<DT> E;
    typedef typename E::raw raw;
    const raw *p0, *p1;                          // slice starts of the (unconditional) row and of the conditional row
    const unsigned int *keys;                    // LDS (RESIDENT)
    int V, head, nvec;                           // head: elements in front of the first 16-byte boundary; nvec: 16-byte pieces
    bool cfg, has_t;
    float w0, w1, t;
    unsigned int badflag;                        // set by key_of where an input or a mixed value is NaN or +inf (this thread)

    // the contract's fp32 arithmetic (no contraction: the library is built with -ffp-contract=off)
    __device__ __forceinline__ unsigned int key_of(float x0, float x1) {
        float a = x0;
        bool bad = !(x0 < __builtin_inff());                                    // NaN or +inf
        if (cfg) {
            bad |= !(x1 < __builtin_inff());
            const float l = w0 * x0, r = w1 * x1;
            a = l + r;
        }
        if (has_t) a = a / t;
        bad |= !(a < __builtin_inff());
        if (a == 0.0f) a = 0.0f;                                                // -0 -> +0: equal values, equal keys
        if (bad) badflag = 1u;
        return sample_key(a);
    }
    __device__ __forceinline__ unsigned int key_global(int i) {
        return key_of(E::f32(p0[i]), cfg ? E::f32(p1[i]) : 0.0f);
    }
    __device__ __forceinline__ unsigned int key_at(int i) { return RESIDENT ? keys[i] : key_global(i); }

    // f(i, key) for every element of the slice, from global memory: head and tail by element, the body in 16-byte pieces
    template <class F>
    __device__ __forceinline__ void sweep_global(F f) {
        const int tid = threadIdx.x;
        for (int i = tid; i < head; i += VQ_SAMPLE_THREADS) f(i, key_global(i));
        for (int v = tid; v < nvec; v += VQ_SAMPLE_THREADS) {
            const int i0 = head + v * E::W;
            alignas(16) raw a[E::W];
            alignas(16) raw b[E::W];
            *reinterpret_cast<uint4 *>(a) = *reinterpret_cast<const uint4 *>(p0 + i0);
            if (cfg) *reinterpret_cast<uint4 *>(b) = *reinterpret_cast<const uint4 *>(p1 + i0);
#pragma unroll
            for (int e = 0; e < E::W; ++e) f(i0 + e, key_of(E::f32(a[e]), cfg ? E::f32(b[e]) : 0.0f));
        }
        for (int i = head + nvec * E::W + tid; i < V; i += VQ_SAMPLE_THREADS) f(i, key_global(i));
    }
    template <class F>
    __device__ __forceinline__ void sweep(F f) {
        if (RESIDENT) {
            for (int i = threadIdx.x; i < V; i += VQ_SAMPLE_THREADS) f(i, keys[i]);
        } else {
            sweep_global(f);
        }
    }
};

// exp(a - max) as a fixed-point integer: fp32 subtraction, expf (<= 1 ulp), times 2^40 exactly, truncated
__device__ __forceinline__ sample_u64 sample_mass(unsigned int key, float maxv) {
    const float m = expf(sample_unkey(key) - maxv);
    return (sample_u64)((double)m * (double)(1ull << VQ_SAMPLE_FRAC_BITS));
}

// k-th largest (kk = 1 .. number of selected elements) of the 32-bit sort keys sel(i, key, &sk) selects; all threads call it and
// all get the result: returns the sort key, *above = selected elements with a larger sort key, *eq = with that sort key.
template <class Row, class Sel>
__device__ unsigned int sample_count_select(Row &row, VqSampleShared &sh, unsigned int kk, Sel sel, unsigned int *above_out,
                                            unsigned int *eq_out) {
    const int tid = threadIdx.x;
    unsigned int prefix = 0, mask = 0, above = 0, eq = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) sh.cnt[tid] = 0;
        if (tid == 0) { sh.r_bin = 0; sh.r_kk = 1; sh.r_above = 0; sh.r_eq = 0; }
        __syncthreads();
        {   // a thread adds up runs of one bin in registers: the top digits of float keys fall into very few bins
            unsigned int cur = 0, run = 0;
            row.sweep([&](int i, unsigned int key) {
                unsigned int sk;
                if (sel(i, key, sk) && (sk & mask) == prefix) {
                    const unsigned int bin = (sk >> shift) & 255u;
                    if (bin != cur && run) { atomicAdd(&sh.cnt[cur], run); run = 0; }
                    cur = bin; ++run;
                }
            });
            if (run) atomicAdd(&sh.cnt[cur], run);
        }
        __syncthreads();
        if (tid < 64) {                                                          // wave 0: lane l owns bins 4l .. 4l + 3
            unsigned int c[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) c[b] = sh.cnt[4 * tid + b];
            const unsigned int mine = (c[0] + c[1]) + (c[2] + c[3]);
            unsigned int suf = mine;                                             // bins of this lane and of the lanes above
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int v = __shfl_down(suf, o, 64);
                if (tid + o < 64) suf += v;
            }
            unsigned int acc = suf - mine;
            if (acc < kk && kk <= suf) {
                for (int b = 3; b >= 0; --b) {
                    if (acc + c[b] >= kk) {
                        sh.r_bin = 4 * tid + b; sh.r_kk = kk - acc; sh.r_above = acc; sh.r_eq = c[b];
                        break;
                    }
                    acc += c[b];
                }
            }
        }
        __syncthreads();
        prefix |= sh.r_bin << shift;
        mask |= 255u << shift;
        above += sh.r_above;
        kk = sh.r_kk;
        eq = sh.r_eq;
        __syncthreads();                                                         // every thread has read r_* before the next round resets them
    }
    *above_out = above;
    *eq_out = eq;
    return prefix;
}

struct SampleCutState {
    unsigned int tcut;          // key of the lowest-ranked kept token
    unsigned int n_eq;          // tokens with that key (among the top-k survivors)
    unsigned int q;             // how many of them are kept (the q lowest indices)
    unsigned int kept;
    sample_u64 zk, zkept;
    bool only_top;
};

template <int DT, bool RESIDENT>
__global__ __launch_bounds__(VQ_SAMPLE_THREADS) void sample_tokens_kernel(VqSampleArgs A) {
    typedef SampleRow<DT, RESIDENT> Row;
    typedef typename Row::raw raw;
    extern __shared__ __attribute__((aligned(16))) unsigned int sample_keys[];
    __shared__ VqSampleShared sh;
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const int V = A.V;

    Row row;
    row.p0 = reinterpret_cast<const raw *>(A.logits) + (int64_t)r * A.row_stride + A.start;
    row.p1 = A.cfg ? row.p0 + (int64_t)A.Ro * A.row_stride : row.p0;
    row.keys = sample_keys;
    row.V = V;
    row.cfg = A.cfg != 0;
    row.has_t = A.temperature != 1.0f;
    row.w0 = A.w_uncond; row.w1 = A.w_cond; row.t = A.temperature;
    row.badflag = 0;
    {   // 16-byte pieces where both rows reach a 16-byte boundary after the same number of whole elements
        const uintptr_t a0 = (uintptr_t)row.p0 % 16, a1 = (uintptr_t)row.p1 % 16;
        const int es = (int)sizeof(raw);
        int head = V, nvec = 0;
        if (a0 == a1 && a0 % es == 0) {
            const int h = (int)(((16 - a0) % 16) / es);
            if (h < V) { head = h; nvec = (V - h) / Row::E::W; }
        }
        row.head = head; row.nvec = nvec;
    }

    // ---- pass 0: keys, extrema, bad flag -----------------------------------------------------------------------------------
    if (tid == 0) { sh.maxkey = 0u; sh.minkey = 0xFFFFFFFFu; sh.bad = 0u; sh.found = -1; sh.last_kept = -1; }
    __syncthreads();
    {
        unsigned int mx = 0u, mn = 0xFFFFFFFFu;
        row.sweep_global([&](int i, unsigned int key) {
            if (RESIDENT) sample_keys[i] = key;
            mx = key > mx ? key : mx;
            mn = key < mn ? key : mn;
        });
        atomicMax(&sh.maxkey, mx);
        atomicMin(&sh.minkey, mn);
        if (row.badflag) atomicOr(&sh.bad, 1u);
    }
    __syncthreads();
    const unsigned int maxkey = sh.maxkey;
    const float maxv = sample_unkey(maxkey);
    if (sh.bad || !(maxv > -__builtin_inff())) {                                 // NaN, +inf, or no finite value: -1, nothing else
        if (tid == 0) {
            A.tokens[r] = -1;
            if (A.cfg) A.tokens[r + A.Ro] = -1;
            if (A.cut) {
                vqhip_sample_cut_t c;
                c.kept = 0; c.topk_kept = 0; c.cut_value = 0.f; c.cut_index = -1; c.max = maxv; c.z = 0.f;
                A.cut[r] = c;
            }
        }
        return;
    }
    row.badflag = 0;

    // ---- top-k: the k-th largest key; every key >= it survives -------------------------------------------------------------
    unsigned int tk = sh.minkey, topk_kept = (unsigned int)V;
    if (A.k > 0 && A.k < V) {
        unsigned int above, eq;
        tk = sample_count_select(row, sh, (unsigned int)A.k,
                                 [](int, unsigned int key, unsigned int &sk) { sk = key; return true; }, &above, &eq);
        topk_kept = above + eq;
    }

    // ---- top-p: the lowest-ranked kept token ---------------------------------------------------------------------------------
    SampleCutState S;
    S.tcut = tk; S.only_top = false;
    if (!A.use_top_p) {
        // one pass: the survivors' mass, the tokens at the cut value
        if (tid == 0) { sh.acc64 = 0; sh.r_eq = 0; }
        __syncthreads();
        sample_u64 m = 0;
        unsigned int n = 0;
        row.sweep([&](int, unsigned int key) {
            if (key >= tk) { m += sample_mass(key, maxv); n += key == tk ? 1u : 0u; }
        });
        atomicAdd(&sh.acc64, m);
        atomicAdd(&sh.r_eq, n);
        __syncthreads();
        S.zk = S.zkept = sh.acc64;
        S.n_eq = S.q = sh.r_eq;
        S.kept = topk_kept;
        __syncthreads();
    } else {
        unsigned int prefix = 0, mask = 0, below_cnt = 0, eq = 0;
        sample_u64 below = 0, eq_mass = 0, zk = 0, thr = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) { sh.cnt[tid] = 0; sh.mass[tid] = 0; }
            if (tid == 0) { sh.r_bin = 0; sh.r_below_mass = 0; sh.r_below_cnt = 0; sh.r_eq = 0; sh.r_eq_mass = 0; sh.r_total = 0; }
            __syncthreads();
            {   // runs of one bin are added up in registers first (integers: the grouping cannot change a sum)
                unsigned int cur = 0, run = 0;
                sample_u64 run_mass = 0;
                row.sweep([&](int, unsigned int key) {
                    if (key >= tk && (key & mask) == prefix) {
                        const unsigned int bin = (key >> shift) & 255u;
                        if (bin != cur && run) {
                            atomicAdd(&sh.cnt[cur], run);
                            if (run_mass) atomicAdd(&sh.mass[cur], run_mass);
                            run = 0; run_mass = 0;
                        }
                        cur = bin; ++run;
                        run_mass += sample_mass(key, maxv);
                    }
                });
                if (run) {
                    atomicAdd(&sh.cnt[cur], run);
                    if (run_mass) atomicAdd(&sh.mass[cur], run_mass);
                }
            }
            __syncthreads();
            if (tid < 64) {                                                      // wave 0, ascending: lane l owns bins 4l .. 4l + 3
                sample_u64 mm[4];
                unsigned int c[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) { mm[b] = sh.mass[4 * tid + b]; c[b] = sh.cnt[4 * tid + b]; }
                const sample_u64 mine = (mm[0] + mm[1]) + (mm[2] + mm[3]);
                const unsigned int cmine = (c[0] + c[1]) + (c[2] + c[3]);
                sample_u64 inc = mine;
                unsigned int cinc = cmine;
                for (int o = 1; o < 64; o <<= 1) {
                    const sample_u64 v = __shfl_up(inc, o, 64);
                    const unsigned int cv = __shfl_up(cinc, o, 64);
                    if (tid >= o) { inc += v; cinc += cv; }
                }
                const sample_u64 total = __shfl(inc, 63, 64);
                sample_u64 t_rel;                                                // the threshold relative to this round's group
                if (shift == 24) {
                    // Z of the survivors, and floor((1 - p) Z): a token is removed iff its cumulative mass is <= it
                    const double t = A.one_minus_p;
                    sample_u64 th = 0;
                    if (t >= 1.0) th = total;
                    else if (t > 0.0) { th = (sample_u64)(t * (double)total); th = th > total ? total : th; }
                    if (tid == 0) { sh.r_total = total; sh.acc64 = th; }
                    t_rel = th;
                } else {
                    t_rel = thr - below;
                }
                sample_u64 acc = inc - mine;
                unsigned int cacc = cinc - cmine;
                if (acc <= t_rel && t_rel < inc) {                               // the crossing lies in this lane's bins
                    for (int b = 0; b < 4; ++b) {
                        if (acc + mm[b] > t_rel) {
                            sh.r_bin = 4 * tid + b; sh.r_below_mass = acc; sh.r_below_cnt = cacc; sh.r_eq = c[b]; sh.r_eq_mass = mm[b];
                            break;
                        }
                        acc += mm[b]; cacc += c[b];
                    }
                }
            }
            __syncthreads();
            if (shift == 24) {
                zk = sh.r_total; thr = sh.acc64;
                if (thr >= zk) S.only_top = true;                                // every token is at or below the threshold: keep the top one
            }
            prefix |= sh.r_bin << shift;
            mask |= 255u << shift;
            below += sh.r_below_mass;
            below_cnt += sh.r_below_cnt;
            eq = sh.r_eq; eq_mass = sh.r_eq_mass;
            __syncthreads();
            if (S.only_top) break;                                               // (uniform)
        }
        S.zk = zk;
        if (S.only_top || eq == 0 || eq_mass == 0) {
            S.only_top = true;
            S.tcut = maxkey; S.n_eq = 0; S.q = 1; S.kept = 1;
            S.zkept = 1ull << VQ_SAMPLE_FRAC_BITS;                               // exp(0) = 1
        } else {
            // tokens of the cut value, from the highest index down, are removed while the cumulative mass stays <= thr
            const sample_u64 m1 = eq_mass / eq;                                  // (all eq masses are equal: one value, one mass)
            sample_u64 removed = (thr - below) / m1;                             // < eq, as below + eq * m1 > thr
            if (removed >= eq) removed = eq - 1;
            S.tcut = prefix; S.n_eq = eq; S.q = eq - (unsigned int)removed;
            S.kept = topk_kept - below_cnt - (unsigned int)removed;
            S.zkept = zk - below - removed * m1;
        }
    }

    // ---- ties: the index of the last kept token of the cut value --------------------------------------------------------------
    const unsigned int tcut = S.tcut;
    int cut_index;
    if (!S.only_top && S.q == S.n_eq) {                                          // all of them: the highest index
        if (tid == 0) sh.acc_max = 0u;
        __syncthreads();
        unsigned int mx = 0u;
        row.sweep([&](int i, unsigned int key) { if (key == tcut) mx = (unsigned int)i > mx ? (unsigned int)i : mx; });
        atomicMax(&sh.acc_max, mx);
        __syncthreads();
        cut_index = (int)sh.acc_max;
        __syncthreads();
    } else {                                                                     // the q-th lowest index = the q-th largest ~index
        unsigned int above, eq;
        const unsigned int sk = sample_count_select(row, sh, S.q,
                                                    [tcut](int i, unsigned int key, unsigned int &s) { s = ~(unsigned int)i; return key == tcut; },
                                                    &above, &eq);
        cut_index = (int)~sk;
        if (cut_index < 0 || cut_index >= V) cut_index = 0;                      // (cannot happen: q >= 1 tokens carry the key)
    }

    // ---- draw: first kept token, in index order, whose running mass exceeds u * Z -----------------------------------------------
    float u = A.u[r];
    if (!(u >= 0.0f)) u = 0.0f;
    sample_u64 thr_u = (sample_u64)((double)u * (double)S.zkept);
    if (thr_u >= S.zkept) thr_u = S.zkept - 1;
    const int chunk = ((V + VQ_SAMPLE_THREADS - 1) / VQ_SAMPLE_THREADS) | 1;     // odd: lanes a chunk apart fall on different LDS banks
    const int64_t lo64 = (int64_t)tid * chunk;
    const int lo = lo64 < V ? (int)lo64 : V, hi = lo64 + chunk < V ? (int)(lo64 + chunk) : V;
    sample_u64 mine = 0;
    int last = -1;
    if (RESIDENT) {
        for (int i = lo; i < hi; ++i) {
            const unsigned int key = sample_keys[i];
            if (key > tcut || (key == tcut && i <= cut_index)) { mine += sample_mass(key, maxv); last = i; }
        }
    } else {
        // the chunk sums by one more coalesced sweep (16-byte loads): every thread adds what it meets to the chunk the element
        // belongs to (runs of one chunk in registers first; integers: the grouping cannot change a sum)
        sh.chunk_mass[tid] = 0;
        __syncthreads();
        int cur = 0;
        sample_u64 run_mass = 0;
        row.sweep_global([&](int i, unsigned int key) {
            if (key > tcut || (key == tcut && i <= cut_index)) {
                const int b = i / chunk;                                         // < VQ_SAMPLE_THREADS: chunk >= ceil(V / threads)
                if (b != cur && run_mass) { atomicAdd(&sh.chunk_mass[cur], run_mass); run_mass = 0; }
                cur = b;
                run_mass += sample_mass(key, maxv);
                last = i > last ? i : last;
            }
        });
        if (run_mass) atomicAdd(&sh.chunk_mass[cur], run_mass);
        __syncthreads();
        mine = sh.chunk_mass[tid];
    }
    sample_u64 inc = mine;
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const sample_u64 v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) sh.wave_tot[wave] = inc;
    if (last >= 0) atomicMax(&sh.last_kept, last);
    __syncthreads();
    sample_u64 base = 0;
    for (int w = 0; w < wave; ++w) base += sh.wave_tot[w];
    const sample_u64 excl = base + inc - mine;
    if (excl <= thr_u && thr_u < excl + mine) {
        sample_u64 c = excl;
        for (int i = lo; i < hi; ++i) {
            const unsigned int key = row.key_at(i);
            if (key > tcut || (key == tcut && i <= cut_index)) {
                c += sample_mass(key, maxv);
                if (c > thr_u) { sh.found = i; break; }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        int j = sh.found;
        if (j < 0) j = sh.last_kept;                                             // rounding left none: the last kept token
        const int64_t token = j < 0 ? -1 : (int64_t)j + A.start;
        A.tokens[r] = token;
        if (A.cfg) A.tokens[r + A.Ro] = token;
        if (A.cut) {
            vqhip_sample_cut_t c;
            c.kept = (int32_t)S.kept; c.topk_kept = (int32_t)topk_kept;
            c.cut_value = sample_unkey(tcut); c.cut_index = cut_index;
            c.max = maxv;
            c.z = (float)((double)S.zkept / (double)(1ull << VQ_SAMPLE_FRAC_BITS));
            A.cut[r] = c;
        }
    }
}
