// libvqhip — host entry points (C ABI in include/vqhip.h) of the proposal pipeline: the dispatch of the proposal pass, the
// decision, second pass and re-rank behind it (argmin_pipeline), the codebook image and the encode / argmin / column-pass
// entry points, with the tuning knobs and the proposal kernel's profiling.  gfx950 only.  The rest of the quantizer core has a
// translation unit per concern — vqhip_exact.hip (the all-fp32 pass), vqhip_decode.hip, vqhip_fsq.hip, vqhip_update.hip,
// vqhip_step.hip — as the other op families have (csrc/Makefile); vqhip_core.h declares what crosses between them.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "vqhip_core.h"
#include "vqhip_prepare_kernels.h"
#include "vqhip_proposal_kernels.h"
#include "vqhip_refine_kernels.h"
#include "vqhip_proposal32_kernels.h"
#include "vqhip_aux_kernels.h"
#include "vqhip_stream_kernels.h"

// ---- optional per-launch timing of the proposal kernel (bench.py roofline) -------------------------------
// Events are recorded on the caller's stream right around the coarse_kernel launch; vqhip_profile_collect
// synchronises on them.  Disabled (zero overhead) unless vqhip_profile_enable(1) was called.
// This unit's process-wide state is limited to this block, the tuning knobs below and the per-kernel LdsCache of a launch helper;
// all of it is safe to touch from several host threads (each with its own stream): the profiling list is mutex-protected (the mutex
// is taken only while profiling is on), the knobs and the attribute caches (vqhip_host.h) are atomics.
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>
static std::atomic<bool> g_prof_on{false};
static std::mutex g_prof_mu;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_events;
static size_t g_prof_used = 0;

// returns the slot the matching prof_end must close, or -1 when profiling is off
static long prof_begin(hipStream_t s) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return -1;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (g_prof_used == g_prof_events.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { g_prof_on = false; return -1; }
        g_prof_events.emplace_back(a, b);
    }
    const long slot = (long)g_prof_used++;
    (void)hipEventRecord(g_prof_events[slot].first, s);
    return slot;
}
static void prof_end(long slot, hipStream_t s) {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if ((size_t)slot < g_prof_events.size()) (void)hipEventRecord(g_prof_events[slot].second, s);
}

// ---- proposal-pass dispatch ------------------------------------------------------------------------
// Verification aids (vqhip_set_tuning; results unchanged): they let the tests reach paths the defaults take only for some shapes
static std::atomic<int> g_tune_slices{0};        // key 2: force the slice count of the proposal pass (1, 2, 4, 8 or 16)
static std::atomic<int> g_tune_force_exact{0};   // key 12: the first V rows of a batch also take the whole-codebook fp32 pass
static std::atomic<int> g_tune_stream{1};        // key 18: 0 = the whole-batch fp32 pass keeps its register form (exact_tiled_kernel)
// The proposal kernel runs the decision stage itself where one slice covers the codebook (the workgroup then decides its own
// tokens, no ticket involved), and for small batches whatever the slice count: the workgroup that draws a token block's last
// arrival ticket merges its slices (a launch less on a chain of ~5 us launches: 12 images -2.6 %, 32 images -0.5 %,
// tools/ab_small_batch.py; at 256 images and more the last-arriving workgroup's merge is the longer tail).  Deciding in-kernel
// at every slice count was measured neutral (the fences cost what the launch saves: profiles/r02_ab_fused_decide.txt).
#define VQ_FUSED_DECIDE_MAX_N 16384

template <int NSTEP, int TT, int WAVES, int TPS, int NBUF = 2, bool FILTER = false, bool NOAUX = false, bool GROUPS = false, int XD = 0>
static int launch_coarse_cfg(const char *ximg, int64_t N, const char *frag, int64_t nstages, int nslices, float *rec,
                             int64_t Np, const VqCbStats *cbst, const float *xh2, const float *rho2, int Dp, int metric,
                             const VqDecideOut &dec, int pad_stage, int tpb, hipStream_t s) {
    constexpr int LDS = NBUF * (TPS * NSTEP + VQ_AUX_CHUNKS(TPS)) * VQ_CHUNK_BYTES;
    auto kern = coarse_kernel<NSTEP, TT, WAVES, TPS, NBUF, FILTER, NOAUX, GROUPS, XD>;
    static LdsCache lds_set;
    if (int rc = ensure_dyn_lds((const void *)kern, LDS, lds_set)) return rc;
    const int64_t ntiles = (N + 15) / 16;
    const int64_t ntb = (ntiles + tpb - 1) / tpb;
    const int grid = (int)(ntb * (XD == 2 ? 1 : nslices));     // XD == 2: one workgroup takes both slices of its token block
    const long slot = prof_begin(s);
    kern<<<grid, WAVES * 64, LDS, s>>>(ximg, N, frag, nstages, nslices, rec, Np, cbst, xh2, rho2, Dp, metric, dec, pad_stage, tpb);
    prof_end(slot, s);
    VQ_CHECK_LAUNCH("coarse_kernel");
    return VQHIP_OK;
}

// D <= 16 (and D <= 32 without aux reads): the proposal pass on v_mfma_f32_32x32x16_f16 (vqhip_proposal32_kernels.h), same
// images; its group records are identified by identify32_kernel (launched by argmin_pipeline)
template <int TT, int WAVES, int TPS, int NBUF, bool NOAUX, int KS>
static int launch_coarse32_cfg(const char *ximg, int64_t N, const char *frag, int64_t nstages, int nslices, float *rec,
                               int64_t Np, const VqCbStats *cbst, const float *xh2, const float *rho2, int Dp, int metric,
                               const int *n_dev, const VqGroupLists &grp, int pad_stage, int tpb, hipStream_t s) {
    constexpr int LDS = NBUF * (TPS * 2 + VQ_AUX_CHUNKS(TPS)) * VQ_CHUNK_BYTES;
    auto kern = coarse32_kernel<TT, WAVES, TPS, NBUF, NOAUX, KS, VQ_GROUP_TILES>;
    static LdsCache lds_set;
    if (int rc = ensure_dyn_lds((const void *)kern, LDS, lds_set)) return rc;
    const int64_t ntiles = (N + 15) / 16;
    const int64_t ntb = (ntiles + tpb - 1) / tpb;
    const long slot = prof_begin(s);
    kern<<<(int)(ntb * nslices), WAVES * 64, LDS, s>>>(ximg, N, frag, nstages, nslices, rec, Np, cbst, xh2, rho2, Dp, metric, n_dev, grp, pad_stage, tpb);
    prof_end(slot, s);
    VQ_CHECK_LAUNCH("coarse32_kernel");
    return VQHIP_OK;
}

template <int NSTEP, int TT, int WAVES, int TPS, int NBUF = 2, int XD = 0>
static int launch_rescan_cfg(const char *ximg, const char *frag, int64_t nstages, const int *rescan_list, const int *counters,
                             const float *thr, int *rescan_cnt, int *cand_list, hipStream_t s, const void *xrows = nullptr) {
    constexpr int LDS = NBUF * (TPS * NSTEP + VQ_AUX_CHUNKS(TPS)) * VQ_CHUNK_BYTES + WAVES * TT * 16 * 4 * (1 + VQ_RESCAN_LOCAL);
    auto kern = rescan_kernel<NSTEP, TT, WAVES, TPS, NBUF, XD>;
    static LdsCache lds_set;
    if (int rc = ensure_dyn_lds((const void *)kern, LDS, lds_set)) return rc;
    kern<<<256, WAVES * 64, LDS, s>>>(ximg, frag, nstages, rescan_list, counters, thr, rescan_cnt, cand_list, xrows);
    VQ_CHECK_LAUNCH("rescan_kernel");
    return VQHIP_OK;
}

#ifndef VQ_W32_MAX_D
#define VQ_W32_MAX_D 32        // the 32x32x16 proposal kernel up to this D (16: one instruction per tile; 32: two)
#endif
#ifndef VQ_NBUF_D32
#define VQ_NBUF_D32 4          // LDS ring depth of the D <= 32 proposal kernels (2 and 3 measured: profiles/r02_smallD_ring.txt)
#endif
#ifndef VQ_D32_SMALL_TT
#define VQ_D32_SMALL_TT 2      // token tiles per wave / waves per workgroup of the D <= 32 kernels below 262 144 tokens
#define VQ_D32_SMALL_W 8
#endif
#ifndef VQ_MIN_SLICES_FILTER
#define VQ_MIN_SLICES_FILTER 1
#endif
// Tiles (of 16 tokens) per workgroup of the proposal kernel when the codebook is not sliced: the workgroups of one launch
// are spread over the 256 CUs by the dispatcher, so the kernel lasts as long as the CU with the most tiles —
// ceil(workgroups / 256) x tiles per workgroup.  Full workgroups are not always the minimum of that: 100 352 tokens
// (BASELINE configs[2]) make 392 workgroups of 16 tiles, two on 136 CUs and one on the other 120 (32 tiles at worst);
// 13 tiles per workgroup make 483, two per CU at worst (26 tiles).  Ties keep the larger workgroup; at least half the
// waves stay busy (and a workgroup covers >= 128 tokens: the arrival counters of the workspace are laid out for that).
static int balanced_tiles_per_block(int64_t N, int full) {
    if (full < 16) return full;
    const int64_t ntiles = (N + 15) / 16;
    int best = full;
    int64_t best_cost = ((ntiles + full - 1) / full + 255) / 256 * full;
    for (int tpb = full - 1; tpb >= full / 2 && tpb >= 8; --tpb) {
        const int64_t cost = ((ntiles + tpb - 1) / tpb + 255) / 256 * tpb;
        if (cost < best_cost) { best_cost = cost; best = tpb; }
    }
    return best;
}

// The token side made inside the proposal kernel's prologue instead of a token image (coarse_kernel<..., XD>):
// the D = 256 form with 64 tokens per wave, rows as the caller holds them, the decision stage in its own launch.  Evaluated
// once per pipeline run, by whoever prepares the token side (encode_fused_front, else argmin_pipeline): VqTokenSide carries the
// answer to the proposal launch and the second pass (which reads the rows instead).
// The two-workgroup form (XD = 1) never decides in-kernel — its statistics are written by slice 0's workgroup and a decision in
// the same launch would read them through the kernel's __restrict__ parameters — so it needs at least two slices: one slice forced
// by key 2 keeps the token image (below), and launch_coarse never gives the form fewer than two whatever the knob says by then.
static bool vq_xdirect(int64_t N, int64_t K, int D, int x_dtype, int metric, const int *n_dev) {
    if (D != 256 || n_dev != nullptr || vq_cb_layout(K, D).nstages < 2 || g_tune_slices.load() == 1) return false;
    // bf16 rows only: a piece of 8 latents has the fragment's own 16 bytes and is converted in place.  fp32 rows (twice the
    // bytes per piece, a round trip per token tile, 58 spilled registers) cost a workgroup +44 us of prologue at 20 000 x 16384 x 256
    // against +3 us for bf16 (profiles/r06_xdirect.txt): they keep the token image
    if (x_dtype != VQHIP_DTYPE_BF16) return false;
    if (!vq_public_metric(metric)) return false;                                      // (not the role-swapped column pass)
    if (N <= VQ_FUSED_DECIDE_MAX_N) return false;                                     // small batches decide inside the proposal kernel
    return !(N <= 4096 || (N <= 256 * 64 && K <= 4096));                               // the 64-tokens-per-wave form (launch_coarse: !small16)
}
// the token side argmin_pipeline finds in its workspace: none (it runs x_prep_kernel itself), the token image, or (vq_xdirect) the housekeeping only
enum VqTokenSide { VQ_TOKENS_UNPREPARED, VQ_TOKENS_IMAGE, VQ_TOKENS_ROWS };

static int pick_slices(int64_t ntb, int64_t nstages, int min_slices = 2);
// ... and whether ONE workgroup per token block streams both slices and decides (coarse_kernel<..., XD = 2>): where
// the slice count is the default's two — never a count forced through key 2 — and the workgroups, half as many and twice as long,
// fill no more rounds of the chip's 256 CUs than the two-workgroup form's: 129..256 token blocks, 385..512, and every count
// from 1024 on a multiple of 256 away (the headline's 1024 make exactly four rounds instead of eight half rounds).
static bool vq_one_workgroup(int64_t N, int64_t nstages) {
    if (g_tune_slices.load() > 0) return false;
    const int64_t ntb = (N + 511) / 512;
    if (nstages < 2 || pick_slices(ntb, nstages) != 2) return false;
    return 2 * ((ntb + 255) / 256) <= (2 * ntb + 255) / 256;
}

static int pick_slices(int64_t ntb, int64_t nstages, int min_slices) {
    if (const int forced = g_tune_slices.load(); forced > 0) { int ns = forced; while (ns > 1 && ns > nstages) ns >>= 1; return ns; }
    // Enough slices to put a workgroup on every CU, no more: fewer, longer workgroups amortise their prologue and
    // record write-back, re-read the token image fewer times and write fewer records.  (Rows whose candidates cannot
    // all be identified get a second proposal pass, so the number of candidate groups does not matter for speed.)
    // ... but at least two: a lane's stream then covers half the codebook, which halves the rows whose runner-up
    // cannot be identified (second proposal pass); measured +0.7 % at 524 288 tokens, nothing lost elsewhere.
    int64_t want = (256 + ntb - 1) / ntb;
    want = want < min_slices ? min_slices : want;
    int ns = 1;
    while (ns < want && ns < VQ_MAX_SLICES) ns <<= 1;
    while (ns > 1 && ns > nstages) ns >>= 1;
    return ns;
}

// grp (nullable lists: the workspace has none beyond VQ_GROUP_MAX_TILES code tiles): where coarse32_kernel files its
// identification requests; *group_path_out = 1 when that kernel ran (argmin_pipeline then launches identify32_kernel and the
// group form of the decision stage), with *group_ks / *group_noaux / *group_pad_stage the parameters identify32_kernel needs
struct VqGroupRun { int used, ks, noaux, pad_stage; };
static int launch_coarse(const char *ximg, int64_t N, const VqCbLayout &L, const char *frag, float *rec, int64_t Np,
                         const VqCbStats *cbst, const float *xh2, const float *rho2, int metric, const VqDecideOut &dec,
                         int *nslices_out, int *fused_decide_out, hipStream_t s, VqGroupLists grp = VqGroupLists{nullptr, nullptr, nullptr, nullptr, 0, 1, 0},
                         VqGroupRun *grun = nullptr, bool xd = false) {
    const int nstep = L.nstep;
    // small batches use fewer tokens per wave so that more workgroups exist
    const bool small = N <= 256 * 64;
    // D = 256: 64 tokens per wave already from 4097 tokens on when the codebook is long (measured at K = 16 384: proposal
    // kernel 76 -> 66 us at 8192 tokens, 140 -> 122 at 16 384, 74 -> 62 at 6144; at 3072 / 4096 tokens and for short
    // codebooks — NearestAnchor's role-swapped pass has K = batch size — 32 tokens per wave stay ahead;
    // profiles/r02_tokens_per_wave_d256.txt)
    const bool small16 = N <= 4096 || (N <= 256 * 64 && L.K <= 4096);
    // D <= 32: 32 tokens per wave until 64-token workgroups would number two per CU (measured at N = 100 352, K = 8192:
    // proposal kernel 128 -> 108 us with 8 tiles per stage, one slice and 32 tokens per wave; at N = 524 288 the
    // 64-token form is the faster one)
    const bool small32 = N < 512 * 512;
    // cosine / dot product: every real code's aux value is 0 (cb_stats_kernel), only padding codes need the aux chunk
    const bool noaux = !VQ_IS_L2(metric);
    const int pad_stage = (L.K % ((int64_t)L.tps * VQ_TILE_CODES)) ? (int)(L.nstages - 1) : -1;
#define VQ_CFG(NS, TT, W, ...)                                                                      \
    {                                                                                               \
        int64_t ntb = (N + (W) * (TT) * 16 - 1) / ((W) * (TT) * 16);                                \
        int ns = pick_slices(ntb, L.nstages, (NS) <= 8 ? VQ_MIN_SLICES_FILTER : 2);                 \
        *nslices_out = ns;                                                                          \
        const int tpb = (ns == 1) ? balanced_tiles_per_block(N, (W) * (TT)) : (W) * (TT);           \
        VqDecideOut dsel = dec;                                                                     \
        if (!(ns == 1 || N <= VQ_FUSED_DECIDE_MAX_N)) dsel.idx = nullptr;                           \
        *fused_decide_out = dsel.idx != nullptr ? 1 : 0;                                            \
        return launch_coarse_cfg<NS, TT, W, __VA_ARGS__>(ximg, N, frag, L.nstages, ns, rec, Np, cbst, xh2, rho2, L.Dp, metric, dsel, pad_stage, tpb, s); \
    }
    switch (nstep) {
        // D <= 128: VALU-issue-bound with the plain epilogue -> filtered epilogue (see coarse_kernel)
        // D <= 16 always; 16 < D <= 32 (two instructions per tile) only without aux reads — measured
        // (profiles/r03_w32_ab.txt): D = 32 cosine +2.5..5 %, D = 32 L2 -4..-14 % (the form is LDS-bound once the four 16-byte aux
        // reads per lane and tile come on top of 2 KiB of fragments)
        case 2: if ((L.D <= 16 || (L.D <= VQ_W32_MAX_D && noaux)) && N >= VQ_W32_MIN_N && grp.bcnt != nullptr && grun != nullptr) {
                    // one 32x32x16 instruction covers the whole inner dimension: a quarter of the MFMA issue, group update per
                    // 16 scores.  Wide token tiles of 32 tokens: 1 (below 262 144 tokens) or 2 per wave.
                    const int tt = small32 ? 1 : 2;
                    const int full = 8 * tt * 2;                                    // 16-token tiles per workgroup
                    const int64_t ntb0 = (N + full * 16 - 1) / (full * 16);
                    int ns = pick_slices(ntb0, L.nstages, VQ_MIN_SLICES_FILTER);
                    ns = ns > VQ_GROUP_MAX_SLICES ? VQ_GROUP_MAX_SLICES : ns;
                    *nslices_out = ns;
                    // (Workgroups of up to sixteen waves, one per CU, where the codebook is not sliced — 13 waves at configs[2]: 3.25 per
                    //  SIMD through ONE ring instead of two workgroups on 192 CUs and one on 64 — were built and measured in round 6:
                    //  -2.4 % at 100 352 x 8192 x 32, -1 % at 131 072, +2 % at D = 8 / 16 and +10 % once a launch needs two rounds of them.
                    //  Not kept: the stream is bound by what the matrix pipe may draw, not by where the waves sit: profiles/r06_c3_notes.txt)
                    int tpb = (ns == 1) ? balanced_tiles_per_block(N, full) : full;
                    tpb = (tpb + 1) & ~1;                                           // whole wide tiles
                    *fused_decide_out = 0;                                          // identification first: the decision stage is its own launch
                    grun->used = 1; grun->ks = L.D <= 16 ? 1 : 2; grun->noaux = noaux ? 1 : 0; grun->pad_stage = pad_stage;
#define VQ_CFG32(TTW, NOAUXV, KSV) return launch_coarse32_cfg<TTW, 8, VQ_TPS_D32, VQ_NBUF_D32, NOAUXV, KSV>(ximg, N, frag, L.nstages, ns, rec, Np, cbst, xh2, rho2, L.Dp, metric, dec.n_dev, grp, pad_stage, tpb, s)
                    if (L.D <= 16) {
                        if (tt == 1) { if (noaux) VQ_CFG32(1, true, 1); else VQ_CFG32(1, false, 1); }
                        else { if (noaux) VQ_CFG32(2, true, 1); else VQ_CFG32(2, false, 1); }
                    } else {
                        if (tt == 1) { if (noaux) VQ_CFG32(1, true, 2); else VQ_CFG32(1, false, 2); }
                        else { if (noaux) VQ_CFG32(2, true, 2); else VQ_CFG32(2, false, 2); }
                    }
#undef VQ_CFG32
                }
                // (N >= 262 144: at least 1024 workgroups of 64 tokens per wave — balance no longer matters and that form is the faster one)
                // group records from VQ_GROUPS_MIN_N tokens on: below, the identification replay at the end of a
                // workgroup (a few L2 round trips) costs more than the stream saves
                if (N >= VQ_GROUPS_MIN_N) {
                    if (noaux) { if (small32) VQ_CFG(2, VQ_D32_SMALL_TT, VQ_D32_SMALL_W, VQ_TPS_D32, VQ_NBUF_D32, true, true, true) else VQ_CFG(2, 4, 8, VQ_TPS_D32, VQ_NBUF_D32, true, true, true) }
                    if (small32) VQ_CFG(2, VQ_D32_SMALL_TT, VQ_D32_SMALL_W, VQ_TPS_D32, VQ_NBUF_D32, true, false, true) else VQ_CFG(2, 4, 8, VQ_TPS_D32, VQ_NBUF_D32, true, false, true)
                }
                if (noaux) { if (small32) VQ_CFG(2, VQ_D32_SMALL_TT, VQ_D32_SMALL_W, VQ_TPS_D32, VQ_NBUF_D32, true, true) else VQ_CFG(2, 4, 8, VQ_TPS_D32, VQ_NBUF_D32, true, true) }
                if (small32) VQ_CFG(2, VQ_D32_SMALL_TT, VQ_D32_SMALL_W, VQ_TPS_D32, VQ_NBUF_D32, true) else VQ_CFG(2, 4, 8, VQ_TPS_D32, VQ_NBUF_D32, true)
        case 4: if (small) VQ_CFG(4, 2, 8, 4, 4, true) else VQ_CFG(4, 4, 8, 4, 4, true)
        case 8: if (small) VQ_CFG(8, 2, 8, 4, 4, true) else VQ_CFG(8, 4, 8, 4, 4, true)
        case 16: if (xd && !small16) {
                     // no token image (vq_xdirect): ONE workgroup per token block that decides in-kernel (vq_one_workgroup), else
                     // a workgroup per slice — at least two, the decision left to refine_decide_kernel
                     const int tpb = 8 * 4;
                     VqDecideOut dsel = dec;
                     if (L.nstages >= 2 && vq_one_workgroup(N, L.nstages)) {
                         *nslices_out = 2;
                         *fused_decide_out = 1;
                         return launch_coarse_cfg<16, 4, 8, VQ_TPS16, 4, false, false, false, 2>(ximg, N, frag, L.nstages, 2, rec, Np, cbst, xh2, rho2, L.Dp, metric, dsel, pad_stage, tpb, s);
                     }
                     if (L.nstages < 2) return fail(VQHIP_EINVAL, "vqhip_argmin: the row-direct proposal form needs two stages");
                     int ns = pick_slices((N + tpb * 16 - 1) / (tpb * 16), L.nstages, 2);
                     ns = ns < 2 ? 2 : ns;
                     *nslices_out = ns;
                     dsel.idx = nullptr;
                     *fused_decide_out = 0;
                     return launch_coarse_cfg<16, 4, 8, VQ_TPS16, 4, false, false, false, 1>(ximg, N, frag, L.nstages, ns, rec, Np, cbst, xh2, rho2, L.Dp, metric, dsel, pad_stage, tpb, s);
                 }
                 if (small16) VQ_CFG(16, 2, 8, VQ_TPS16, 4) else VQ_CFG(16, 4, 8, VQ_TPS16, 4)
        // large D: the token fragments of a wave must stay in registers for the whole stream
        case 32: VQ_CFG(32, 2, 8, 2)
        case 48: VQ_CFG(48, 2, 8, 1)
        case 64: {
            // D = 1024, two forms: eight waves x 16 tokens (two waves per SIMD; one 1 KiB LDS read per MFMA), or four waves x 48
            // tokens (one wave per SIMD with the whole register file: coarse_kernel, PIPE_H; a third of the LDS bytes per flop).
            // Per unit of work the second is 1.06-1.29x faster (1.013 against 1.095 ms at 65 536 x 8192, 2.71 against 3.22 at
            // 196 608), but its 192-token workgroups fill the chip in other multiples than the 128-token ones: 16 384 and
            // 32 768 tokens are faster on the first form, 24 576 and 49 152 on the second (profiles/r03_large_d_experiments.txt).
            // Whole rounds of 256 workgroups times the work of one, the second form's divided by 1.18, decide.
            // (At D = 768 the one-wave form with 64 tokens per wave is 1-6 % BEHIND the eight-wave form: not taken.)
            auto cost = [&](int tokens, double eff) {
                const int64_t ntb = (N + tokens - 1) / tokens;
                const int ns = pick_slices(ntb, L.nstages, 2);
                return (double)((ntb * ns + 255) / 256) * tokens * ((double)L.nstages / ns) / eff;
            };
            if (cost(192, 1.18) < cost(128, 1.0)) VQ_CFG(64, 3, 4, 1) else VQ_CFG(64, 1, 8, 1)
        }
        default: break;
    }
#undef VQ_CFG
    return fail(VQHIP_EINVAL, "vqhip_argmin: unsupported padded D");
}

// Workgroups a persistent kernel can keep resident: compute units of the current device x workgroups per CU.
static int resident_grid(int per_cu) {
    static std::atomic<int> cus[VQ_MAX_DEVICES];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256 * per_cu;
    if (dev >= 0 && dev < VQ_MAX_DEVICES && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n * per_cu;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    if (dev >= 0 && dev < VQ_MAX_DEVICES) cus[dev].store(n, std::memory_order_relaxed);
    return n * per_cu;
}

// The streamed form of the all-fp32 pass over a whole batch (run_exact_tiled in vqhip_exact.hip decides when), launched from
// this unit: vqhip_core.h says why.
template <int MODE>
int run_exact_stream(const void *x, int bf, const float *e, const float *en, const float *xn, int64_t N, int64_t K, int D, int metric,
                     u64 *keys, float *dout, int64_t items, hipStream_t s) {
    static LdsCache ssets[2];
    const int lds = vq_xs_lds_bytes(bf);
    const void *kern = bf ? (const void *)exact_stream_kernel<1, MODE> : (const void *)exact_stream_kernel<0, MODE>;
    if (int rc = ensure_dyn_lds(kern, lds, ssets[bf])) return rc;
    const int cap = resident_grid(2);
    const int grid = (int)(items < cap ? items : cap);
    if (bf) exact_stream_kernel<1, MODE><<<grid, 256, lds, s>>>(x, e, en, xn, N, K, D, metric, keys, dout);
    else exact_stream_kernel<0, MODE><<<grid, 256, lds, s>>>(x, e, en, xn, N, K, D, metric, keys, dout);
    VQ_CHECK_LAUNCH("exact_stream_kernel");
    return VQHIP_OK;
}
template int run_exact_stream<0>(const void *, int, const float *, const float *, const float *, int64_t, int64_t, int, int, u64 *, float *, int64_t, hipStream_t);
template int run_exact_stream<1>(const void *, int, const float *, const float *, const float *, int64_t, int64_t, int, int, u64 *, float *, int64_t, hipStream_t);
template int run_exact_stream<2>(const void *, int, const float *, const float *, const float *, int64_t, int64_t, int, int, u64 *, float *, int64_t, hipStream_t);

extern "C" {

int64_t vqhip_codebook_exact_offset(int64_t K, int D) {
    if (K <= 0 || D <= 0) return -1;
    return vq_cb_layout(K, D).off_eexact;
}

int64_t vqhip_codebook_bytes(int64_t K, int D) {
    if (K <= 0 || D <= 0) return 0;
    return vq_cb_layout(K, D).total;
}

int64_t vqhip_workspace_bytes(int64_t N, int64_t K, int D) {
    if (N < 0 || K <= 0 || D <= 0) return 0;
    return vq_ws_layout(N > 0 ? N : 1, K, D).total;
}

// metric may carry the internal words (VQ_METRIC_DOT, VQ_METRIC_SWAP)
static int codebook_prepare_impl(const float *e, int64_t K, int D, int metric, void *cb, void *stream) {
    if (K >= (1ll << 31)) return fail(VQHIP_EINVAL, "vqhip_codebook_prepare: K too large");
    hipStream_t s = (hipStream_t)stream;
    VqCbLayout L = vq_cb_layout(K, D);
    char *c = (char *)cb;
    if (VQ_IS_COS(metric) && vq_coarse_supported(D)) {      // cosine: statistics and image in ONE launch (cb_cos_body)
        cb_cos_kernel<<<(int)(L.nstages * L.tps), 256, 0, s>>>(e, K, D, metric, c, L);
        VQ_CHECK_LAUNCH("cb_cos_kernel");
        return VQHIP_OK;
    }
    cb_stats_kernel<<<(int)((K + 15) / 16), 256, 0, s>>>(e, K, D, metric, c, L);
    VQ_CHECK_LAUNCH("cb_stats_kernel");
    if (vq_coarse_supported(D)) {
        cb_image_kernel<<<(int)(L.nstages * L.tps), 256, 0, s>>>(e, K, D, metric, c, L);
        VQ_CHECK_LAUNCH("cb_image_kernel");
    }
    return VQHIP_OK;
}

int vqhip_codebook_prepare(const float *e, int64_t K, int D, int metric, void *cb, int64_t cb_bytes, void *stream) {
    VQ_REQUIRE(e && cb && K > 0 && D > 0 && vq_public_metric(metric), "vqhip_codebook_prepare: bad argument");
    VQ_NEED("vqhip_codebook_prepare: cb too small", cb_bytes, vqhip_codebook_bytes(K, D));
    return codebook_prepare_impl(e, K, D, metric, cb, stream);
}

// The proposal + decision pipeline: N rows `x` against the K codes whose prepared image is `cb` and whose fp32 rows
// (as used by the exact definition) are `e_exact`.  `metric` may carry the internal words (DOT, SWAP).
// tokens: what the front of the call (encode_fused_front) left in `ws`; VQ_TOKENS_UNPREPARED: the token side is made here
// n_dev (nullable DEVICE int): only rows [0, min(N, *n_dev)) are live; the launches are sized for N
static int argmin_pipeline(const void *x, int x_dtype, const float *e_exact, const void *cb, int64_t N, int64_t K, int D,
                           int metric, int64_t *idx, int32_t *hist, void *ws, void *stream, VqTokenSide tokens = VQ_TOKENS_UNPREPARED,
                           const int *n_dev = nullptr) {
    hipStream_t s = (hipStream_t)stream;
    VqCbLayout L = vq_cb_layout(K, D);
    VqWsLayout W = vq_ws_layout(N, K, D);
    const VqWsView V = vq_ws_view(ws, W);
    const char *c = (const char *)cb;
    const int64_t Np = (N + 63) / 64 * 64;
    const float *en = (const float *)(c + L.off_en);

    int nslices = 1, rc;
    // no token image: the proposal kernel converts the rows it loads (coarse_kernel<..., XD>); the front only does the housekeeping
    bool xd = tokens == VQ_TOKENS_ROWS;
    if (tokens == VQ_TOKENS_UNPREPARED) {
        xd = vq_xdirect(N, K, D, x_dtype, metric, n_dev);
        int xgrid = (int)((N + 31) / 32);
        if (xd) xgrid = xgrid < 64 ? xgrid : 64;
        const int narrive = (int)W.narrive;      // arrival counters + the group path's bucket counters (one zeroed range)
        if (x_dtype == VQHIP_DTYPE_F32) x_prep_kernel<0><<<xgrid, 256, 0, s>>>(x, N, D, L.nstep, V.ximg, V.xh2, V.rho2, V.xn, V.counters, (char *)cb, L, V.arrive, narrive, xd);
        else x_prep_kernel<1><<<xgrid, 256, 0, s>>>(x, N, D, L.nstep, V.ximg, V.xh2, V.rho2, V.xn, V.counters, (char *)cb, L, V.arrive, narrive, xd);
        VQ_CHECK_LAUNCH("x_prep_kernel");
    }
    // the proposal kernel also runs the decision stage (the workgroup that completes a token block merges its slices)
    VqDecideOut dec{idx, hist, V.rescan_list, V.multi_list, V.exact_list, V.counters, V.keys, V.thr, V.rescan_cnt, V.arrive, n_dev,
                    x, V.xh2, V.rho2, V.xn};
    VqDecideOut dec_arg = dec;                   // launch_coarse decides (slice count, batch size) whether the proposal kernel runs the
    int fused_done = 0;                          // decision stage itself and reports it here
    // D <= 32 group path: request lists of the proposal kernel (cap = an equal share of the pool per code tile, whole batches of 32)
    VqGroupLists grp{nullptr, nullptr, nullptr, nullptr, 0, 1, 0};
    VqGroupRun grun{0, 0, 0, -1};
    const int ntiles_cb = (int)(L.nstages * L.tps);
    int nbuckets = 0;
    if (W.nbkt > 0 && ntiles_cb <= VQ_GROUP_MAX_TILES && N < (1ll << 30)) {
        grp.R = vq_group_replicas(ntiles_cb / VQ_GROUP_TILES);
        nbuckets = ntiles_cb / VQ_GROUP_TILES * grp.R;
        grp.bcnt = V.bcnt; grp.blist = V.blist; grp.bfrag = V.bfrag; grp.rece2 = V.rece2;
        grp.cap = (int)(W.blist_entries / nbuckets / 32 * 32);
        uint32_t bits = 1;                                   // group ids ride in the low mantissa bits of the running group maxima
        while ((1u << bits) < (uint32_t)(ntiles_cb / VQ_GROUP_TILES)) ++bits;
        grp.idmask = (1u << bits) - 1u;
    }
    rc = launch_coarse(V.ximg, N, L, c + L.off_frag, V.rec, Np, (const VqCbStats *)(c + L.off_stats), V.xh2, V.rho2, metric, dec_arg, &nslices, &fused_done, s, grp, &grun, xd);
    if (rc) return rc;
    const float *rece2 = nullptr;
    if (grun.used) {             // identify the group records: one candidate per request, written into the records
        const int igrid = (nbuckets + 3) / 4;                   // one wave per bucket
        if (grun.ks == 1) identify32_kernel<1, VQ_GROUP_TILES><<<igrid, 256, 0, s>>>(c + L.off_frag, L.nstages, nslices, nbuckets, V.rec, Np, (const VqCbStats *)(c + L.off_stats), grp, grun.pad_stage, grun.noaux);
        else identify32_kernel<2, VQ_GROUP_TILES><<<igrid, 256, 0, s>>>(c + L.off_frag, L.nstages, nslices, nbuckets, V.rec, Np, (const VqCbStats *)(c + L.off_stats), grp, grun.pad_stage, grun.noaux);
        VQ_CHECK_LAUNCH("identify32_kernel");
        rece2 = grp.rece2;
    }
    if (!fused_done) {
        // (1024-thread workgroups: 256 and 512 measured 1-2 % slower per encode at configs[2] and the tokenizer shape, level at D = 256)
        refine_decide_kernel<<<(int)((N + 1023) / 1024), 1024, 0, s>>>(c, L, N, metric, nslices, V.rec, V.xh2, V.rho2, Np, dec, rece2);
        VQ_CHECK_LAUNCH("refine_decide_kernel");
    }
    // second-chance proposals for rows with a possibly unidentified candidate (the kernel gathers their fragments from
    // the token image itself) ...
    {
        const char *frag = c + L.off_frag;
        int rrc = VQHIP_OK;
        if (xd) rrc = launch_rescan_cfg<16, 2, 8, VQ_TPS16, 4, 1>(V.ximg, frag, L.nstages, V.rescan_list, V.counters, V.thr, V.rescan_cnt, V.cand_list, s, x);
        else switch (L.nstep) {
#define VQ_RESCAN(NS, TT, ...) case NS: rrc = launch_rescan_cfg<NS, TT, 8, __VA_ARGS__>(V.ximg, frag, L.nstages, V.rescan_list, V.counters, V.thr, V.rescan_cnt, V.cand_list, s); break;
            VQ_RESCAN(2, 2, VQ_TPS_D32, 4) VQ_RESCAN(4, 2, 4, 4) VQ_RESCAN(8, 2, 4, 4) VQ_RESCAN(16, 2, VQ_TPS16, 4) VQ_RESCAN(32, 2, 2) VQ_RESCAN(48, 2, 1) VQ_RESCAN(64, 1, 1)
#undef VQ_RESCAN
            default: return fail(VQHIP_EINVAL, "vqhip_argmin: unsupported padded D");
        }
        if (rrc) return rrc;
        VQ_CHECK_LAUNCH("rescan_kernel");
    }
    // ... then ONE launch re-ranks exactly both the rows with several identified candidates (one lane per (row, record
    // slot)) and the rescanned rows' candidate lists
    {
        int S0 = 4;                                           // slot lanes per multi row: power of two >= max(4, 2*nslices)
        while (S0 < 2 * nslices) S0 <<= 1;
        // the re-rank is a latency chain per (row, candidate) pair: it wants one row per wave however short the queues
        // are (64 + 64 workgroups made it 80 us instead of 14 at N = 3072, cosine, 16 slices); idle workgroups exit at once
        const int64_t g0 = 2048, g1 = 1024;
#define VQ_RERANK(DT) refine_rerank_kernel<DT><<<(int)(g0 + g1), 256, 0, s>>>(x, e_exact, c, L, D, metric, nslices, S0, (int)g0, V.rec, V.xh2, V.rho2, \
        V.xn, Np, idx, hist, V.multi_list, V.rescan_list, V.counters, V.rescan_cnt, V.cand_list, V.exact_list, V.keys, grun.used)
        if (x_dtype == VQHIP_DTYPE_F32) VQ_RERANK(0); else VQ_RERANK(1);
#undef VQ_RERANK
        VQ_CHECK_LAUNCH("refine_rerank_kernel");
    }
    // last resort: whole-codebook fp32 pass (non-finite data, overflowing candidate lists)
    if (const int force = g_tune_force_exact.load()) {
        if (int frc = force_exact_rows((int)(force < N ? force : N), V.exact_list, V.counters, V.keys, s)) return frc;
    }
    return run_exact_rows(x, x_dtype, e_exact, en, V.xn, N, K, D, metric, V.exact_list, V.counters + 2, V.keys, V.counters + 3, idx, hist, s);
}

// Front of an encode whose codebook image is made in the same call: ONE launch for the codebook statistics and the whole
// token side (they are independent), then the image kernel.  `rows` are the N rows to quantize (normalised into `xq`
// first when xnorm), `codes` the Kc rows the image is made from, `ws` the workspace of argmin_pipeline(N rows, Kc codes).
// hw > 0: `rows` is the feature map [N / hw, D, hw] (NCHW); the token-major rows go to `xrows` (input dtype; cosine: xq)
// grows != nullptr (vqhip_col_argmin_rows, fp32 `rows` = the codebook, no normalisation): row t of the call is rows[grows[t]] for
// t < *gcount and zeros up to N; the gathered rows are written to `xrows`
// *tokens: the form of the token side argmin_pipeline is to go on from
static int encode_fused_front(const void *rows, int rows_dtype, int64_t N, const float *codes, int64_t Kc, int D, int cb_metric,
                              void *cb, void *ws, bool xnorm, float *xq, VqTokenSide *tokens, hipStream_t s, int32_t *hist_zero = nullptr,
                              int64_t hw = 0, void *xrows = nullptr, const int32_t *grows = nullptr, const int32_t *gcount = nullptr) {
    VqCbLayout L = vq_cb_layout(Kc, D);
    VqWsLayout W = vq_ws_layout(N, Kc, D);
    const VqWsView V = vq_ws_view(ws, W);
    char *c = (char *)cb;
    // cosine: the whole codebook preparation rides in the same launch (normalised rows need no statistics pass for their
    // scale).  DOT — the role-swapped NearestAnchor pass under the cosine metric, whose operands the caller has normalised
    // (include/vqhip.h: "COS: x and e already normalised") — takes the same form on the rows as given: constant scale 2^13,
    // the tile maxima from the actual data (rows that are not unit-norm keep exact results: values beyond fp16 range at that
    // scale raise the non-finite flag and the rows take the fp32 pass)
    const bool cosimg = VQ_IS_COS(cb_metric) || (cb_metric & 3) == VQ_METRIC_DOT;
    const int nblk_stats = cosimg ? (int)(L.nstages * L.tps) : (int)((Kc + 15) / 16);
    // the pipeline is handed the rows given here (hw > 0: their token-major copy), no normalisation, no gather: where the proposal kernel
    // makes its own fragments of them (vq_xdirect) the token side is housekeeping only (hw > 0: the blocks that write the copy still run in full)
    const bool xd = !xnorm && grows == nullptr && vq_xdirect(N, Kc, D, rows_dtype, cb_metric, nullptr);
    *tokens = xd ? VQ_TOKENS_ROWS : VQ_TOKENS_IMAGE;
    const int toff = (xd && hw == 0) ? 1 : 0;
    int xgrid = (int)((N + 31) / 32);
    if (toff) xgrid = xgrid < 64 ? xgrid : 64;
#define VQ_PRE_ARGS codes, Kc, cb_metric, c, L, nblk_stats, rows, N, D, L.nstep, V.ximg, V.xh2, V.rho2, V.xn, V.counters, V.arrive, (int)W.narrive, xq, 1e-12f, hist_zero, hw, xrows
#define VQ_PRE(DT, XN, MAP, COSI) pre_kernel<DT, XN, MAP, COSI><<<nblk_stats + xgrid, 256, 0, s>>>(VQ_PRE_ARGS, nullptr, nullptr, toff)
#define VQ_PRE2(DT, XN, MAP) do { if (cosimg) VQ_PRE(DT, XN, MAP, true); else VQ_PRE(DT, XN, MAP, false); } while (0)
    if (grows != nullptr) {
        if (rows_dtype != VQHIP_DTYPE_F32 || xnorm || hw > 0 || L.nstep == 2) return fail(VQHIP_EINVAL, "encode_fused_front: gather form");
        if (cosimg) pre_kernel<0, false, false, true, true><<<nblk_stats + xgrid, 256, 0, s>>>(VQ_PRE_ARGS, grows, gcount);
        else pre_kernel<0, false, false, false, true><<<nblk_stats + xgrid, 256, 0, s>>>(VQ_PRE_ARGS, grows, gcount);
    } else
    if (hw > 0) {
        if (rows_dtype == VQHIP_DTYPE_F32) { if (xnorm) VQ_PRE2(0, true, true); else VQ_PRE2(0, false, true); }
        else { if (xnorm) VQ_PRE2(1, true, true); else VQ_PRE2(1, false, true); }
    } else {
        if (rows_dtype == VQHIP_DTYPE_F32) { if (xnorm) VQ_PRE2(0, true, false); else VQ_PRE2(0, false, false); }
        else { if (xnorm) VQ_PRE2(1, true, false); else VQ_PRE2(1, false, false); }
    }
#undef VQ_PRE2
#undef VQ_PRE
#undef VQ_PRE_ARGS
    VQ_CHECK_LAUNCH("pre_kernel");
    if (cosimg) return VQHIP_OK;
    cb_image_kernel<<<(int)(L.nstages * L.tps), 256, 0, s>>>(codes, Kc, D, cb_metric, c, L);
    VQ_CHECK_LAUNCH("cb_image_kernel");
    return VQHIP_OK;
}

int vqhip_encode(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, void *cb, int64_t cb_bytes,
                 int64_t *idx, int32_t *hist, float *xq, void *ws, int64_t ws_bytes, void *stream) {
    return vqhip_encode_ex(x, x_dtype, e, N, K, D, metric, cb, cb_bytes, idx, hist, xq, ws, ws_bytes, 0, stream);
}

int vqhip_encode_ex(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric, void *cb, int64_t cb_bytes,
                    int64_t *idx, int32_t *hist, float *xq, void *ws, int64_t ws_bytes, int flags, void *stream) {
    const bool zero_hist = hist != nullptr && (flags & VQHIP_ENCODE_ZERO_HIST) != 0;
    if (N == 0 || !vq_coarse_supported(D)) {                 // paths without the fused front: plain memset
        if (zero_hist && K > 0) VQ_HIP(hipMemsetAsync(hist, 0, (size_t)K * 4, (hipStream_t)stream));
    }
    if (N == 0) return e && cb && K > 0 && D > 0 ? vqhip_codebook_prepare(e, K, D, metric, cb, cb_bytes, stream) : fail(VQHIP_EINVAL, "vqhip_encode: bad argument");
    if (!x || !e || !cb || !idx || !ws || N < 0 || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_encode: bad argument");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_encode: metric");
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_encode: x_dtype");
    if (VQ_IS_COS(metric) && !xq) return fail(VQHIP_EINVAL, "vqhip_encode: the cosine metric needs the xq buffer");
    VQ_REQUIRE(vq_fits_i31(N, K), "vqhip_encode: N or K too large");
    VQ_NEED("vqhip_encode: cb too small", cb_bytes, vqhip_codebook_bytes(K, D));
    VQ_NEED("vqhip_encode: ws too small", ws_bytes, vqhip_workspace_bytes(N, K, D));
    if (!vq_coarse_supported(D)) {          // no fp16 proposal image for this D: the separate entry points do the work
        if (int rc = vqhip_codebook_prepare(e, K, D, metric, cb, cb_bytes, stream)) return rc;
        const void *rows = x; int rows_dtype = x_dtype;
        if (VQ_IS_COS(metric)) {
            if (VQ_IS_BF16(metric)) return fail(VQHIP_EINVAL, "vqhip_encode: the bf16-autocast cosine metric needs D <= 1024, D % 8 == 0");
            if (int rc = vqhip_normalize_rows(x, x_dtype, N, D, 1e-12f, xq, stream)) return rc;
            rows = xq; rows_dtype = VQHIP_DTYPE_F32;
        }
        return vqhip_argmin(rows, rows_dtype, e, cb, cb_bytes, N, K, D, metric, idx, hist, ws, ws_bytes, stream);
    }
    hipStream_t s = (hipStream_t)stream;
    const bool cos = VQ_IS_COS(metric);
    VqTokenSide tokens;
    if (int rc = encode_fused_front(x, x_dtype, N, e, K, D, metric, cb, ws, cos, xq, &tokens, s, zero_hist ? hist : nullptr)) return rc;
    VqCbLayout L = vq_cb_layout(K, D);
    const float *e_exact = cos ? (const float *)((const char *)cb + L.off_eexact) : e;
    // from here on the rows are what vqhip_argmin would have been given: the normalised fp32 rows for cosine
    return argmin_pipeline(cos ? (const void *)xq : x, cos ? VQHIP_DTYPE_F32 : x_dtype, e_exact, cb, N, K, D, metric, idx, hist, ws,
                           stream, tokens);
}

int vqhip_encode_map(const void *x_map, int x_dtype, const float *e, int64_t B, int64_t HW, int64_t K, int D, int metric, void *cb,
                     int64_t cb_bytes, int64_t *idx, int32_t *hist, void *xrows, float *xq, void *ws, int64_t ws_bytes, int flags,
                     void *stream) {
    const int64_t N = B * HW;
    if (!x_map || !e || !cb || !idx || !xrows || !ws || B <= 0 || HW <= 0 || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_encode_map: bad argument");
    if (VQ_IS_COS(metric) && !xq) return fail(VQHIP_EINVAL, "vqhip_encode_map: the cosine metric needs the xq buffer");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_encode_map: metric");
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_encode_map: x_dtype");
    VQ_REQUIRE(vq_fits_i31(N, K), "vqhip_encode_map: N or K too large");
    if (!vq_coarse_supported(D)) return fail(VQHIP_EINVAL, "vqhip_encode_map: needs D <= 1024, D % 8 == 0 (transpose and use vqhip_encode)");
    VQ_NEED("vqhip_encode_map: cb too small", cb_bytes, vqhip_codebook_bytes(K, D));
    VQ_NEED("vqhip_encode_map: ws too small", ws_bytes, vqhip_workspace_bytes(N, K, D));
    hipStream_t s = (hipStream_t)stream;
    const bool cos = VQ_IS_COS(metric);
    const bool zero_hist = hist != nullptr && (flags & VQHIP_ENCODE_ZERO_HIST) != 0;
    VqTokenSide tokens;
    if (int rc = encode_fused_front(x_map, x_dtype, N, e, K, D, metric, cb, ws, cos, cos ? xq : nullptr, &tokens, s,
                                    zero_hist ? hist : nullptr, HW, xrows)) return rc;
    VqCbLayout L = vq_cb_layout(K, D);
    const float *e_exact = cos ? (const float *)((const char *)cb + L.off_eexact) : e;
    // from here on the rows are token-major: what the front wrote (L2: the copy in the input dtype; cosine: the normalised fp32 rows)
    return argmin_pipeline(cos ? (const void *)xq : (const void *)xrows, cos ? VQHIP_DTYPE_F32 : x_dtype, e_exact, cb, N, K, D, metric,
                           idx, hist, ws, stream, tokens);
}

int vqhip_argmin(const void *x, int x_dtype, const float *e, const void *cb, int64_t cb_bytes, int64_t N, int64_t K, int D, int metric,
                 int64_t *idx, int32_t *hist, void *ws, int64_t ws_bytes, void *stream) {
    if (N == 0) return VQHIP_OK;
    if (!x || !cb || !idx || !ws || N < 0 || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_argmin: bad argument");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_argmin: metric");
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_argmin: x_dtype");
    if (metric == VQHIP_METRIC_L2 && !e) return fail(VQHIP_EINVAL, "vqhip_argmin: e is required for L2");
    VQ_REQUIRE(vq_fits_i31(N, K), "vqhip_argmin: N or K too large");
    VQ_NEED("vqhip_argmin: cb too small", cb_bytes, vqhip_codebook_bytes(K, D));
    VQ_NEED("vqhip_argmin: ws too small", ws_bytes, vqhip_workspace_bytes(N, K, D));
    VqCbLayout L = vq_cb_layout(K, D);
    const float *e_exact = VQ_IS_COS(metric) ? (const float *)((const char *)cb + L.off_eexact) : e;
    if (!vq_coarse_supported(D)) {
        // no fp16 proposal image for this D: whole-codebook fp32 pass for every row
        VQ_HIP(hipMemsetAsync(ws, 0, 256, (hipStream_t)stream));
        return vqhip_argmin_exact(x, x_dtype, e_exact, N, K, D, metric, idx, nullptr, hist, ws, ws_bytes, stream);
    }
    return argmin_pipeline(x, x_dtype, e_exact, cb, N, K, D, metric, idx, hist, ws, stream);
}

// the latents as the fp32 rows an image is made from: themselves, or (bf16) their copy in `copy`
static int latents_as_f32(const void *x, int x_dtype, int64_t N, int D, float *copy, hipStream_t s, const float **rows) {
    *rows = (const float *)x;
    if (x_dtype != VQHIP_DTYPE_BF16) return VQHIP_OK;
    int64_t n = N * (int64_t)D;
    int grid = (int)((n + 255) / 256); grid = grid > 4096 ? 4096 : grid;
    bf16_to_f32_kernel<<<grid, 256, 0, s>>>((const uint16_t *)x, n, copy);
    VQ_CHECK_LAUNCH("bf16_to_f32_kernel");
    *rows = copy;
    return VQHIP_OK;
}

int64_t vqhip_col_workspace_bytes(int64_t N, int64_t K, int D) {
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    const int64_t legacy = vq_ws_layout(N, K, D).total;        // fp32-only route (D without a proposal image)
    const int64_t t = vq_col_layout(K, N, D, false).total;
    return t > legacy ? t : legacy;
}

int vqhip_col_argmin(const void *x, int x_dtype, const float *e, int64_t N, int64_t K, int D, int metric,
                     int64_t *col_idx, void *ws, int64_t ws_bytes, void *stream) {
    if (!x || !e || !col_idx || !ws || N <= 0 || K <= 0 || D <= 0) return fail(VQHIP_EINVAL, "vqhip_col_argmin: bad argument");
    VQ_REQUIRE(vq_fits_i31(N, K), "vqhip_col_argmin: N or K too large");
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_col_argmin: x_dtype");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_col_argmin: metric");
    VQ_NEED("vqhip_col_argmin: ws too small", ws_bytes, vqhip_col_workspace_bytes(N, K, D));
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws;
    if (vq_coarse_supported(D)) {
        const VqColLayout C = vq_col_layout(K, N, D, false);
        char *pipe_ws = w, *img = w + C.off_img;
        const float *codes;
        if (int rc = latents_as_f32(x, x_dtype, N, D, (float *)(w + C.off_copy), s, &codes)) return rc;
        const int m = vq_swapped_metric(metric);
        // statistics of the latents-as-codebook and the token side of the codes-as-rows in one launch, then the image
        VqTokenSide tokens;
        if (int rc = encode_fused_front(e, VQHIP_DTYPE_F32, K, codes, N, D, m, img, pipe_ws, false, nullptr, &tokens, s)) return rc;
        return argmin_pipeline(e, VQHIP_DTYPE_F32, codes, img, K, N, D, m, col_idx, nullptr, pipe_ws, stream, tokens);
    }
    // D without a proposal image: the fp32-only route with one key per code
    return exact_whole_cols(x, x_dtype, e, N, K, D, metric, vq_ws_view(ws, vq_ws_layout(N, K, D)), col_idx, s);
}

// ---- the column pass over a SHORT list, directly in fp32 ----------------------------------------------------------------
// NearestAnchor over the listed codes is the proposal pipeline with the roles swapped: 5 launches, ~65 us at 3072 tokens x 256
// dims (83 at 6272 x 768) however few codes are listed — and a CVQ-VAE run in its steady state lists a few dozen.  For such a
// list the whole-codebook fp32 pass of the pipeline (exact_kernel: the oracle's k-ordered fma chains, the definition itself)
// IS the cheaper way to the same indices: listed rows x all tokens, one launch behind a tiny one that arms the keys.
// Limit: the pass's work items (32 listed rows x 128 tokens each, a chain of D/2 dependent fp32 MFMAs of 64 cycles) times D —
// up to about one item per SIMD of the chip at D = 256 the pass is one chain long (4-12 us); beyond, the proposal pipeline wins.
#ifndef VQ_COL_DIRECT_MAX_WORK
#define VQ_COL_DIRECT_MAX_WORK (1ll << 18)
#endif
static bool col_direct_ok(int x_dtype, int metric, int64_t cap, int64_t N, int64_t K, int D, int64_t ws_bytes) {
    if (cap <= 0 || (D % 4) != 0) return false;
    if (x_dtype != VQHIP_DTYPE_F32) return false;        // the pass reads the tokens as fp32 rows, whatever the metric
    if (((cap + 31) / 32) * ((N + 127) / 128) * (int64_t)D > VQ_COL_DIRECT_MAX_WORK) return false;
    return ws_bytes >= vq_col_direct_layout(N, K).total;
}

int64_t vqhip_col_rows_workspace_bytes(int64_t N, int64_t cap, int D) {
    if (N <= 0 || cap <= 0 || D <= 0 || !vq_coarse_supported(D)) return 0;
    // (the direct form of a short list, col_rows_direct, lives in the same buffer: 12 K + 4 N bytes — it is taken only where the
    //  buffer it is handed is large enough for it, which the size below is unless K exceeds ~N D / 2)
    return vq_col_layout(cap, N, D, true).total;
}

int vqhip_col_argmin_rows(const void *x, int x_dtype, const float *e, const int32_t *rows, const int32_t *count, int64_t cap,
                          int64_t N, int64_t K, int D, int metric, int64_t *col_idx, void *ws, int64_t ws_bytes, void *stream) {
    if (!x || !e || !rows || !count || !col_idx || !ws || N <= 0 || K <= 0 || D <= 0 || cap < 0 || cap > K)
        return fail(VQHIP_EINVAL, "vqhip_col_argmin_rows: bad argument");
    if (cap == 0) return VQHIP_OK;
    if (!vq_coarse_supported(D)) return fail(VQHIP_EINVAL, "vqhip_col_argmin_rows: needs D <= 1024, D % 8 == 0 (use vqhip_col_argmin)");
    VQ_REQUIRE(vq_fits_i31(N, K), "vqhip_col_argmin_rows: N or K too large");
    VQ_REQUIRE(vq_row_dtype(x_dtype), "vqhip_col_argmin_rows: x_dtype");
    VQ_REQUIRE(vq_public_metric(metric), "vqhip_col_argmin_rows: metric");
    VQ_NEED("vqhip_col_argmin_rows: ws too small", ws_bytes, vqhip_col_rows_workspace_bytes(N, cap, D));
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws;
    if (col_direct_ok(x_dtype, metric, cap, N, K, D, ws_bytes))      // a short list: the fp32 pass itself, two launches (four for L2)
        return col_rows_direct(x, e, rows, count, cap, N, K, D, metric, col_idx, w, nullptr, nullptr, s);
    const VqColLayout C = vq_col_layout(cap, N, D, true);
    char *pipe_ws = w, *img = w + C.off_img;
    float *esub = (float *)(w + C.off_rows);
    // the gather of the listed rows rides in the front launch of the pipeline (token side of pre_kernel) except at a padded
    // dimension of 32, whose token side is the wave-level form
    const bool fused_gather = vq_cb_layout(N, D).nstep != 2;
    if (!fused_gather) {
        gather_listed_rows_kernel<<<waves_grid(cap, 4), 256, 0, s>>>(e, rows, count, cap, D, esub);
        VQ_CHECK_LAUNCH("gather_listed_rows_kernel");
    }
    const float *codes;
    if (int rc = latents_as_f32(x, x_dtype, N, D, (float *)(w + C.off_copy), s, &codes)) return rc;
    // the role-swapped pipeline of vqhip_col_argmin on the listed codes: sized for `cap` rows, live for *count of them
    const int m = vq_swapped_metric(metric);
    VqTokenSide tokens;
    int rc = fused_gather ? encode_fused_front(e, VQHIP_DTYPE_F32, cap, codes, N, D, m, img, pipe_ws, false, nullptr, &tokens, s, nullptr, 0, esub, rows, count)
                          : encode_fused_front(esub, VQHIP_DTYPE_F32, cap, codes, N, D, m, img, pipe_ws, false, nullptr, &tokens, s);
    if (rc) return rc;
    return argmin_pipeline(esub, VQHIP_DTYPE_F32, codes, img, cap, N, D, m, col_idx, nullptr, pipe_ws, stream, tokens, count);
}

int vqhip_argmin_stats(const void *ws, int32_t *out, void *stream) {
    if (!ws || !out) return fail(VQHIP_EINVAL, "vqhip_argmin_stats: bad argument");
    VQ_HIP(hipMemcpyAsync(out, ws, 16, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VQHIP_OK;
}

int vqhip_debug_proposal_scores(const void *x, int x_dtype, const void *cb, int64_t N, int64_t K, int D, int metric,
                                float *scores, float *margin, float *scale, void *ws, int64_t ws_bytes, void *stream) {
    if (!x || !cb || !scores || !margin || !scale || !ws || N <= 0 || K <= 0 || !vq_coarse_supported(D))
        return fail(VQHIP_EINVAL, "vqhip_debug_proposal_scores: bad argument");
    VQ_NEED("vqhip_debug_proposal_scores: ws too small", ws_bytes, vqhip_workspace_bytes(N, K, D));
    hipStream_t s = (hipStream_t)stream;
    VqCbLayout L = vq_cb_layout(K, D);
    const VqWsView V = vq_ws_view(ws, vq_ws_layout(N, K, D));
    const char *c = (const char *)cb;
    const int xgrid = (int)((N + 31) / 32);
    if (x_dtype == VQHIP_DTYPE_F32) x_prep_kernel<0><<<xgrid, 256, 0, s>>>(x, N, D, L.nstep, V.ximg, V.xh2, V.rho2, V.xn, V.counters, (char *)cb, L);
    else if (x_dtype == VQHIP_DTYPE_BF16) x_prep_kernel<1><<<xgrid, 256, 0, s>>>(x, N, D, L.nstep, V.ximg, V.xh2, V.rho2, V.xn, V.counters, (char *)cb, L);
    else return fail(VQHIP_EINVAL, "vqhip_debug_proposal_scores: x_dtype");
    VQ_CHECK_LAUNCH("x_prep_kernel");
    const char *frag = c + L.off_frag;
    switch (L.nstep) {
#define VQ_DBG(NS, TPS) case NS: debug_scores_kernel<NS, TPS><<<512, 256, 0, s>>>(V.ximg, frag, L.nstages, N, K, scores); break;
        VQ_DBG(2, VQ_TPS_D32) VQ_DBG(4, 4) VQ_DBG(8, 4) VQ_DBG(16, VQ_TPS16) VQ_DBG(32, 2) VQ_DBG(48, 1) VQ_DBG(64, 1)
#undef VQ_DBG
        default: return fail(VQHIP_EINVAL, "vqhip_debug_proposal_scores: unsupported padded D");
    }
    VQ_CHECK_LAUNCH("debug_scores_kernel");
    debug_margin_kernel<<<(int)((N + 255) / 256), 256, 0, s>>>(c, L, N, metric, V.xh2, V.rho2, margin, scale);
    VQ_CHECK_LAUNCH("debug_margin_kernel");
    return VQHIP_OK;
}

}  // extern "C"
int vq_tune_stream() { return g_tune_stream.load(); }
extern "C" {

int vqhip_set_tuning(int key, int value) {
    if (key == 2) g_tune_slices = (value == 1 || value == 2 || value == 4 || value == 8 || value == 16) ? value : 0;
    else if (key == 18) g_tune_stream = value != 0;
    else if (key == 12) g_tune_force_exact = value > 0 ? (value < 1024 ? value : 1024) : 0;
    else return fail(VQHIP_EINVAL, "vqhip_set_tuning: unknown key");
    return VQHIP_OK;
}

int vqhip_profile_enable(int on) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof_on = on != 0;
    g_prof_used = 0;
    return VQHIP_OK;
}

int vqhip_profile_collect(double *ms_sum, int64_t *launches) {
    if (!ms_sum || !launches) return fail(VQHIP_EINVAL, "vqhip_profile_collect: bad argument");
    std::lock_guard<std::mutex> lock(g_prof_mu);
    double total = 0.0;
    for (size_t i = 0; i < g_prof_used; ++i) {
        VQ_HIP(hipEventSynchronize(g_prof_events[i].second));
        float ms = 0.0f;
        VQ_HIP(hipEventElapsedTime(&ms, g_prof_events[i].first, g_prof_events[i].second));
        total += ms;
    }
    *ms_sum = total;
    *launches = (int64_t)g_prof_used;
    g_prof_used = 0;
    return VQHIP_OK;
}

}  // extern "C"
