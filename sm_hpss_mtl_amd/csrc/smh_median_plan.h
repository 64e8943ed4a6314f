// Launch plan of the HPSS median filters (smh_median.hip; kernels: smh_median_kernel.h, smh_median_split.h): which kernel family a call
// takes, which harm layout it writes, how the clip is tiled and the tile's lines are shared among the waves, on which grid with how
// much LDS, and how the block-split kernel stages a whole clip -- decided here, once, as a plain value.  The five entry points, the
// fused pipeline (launch_hpss), the ragged launch, the routers of the front ends (smh_frontend.hip, smh_ragged.hip) and the test query
// (smh_internal_median_plan) all take it from these functions.  Host arithmetic only, no HIP: a stand-alone host program can include
// this header by itself.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "smh_xcd.h"

namespace smh_median {

constexpr int kLdsBytesPerCU = 160 * 1024;  // smh_common.h: smh::kLdsBytesPerCU (held equal in smh_median.hip)

// The implementation switches of the median launches (A/B runs, tuning, tests), the only getenv of these launches.  Read once per call
// of a public entry point and handed down: tests flip them between calls.  (SMH_MEDIAN_PROBE_NOLOAD makes outputs invalid: a probe_env
// read in the launcher, an input of the plan.)
struct MedianSwitches {
    bool nosplit = false;            // SMH_MEDIAN_NOSPLIT set: neither the block-split nor the persistent kernel
    int persist = -1;                // SMH_MEDIAN_PERSIST=0 / 1: never / whenever it can run; unset (-1): windows above 17
    int pthreads = 512;              // SMH_MEDIAN_PTHREADS: the 512 / 768 / 1024-thread persistent build (tools/gpu/tune_split.sh)
    bool seg = false;                // SMH_MEDIAN_SEG="nsh,nsp": the segment counts (tools/tune_median.py)
    int seg_h = 0, seg_p = 0;
    bool dma = true;                 // SMH_MEDIAN_DMA_STAGE=0: the block-split kernel stages whole clips through registers; same bits
};
inline MedianSwitches read_median_switches() {
    MedianSwitches s;
    s.nosplit = getenv("SMH_MEDIAN_NOSPLIT") != nullptr;
    const char *ev = getenv("SMH_MEDIAN_PERSIST");
    if (ev) s.persist = atoi(ev) != 0;
    if ((ev = getenv("SMH_MEDIAN_PTHREADS"))) s.pthreads = atoi(ev);
    if ((ev = getenv("SMH_MEDIAN_SEG"))) s.seg = sscanf(ev, "%d,%d", &s.seg_h, &s.seg_p) == 2;
    ev = getenv("SMH_MEDIAN_DMA_STAGE");
    s.dma = !(ev && atoi(ev) == 0);
    return s;
}

// ---- the window lists: every instantiation the library holds, in the order of the instantiation tables ---------------------------
// both filters in ONE launch of hpss_median_kernel: the reference's configuration (21,11), BASELINE config 2 (17,17) and the
// reference's sweep {11,21,31,41,51}^2 (Hyperparameter_Selection.py:543-544)
#define SMH_MEDIAN_PAIRS(X)                                                                                    \
    X(21, 11) X(17, 17)                                                                                        \
    X(11, 11) X(11, 21) X(11, 31) X(11, 41) X(11, 51) X(21, 21) X(21, 31) X(21, 41) X(21, 51)                  \
    X(31, 11) X(31, 21) X(31, 31) X(31, 41) X(31, 51) X(41, 11) X(41, 21) X(41, 31) X(41, 41) X(41, 51)        \
    X(51, 11) X(51, 21) X(51, 31) X(51, 41) X(51, 51)
// one filter, w = (w, 0) and (0, w): hpss_median_kernel for any odd window 3 .. 63
#define SMH_MEDIAN_SINGLES(X)                                                                                  \
    X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) X(23) X(25) X(27) X(29) X(31) X(33) X(35) X(37)    \
    X(39) X(41) X(43) X(45) X(47) X(49) X(51) X(53) X(55) X(57) X(59) X(61) X(63)
// hpss_median_split_kernel: the reference's configuration, BASELINE config 2, the small end of the sweep; single filters
#define SMH_MEDIAN_SPLIT_PAIRS(X) X(21, 11) X(17, 17) X(11, 11) X(11, 21) X(21, 21)
#define SMH_MEDIAN_SPLIT_SINGLES(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21)
// hpss_median_persist_kernel: (l_harm, l_perc, threads)
#define SMH_MEDIAN_PERSIST_BUILDS(X)                                                                           \
    X(21, 11, 512) X(21, 11, 768) X(17, 17, 512) X(17, 17, 768) X(11, 11, 512) X(11, 11, 768)                  \
    X(11, 21, 512) X(11, 21, 768) X(21, 21, 512) X(21, 21, 768) X(17, 17, 1024)

constexpr int kSplitMaxWindow = 21;  // 120 history registers; larger windows keep the delete/insert kernel

#define SMH_MEDIAN_IS2(a, b) || (lh == a && lp == b)
#define SMH_MEDIAN_IS1(w) || ((lh == w && lp == 0) || (lh == 0 && lp == w))
#define SMH_MEDIAN_IS3(a, b, t) || (lh == a && lp == b && threads == t)
constexpr bool has_pair(int lh, int lp) { return false SMH_MEDIAN_PAIRS(SMH_MEDIAN_IS2); }
constexpr bool has_single(int lh, int lp) { return false SMH_MEDIAN_SINGLES(SMH_MEDIAN_IS1); }
constexpr bool has_persist(int lh, int lp, int threads) { return false SMH_MEDIAN_PERSIST_BUILDS(SMH_MEDIAN_IS3); }
// Workgroup size of the block-split build of (lh, lp), 0: none.  Register budget: the history is H*(H+1)-1 registers (80 for W = 17,
// 120 for W = 21), so the size is chosen for 4 waves per SIMD (128 VGPRs) up to W = 17 and 3 waves per SIMD (168 VGPRs) above.
constexpr int split_threads(int lh, int lp) {
    return !(false SMH_MEDIAN_SPLIT_PAIRS(SMH_MEDIAN_IS2) SMH_MEDIAN_SPLIT_SINGLES(SMH_MEDIAN_IS1)) ? 0 : (lh > lp ? lh : lp) <= 17 ? 512 : 384;
}
#undef SMH_MEDIAN_IS2
#undef SMH_MEDIAN_IS1
#undef SMH_MEDIAN_IS3
static_assert(!split_threads(kSplitMaxWindow + 2, 0) && split_threads(kSplitMaxWindow, 0) && split_threads(21, 11) == 384 &&
                  split_threads(17, 17) == 512 && !split_threads(31, 31) && has_pair(31, 31) && has_single(0, 63) && !has_single(0, 0),
              "the window lists");

// ---- predicates and sizes ----------------------------------------------------------------------------------------------------------
// the register-window kernels fold once per side: they need window / 2 + 4 < axis length
constexpr bool fast_ok(int n, int w) { return w >= 3 && w / 2 + 4 < n; }
// both filters in one launch: the pair kernel's folds fit both axes
constexpr bool pair_fused(int K, int T, int lh, int lp) { return fast_ok(T, lh) && fast_ok(K, lp) && has_pair(lh, lp); }
// gcd(T, 64) <= 2: the flat K x T image (row stride T) is conflict-free for the harmonic lanes (ds_read_b32 is serviced in 32-lane halves)
constexpr bool conflict_free(int T) { return (T & 1) || ((T & 63) % 4 == 2); }
// one tile of the persistent kernel: the clip and the 16 bytes its misalignment may add, in whole KiB
constexpr int persist_tile_bytes(int K, int T) { return ((K * T * 4 + 16) + 1023) & ~1023; }
// LDS bytes the LDS-DMA copy may write for a clip of `bytes` bytes whose start is only known to lie on a multiple of `align` bytes
constexpr size_t dma_stage_bytes(size_t bytes, size_t align) { return (bytes + (16 - align) + 15) & ~(size_t)15; }
constexpr int waves_of(int n, int seg) { return seg ? (n * seg + 63) / 64 : 0; }  // lanes = lines x segments

// Tile budgets in words: two workgroups per CU, each its half of the 160 KiB less 1 KiB; a very tall spectrogram gives one workgroup
// the whole.  The columns of K rows that fit, made odd (the tile's row stride is odd: both walks are conflict-free).
constexpr int kPairBudgetWords = (kLdsBytesPerCU / 2 - 1024) / 4, kTallBudgetWords = (kLdsBytesPerCU - 1024) / 4;
constexpr int odd_cols(int budget_words, int K) { return (budget_words / K - 1) | 1; }

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// kernel families, numbered as smh_internal_median_plan answers (-1: nothing is launched)
enum Family { kFamNone = -1, kFamCopy = 0, kFamSmall = 1, kFamSplit = 2, kFamPersist = 3, kFamDeleteInsert = 4, kFamTwoSingles = 5 };
struct MedianPlan {
    int family;
    int layout;       // the harm layout written: 0 = (B,K,T), 1 = (B,T,K), 2 = (B, ceil(T/16), K, 16) (block-split and persistent kernels)
    int ntiles, TT;   // frame tiles per clip (0 in a ragged call) of TT frames
    int stride;       // row stride of the LDS tile in words (a clip staged by DMA, and the persistent kernel: rows of T)
    int nsh, nsp;     // segments per harmonic / percussive line
    int nwh, nwp;     // waves of the harmonic / percussive lanes: the launch runs (nwh + nwp) * 64 threads
    int threads;      // workgroup size the chosen build is compiled for
    size_t lds;       // dynamic LDS bytes
    unsigned grid_x, grid_y;
    int dma;          // block-split kernel: 1 = the whole clip staged by LDS-DMA (the <LH, LP, true> instantiation)
    char refusal[96]; // non-empty: the launch is refused (SMH_E_INVALID) with this text
    // (families 0, 1 and 5 -- copy, rank counting, one launch per filter -- carry a family and layout 0 only)
};
inline MedianPlan plan_of(int family, int layout) {
    MedianPlan p{};
    p.family = family, p.layout = layout;
    return p;
}

// The frame tile: the whole clip when two workgroups per CU can hold it, else the widest tile whose halo columns fit.
inline bool plan_tile(int K, int T, int lh, MedianPlan &p) {
    const int hh = lh / 2;
    if ((size_t)K * (T | 1) <= (size_t)kPairBudgetWords) {
        p.TT = T, p.stride = T | 1;
    } else {
        p.TT = odd_cols(kPairBudgetWords, K) - 2 * hh;
        if (p.TT < 8) {  // very tall spectrograms: give one workgroup the whole 160 KiB
            p.TT = odd_cols(kTallBudgetWords, K) - 2 * hh;
            if (p.TT < 1) return snprintf(p.refusal, sizeof p.refusal, "K=%d too large for an LDS tile with l_harm=%d", K, lh), false;
        }
        if (p.TT > T) p.TT = T;
        p.stride = (p.TT + 2 * hh) | 1;
    }
    p.ntiles = (T + p.TT - 1) / p.TT;
    p.lds = (size_t)K * p.stride * sizeof(float);
    return true;
}
// Frame tile of the ragged launch: the widest tile -- a multiple of 4 frames, so that the blocked harm rows start on float4
// boundaries, and at least 2 hh + 8 -- whose halo columns fit the budget of two workgroups per CU (K = 201, l_harm = 21: 76 frames,
// 96 columns).  0: (lh, lp) has no block-split kernel, or K is too large.
inline int rag_tile_frames(int K, int lh, int lp, const MedianSwitches &sw, int *stride = nullptr) {
    if (sw.nosplit || !(lh && lp) || !split_threads(lh, lp)) return 0;
    const int hh = lh / 2;
    const int TT = (odd_cols(kPairBudgetWords, K) - 2 * hh) & ~3;
    if (TT < 2 * hh + 8) return 0;
    if (stride) *stride = (TT + 2 * hh) | 1;
    return TT;
}

// Roles of the delete/insert kernel on a tile of nt frames: aim at similar lane-task lengths and <= 16 waves per workgroup
inline bool delete_insert_roles(int K, int nt, int lh, int lp, const MedianSwitches &sw, MedianPlan &p) {
    int nsh = lh ? 2 : 0, nsp = lp ? 3 : 0;
    if (sw.seg) {
        if (lh && sw.seg_h >= 1) nsh = sw.seg_h;
        if (lp && sw.seg_p >= 1) nsp = sw.seg_p;
    }
    if (lh && nt < 2 * lh) nsh = 1;
    if (lp && K < 6 * lp) nsp = 1;
    int nwh = waves_of(K, nsh), nwp = waves_of(nt, nsp);
    while (nwh + nwp > 16) {
        if (nsh > 1 && nwh >= nwp) nsh--;
        else if (nsp > 1) nsp--;
        else if (nsh > 1) nsh--;
        else break;
        nwh = waves_of(K, nsh), nwp = waves_of(nt, nsp);
    }
    if (nwh + nwp > 16) return snprintf(p.refusal, sizeof p.refusal, "tile %dx%d needs more than 16 waves per workgroup", K, nt), false;
    p.nsh = nsh, p.nsp = nsp, p.nwh = nwh, p.nwp = nwp;
    return true;
}
// Roles of the block-split and persistent kernels: per-lane cost ~ (outputs + one block of start-up) x (VALU per output ~ W + 6);
// the segment counts that minimise the longest lane within the build's waves.  false: no pair of counts fits.
inline bool split_roles(int K, int nt, int lh, int lp, int maxwaves, const MedianSwitches &sw, MedianPlan &p) {
    long best = -1;
    int bh = 0, bp = 0;
    for (int nsh = lh ? 1 : 0; nsh <= (lh ? 4 : 0); ++nsh) {
        if (lh && nsh > 1 && nt < 2 * lh * nsh) break;
        for (int nsp = lp ? 1 : 0; nsp <= (lp ? 6 : 0); ++nsp) {
            if (lp && nsp > 1 && K < 2 * lp * nsp) break;
            if (waves_of(K, nsh) + waves_of(nt, nsp) > maxwaves) continue;
            const long ch = lh ? (long)((nt + nsh - 1) / nsh + lh) * (lh + 6) : 0;
            const long cp = lp ? (long)((K + nsp - 1) / nsp + lp) * (lp + 6) : 0;
            const long c = ch > cp ? ch : cp;
            if (best < 0 || c < best) best = c, bh = nsh, bp = nsp;
        }
    }
    if (best < 0) return false;
    if (sw.seg && (!lh || sw.seg_h >= 1) && (!lp || sw.seg_p >= 1) &&
        waves_of(K, lh ? sw.seg_h : 0) + waves_of(nt, lp ? sw.seg_p : 0) <= maxwaves)
        bh = lh ? sw.seg_h : 0, bp = lp ? sw.seg_p : 0;
    p.nsh = bh, p.nsp = bp, p.nwh = waves_of(K, bh), p.nwp = waves_of(nt, bp);
    return true;
}
// the block-split kernel (windows up to 21) on tiles of nt frames, when its build's waves cover the tile
inline bool split_covers(int K, int nt, int lh, int lp, const MedianSwitches &sw, MedianPlan &p) {
    const int threads = sw.nosplit ? 0 : split_threads(lh, lp);
    if (!threads || !split_roles(K, nt, lh, lp, threads / 64, sw, p)) return false;
    p.family = kFamSplit, p.threads = threads;
    return true;
}
// Whether a call asks for the persistent kernel at all (the launcher then needs the device's CU count).  Windows above 17 (history > 128
// VGPRs, so only 6 waves per block-split workgroup) take it, one 8-wave workgroup per CU with 256 VGPRs; up to 17 two ordinary 8-wave
// workgroups per CU measure 3-5 % faster (4 waves per SIMD).
inline bool persist_asked(int lh, int lp, const MedianSwitches &sw) {
    const bool want = sw.persist < 0 ? (lh > 17 || lp > 17) : sw.persist != 0;
    return !sw.nosplit && want && lh && lp && has_persist(lh, lp, sw.pthreads);
}
// Whole clip per tile of the block-split kernel: staged by LDS-DMA as the flat K x T image (row stride T) when that image is
// conflict-free and the copy, which starts at the 16-byte boundary below the clip and ends at the one above it, fits the tile.
// align: the clip's alignment class, 16 / 8 / 4 (the input pointer and K T 4 are both multiples of it), 0: not 4-byte aligned.
inline bool dma_staged(int K, int T, const MedianPlan &p, const MedianSwitches &sw, int align, bool probe_noload) {
    return sw.dma && !probe_noload && p.ntiles == 1 && p.TT >= T && align != 0 && conflict_free(T) &&
           dma_stage_bytes((size_t)K * T * sizeof(float), (size_t)align) <= p.lds;
}

// One launch of B clips with filters (lh, lp), 0 = that filter off: the persistent kernel (whole clip per tile, conflict-free, two
// tiles in LDS, at least two clips per CU), else the block-split kernel, else the delete/insert kernel, which has no blocked store
// (layout 2 -> 1; layout 2 is also written tile by tile: the blocked walker addresses harm[t / 16][k][t % 16] by absolute frame).
inline MedianPlan plan_launch(int K, int T, int lh, int lp, int B, int layout, const MedianSwitches &sw, int n_cu, int align, bool probe_noload) {
    MedianPlan p = plan_of(kFamDeleteInsert, layout);
    if (!((lh && lp) ? has_pair(lh, lp) : has_single(lh, lp))) {
        snprintf(p.refusal, sizeof p.refusal, "no median kernel for (l_harm,l_perc)=(%d,%d)", lh, lp);
        return p;
    }
    if (!plan_tile(K, T, lh, p) || !delete_insert_roles(K, p.TT, lh, lp, sw, p)) return p;
    p.grid_x = (unsigned)p.ntiles, p.grid_y = (unsigned)B;
    MedianPlan q = p;
    if (persist_asked(lh, lp, sw) && p.ntiles == 1 && conflict_free(T) && 2 * persist_tile_bytes(K, T) <= kLdsBytesPerCU && B >= 2 * n_cu &&
        split_roles(K, T, lh, lp, sw.pthreads / 64, sw, q)) {
        q.family = kFamPersist, q.threads = sw.pthreads, q.stride = T;
        q.lds = 2 * (size_t)persist_tile_bytes(K, T), q.grid_x = (unsigned)n_cu, q.grid_y = 1;
        return q;
    }
    if (split_covers(K, p.TT, lh, lp, sw, q)) {
        q.dma = dma_staged(K, T, q, sw, align, probe_noload);
        if (q.dma) q.stride = T;
        return q;
    }
    p.threads = 1024;
    if (layout == 2) p.layout = 1;
    return p;
}

// ---- one plan function per entry point -----------------------------------------------------------------------------------------------
// smh_median_time_ex_f32: copy for a window of one, the rank-counting kernel (layout 0) for axes the register window cannot fold
inline MedianPlan plan_time_ex(int K, int T, int lh, int B, int layout, const MedianSwitches &sw, int n_cu, int align, bool probe_noload = false) {
    if (lh == 1 || !fast_ok(T, lh)) return plan_of(lh == 1 ? kFamCopy : kFamSmall, 0);
    return plan_launch(K, T, lh, 0, B, layout, sw, n_cu, align, probe_noload);
}
inline MedianPlan plan_time(int K, int T, int lh, int B, const MedianSwitches &sw, int n_cu, int align, bool probe_noload = false) {  // smh_median_time_f32
    return plan_time_ex(K, T, lh, B, 0, sw, n_cu, align, probe_noload);
}
// smh_median_freq_f32
inline MedianPlan plan_freq(int K, int T, int lp, int B, const MedianSwitches &sw, int n_cu, int align, bool probe_noload = false) {
    if (lp == 1 || !fast_ok(K, lp)) return plan_of(lp == 1 ? kFamCopy : kFamSmall, 0);
    return plan_launch(K, T, 0, lp, B, 0, sw, n_cu, align, probe_noload);
}
// smh_hpss_median_ex_f32 and the fused pipeline (launch_hpss): the fused launch, else one launch per filter (window pairs outside the
// fused list, or tiny axes) -- plan_time and plan_freq --, which writes the reference layout
inline MedianPlan plan_hpss_ex(int K, int T, int lh, int lp, int B, int layout, const MedianSwitches &sw, int n_cu, int align,
                               bool probe_noload = false) {
    if (!pair_fused(K, T, lh, lp)) return plan_of(kFamTwoSingles, 0);
    return plan_launch(K, T, lh, lp, B, layout, sw, n_cu, align, probe_noload);
}
inline MedianPlan plan_hpss(int K, int T, int lh, int lp, int B, const MedianSwitches &sw, int n_cu, int align, bool probe_noload = false) {  // smh_hpss_median_f32
    return plan_hpss_ex(K, T, lh, lp, B, 0, sw, n_cu, align, probe_noload);
}
// n_items (clip, frame tile) items of clips of different lengths: the block-split kernel on tiles of rag_tile_frames, register
// staging, harm in the 16-frame blocked layout, the per-XCD grid (smh_xcd.h)
inline MedianPlan plan_rag(int K, int lh, int lp, const MedianSwitches &sw, int n_items) {
    MedianPlan p = plan_of(kFamSplit, 2);
    p.TT = rag_tile_frames(K, lh, lp, sw, &p.stride);
    if (!p.TT || !split_covers(K, p.TT, lh, lp, sw, p)) {
        snprintf(p.refusal, sizeof p.refusal, "ragged medians: no block-split kernel for (l_harm,l_perc)=(%d,%d), K=%d", lh, lp, K);
        return p;
    }
    p.lds = (size_t)K * p.stride * sizeof(float);
    p.grid_x = smh::xcd_grid(n_items), p.grid_y = 1;
    return p;
}

// Whether the fused pipeline, asked for layout 2, writes the 16-frame blocked harm image: the pair is fused and the block-split kernel
// covers a tile of the plan, whatever B (the persistent kernel, tried first, writes the same layout; smh_frontend_f32 refuses a call
// whose medians came back in another layout than this promised).
inline bool blocked_harm_ok(int K, int T, int lh, int lp, const MedianSwitches &sw) {
    MedianPlan p{};
    return pair_fused(K, T, lh, lp) && plan_tile(K, T, lh, p) && delete_insert_roles(K, p.TT, lh, lp, sw, p) && split_covers(K, p.TT, lh, lp, sw, p);
}

// smh_internal_median_plan's answer: fourteen ints
inline void median_plan_ints(const MedianPlan &p, int *out) {
    const int v[14] = {p.family, p.layout, p.ntiles, p.TT,       p.nsh,         p.nsp,         p.stride,
                       p.nwh,    p.nwp,    p.threads, (int)p.lds, (int)p.grid_x, (int)p.grid_y, p.dma};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
}

}  // namespace smh_median
