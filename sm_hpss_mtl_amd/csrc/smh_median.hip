// Entry points of the HPSS median filters (kernel template: smh_median_kernel.h).
#include <cstdlib>

#include "smh_median_kernel.h"
#include "smh_median_split.h"

namespace smh_median {

const Entry kPairs[] = {
    // both filters in ONE launch: the reference's configuration (21,11), BASELINE config 2 (17,17)
    // and the reference's sweep {11,21,31,41,51}^2 (Hyperparameter_Selection.py:543-544)
    SMH_MEDIAN_E2(21, 11) SMH_MEDIAN_E2(17, 17)
    SMH_MEDIAN_E2(11, 11) SMH_MEDIAN_E2(11, 21) SMH_MEDIAN_E2(11, 31) SMH_MEDIAN_E2(11, 41) SMH_MEDIAN_E2(11, 51)
    SMH_MEDIAN_E2(21, 21) SMH_MEDIAN_E2(21, 31) SMH_MEDIAN_E2(21, 41) SMH_MEDIAN_E2(21, 51)
    SMH_MEDIAN_E2(31, 11) SMH_MEDIAN_E2(31, 21) SMH_MEDIAN_E2(31, 31) SMH_MEDIAN_E2(31, 41) SMH_MEDIAN_E2(31, 51)
    SMH_MEDIAN_E2(41, 11) SMH_MEDIAN_E2(41, 21) SMH_MEDIAN_E2(41, 31) SMH_MEDIAN_E2(41, 41) SMH_MEDIAN_E2(41, 51)
    SMH_MEDIAN_E2(51, 11) SMH_MEDIAN_E2(51, 21) SMH_MEDIAN_E2(51, 31) SMH_MEDIAN_E2(51, 41) SMH_MEDIAN_E2(51, 51)};

KernelFn find_pair_kernel(int lh, int lp) {
    for (const Entry &e : kPairs)
        if (e.lh == lh && e.lp == lp) return e.fn;
    return nullptr;
}

}  // namespace smh_median

namespace {

using namespace smh_median;

// Slow, fully general path for axes not longer than half the window (multiple reflections):
// one thread per output, rank-counting selection.  Only tiny inputs ever reach it.
__global__ void median_small_kernel(const float *__restrict__ S, float *__restrict__ out, int K, int T, int w,
                                    int along_t, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    const int k = (int)((i / T) % K);
    const size_t base = i - (size_t)k * T - t;
    const int n = along_t ? T : K;
    const int pos = along_t ? t : k;
    const int h = w / 2;
    auto at = [&](int j) {
        int q = pos - h + j;
        const int p = 2 * n;
        int r = q % p;
        if (r < 0) r += p;
        if (r >= n) r = p - 1 - r;
        return along_t ? S[base + (size_t)k * T + r] : S[base + (size_t)r * T + t];
    };
    // the median is the element with exactly h elements before it in the stable (value, index) order
    for (int a = 0; a < w; ++a) {
        const float va = at(a);
        int rank = 0;
        for (int c = 0; c < w; ++c) {
            const float vc = at(c);
            rank += (vc < va) || (vc == va && c < a);
        }
        if (rank == h) {
            out[i] = va;
            return;
        }
    }
}

struct Plan {
    int TT, ntiles, stride, nsh, nsp, nwh, nwp;
    size_t lds;
};

// Tile so that two workgroups fit one CU's 160 KiB LDS whenever the clip allows it.
int make_plan(int K, int T, int lh, int lp, Plan *p) {
    const int hh = lh / 2;
    const int budget_words = (smh::kLdsBytesPerCU / 2 - 1024) / 4;
    auto odd = [](int x) { return x | 1; };
    int TT, stride;
    if ((size_t)K * odd(T) <= (size_t)budget_words) {
        TT = T;
        stride = odd(T);
    } else {
        int maxcols = budget_words / K;
        if ((maxcols & 1) == 0) maxcols -= 1;
        TT = maxcols - 2 * hh;
        if (TT < 8) {
            // very tall spectrograms: give one workgroup the whole 160 KiB
            maxcols = ((smh::kLdsBytesPerCU - 1024) / 4) / K;
            if ((maxcols & 1) == 0) maxcols -= 1;
            TT = maxcols - 2 * hh;
            if (TT < 1) return smh::set_error(SMH_E_INVALID, "K=%d too large for an LDS tile with l_harm=%d", K, lh);
        }
        if (TT > T) TT = T;
        stride = odd(TT + 2 * hh);
    }
    p->TT = TT;
    p->ntiles = (T + TT - 1) / TT;
    p->stride = stride;
    p->lds = (size_t)K * stride * sizeof(float);
    // segments: aim at similar lane-task lengths and <= 16 waves per workgroup
    const int nt = TT;
    int nsh = lh ? 2 : 0, nsp = lp ? 3 : 0;
    // tuning override for experiments (tools/tune_median.py): SMH_MEDIAN_SEG="nsh,nsp"
    if (const char *ev = getenv("SMH_MEDIAN_SEG")) {
        int a = 0, b = 0;
        if (sscanf(ev, "%d,%d", &a, &b) == 2) {
            if (lh && a >= 1) nsh = a;
            if (lp && b >= 1) nsp = b;
        }
    }
    if (lh && nt < 2 * lh) nsh = 1;
    if (lp && K < 6 * lp) nsp = 1;
    auto waves = [&](int n, int seg) { return seg ? (n * seg + 63) / 64 : 0; };
    int nwh = waves(K, nsh), nwp = waves(nt, nsp);
    while (nwh + nwp > 16) {
        if (nsh > 1 && nwh >= nwp) nsh--;
        else if (nsp > 1) nsp--;
        else if (nsh > 1) nsh--;
        else break;
        nwh = waves(K, nsh), nwp = waves(nt, nsp);
    }
    if (nwh + nwp > 16)
        return smh::set_error(SMH_E_INVALID, "tile %dx%d needs more than 16 waves per workgroup", K, nt);
    p->nsh = nsh, p->nsp = nsp, p->nwh = nwh, p->nwp = nwp;
    return SMH_OK;
}

// Roles of the block-split kernel: per-lane cost ~ (outputs + one block of start-up) x (VALU per output ~ W + 6);
// pick the segment counts that minimise the longest lane within the workgroup's wave budget.
bool make_split_roles(int K, int nt, int lh, int lp, int maxwaves, Plan *p) {
    auto waves = [](int n, int seg) { return seg ? (n * seg + 63) / 64 : 0; };
    long best = -1;
    int bh = 0, bp = 0;
    for (int nsh = lh ? 1 : 0; nsh <= (lh ? 4 : 0); ++nsh) {
        if (lh && nsh > 1 && nt < 2 * lh * nsh) break;
        for (int nsp = lp ? 1 : 0; nsp <= (lp ? 6 : 0); ++nsp) {
            if (lp && nsp > 1 && K < 2 * lp * nsp) break;
            if (waves(K, nsh) + waves(nt, nsp) > maxwaves) continue;
            const long ch = lh ? (long)((nt + nsh - 1) / nsh + lh) * (lh + 6) : 0;
            const long cp = lp ? (long)((K + nsp - 1) / nsp + lp) * (lp + 6) : 0;
            const long c = ch > cp ? ch : cp;
            if (best < 0 || c < best) best = c, bh = nsh, bp = nsp;
        }
    }
    if (best < 0) return false;
    if (const char *ev = getenv("SMH_MEDIAN_SEG")) {  // tuning override (tools/tune_median.py): "nsh,nsp"
        int a = 0, b = 0;
        if (sscanf(ev, "%d,%d", &a, &b) == 2 && (!lh || a >= 1) && (!lp || b >= 1) &&
            waves(K, lh ? a : 0) + waves(nt, lp ? b : 0) <= maxwaves)
            bh = lh ? a : 0, bp = lp ? b : 0;
    }
    p->nsh = bh, p->nsp = bp, p->nwh = waves(K, bh), p->nwp = waves(nt, bp);
    return true;
}

int launch_small(const float *S, int B, int K, int T, int w, int along_t, float *out, hipStream_t st) {
    const size_t total = (size_t)B * K * T;
    const int bs = 256;
    hipLaunchKernelGGL(median_small_kernel, dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, st, S, out, K, T, w,
                       along_t, total);
    return smh::launch_status("median_small_kernel");
}

// The kernel a launch takes and what it writes: the one decision of launch(), which the test-only smh_internal_median_route reports.
enum Family { kFamCopy = 0, kFamSmall = 1, kFamSplit = 2, kFamPersist = 3, kFamDeleteInsert = 4, kFamTwoSingles = 5 };
struct Route {
    int family, layout;  // layout: the harm layout that is written
    Plan plan;           // tile and roles of the chosen kernel (copy, small, two singles: zero)
    KernelFn fn;
    const SplitEntry *se;
    const PersistEntry *pe;
    int n_cu;
};

// harm_tmajor: 0 = (B,K,T), 1 = (B,T,K), 2 = (B, ceil(T/16), K, 16) (block-split kernels; any other kernel writes layout 1
// instead).  r->layout receives the layout that will be produced.
int launch_route(int B, int K, int T, int lh, int lp, int harm_tmajor, Route *r) {
    *r = Route{};
    r->layout = harm_tmajor;
    r->fn = (lh && lp) ? find_pair_kernel(lh, lp) : find_single_kernel(lh, lp);
    if (!r->fn) return smh::set_error(SMH_E_INVALID, "no median kernel for (l_harm,l_perc)=(%d,%d)", lh, lp);
    Plan p;
    int rc = make_plan(K, T, lh, lp, &p);
    if (rc) return rc;
    // windows up to 21: the block-split kernel (smh_median_split.h) when its wave budget covers the tile
    static const bool no_split = getenv("SMH_MEDIAN_NOSPLIT") != nullptr;  // A/B switches for tools/tune_median.py
    // Whole clip per tile and at least two clips per CU: windows above 17 (history > 128 VGPRs, so only 6 waves per
    // workgroup otherwise) take the persistent double-buffered kernel, one 8-wave workgroup per CU with 256 VGPRs;
    // up to 17 two ordinary 8-wave workgroups per CU measure 3-5 % faster (4 waves per SIMD).  SMH_MEDIAN_PERSIST=0/1
    // forces either, SMH_MEDIAN_PTHREADS picks the 512 / 768 / 1024-thread build (tools/gpu/tune_split.sh).
    bool want_persist = (lh > 17 || lp > 17);
    if (const char *ev = getenv("SMH_MEDIAN_PERSIST")) want_persist = atoi(ev) != 0;
    int pthreads = 512;
    if (const char *ev = getenv("SMH_MEDIAN_PTHREADS")) pthreads = atoi(ev);
    if (const PersistEntry *pe = (no_split || !want_persist || !(lh && lp)) ? nullptr : find_persist_kernel(lh, lp, pthreads)) {
        static int n_cu = 0;
        if (n_cu == 0) {
            int dev = 0;
            SMH_CHECK_HIP(hipGetDevice(&dev));
            SMH_CHECK_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        }
        const int tile_bytes = persist_tile_bytes(K, T);
        const int g = T & 63;
        const bool conflict_free = (T & 1) || (g % 4 == 2);  // gcd(T, 64) <= 2
        Plan q = p;
        if (p.ntiles == 1 && conflict_free && 2 * tile_bytes <= smh::kLdsBytesPerCU && B >= 2 * n_cu &&
            make_split_roles(K, T, lh, lp, pe->threads / 64, &q)) {
            r->family = kFamPersist, r->plan = q, r->pe = pe, r->n_cu = n_cu;
            return SMH_OK;
        }
    }
    // (layout 2 is also written tile by tile: the blocked walker addresses harm[t / 16][k][t % 16] by absolute frame)
    if (const SplitEntry *se = no_split ? nullptr : find_split_kernel(lh, lp)) {
        Plan q = p;
        if (make_split_roles(K, p.TT, lh, lp, se->threads / 64, &q)) {
            r->family = kFamSplit, r->plan = q, r->se = se;
            return SMH_OK;
        }
    }
    if (harm_tmajor == 2) r->layout = 1;  // the delete/insert kernel has no blocked store
    r->family = kFamDeleteInsert, r->plan = p;
    return SMH_OK;
}

int launch_routed(const Route &r, const float *S, int B, int K, int T, float *harm, float *perc, hipStream_t st) {
    if (r.family == kFamPersist) {
        const Plan &q = r.plan;
        const int lds = 2 * persist_tile_bytes(K, T);
        SMH_CHECK_HIP(hipFuncSetAttribute((const void *)r.pe->fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(r.pe->fn, dim3(r.n_cu), dim3((q.nwh + q.nwp) * 64), lds, st, S, harm, perc, B, K, T, q.nsh,
                           q.nsp, q.nwh, r.layout);
        return smh::launch_status("hpss_median_persist_kernel");
    }
    if (r.family == kFamSplit) {
        const Plan &q = r.plan;
        SMH_CHECK_HIP(hipFuncSetAttribute((const void *)r.se->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.lds));
        SMH_CHECK_HIP(hipFuncSetAttribute((const void *)r.se->fn_dma, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.lds));
        dim3 grid(q.ntiles, B), block((q.nwh + q.nwp) * 64);
        const bool probe_noload = smh::probe_env("SMH_MEDIAN_PROBE_NOLOAD") != nullptr;  // timing experiment, outputs invalid
        // Whole clip per tile: staged by LDS-DMA as the flat K x T image (row stride T) when that image is conflict-free for the
        // harmonic lanes (gcd(T, 64) <= 2, as for the persistent kernel) and the copy, which starts at the 16-byte boundary below
        // the clip and ends at the one above it, fits the tile the plan allocates.  SMH_MEDIAN_DMA_STAGE=0: the register staging.
        const char *ev = getenv("SMH_MEDIAN_DMA_STAGE");
        const size_t clip_bytes = (size_t)K * T * sizeof(float);
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(S);
        const size_t align = (s0 % 16 == 0 && clip_bytes % 16 == 0) ? 16 : (s0 % 8 == 0 && clip_bytes % 8 == 0) ? 8 : 4;
        const bool dma = !(ev && atoi(ev) == 0) && !probe_noload && q.ntiles == 1 && q.TT >= T && s0 % 4 == 0 &&
                         ((T & 1) || ((T & 63) % 4 == 2)) && dma_stage_bytes(clip_bytes, align) <= q.lds;
        hipLaunchKernelGGL(dma ? r.se->fn_dma : r.se->fn, grid, block, q.lds, st, S, harm, perc, K, T, q.TT, dma ? T : q.stride, q.nsh,
                           q.nsp, q.nwh, r.layout, probe_noload ? 1.f : -__builtin_inff(), __builtin_inff(), nullptr, nullptr, 0);
        return smh::launch_status("hpss_median_split_kernel");
    }
    const Plan &p = r.plan;
    SMH_CHECK_HIP(hipFuncSetAttribute((const void *)r.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    dim3 grid(p.ntiles, B), block((p.nwh + p.nwp) * 64);
    hipLaunchKernelGGL(r.fn, grid, block, p.lds, st, S, harm, perc, K, T, p.TT, p.stride, p.nsh, p.nsp, p.nwh,
                       r.layout, -__builtin_inff(), __builtin_inff());
    return smh::launch_status("hpss_median_kernel");
}

// *written (optional) receives the layout that was produced.
int launch(const float *S, int B, int K, int T, int lh, int lp, float *harm, float *perc, hipStream_t st,
           int harm_tmajor = 0, int *written = nullptr) {
    if (written) *written = harm_tmajor;
    Route r;
    int rc = launch_route(B, K, T, lh, lp, harm_tmajor, &r);
    if (rc) return rc;
    if (written) *written = r.layout;
    return launch_routed(r, S, B, K, T, harm, perc, st);
}

int check_args(const void *S, int B, int K, int T, int w, const char *name) {
    SMH_REQUIRE(S != nullptr || B == 0, "%s: null input", name);
    SMH_REQUIRE(B >= 0 && K >= 1 && T >= 1, "%s: bad shape B=%d K=%d T=%d", name, B, K, T);
    SMH_REQUIRE(w >= 1 && w <= SMH_MAX_MEDIAN && (w & 1), "%s: window must be odd in [1,%d], got %d", name,
                SMH_MAX_MEDIAN, w);
    SMH_REQUIRE(B <= 65535, "%s: B=%d exceeds the grid limit; split the batch", name, B);
    return SMH_OK;
}

// the register-window kernel folds once per side: it needs window/2 < axis length
bool fast_ok(int n, int w) { return w >= 3 && w / 2 + 4 < n; }

// both filters in one launch: the pair kernel's folds fit both axes
bool pair_fused(int K, int T, int lh, int lp) { return fast_ok(T, lh) && fast_ok(K, lp) && find_pair_kernel(lh, lp); }

// smh_hpss_median_f32 and launch_hpss: the fused launch, else one launch per filter (window pairs outside the fused table, or
// tiny axes), which writes the reference layout
int hpss_route(int B, int K, int T, int lh, int lp, int want_tmajor, Route *r) {
    if (pair_fused(K, T, lh, lp)) return launch_route(B, K, T, lh, lp, want_tmajor, r);
    *r = Route{};
    r->family = kFamTwoSingles;
    return SMH_OK;
}

// smh_median_time_f32: copy for a window of one, the rank-counting kernel for axes the register window cannot fold
int time_route(int B, int K, int T, int lh, Route *r) {
    if (lh == 1 || !fast_ok(T, lh)) {
        *r = Route{};
        r->family = lh == 1 ? kFamCopy : kFamSmall;
        return SMH_OK;
    }
    return launch_route(B, K, T, lh, 0, 0, r);
}

// smh_median_time_ex_f32: whatever smh_median_time_f32 cannot launch, and a requested layout 0, is that entry's
int time_ex_route(int B, int K, int T, int lh, int harm_layout, Route *r) {
    if (lh == 1 || !fast_ok(T, lh) || harm_layout == 0) return time_route(B, K, T, lh, r);
    return launch_route(B, K, T, lh, 0, harm_layout, r);
}

}  // namespace

namespace smh_median {
// ---- clips of different lengths in one launch (smh_rag.h) ----
// Frame tile of the ragged launch: the widest tile -- a multiple of 4 frames, so that the blocked harm rows start on float4
// boundaries -- whose halo columns fit the LDS budget of two workgroups per CU (K = 201, l_harm = 21: 76 frames, 96 columns).
int rag_tile_frames(int K, int lh, int lp, int *stride) {
    static const bool no_split = getenv("SMH_MEDIAN_NOSPLIT") != nullptr;
    if (no_split || !(lh && lp) || !find_split_kernel(lh, lp)) return 0;
    const int hh = lh / 2;
    const int budget_words = (smh::kLdsBytesPerCU / 2 - 1024) / 4;
    int maxcols = budget_words / K;
    if ((maxcols & 1) == 0) maxcols -= 1;
    int TT = (maxcols - 2 * hh) & ~3;
    if (TT < 2 * hh + 8) return 0;
    if (stride) *stride = (TT + 2 * hh) | 1;
    return TT;
}

int launch_rag(const float *d_S, float *d_harm, float *d_perc, int K, int lh, int lp, const smh_rag::Clip *d_clips,
               const smh_rag::Item *d_items, int n_items, hipStream_t st) {
    if (n_items <= 0) return SMH_OK;
    int stride = 0;
    const int TT = rag_tile_frames(K, lh, lp, &stride);
    const SplitEntry *se = TT ? find_split_kernel(lh, lp) : nullptr;
    Plan q;
    if (!se || !make_split_roles(K, TT, lh, lp, se->threads / 64, &q))
        return smh::set_error(SMH_E_INVALID, "ragged medians: no block-split kernel for (l_harm,l_perc)=(%d,%d), K=%d", lh, lp, K);
    const size_t lds = (size_t)K * stride * sizeof(float);
    SMH_CHECK_HIP(hipFuncSetAttribute((const void *)se->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned grid = smh::xcd_grid(n_items);
    hipLaunchKernelGGL(se->fn, dim3(grid), dim3((q.nwh + q.nwp) * 64), lds, st, d_S, d_harm, d_perc, K, 0, TT, stride, q.nsh, q.nsp,
                       q.nwh, 2, -__builtin_inff(), __builtin_inff(), d_clips, d_items, n_items);
    return smh::launch_status("hpss_median_split_kernel (ragged)");
}

// Fused-pipeline entry: both filters in one launch, harm optionally time-major (B,T,K).
// Returns 1 if the time-major layout was produced, 0 if the reference layout was used, <0 on error.
int launch_hpss(const float *S, int B, int K, int T, int lh, int lp, float *harm, float *perc, int want_tmajor,
                hipStream_t st) {
    Route r;
    int rc = hpss_route(B, K, T, lh, lp, want_tmajor, &r);
    if (rc) return rc;
    rc = r.family == kFamTwoSingles ? smh_hpss_median_f32(nullptr, S, B, K, T, lh, lp, harm, perc, (void *)st)
                                    : launch_routed(r, S, B, K, T, harm, perc, st);
    return rc ? rc : r.layout;
}

// whether launch_hpss(want_tmajor = 2) writes the 16-frame blocked harm image: the pair kernel's folds fit both axes and the
// block-split kernel covers a tile of the plan (the persistent kernel, tried first, writes the same layout; smh_frontend_f32 refuses
// a call whose medians came back in another layout than this promised)
bool blocked_harm_ok(int K, int T, int lh, int lp) {
    static const bool no_split = getenv("SMH_MEDIAN_NOSPLIT") != nullptr;
    if (no_split || !pair_fused(K, T, lh, lp)) return false;
    const SplitEntry *se = find_split_kernel(lh, lp);
    Plan p, q;
    return se && make_plan(K, T, lh, lp, &p) == SMH_OK && make_split_roles(K, p.TT, lh, lp, se->threads / 64, &q);
}
}  // namespace smh_median

extern "C" int smh_median_time_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_harm, float *d_harm,
                                   void *stream) {
    int rc = check_args(d_S, B, K, T, l_harm, "smh_median_time_f32");
    if (rc) return rc;
    SMH_REQUIRE(d_harm || B == 0, "smh_median_time_f32: null output");
    if (B == 0) return SMH_OK;
    hipStream_t st = (hipStream_t)stream;
    Route r;
    rc = time_route(B, K, T, l_harm, &r);
    if (rc) return rc;
    if (r.family == kFamCopy) {
        SMH_CHECK_HIP(hipMemcpyAsync(d_harm, d_S, (size_t)B * K * T * sizeof(float), hipMemcpyDeviceToDevice, st));
        return SMH_OK;
    }
    if (r.family == kFamSmall) return launch_small(d_S, B, K, T, l_harm, 1, d_harm, st);
    return launch_routed(r, d_S, B, K, T, d_harm, nullptr, st);
}

// the harmonic median alone in any of the three layouts of smh_hpss_median_ex_f32 (returns the layout written)
extern "C" int smh_median_time_ex_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_harm, float *d_harm,
                                      int harm_layout, void *stream) {
    int rc = check_args(d_S, B, K, T, l_harm, "smh_median_time_ex_f32");
    if (rc) return rc;
    SMH_REQUIRE(harm_layout >= 0 && harm_layout <= 2, "smh_median_time_ex_f32: harm_layout must be 0, 1 or 2");
    SMH_REQUIRE(d_harm || B == 0, "smh_median_time_ex_f32: null output");
    if (B == 0) return harm_layout;
    Route r;
    rc = time_ex_route(B, K, T, l_harm, harm_layout, &r);
    if (rc) return rc;
    if (r.family == kFamCopy || r.family == kFamSmall) {
        rc = smh_median_time_f32(nullptr, d_S, B, K, T, l_harm, d_harm, stream);
        return rc ? rc : 0;
    }
    rc = launch_routed(r, d_S, B, K, T, d_harm, nullptr, (hipStream_t)stream);
    return rc ? rc : r.layout;
}

extern "C" int smh_median_freq_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_perc, float *d_perc,
                                   void *stream) {
    int rc = check_args(d_S, B, K, T, l_perc, "smh_median_freq_f32");
    if (rc) return rc;
    SMH_REQUIRE(d_perc || B == 0, "smh_median_freq_f32: null output");
    if (B == 0) return SMH_OK;
    hipStream_t st = (hipStream_t)stream;
    if (l_perc == 1) {
        SMH_CHECK_HIP(hipMemcpyAsync(d_perc, d_S, (size_t)B * K * T * sizeof(float), hipMemcpyDeviceToDevice, st));
        return SMH_OK;
    }
    if (!fast_ok(K, l_perc)) return launch_small(d_S, B, K, T, l_perc, 0, d_perc, st);
    return launch(d_S, B, K, T, 0, l_perc, nullptr, d_perc, st);
}

extern "C" int smh_hpss_median_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_harm, int l_perc,
                                   float *d_harm, float *d_perc, void *stream) {
    int rc = check_args(d_S, B, K, T, l_harm, "smh_hpss_median_f32");
    if (rc) return rc;
    rc = check_args(d_S, B, K, T, l_perc, "smh_hpss_median_f32");
    if (rc) return rc;
    SMH_REQUIRE((d_harm && d_perc) || B == 0, "smh_hpss_median_f32: null output");
    if (B == 0) return SMH_OK;
    Route r;
    rc = hpss_route(B, K, T, l_harm, l_perc, 0, &r);
    if (rc) return rc;
    if (r.family != kFamTwoSingles) return launch_routed(r, d_S, B, K, T, d_harm, d_perc, (hipStream_t)stream);
    // window pairs outside the fused table, or tiny axes: one launch per filter
    rc = smh_median_time_f32(nullptr, d_S, B, K, T, l_harm, d_harm, stream);
    if (rc) return rc;
    return smh_median_freq_f32(nullptr, d_S, B, K, T, l_perc, d_perc, stream);
}

extern "C" int smh_hpss_median_ex_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_harm, int l_perc,
                                      float *d_harm, float *d_perc, int harm_layout, void *stream) {
    int rc = check_args(d_S, B, K, T, l_harm, "smh_hpss_median_ex_f32");
    if (rc) return rc;
    rc = check_args(d_S, B, K, T, l_perc, "smh_hpss_median_ex_f32");
    if (rc) return rc;
    SMH_REQUIRE(harm_layout >= 0 && harm_layout <= 2, "smh_hpss_median_ex_f32: harm_layout must be 0, 1 or 2");
    SMH_REQUIRE((d_harm && d_perc) || B == 0, "smh_hpss_median_ex_f32: null output");
    if (B == 0) return harm_layout;
    return smh_median::launch_hpss(d_S, B, K, T, l_harm, l_perc, d_harm, d_perc, harm_layout, (hipStream_t)stream);
}

// Test-only (not in include/smh.h): the route one call of a median entry point takes, from the functions the entry points themselves
// decide with; launches nothing.  entry: 0 smh_hpss_median_ex_f32, 1 smh_median_time_ex_f32, 2 smh_hpss_median_f32,
// 3 smh_median_time_f32 (l_perc / harm_layout are ignored where the entry has no such argument).  out[0..5] = family (0 copy,
// 1 rank counting, 2 block-split, 3 persistent, 4 delete/insert, 5 one launch per filter; -1 for B == 0: no launch), harm layout
// written, ntiles, TT, nsh, nsp (zero for families 0, 1 and 5).  Returns SMH_OK, or the error the entry point would return.
extern "C" int smh_internal_median_route(int entry, int K, int T, int l_harm, int l_perc, int B, int harm_layout, int *out) {
    static const char *const names[] = {"smh_hpss_median_ex_f32", "smh_median_time_ex_f32", "smh_hpss_median_f32", "smh_median_time_f32"};
    SMH_REQUIRE(entry >= 0 && entry <= 3 && out, "smh_internal_median_route: bad entry or null output");
    const bool pair = entry == 0 || entry == 2;
    if (entry >= 2) harm_layout = 0;
    int rc = check_args(out, B, K, T, l_harm, names[entry]);
    if (rc) return rc;
    if (pair && (rc = check_args(out, B, K, T, l_perc, names[entry]))) return rc;
    SMH_REQUIRE(harm_layout >= 0 && harm_layout <= 2, "%s: harm_layout must be 0, 1 or 2", names[entry]);
    Route r{};
    r.family = -1, r.layout = harm_layout;
    if (B > 0) {
        rc = pair ? hpss_route(B, K, T, l_harm, l_perc, harm_layout, &r)
                  : entry == 1 ? time_ex_route(B, K, T, l_harm, harm_layout, &r) : time_route(B, K, T, l_harm, &r);
        if (rc) return rc;
        if (r.family == kFamTwoSingles) {  // either single launch may still refuse the shape
            Route one;
            if ((rc = time_route(B, K, T, l_harm, &one))) return rc;
            if (l_perc != 1 && fast_ok(K, l_perc) && (rc = launch_route(B, K, T, 0, l_perc, 0, &one))) return rc;
        }
    }
    out[0] = r.family, out[1] = r.layout, out[2] = r.plan.ntiles, out[3] = r.plan.TT, out[4] = r.plan.nsh, out[5] = r.plan.nsp;
    return SMH_OK;
}
