// Entry points of the HPSS median filters (kernel templates: smh_median_kernel.h, smh_median_split.h).  What a call launches is
// decided in smh_median_plan.h; the launchers here execute the plan.
#include "smh_median_kernel.h"
#include "smh_median_split.h"

namespace smh_median {

KernelFn find_pair_kernel(int lh, int lp) {
#define SMH_MEDIAN_E2(a, b) \
    if (lh == a && lp == b) return hpss_median_kernel<a, b>;
    SMH_MEDIAN_PAIRS(SMH_MEDIAN_E2)
    return nullptr;
}

}  // namespace smh_median

namespace {

using namespace smh_median;
static_assert(smh_median::kLdsBytesPerCU == smh::kLdsBytesPerCU, "smh_median_plan.h restates smh_common.h's LDS size");

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

int launch_small(const float *S, int B, int K, int T, int w, int along_t, float *out, hipStream_t st) {
    const size_t total = (size_t)B * K * T;
    const int bs = 256;
    hipLaunchKernelGGL(median_small_kernel, dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, st, S, out, K, T, w,
                       along_t, total);
    return smh::launch_status("median_small_kernel");
}

// What a plan depends on besides the call's arguments and switches: the device's CU count (asked once, and only by a fused call that
// asks for the persistent kernel), the input clip's alignment class and the probe SMH_MEDIAN_PROBE_NOLOAD (timing experiment, outputs
// invalid).
struct Call {
    int n_cu, align;
    bool probe_noload;
};
int device_cus(int K, int T, int lh, int lp, const MedianSwitches &sw, int *n_cu) {
    static int cached = 0;
    if (pair_fused(K, T, lh, lp) && persist_asked(lh, lp, sw) && cached == 0) {
        int dev = 0;
        SMH_CHECK_HIP(hipGetDevice(&dev));
        SMH_CHECK_HIP(hipDeviceGetAttribute(&cached, hipDeviceAttributeMultiprocessorCount, dev));
    }
    *n_cu = cached;
    return SMH_OK;
}
int call_of(const MedianSwitches &sw, const float *S, int K, int T, int lh, int lp, Call *c) {
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(S);
    const size_t clip_bytes = (size_t)K * T * sizeof(float);
    c->align = s0 % 4 != 0 ? 0 : (s0 % 16 == 0 && clip_bytes % 16 == 0) ? 16 : (s0 % 8 == 0 && clip_bytes % 8 == 0) ? 8 : 4;
    c->probe_noload = smh::probe_env("SMH_MEDIAN_PROBE_NOLOAD") != nullptr;
    return device_cus(K, T, lh, lp, sw, &c->n_cu);
}

// Execute a plan of plan_launch or plan_rag (clips != nullptr: T and B are not read).
int run_plan(const MedianPlan &p, int lh, int lp, const float *S, int B, int K, int T, float *harm, float *perc, bool probe_noload,
             hipStream_t st, const smh_rag::Clip *clips = nullptr, const smh_rag::Item *items = nullptr, int n_items = 0) {
    if (p.refusal[0]) return smh::set_error(SMH_E_INVALID, "%s", p.refusal);
    const dim3 grid(p.grid_x, p.grid_y), block((p.nwh + p.nwp) * 64);
    const float ninf = -__builtin_inff(), pinf = __builtin_inff();
    if (p.family == kFamPersist)
        return smh::launch_lds(find_persist_kernel(lh, lp, p.threads), "hpss_median_persist_kernel", grid, block, p.lds, p.lds, st, S, harm,
                               perc, B, K, T, p.nsh, p.nsp, p.nwh, p.layout);
    if (p.family == kFamSplit)
        return smh::launch_lds(find_split_kernel(lh, lp, p.dma != 0), clips ? "hpss_median_split_kernel (ragged)" : "hpss_median_split_kernel",
                               grid, block, p.lds, p.lds, st, S, harm, perc, K, T, p.TT, p.stride, p.nsh, p.nsp, p.nwh, p.layout,
                               probe_noload ? 1.f : ninf, pinf, clips, items, n_items);
    return smh::launch_lds((lh && lp) ? find_pair_kernel(lh, lp) : find_single_kernel(lh, lp), "hpss_median_kernel", grid, block, p.lds,
                           p.lds, st, S, harm, perc, K, T, p.TT, p.stride, p.nsh, p.nsp, p.nwh, p.layout, ninf, pinf);
}

// One filter of window w, along frames (smh_median_time_f32, _ex) or along bins (smh_median_freq_f32: layout 0), behind the entry's
// argument checks.  Returns the layout written, < 0 on error.
int run_single(const MedianSwitches &sw, const float *S, int B, int K, int T, int w, bool along_t, int layout, float *out, hipStream_t st) {
    const int lh = along_t ? w : 0, lp = along_t ? 0 : w;
    Call c;
    int rc = call_of(sw, S, K, T, lh, lp, &c);
    if (rc) return rc;
    const MedianPlan p = along_t ? plan_time_ex(K, T, w, B, layout, sw, c.n_cu, c.align, c.probe_noload)
                                 : plan_freq(K, T, w, B, sw, c.n_cu, c.align, c.probe_noload);
    if (p.family == kFamCopy) {
        SMH_CHECK_HIP(hipMemcpyAsync(out, S, (size_t)B * K * T * sizeof(float), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (p.family == kFamSmall) rc = launch_small(S, B, K, T, w, along_t, out, st);
    else rc = run_plan(p, lh, lp, S, B, K, T, along_t ? out : nullptr, along_t ? nullptr : out, c.probe_noload, st);
    return rc ? rc : p.layout;
}

int check_args(const void *S, int B, int K, int T, int w, const char *name) {
    SMH_REQUIRE(S != nullptr || B == 0, "%s: null input", name);
    SMH_REQUIRE(B >= 0 && K >= 1 && T >= 1, "%s: bad shape B=%d K=%d T=%d", name, B, K, T);
    SMH_REQUIRE(w >= 1 && w <= SMH_MAX_MEDIAN && (w & 1), "%s: window must be odd in [1,%d], got %d", name,
                SMH_MAX_MEDIAN, w);
    SMH_REQUIRE(B <= 65535, "%s: B=%d exceeds the grid limit; split the batch", name, B);
    return SMH_OK;
}

}  // namespace

namespace smh_median {
// ---- clips of different lengths in one launch (smh_rag.h) ----
int launch_rag(const MedianSwitches &sw, const float *d_S, float *d_harm, float *d_perc, int K, int lh, int lp, const smh_rag::Clip *d_clips,
               const smh_rag::Item *d_items, int n_items, hipStream_t st) {
    if (n_items <= 0) return SMH_OK;
    return run_plan(plan_rag(K, lh, lp, sw, n_items), lh, lp, d_S, 0, K, 0, d_harm, d_perc, false, st, d_clips, d_items, n_items);
}

// Fused-pipeline entry and smh_hpss_median_*: both filters in one launch, harm in the layout asked for where the kernel has it, else
// one launch per filter.  Returns the layout written (0, 1 or 2), < 0 on error.
int launch_hpss(const MedianSwitches &sw, const float *S, int B, int K, int T, int lh, int lp, float *harm, float *perc, int want_layout,
                hipStream_t st) {
    Call c;
    int rc = call_of(sw, S, K, T, lh, lp, &c);
    if (rc) return rc;
    const MedianPlan p = plan_hpss_ex(K, T, lh, lp, B, want_layout, sw, c.n_cu, c.align, c.probe_noload);
    if (p.family == kFamTwoSingles) {
        rc = run_single(sw, S, B, K, T, lh, true, 0, harm, st);
        return rc ? rc : run_single(sw, S, B, K, T, lp, false, 0, perc, st);
    }
    rc = run_plan(p, lh, lp, S, B, K, T, harm, perc, c.probe_noload, st);
    return rc ? rc : p.layout;
}
}  // namespace smh_median

extern "C" int smh_median_time_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_harm, float *d_harm,
                                   void *stream) {
    int rc = check_args(d_S, B, K, T, l_harm, "smh_median_time_f32");
    if (rc) return rc;
    SMH_REQUIRE(d_harm || B == 0, "smh_median_time_f32: null output");
    if (B == 0) return SMH_OK;
    return run_single(read_median_switches(), d_S, B, K, T, l_harm, true, 0, d_harm, (hipStream_t)stream);
}

// the harmonic median alone in any of the three layouts of smh_hpss_median_ex_f32 (returns the layout written)
extern "C" int smh_median_time_ex_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_harm, float *d_harm,
                                      int harm_layout, void *stream) {
    int rc = check_args(d_S, B, K, T, l_harm, "smh_median_time_ex_f32");
    if (rc) return rc;
    SMH_REQUIRE(harm_layout >= 0 && harm_layout <= 2, "smh_median_time_ex_f32: harm_layout must be 0, 1 or 2");
    SMH_REQUIRE(d_harm || B == 0, "smh_median_time_ex_f32: null output");
    if (B == 0) return harm_layout;
    return run_single(read_median_switches(), d_S, B, K, T, l_harm, true, harm_layout, d_harm, (hipStream_t)stream);
}

extern "C" int smh_median_freq_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_perc, float *d_perc,
                                   void *stream) {
    int rc = check_args(d_S, B, K, T, l_perc, "smh_median_freq_f32");
    if (rc) return rc;
    SMH_REQUIRE(d_perc || B == 0, "smh_median_freq_f32: null output");
    if (B == 0) return SMH_OK;
    return run_single(read_median_switches(), d_S, B, K, T, l_perc, false, 0, d_perc, (hipStream_t)stream);
}

extern "C" int smh_hpss_median_f32(const smh_ctx *, const float *d_S, int B, int K, int T, int l_harm, int l_perc,
                                   float *d_harm, float *d_perc, void *stream) {
    int rc = check_args(d_S, B, K, T, l_harm, "smh_hpss_median_f32");
    if (rc) return rc;
    rc = check_args(d_S, B, K, T, l_perc, "smh_hpss_median_f32");
    if (rc) return rc;
    SMH_REQUIRE((d_harm && d_perc) || B == 0, "smh_hpss_median_f32: null output");
    if (B == 0) return SMH_OK;
    return smh_median::launch_hpss(read_median_switches(), d_S, B, K, T, l_harm, l_perc, d_harm, d_perc, 0, (hipStream_t)stream);
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
    return smh_median::launch_hpss(read_median_switches(), d_S, B, K, T, l_harm, l_perc, d_harm, d_perc, harm_layout, (hipStream_t)stream);
}

// Test-only (not in include/smh.h): the plan one call of a median entry point executes, from the functions the entry points themselves
// plan with; launches nothing and, with n_cu > 0, initialises no device (n_cu == 0: the device's own count, asked as a launch does).
// entry: 0 smh_hpss_median_ex_f32, 1 smh_median_time_ex_f32, 2 smh_hpss_median_f32, 3 smh_median_time_f32, 4 smh_median_freq_f32,
// 5 the ragged launch (B = n_items; T and harm_layout are ignored); arguments an entry does not have are ignored.  align: the input
// clip's alignment class (16, 8, 4; 0: not 4-byte aligned).  out[0..13]: median_plan_ints -- family (-1 for B == 0: no launch), harm
// layout written, ntiles, TT, nsh, nsp, stride, nwh, nwp, threads, lds, grid_x, grid_y, dma (zero beyond the layout for families 0, 1
// and 5).  Returns SMH_OK, or the error and text the entry point would return.
extern "C" int smh_internal_median_plan(int entry, int K, int T, int l_harm, int l_perc, int B, int harm_layout, int n_cu, int align,
                                        int *out) {
    static const char *const names[] = {"smh_hpss_median_ex_f32", "smh_median_time_ex_f32", "smh_hpss_median_f32", "smh_median_time_f32",
                                        "smh_median_freq_f32"};
    SMH_REQUIRE(entry >= 0 && entry <= 5 && out && n_cu >= 0 && (align == 0 || align == 4 || align == 8 || align == 16),
                "smh_internal_median_plan: bad entry, CU count or alignment class, or null output");
    const MedianSwitches sw = read_median_switches();
    const bool pair = entry == 0 || entry == 2;
    const int lh = entry == 4 ? 0 : l_harm, lp = pair || entry >= 4 ? l_perc : 0;  // the filters the entry has
    MedianPlan p = plan_of(kFamNone, entry == 5 ? 2 : entry >= 2 ? 0 : harm_layout);
    if (entry == 5) {
        SMH_REQUIRE(K >= 1, "smh_internal_median_plan: bad shape K=%d", K);
        if (B > 0) p = plan_rag(K, lh, lp, sw, B);
    } else {
        int rc = check_args(out, B, K, T, entry == 4 ? lp : lh, names[entry]);
        if (rc) return rc;
        if (pair && (rc = check_args(out, B, K, T, lp, names[entry]))) return rc;
        SMH_REQUIRE(p.layout >= 0 && p.layout <= 2, "%s: harm_layout must be 0, 1 or 2", names[entry]);
        if (n_cu == 0 && B > 0 && (rc = device_cus(K, T, lh, lp, sw, &n_cu))) return rc;
        if (B > 0) {
            p = pair         ? plan_hpss_ex(K, T, lh, lp, B, p.layout, sw, n_cu, align)
                : entry == 4 ? plan_freq(K, T, lp, B, sw, n_cu, align) : plan_time_ex(K, T, lh, B, p.layout, sw, n_cu, align);
            if (p.family == kFamTwoSingles) {  // one launch per filter: either may still refuse the shape
                const MedianPlan h = plan_time(K, T, lh, B, sw, n_cu, align), q = plan_freq(K, T, lp, B, sw, n_cu, align);
                if (h.refusal[0] || q.refusal[0]) p = h.refusal[0] ? h : q;
            }
        }
    }
    if (p.refusal[0]) return smh::set_error(SMH_E_INVALID, "%s", p.refusal);
    median_plan_ints(p, out);
    return SMH_OK;
}

// The query's earlier form, kept for its callers: entries 0 - 3 on the device's own CU count, out[0..5] = the plan's first six ints.
extern "C" int smh_internal_median_route(int entry, int K, int T, int l_harm, int l_perc, int B, int harm_layout, int *out) {
    SMH_REQUIRE(entry >= 0 && entry <= 3 && out, "smh_internal_median_route: bad entry or null output");
    int v[14];
    const int rc = smh_internal_median_plan(entry, K, T, l_harm, l_perc, B, harm_layout, 0, 16, v);
    for (int i = 0; i < 6 && !rc; ++i) out[i] = v[i];
    return rc;
}
