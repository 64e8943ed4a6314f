// Internal interface between smh_feat.hip and smh_frontend.hip.
#pragma once
#include "smh_common.h"

namespace smh_feat {

constexpr int kMaxMels = 256;     // filters held in LDS by the fused feature kernel
constexpr int kMaxMelNnz = 2048;  // taps held in LDS

// patch layouts of the finishing kernels, numbered as smh_extract_patches_f32 numbers its `layout` argument (include/smh.h)
constexpr int kLayoutImage = 0;      // (nP, 2*rows, W): the Conv2D models' images, harmonic rows first
constexpr int kLayoutTimeMajor = 1;  // (nP, W, 2*rows): the TCN's input

struct MelTable {
    int n_mels, nnz;
    const int *start, *count, *off;
    const float *w;
};

MelTable mel_table(const smh_ctx *c);

// the bin walk's per-context plan as a kernel argument (smh_ctx.hip builds it): row segments, their bin ranges, and where each
// segment's per-bin records {w0, w1, w2, w3, n_emit, -, -, -} start in `plan`
struct FeatPlan {
    int nseg, pend;  // pend: most filters pending at any bin (2 or 4 accumulators)
    int m0[smh_ctx::kMaxFeatSegs], m1[smh_ctx::kMaxFeatSegs], kbeg[smh_ctx::kMaxFeatSegs], kend[smh_ctx::kMaxFeatSegs],
        off[smh_ctx::kMaxFeatSegs];
    const float *plan;
    unsigned long long *trace;  // tools/trace_features.py: phase stamps (s_memrealtime) per workgroup and wave, or nullptr
};
FeatPlan feat_plan(const smh_ctx *c, int which /* 0: four segments, 1: eight */);

// (S, harm, perc) -> featuregram fv (B, 2*rows, T) with un-clipped dB values + per-array max keys
// harm_tmajor != 0: harm is (B, T, K) as written by smh_median::launch_hpss(want_tmajor = 1)
int launch_hp_feat(const smh_ctx *c, const float *S, const float *harm, const float *perc, int harm_tmajor, int B, int T,
                   float *fv, int *maxkeys, hipStream_t st);
// top_db clip (in place) + StandardScaler + patches (launch_std_patch below)
// everything after the medians in one kernel per clip; harmb = harm in layout 2 (B, ceil(T/16), K, 16).
// Returns 1 if it ran, 0 if the shape does not qualify (the caller must then not have asked for layout 2), < 0 on error
int launch_features_clip(const smh_ctx *c, const float *S, const float *harmb, const float *perc, int B, int T, int W,
                         int shift, int nP, float *fv, float *patches, const float *w0, float *x0p, hipStream_t st,
                         int layout = kLayoutTimeMajor);
// w0 / x0p non-null: also emit this half's share of the network's first Conv1D (see smh_features_l0_f32)
// scratch (scratch_bytes): device memory the long-clip path may use for its standardised copy of the featuregram (2 * B * rows * T
// floats) instead of a stream-ordered allocation per call -- smh_frontend_f32 hands it the S / perc part of its workspace, dead by then
int launch_std_patch(const smh_ctx *c, float *fv, const int *maxkeys, int B, int T, int W, int shift, int nP,
                     float *patches, hipStream_t st, const float *w0 = nullptr, float *x0p = nullptr, void *scratch = nullptr,
                     size_t scratch_bytes = 0, int layout = kLayoutTimeMajor);

// ---- device helpers of the finishing kernels (smh_ragged.hip, smh_plain.hip) ------------------------------------------------------
constexpr float kAmin = 1e-10f;  // librosa.power_to_db amin

// item n of a 1-D grid whose workgroup i runs on XCD i % 8: the list in 8 contiguous ranges, one per XCD (smh_stft.hip has the reasoning)
__device__ __forceinline__ bool xcd_item(int n_items, unsigned &n) {
    const unsigned total = (unsigned)n_items, per_xcd = (total + 7u) >> 3;
    const unsigned j = blockIdx.x >> 3;
    n = (blockIdx.x & 7u) * per_xcd + j;
    return j < per_xcd && n < total;
}

// top-dB floor in the power domain (features_clip_kernel has the derivation):
//   max(10 log10(max(amin, x^2)), dBmax - 80) = 10 log10(max(x^2, lim)),  lim = max(amin, max(amin, xmax^2) * 1e-8)
// -- the amin clamp acts on the f32 square
__device__ __forceinline__ float floor_of_max(int key) {
    const float xm = __int_as_float(key);
    return fmaxf(kAmin, fmaxf(kAmin, xm * xm) * 1e-8f);
}
__device__ __forceinline__ float final_value(float x, float lim, int log_db) {
    return log_db ? 3.0102999566398120f * __builtin_amdgcn_logf(fmaxf(x * x, lim)) : x;
}

// StandardScaler of one row (lib/preprocessing.py:211-214) from one shifted pass: x0 the row's first value, s and q the f64 sums of
// d = value - x0 and of d^2 over its T frames -> the f64 mean and 1 / scale.  Population variance; constant rows stay unscaled by
// sklearn's _is_constant_feature / _handle_zeros_in_scale, whose bound grows with the number of samples the scaler was fitted on:
// n_fit, which the caller decides (T, or the tiled-if-short length).
__device__ __forceinline__ void scaler_of_sums(double x0, double s, double q, int T, int n_fit, double &mean, double &inv_scale) {
    const double md = s / (double)T;
    mean = x0 + md;
    const double var = fmax(q / (double)T - md * md, 0.0);
    const double eps = 2.220446049250313e-16;
    const double nm = (double)n_fit * mean * eps;
    const bool constant = var <= (double)n_fit * eps * var + nm * nm;
    double scale = sqrt(var);
    if (constant || scale == 0.0) scale = 1.0;
    inv_scale = 1.0 / scale;
}

// the patches p_lo .. p_hi that hold position u of the tiled featuregram (tools.extract_patches' grid, lib/cython_impl/tools.pyx:21-38:
// patch p = frames p * shift .. p * shift + W - 1); patch starts are never clamped, so u sits at j = u - p * shift, 0 <= j < W
__device__ __forceinline__ void patch_range(int u, int W, int shift, int nP, int &p_lo, int &p_hi) {
    p_hi = u / shift;
    if (p_hi > nP - 1) p_hi = nP - 1;
    p_lo = u - W + 1 <= 0 ? 0 : (u - W + shift) / shift;  // ceil((u - W + 1) / shift)
}

}  // namespace smh_feat

namespace smh_median {
// both HPSS medians in one launch; returns 1 if harm was written time-major (B,T,K), 0 if (B,K,T), <0 on error
int launch_hpss(const float *S, int B, int K, int T, int lh, int lp, float *harm, float *perc, int want_tmajor,
                hipStream_t st);
}  // namespace smh_median
