// Internal interface between smh_feat.hip and smh_frontend.hip.
#pragma once
#include "smh_common.h"
#include "smh_wave.h"

namespace smh_rag {
struct Clip;
}

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

// ---- LDS budgets of the feature stage: the one place they are written ("Feature routes") --------------------------------
// Every router (smh_features_blocked_ok, smh_rag::feature_route and through it smh_frontend_f32, the ragged planner's classes and
// pipeline.HotPath) and every launcher sizes its image with these, so a clip cannot be routed to a kernel whose image does not fit.
constexpr size_t kClipImageLimit = 158 * 1024;  // both halves of a clip in one workgroup, or as two workgroups of one CU
constexpr size_t kHalfImageLimit = 150 * 1024;  // one half (always met by a clip that met kClipImageLimit; the launcher asserts it)
constexpr size_t kStdPatchLimit = 150 * 1024;   // std_patch_kernel's tile of one half; beyond it the long-clip kernels

// features_clip_kernel: [2*rows][T|1] values + three per-row scaler tables + 32 ints; with layer 0 the (2*rows, 32) weights
inline size_t clip_image_bytes(int rows, int T, bool with_l0) {
    size_t b = sizeof(float) * ((size_t)2 * rows * (T | 1) + 3 * (size_t)2 * rows) + 128;
    if (with_l0) b += sizeof(float) * 2 * rows * 32;
    return b;
}
// features_half_kernel: one half of the same; w0_copy: its (rows, 32) share of the layer-0 weights in LDS (lab builds only)
inline size_t half_image_bytes(int rows, int T, bool w0_copy) {
    size_t b = sizeof(float) * ((size_t)rows * (T | 1) + 3 * (size_t)rows) + 64;
    if (w0_copy) b += sizeof(float) * rows * 32;
    return b;
}
inline size_t std_patch_tile_bytes(int rows, int T) { return sizeof(float) * ((size_t)rows * (T | 1) + 3 * (size_t)rows); }
// "the single-kernel feature path takes a clip of T frames in this context [and emits layer 0 with it]"
bool features_image_ok(const smh_ctx *c, int T, bool with_l0);

// where a call's patches go.  Built once per entry by patch_out and handed down to the launchers.
struct PatchOut {
    float *patches;  // nullptr: none asked for, or none fit
    int W, shift;    // >= 1 also without patches
    int nP;          // patches per clip of T frames; 0 in a ragged call, whose clips carry their own (smh_rag::Clip)
    int layout;      // kLayoutImage / kLayoutTimeMajor
};
// `who` names the entry in the error text.  always: the geometry counts without a patch buffer too (layer 0 reads W-frame windows).
// T = 0: a ragged call.
inline int patch_out(const char *who, float *d_patches, bool always, int T, int W, int shift, int layout, PatchOut &po) {
    po = PatchOut{d_patches, W > 0 ? W : 1, shift > 0 ? shift : 1, 0, layout};
    if (!d_patches && !always) return SMH_OK;
    SMH_REQUIRE(W >= 1 && shift >= 1, "%s: bad patch geometry W=%d shift=%d", who, W, shift);
    if (T > 0) {
        po.nP = smh_num_patches(smh_tiled_frames(T, W), W, shift);
        if (po.nP <= 0) po.patches = nullptr;
    }
    return SMH_OK;
}

// (S, harm, perc) -> featuregram fv (B, 2*rows, T) with un-clipped dB values + per-array max keys
// harm_tmajor != 0: harm is (B, T, K) as written by smh_median::launch_hpss(want_tmajor = 1)
int launch_hp_feat(const smh_ctx *c, const float *S, const float *harm, const float *perc, int harm_tmajor, int B, int T,
                   float *fv, int *maxkeys, hipStream_t st);
// The clips one launch of the LDS-image kernels covers: n equal clips of T frames (d_clips == nullptr), or the n clips of a ragged
// call that d_list names, whose shapes the kernels read from d_clips; T is then the most frames of any and sizes the image.
struct ImageClips {
    int n, T;
    const smh_rag::Clip *d_clips;
    const int *d_list;
    int even_T;  // list only: all of even T (features_half_kernel) or all of odd T (features_clip_kernel)
};
// everything after the medians in one kernel per clip; harmb = harm in layout 2 (B, ceil(T/16), K, 16).
// w0 / x0p non-null (equal clips only): also emit each half's share of the network's first Conv1D (see smh_features_l0_f32).
// Returns 1 if it ran, 0 if the shape does not qualify (the caller must then not have asked for layout 2), < 0 on error
int launch_features_image(const smh_ctx *c, const float *S, const float *harmb, const float *perc, const ImageClips &clips,
                          const PatchOut &po, float *fv, const float *w0, float *x0p, hipStream_t st);
// top_db clip (in place) + StandardScaler + patches
// scratch (scratch_bytes): device memory the long-clip path may use for its standardised copy of the featuregram (2 * B * rows * T
// floats) instead of a stream-ordered allocation per call -- smh_frontend_f32 hands it the S / perc part of its workspace, dead by then
int launch_std_patch(const smh_ctx *c, float *fv, const int *maxkeys, int B, int T, const PatchOut &po, hipStream_t st,
                     const float *w0, float *x0p, void *scratch, size_t scratch_bytes);

// ---- device helpers of the finishing kernels (smh_ragged.hip, smh_plain.hip) ------------------------------------------------------
constexpr float kAmin = 1e-10f;  // librosa.power_to_db amin

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

// ---- the per-file StandardScaler of smh_standardize_rows_f32, shared with the patch statistics (smh_skew.hip): ONE definition, so
// that a value standardised there is bit for bit the patch element written here ------------------------------------------------------
using smh::wave_sum;  // smh_wave.h: the xor-tree order

// sklearn StandardScaler statistics of one row held by one wave: float64 mean / population variance,
// (near-)constant rows are left unscaled (sklearn _is_constant_feature / _handle_zeros_in_scale).
template <typename Load>
__device__ __forceinline__ void row_stats(int T, int lane, Load &&load, double &mean, double &scale) {
    double s = 0.0;
    for (int t = lane; t < T; t += 64) s += (double)load(t);
    mean = wave_sum(s) / (double)T;
    double q = 0.0;
    for (int t = lane; t < T; t += 64) {
        const double d = (double)load(t) - mean;
        q += d * d;
    }
    const double var = wave_sum(q) / (double)T;
    const double eps = 2.220446049250313e-16;
    const double nm = (double)T * mean * eps;
    const bool constant = var <= (double)T * eps * var + nm * nm;
    scale = sqrt(var);
    if (constant || scale == 0.0) scale = 1.0;
}

// `X -= mean; X /= scale` applied to a float32 array with float64 statistics: two roundings.
__device__ __forceinline__ float standardize(float x, double mean, double scale) {
    const float c = (float)((double)x - mean);
    return (float)((double)c / scale);
}

}  // namespace smh_feat
