// Late fusion (Late_Fusion_Results.py:388-513): an ensemble of two COMPLETE single-input models of one architecture -- model H trained
// on the harmonic half of the H||P featuregram, model P on the percussive half -- whose '3C' outputs are blended,
//   pred = alpha * pred_H + (1 - alpha) * pred_P,   label = argmax(pred).
// Both models run in the B3_MTL forward kernel (smh_tcn.hip) as ONE grid of (workgroups, 2): row 1 reads model P's input and operands
// and writes model P's own output (ForwardOpts::pair_out).  Every workgroup does exactly what it does in a launch of its own, so the
// heads are bit-identical to two smh_model_forward_f32 calls under every schedule the single launch takes.  This file holds the
// ensemble handle, the blend kernel and the three entry points (patches, layer-0 partials, dense featuregram).
#include <algorithm>
#include <cstdint>

#include "smh_model.h"

using namespace smh_tcn;

struct smh_late_fusion {
    smh_model *m[2];           // model H, model P: borrowed, not owned
    float *d_w0cat = nullptr;  // (2 n_feat, 32): model H's layer-0 kernel, then model P's (smh_late_fusion_w0_ptr)
    unsigned long long w0_version[2] = {0, 0};  // the models' weight versions d_w0cat was built from
};

namespace {

constexpr int kMaxClasses = 5;

// One thread per patch.  pred[n][c] = fl(fl(a pH[n][c]) + fl(b pP[n][c])): two rounded products and one rounded sum, no contraction
// into an FMA -- what numpy computes for float32 arrays.  label[n]: the first maximum (np.argmax; a NaN counts as the maximum).
// hH / hP: each model's (N, out_dim) output, '3C' in its last n_classes columns.
__global__ void __launch_bounds__(256) late_blend_kernel(int N, int out_dim, int n_classes, float a, float b,
                                                         const float *__restrict__ hH, const float *__restrict__ hP,
                                                         float *__restrict__ pred, int *__restrict__ label) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const size_t row = (size_t)n * out_dim + (out_dim - n_classes);
    float best = 0.f;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
        if (c < n_classes) {
            const float v = __fadd_rn(__fmul_rn(a, hH[row + c]), __fmul_rn(b, hP[row + c]));
            pred[(size_t)n * n_classes + c] = v;
            if (c == 0 || v > best || (v != v && best == best)) best = v, arg = c;
        }
    }
    if (label) label[n] = arg;
}

int launch_blend(const smh_late_fusion *e, int N, double alpha, const float *hH, const float *hP, float *pred, int *label, hipStream_t st) {
    const smh_model *m = e->m[0];
    const float a = (float)alpha, b = (float)(1.0 - alpha);
    hipLaunchKernelGGL(late_blend_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, m->out_dim, m->cfg.n_classes, a, b, hH, hP, pred, label);
    return smh::launch_status("late_blend_kernel");
}

// both models over N patches, each to its own (N, out_dim) output: one grid of (workgroups, 2), or two launches back to back under
// SMH_LATE_FUSION_TWO_LAUNCH=1 (read per call; A/B runs and tests -- the two forms are bit-identical)
int launch_models(const smh_late_fusion *e, const float *xh, const float *xp, int N, float *out_h, float *out_p, ForwardOpts fo,
                  hipStream_t st) {
    const char *ev = getenv("SMH_LATE_FUSION_TWO_LAUNCH");
    if (ev && atoi(ev) != 0) {
        const int rc = launch_forward(e->m[0], xh, N, out_h, nullptr, nullptr, st, fo);
        return rc ? rc : launch_forward(e->m[1], xp, N, out_p, nullptr, nullptr, st, fo);
    }
    fo.pair = e->m[1], fo.pair_x = xp, fo.pair_out = out_p;
    return launch_forward(e->m[0], xh, N, out_h, nullptr, nullptr, st, fo);
}

// d_w0cat follows the two models' weights: every change of a model's master weights moves its version (repack)
int refresh_w0(smh_late_fusion *e, hipStream_t st) {
    const size_t k0 = (size_t)e->m[0]->cfg.n_feat * C;
    for (int b = 0; b < 2; ++b) {
        if (e->w0_version[b] == e->m[b]->version) continue;
        SMH_CHECK_HIP(hipMemcpyAsync(e->d_w0cat + b * k0, e->m[b]->d_flat + offsets(e->m[b]).w0_k, k0 * sizeof(float),
                                     hipMemcpyDeviceToDevice, st));
        e->w0_version[b] = e->m[b]->version;
    }
    return SMH_OK;
}

size_t heads_floats(const smh_late_fusion *e, size_t N) { return (2 * N * e->m[0]->out_dim + 3) / 4 * 4; }  // (whole 16-byte units)

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; }

}  // namespace

extern "C" int smh_late_fusion_create(smh_model *mH, smh_model *mP, smh_late_fusion **out) {
    SMH_REQUIRE(mH && mP && out, "smh_late_fusion_create: null argument");
    SMH_REQUIRE(mH != mP, "smh_late_fusion_create: the same model passed twice; the ensemble blends two models");
    for (const smh_model *m : {mH, mP}) {
        SMH_REQUIRE(m->heads != SMH_HEADS_FUSION, "smh_late_fusion_create: an intermediate-fusion model has two inputs; the ensemble takes "
                    "two single-input B3_MTL or cascaded models");
        SMH_REQUIRE(m->heads != SMH_HEADS_SINGLE, "smh_late_fusion_create: a single-task model has no H / P counterpart to blend with; the "
                    "ensemble takes two B3_MTL or two cascaded models");
        SMH_REQUIRE(m->cfg.block_variant == 0, "smh_late_fusion_create: built for the keras-tcn 2.3.x block (block_variant 0) only");
    }
    SMH_REQUIRE(mH->heads == mP->heads, "smh_late_fusion_create: the two models differ in head kind (%d and %d): both B3_MTL or both cascaded",
                mH->heads, mP->heads);
    const smh_model_cfg &a = mH->cfg, &b = mP->cfg;
    SMH_REQUIRE(a.n_feat == b.n_feat && a.patch_size == b.patch_size && a.n_classes == b.n_classes && a.nb_stacks == b.nb_stacks &&
                    a.n_dilations == b.n_dilations && a.nb_filters == b.nb_filters && a.kernel_size == b.kernel_size,
                "smh_late_fusion_create: the two models differ in geometry: (n_feat, patch_size, n_classes, stacks, dilations) = "
                "(%d, %d, %d, %d, %d) and (%d, %d, %d, %d, %d)", a.n_feat, a.patch_size, a.n_classes, a.nb_stacks, a.n_dilations,
                b.n_feat, b.patch_size, b.n_classes, b.nb_stacks, b.n_dilations);
    SMH_REQUIRE(a.n_classes <= kMaxClasses, "smh_late_fusion_create: n_classes=%d", a.n_classes);
    auto *e = new smh_late_fusion;
    e->m[0] = mH, e->m[1] = mP;
    const hipError_t err = hipMalloc(&e->d_w0cat, 2 * (size_t)a.n_feat * C * sizeof(float));
    if (err != hipSuccess) {
        delete e;
        return smh::set_error(SMH_E_HIP, "smh_late_fusion_create: hipMalloc failed: %s", hipGetErrorString(err));
    }
    *out = e;
    return SMH_OK;
}

extern "C" void smh_late_fusion_destroy(smh_late_fusion *e) {
    if (!e) return;
    (void)hipFree(e->d_w0cat);
    delete e;
}

extern "C" const float *smh_late_fusion_w0_ptr(smh_late_fusion *e, void *stream) {
    if (!e || refresh_w0(e, (hipStream_t)stream) != SMH_OK) return nullptr;
    return e->d_w0cat;
}

// workspace of the patch and the layer-0 entries: the two models' outputs (2, N, out_dim) (unused when the caller gives d_heads)
extern "C" size_t smh_late_fusion_workspace_bytes(const smh_late_fusion *e, int N) {
    return (e && N > 0) ? sizeof(float) * heads_floats(e, (size_t)N) : 0;
}
extern "C" size_t smh_late_fusion_x0_workspace_bytes(const smh_late_fusion *e, int N) { return smh_late_fusion_workspace_bytes(e, N); }

namespace {
// the checks the three entries share; `who` names the entry in the message
int check_args(const char *who, const smh_late_fusion *e, const void *in, const float *d_pred, double alpha) {
    SMH_REQUIRE(e && in && d_pred, "%s: null argument", who);
    SMH_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "%s: alpha=%g outside [0, 1]", who, alpha);
    return SMH_OK;
}
int check_work(const char *who, const void *d_work, size_t work_bytes, size_t need) {
    SMH_REQUIRE(d_work, "%s: null workspace", who);
    SMH_REQUIRE(aligned16(d_work), "%s: d_work must start on a 16-byte boundary", who);
    SMH_REQUIRE(work_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, work_bytes, need);
    return SMH_OK;
}

int run_patches(smh_late_fusion *e, const float *xh, const float *xp, int N, double alpha, void *d_work,
                float *d_pred, int *d_labels, float *d_heads, const ForwardOpts &fo, hipStream_t st) {
    float *heads = d_heads ? d_heads : static_cast<float *>(d_work);
    float *hH = heads, *hP = heads + (size_t)N * e->m[0]->out_dim;
    const int rc = launch_models(e, xh, xp, N, hH, hP, fo, st);
    return rc ? rc : launch_blend(e, N, alpha, hH, hP, d_pred, d_labels, st);
}
}  // namespace

extern "C" int smh_late_fusion_forward_f32(smh_late_fusion *e, const float *d_xH, const float *d_xP, int N, double alpha, void *d_work,
                                           size_t work_bytes, float *d_pred, int *d_labels, float *d_heads, void *stream) {
    static const char *who = "smh_late_fusion_forward_f32";
    SMH_REQUIRE(N >= 0 && d_xP, "%s: N=%d, or a null input", who, N);
    int rc = check_args(who, e, d_xH, d_pred, alpha);
    if (rc || N == 0) return rc;
    rc = check_work(who, d_work, work_bytes, smh_late_fusion_workspace_bytes(e, N));
    if (rc) return rc;
    return run_patches(e, d_xH, d_xP, N, alpha, d_work, d_pred, d_labels, d_heads, ForwardOpts{}, (hipStream_t)stream);
}

// From the feature kernel's per-half layer-0 partials (N, 2, W, 32), written with w0 = smh_late_fusion_w0_ptr: half 0 IS model H's
// complete first layer and half 1 model P's (each model reads one half of the featuregram), so both models read them in the x0_one
// mode, packed form, and nothing is added up.
extern "C" int smh_late_fusion_forward_x0_f32(smh_late_fusion *e, const float *d_x0p, int N, double alpha, void *d_work, size_t work_bytes,
                                              float *d_pred, int *d_labels, float *d_heads, void *stream) {
    static const char *who = "smh_late_fusion_forward_x0_f32";
    SMH_REQUIRE(N >= 0, "%s: N=%d", who, N);
    int rc = check_args(who, e, d_x0p, d_pred, alpha);
    if (rc || N == 0) return rc;
    rc = check_work(who, d_work, work_bytes, smh_late_fusion_x0_workspace_bytes(e, N));
    if (rc) return rc;
    SMH_REQUIRE(aligned16(d_x0p), "%s: d_x0p is read with 16-byte accesses and must start on a 16-byte boundary", who);
    const size_t half = (size_t)e->m[0]->cfg.patch_size * C;
    ForwardOpts fo;
    fo.from_x0 = 1, fo.x0_one = 1;
    return run_patches(e, d_x0p, d_x0p + half, N, alpha, d_work, d_pred, d_labels, d_heads, fo, (hipStream_t)stream);
}

// Dense file-level inference: layer 0 of both models once per frame (l0_frames_kernel on the concatenated kernel), every hop-`shift`
// patch a window of it.  The patches pass the models and the blend in chunks of kLateDenseChunk, so the workspace is
// [x0 (2, Tc, 32) | the two models' outputs of one chunk] however many patches the featuregram has.
constexpr int kLateDenseChunk = 2048;

extern "C" size_t smh_late_fusion_dense_workspace_bytes(const smh_late_fusion *e, int Tc, int shift) {
    if (!e || Tc < e->m[0]->cfg.patch_size || shift < 1) return 0;
    const int nP = smh_num_patches(Tc, e->m[0]->cfg.patch_size, shift);
    const size_t chunk = (size_t)std::min(std::max(nP, 0), kLateDenseChunk);
    return sizeof(float) * (2 * (size_t)Tc * C + heads_floats(e, chunk));
}

extern "C" int smh_late_fusion_forward_dense_f32(smh_late_fusion *e, const float *d_fv, int Tc, int shift, double alpha, void *d_work,
                                                 size_t work_bytes, float *d_pred, int *d_labels, float *d_heads, void *stream) {
    static const char *who = "smh_late_fusion_forward_dense_f32";
    int rc = check_args(who, e, d_fv, d_pred, alpha);
    if (rc) return rc;
    const int W = e->m[0]->cfg.patch_size, F = e->m[0]->cfg.n_feat, od = e->m[0]->out_dim;
    SMH_REQUIRE(shift >= 1 && Tc >= W, "%s: needs shift >= 1 and at least patch_size=%d frames (Tc=%d, shift=%d); shorter chunks are "
                "tiled by get_feature_patches and take smh_late_fusion_forward_f32", who, W, Tc, shift);
    SMH_REQUIRE(F % 4 == 0, "%s: the per-model n_feat=%d must be a multiple of 4 (whole k steps per half)", who, F);
    rc = check_work(who, d_work, work_bytes, smh_late_fusion_dense_workspace_bytes(e, Tc, shift));
    if (rc) return rc;
    SMH_REQUIRE(aligned16(d_fv), "%s: d_fv is read with 16-byte accesses and must start on a 16-byte boundary", who);
    const int nP = smh_num_patches(Tc, W, shift);
    if (nP <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    rc = refresh_w0(e, st);
    if (rc) return rc;
    float *x0 = static_cast<float *>(d_work);
    rc = launch_l0_frames(d_fv, e->d_w0cat, x0, F, Tc, st);
    if (rc) return rc;
    const int chunk = std::min(nP, kLateDenseChunk);
    float *wk = x0 + 2 * (size_t)Tc * C;
    for (int p0 = 0; p0 < nP; p0 += chunk) {
        const int n = std::min(chunk, nP - p0);
        // patch p0 + i starts at min((p0 + i) shift, Tc - W): the window array advanced by p0 shift frames and shortened by as many
        // (p0 shift <= Tc - W: patch p0's centre lies inside the featuregram)
        const size_t adv = (size_t)p0 * shift;
        ForwardOpts fo;
        fo.from_x0 = 1, fo.x0_one = 1, fo.x0_shift = shift, fo.x0_T = Tc - (int)adv;
        float *hH = d_heads ? d_heads + (size_t)p0 * od : wk;
        float *hP = d_heads ? d_heads + ((size_t)nP + p0) * od : wk + (size_t)n * od;
        rc = launch_models(e, x0 + adv * C, x0 + ((size_t)Tc + adv) * C, n, hH, hP, fo, st);
        if (rc) return rc;
        rc = launch_blend(e, n, alpha, hH, hP, d_pred + (size_t)p0 * e->m[0]->cfg.n_classes, d_labels ? d_labels + p0 : nullptr, st);
        if (rc) return rc;
    }
    return nP;
}
