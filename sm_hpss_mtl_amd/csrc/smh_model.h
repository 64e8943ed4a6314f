// Internal definition of the B3_MTL model object shared by the inference (smh_tcn.hip) and training
// (smh_train.hip) translation units.
#pragma once
#include "smh_common.h"

namespace smh_tcn {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int C = 32;          // nb_filters (fixed by the MFMA tiling)
constexpr int SX = 36;         // LDS row stride of x in floats (16-byte aligned rows)
constexpr int kMaxHeads = 4;
constexpr int kHidden = 16;    // Dense(16) of every MTL head
constexpr int kMaxG = 16;      // patches per workgroup <= MFMA N
constexpr int kPS = 80;        // row stride of the Dense-on-trunk outputs: up to 5 M-tiles (5-class: 69 outputs)
constexpr float kNormEps = 1e-5f;
constexpr float kBnEps = 1e-3f;
constexpr int kCat = kHidden + 2;  // cascaded heads: width of concat[Dropout(16) of S or M, R's two outputs]
// packed per-head tail of a cascaded S / M head in `hp` and in canonical order: [gamma, beta, moving_mean, moving_var (16 each),
// cat gamma, cat beta, cat moving_mean, cat moving_var (18 each), out kernel (18, 1), out bias]
constexpr int kCatTail = 4 * kHidden + 4 * kCat + kCat + 1;
// Packed per-block weights: 64 A-operand slots per lane (48 dilated-conv + 16 1x1), four slots per lane contiguous
// ([slot / 4][lane][slot % 4], see load_block_lds), then [b1 32][b2 32]
constexpr int kBlockFloats = 24 * 2 * 64 + 8 * 2 * 64 + 32 + 32;
// LDS budget of every network kernel (the f32, 2.8-block and split-bf16 forwards, the MFMA and the scalar backward): 4 KB under
// smh::kLdsBytesPerCU.  Inherited -- neither the code nor its history says what the 4 KB are left for.
constexpr size_t kNetLdsLimit = smh::kLdsBytesPerCU - 4 * 1024;

struct TcnArgs {
    int N, T, F, FQ, G, GRP, n_blocks, n_dil, vec_ok;
    int D, NH, n_mt, n_classes, n_heads, out_dim, skip_heads;
    int wlds;     // block weights staged through two LDS slots (0: read from L2 by every wave -- patches too long for the slots)
    unsigned long long *trace;  // tools only (tools/trace_model.py): per-task timestamps of workgroup 0, or nullptr
    int tune;     // experiment switches of the skewed schedule (SMH_TCN_TUNE; tools only)
    int *status;  // device error word of the model (smh_model_status): bit 0 = a wave of the skewed schedule gave up on a dependency
    int spin_limit;  // polls before a wave of the skewed schedule gives up (kSkewSpinLimit; lowered only by the debug knob of the test)
    int split_last;  // barrier schedule, two register sets: the last column tile is computed by TWO waves, 16 output channels each (smh_tcn.hip: half_tile_compute)
    int from_x0;  // X holds the two per-half partials of layer 0, (N, 2, T, 32) (smh_features_l0_f32), instead of patches
    int x0_shift, x0_T;  // from_x0 with x0_shift > 0 (smh_model_forward_dense_f32): X is (2, x0_T, 32), the partials of EVERY frame of a
                         // featuregram of x0_T frames; patch n is the window of T frames starting at min(n * x0_shift, x0_T - T)
    int head_odim[kMaxHeads];
    int head_sigmoid[kMaxHeads];
    int cascade;  // SMH_HEADS_CASCADED: heads S and M read BN18(concat[their Dropout(16), R's output]) (smh_tcn_heads.h)
    int single;   // SMH_HEADS_SINGLE: the tail is single_tail (smh_tcn_heads.h) -- one softmax per patch, no heads
    int trunk_only;  // 1: the forward ends at the trunk (its tap / saved activations); no Dense-on-trunk, no heads (the fusion model's trunks)
    int x0_one;   // from_x0 with ONE partial per frame and channel: X (advanced by the caller to its half) already holds the complete
                  // layer-0 product of this trunk and nothing but the bias is added.  The two addressing forms of the two-half mode:
                  // packed (N, 2, T, 32) read at the full 2 T 32 patch stride, or with x0_shift windows of (x0_T, 32)
    // A second trunk in the same grid (the fusion model; inference, trunk_only): with pair_Wb != nullptr the grid is (workgroups, 2)
    // and the workgroups of row 1 read pair_X / pair_W0 / pair_Wb and write pair_trunk instead of the kernel's parameters; apart
    // from that they do exactly what a launch of their own would
    const float *pair_X, *pair_W0, *pair_Wb;
    float *pair_trunk;
    // A second COMPLETE model in the same grid (the late-fusion ensemble, smh_late_fusion.hip; inference, not trunk_only): row 1 also
    // reads pair_WhA / pair_hp and writes its own (N, out_dim) pair_out.  pair_status: the error word row 1 reports to -- the second model's
    // here, `status` itself for the trunk pair.  The kernel copies these into locals: do not write to the kernel-argument struct in
    // device code, or the compiler copies the whole struct to scratch
    const float *pair_WhA, *pair_hp;
    float *pair_out;
    int *pair_status;
};

// training-mode extras of the forward kernel (all optional)
struct TrainIO {
    float *acts;            // (N, n_blocks + 1, T, 32): input of every block, then the pre-relu TCN output
    const float *drop_tcn;  // (N, n_blocks, 32) SpatialDropout1D masks (0 or 1/(1-rate)), or nullptr
    float *pre;             // (N, kPS): Dense-on-trunk outputs incl. bias (3C logits | head Dense(16)s)
    float *upre;            // (N, n_blocks, T, 32): every block's dilated-conv output incl. bias, before the relu -- the gates of
                            // the backward's relu / channel-max normalisation (it used to recompute them: 48 products per tile)
    int acts_last_only;     // (split-bf16 forward only) save slot n_blocks of `acts` alone: the split-bf16 backward rebuilds every
                            // block's input from its output (x_b = x_b+1 - W2 . y_b - b2), half of the saved bytes never move
};

// heads_train_kernel (smh_train.hip): batch-statistics BN, Dropout, the four losses and d loss / d pre for the '3C'
// softmax and the MTL heads, from the Dense-on-features outputs `pre` (N, kPS) = [3C logits | Dense(16) per head].
// Shared by the B3_MTL trainer and the Conv2D baselines' trainer (smh_cnn_train.hip).
struct HeadsArgs {
    int N, D, NH, n_classes, n_heads, out_dim;
    int head_odim[kMaxHeads], head_sigmoid[kMaxHeads];
    float lw[kMaxHeads + 1];
    size_t goff_head[kMaxHeads];  // canonical offset of each head's first tensor (dense kernel) in `grad`
    size_t goff_c3b;              // canonical offset of the 3C bias
    size_t hp_off[kMaxHeads];     // offset in `hp` of each head's [gamma, beta, mean, var (16 each), out kernel, out bias]
    int ext_losses;               // 1: `losses` has 3 n_heads + 4 floats and gets the per-head binary accuracies at [2 nh + 4 + h]
    int stamps;                   // tools only (SMH_HEADS_STAMPS): thread 0 prints the phase durations (100 MHz ticks)
};
// p: the kernel form, grid and LDS of this batch (smh_train_plan.h: plan_heads), which the heads launchers execute.
// ticket: one zero-initialised device word the kernel's workgroups count themselves on (left at zero again)
struct HeadsPlan;
int launch_heads_train(const HeadsArgs &a, const HeadsPlan &p, const float *pre, const float *y, const float *hp, const float *drop,
                       float *dpre, float *dxh, float *grad, float *bnstat, float *losses, unsigned *ticket, hipStream_t st);
// The same for the cascaded heads (smh_train_cascade.hip; a.n_heads = 3: S, M, R[2]).  dr: (2, N, 2) scratch for d loss / d r of
// S and M; bnstat also receives the BN18 batch statistics of S and M at kMaxHeads * 32 + h * 2 * kCat (means, then variances).
int launch_cascade_heads_train(const HeadsArgs &a, const HeadsPlan &p, const float *pre, const float *y, const float *hp,
                               const float *drop, float *dpre, float *dxh, float *dr, float *grad, float *bnstat, float *losses,
                               hipStream_t st);
// The head of the single-task baseline (smh_train_single.hip; a.n_heads = 0): softmax, the loss (binary cross-entropy over the two
// outputs for n_classes == 2, else categorical cross-entropy), the accuracy, d loss / d logits (-> dpre) and the Dense bias gradient.
// losses: [loss, lw[0] * loss, accuracy, 0]
int launch_single_head_train(const HeadsArgs &a, const float *pre, const float *y, float *dpre, float *grad, float *losses,
                             hipStream_t st);
// floats of the BatchNorm batch-statistics part of the trainer's bucket
constexpr int kBnStatFloats = kMaxHeads * 32;
constexpr int kCatStatFloats = 2 * 2 * kCat;

}  // namespace smh_tcn

struct smh_model {
    smh_model_cfg cfg;
    int n_blocks, n_heads, NH, n_mt, D, out_dim, FQ;
    int head_odim[smh_tcn::kMaxHeads], head_sigmoid[smh_tcn::kMaxHeads];
    int heads = 0;                      // SMH_HEADS_MTL / SMH_HEADS_CASCADED / SMH_HEADS_FUSION / SMH_HEADS_SINGLE
    // SMH_HEADS_FUSION: the two trunks as models of their own (B3_MTL objects whose Dense / heads are never run).  Their master
    // weights are copies of the fusion model's trunk tensors, refreshed by repack(); their operand buffers are what the trunk
    // forwards read.  The fusion model itself packs only the Dense layers on the fused features (D = 2 W 32) and the heads.
    smh_model *trunk[2] = {nullptr, nullptr};
    int head_cat[smh_tcn::kMaxHeads];   // kCat for a head that reads the concatenation (cascaded S, M), else 0
    size_t n_params;
    float *d_flat = nullptr;  // master weights, canonical (Keras-layout) order, n_params floats
    float *d_W0 = nullptr;    // layer-0 A operands + bias0
    float *d_Wb = nullptr;    // per-block packed weights
    float *d_WhA = nullptr;   // Dense-on-trunk weights in A-operand order + biases
    float *d_hp = nullptr;    // per-head BN / out params
    float *d_w0cat = nullptr; // SMH_HEADS_FUSION: the layer-0 kernels of trunk H, then of trunk P, (2 n_feat, 32) in canonical layout -- the
                              // `w0` of the feature kernel and of l0_frames_kernel (smh_fusion_w0_ptr); rebuilt by repack()
    int *d_map = nullptr;     // gather map: packed[i] = map[i] ? flat[map[i]-1] : 0 for [W0 | Wb | WhA | hp]
    size_t nW0, nWb, nWhA, nhp;
    // bf16 operand cache of smh_model_forward_bf16 (smh_tcn_bf16.hip): rebuilt when `version` moves
    void *d_bf16 = nullptr;
    unsigned long long version = 1, bf16_version = 0;
    // Device error word (smh_model_status).  A kernel that cannot produce results -- today: a wave of the skewed schedule, or one
    // half of a split last-round tile of the barrier schedule, whose partner never arrived within its bounded spin -- ORs a bit in;
    // the skewed schedule also zero-fills its workgroup's outputs, the split tile leaves whatever it computed from the stale
    // exchange (NOT results either way).  The host reads and clears the word in smh_model_status.  Never a NaN payload:
    // smh_tcn.hip is compiled -fno-honor-nans.
    int *d_status = nullptr;
};

namespace smh_tcn {
// floats of head h behind its Dense(16) kernel and bias (canonical order = the packed `hp` block)
inline size_t head_tail_floats(const smh_model *m, int h) {
    const int od = m->head_odim[h], cat = m->head_cat[h];
    return cat ? (size_t)4 * kHidden + 4 * cat + (size_t)cat * od + od : (size_t)4 * kHidden + (size_t)kHidden * od + od;
}
// canonical offsets
struct Offsets {
    size_t w0_k, w0_b;                 // initial conv kernel / bias
    size_t blk0, blk_stride;           // first block; per block: k1 (3*C*C), b1 (C), k2 (C*C), b2 (C)
    size_t c3_k, c3_b;                 // 3C kernel (D x ncls), bias
    size_t head[kMaxHeads];            // per head: dense k (D x 16), dense b, gamma, beta, mean, var, out k, out b
    size_t trunk_p = 0;                // fusion: canonical offset of trunk P (trunk H starts at 0, as w0_k ...); else 0
    size_t fbn = 0;                    // fusion: the fused BatchNorm's gamma, beta, moving_mean, moving_variance (D each)
};
// floats of one keras-tcn 2.3 trunk in canonical order
inline size_t trunk_floats(const smh_model_cfg &c) {
    return (size_t)c.n_feat * C + C + (size_t)c.nb_stacks * c.n_dilations * (3 * C * C + C + C * C + C);
}
// floats of one keras-tcn >= 2.8 trunk (block_variant 1) in canonical order: block 0 = [conv0 (3, F, 32), b, conv1 (3, 32, 32), b] and,
// only where n_feat != 32, [matching (1, F, 32), b] -- Keras builds the 1x1 'matching' convolution when the channel counts differ
// and takes the identity shortcut otherwise; later blocks = [conv0 (3, 32, 32), b, conv1 (3, 32, 32), b]
__host__ __device__ inline size_t v2_block0_floats(int F) {
    return (size_t)3 * F * C + C + 3 * C * C + C + (F != C ? (size_t)F * C + C : 0);
}
constexpr size_t kV2BlockFloats = 2 * (3 * C * C + C);
inline size_t trunk_floats_v2(const smh_model_cfg &c) {
    return v2_block0_floats(c.n_feat) + (size_t)(c.nb_stacks * c.n_dilations - 1) * kV2BlockFloats;
}
Offsets offsets(const smh_model *m);
// How a forward of N patches is launched (smh_tcn.hip; DESIGN 4.4 "Forward plan: one function").  ForwardSwitches: the SMH_TCN_*
// switches as read_forward_switches reads them once per launch / query (G 0, skew -1: not set; skew16: lab builds only).  ForwardPlan:
// patches and LDS rows per workgroup, column tiles, waves, the kernel's MODE (kOneSet .. kSkew16), weight slots, split last tile, LDS
// bytes.  plan_forward is host arithmetic alone -- no HIP call, no getenv -- and returns SMH_OK or the refusal of a patch too long
// for the LDS; the launcher, both test queries, launch_forward_v2 and the bf16 forward's plan take their geometry from it.
struct ForwardSwitches {
    int G = 0, skew = -1, waves = 0;
    bool has_waves = false, prefetch = true, split = true, skew16 = false;
};
ForwardSwitches read_forward_switches();
struct ForwardPlan {
    int G, GRP, units, nwaves, mode, wlds, split_last;
    size_t lds;
};
int plan_forward(const smh_model *m, int N, bool train, bool trace, const ForwardSwitches &sw, ForwardPlan *p);
void fill_args(const smh_model *m, int N, const ForwardPlan &p, TcnArgs *a);
// the argument checks shared by the dense file-level entries (`name`): pointers and their alignment, n_feat a multiple of
// feat_multiple, shift and chunk length (short_clip_entry: where shorter chunks go), the workspace size
int dense_entry_ok(const char *name, const smh_model *m, const float *d_fv, int Tc, int shift, const void *d_work, size_t work_bytes,
                   size_t need_bytes, const float *d_out, int feat_multiple, const char *short_clip_entry);
int repack(smh_model *m, hipStream_t st);  // d_flat -> packed operand buffers
int launch_forward_bf16_train(smh_model *m, const float *d_x, int N, const TrainIO *tio, hipStream_t st);  // smh_tcn_bf16.hip
int forward_bf16_supported(const smh_model *m);  // smh_tcn_bf16.hip: SMH_OK, or why the split-bf16 training forward refuses m
// what launch_forward reads and where it ends (the TcnArgs members of the same names); the defaults: patches in, heads out
struct ForwardOpts {
    int from_x0 = 0, x0_shift = 0, x0_T = 0;
    int trunk_only = 0;  // 1: the forward ends at the trunk (d_trunk tap / tio's saved activations); d_out is not written
    int x0_one = 0;      // from_x0: d_x holds one complete layer-0 partial per frame (TcnArgs::x0_one), already advanced to its half
    // a second trunk in the same grid (inference, trunk_only): `pair`'s operands, its input and its tap; same geometry as m
    const smh_model *pair = nullptr;
    const float *pair_x = nullptr;
    float *pair_trunk = nullptr;
    // pair_out != nullptr: the paired launch runs the WHOLE forward of both models (not trunk_only): `pair`'s Dense-on-trunk and
    // heads too, its (N, out_dim) output to pair_out; pair_trunk is then optional like d_trunk.  Same geometry and head kind as m
    float *pair_out = nullptr;
};
int launch_forward(const smh_model *m, const float *d_x, int N, float *d_out, float *d_trunk, const TrainIO *tio,
                   hipStream_t st, const ForwardOpts &opt = {});
// l0_frames_kernel (smh_tcn.hip): x0 (2, Tc, 32) = per half the 1x1 convolution of fv's rows [half * rows, + rows) (fv: (2 rows, Tc))
// with w0's rows of the same range (w0: (2 rows, 32)); rows % 4 == 0
int launch_l0_frames(const float *fv, const float *w0, float *x0, int rows, int Tc, hipStream_t st);
// smh_fusion.hip: the layers behind the intermediate-fusion model's two trunks (SMH_HEADS_FUSION).
// launch_fusion_dense: the Dense layers on the fused features; train = false: xh / xp = the trunk taps (N, W, 32), BN with the moving
// statistics, out = the heads' outputs (N, out_dim); train = true: xh = xhat (N, D), out = pre (N, kPS) incl. biases.
int launch_fusion_dense(const smh_model *m, int N, const float *xh, const float *xp, float *out, bool train, hipStream_t st);
// trainer scratch of the fusion layers (floats) at a batch capacity of max_batch
size_t fusion_scratch_floats(const smh_model *m, int max_batch);
// phase 0: batch statistics (-> bnstat: mean D | variance D), xhat, pre (-> pd); phase 1 (pd = dpre): the Dense kernels' and the fused
// BatchNorm's gradients (stored into `grad`), d loss / d trunk output of both trunks (fusion_gt)
int launch_fusion_train(const smh_model *m, int N, int max_batch, const float *acts_h, const float *acts_p, float *scratch,
                        float *bnstat, float *pd, float *grad, int phase, hipStream_t st);
const float *fusion_gt(const smh_model *m, int max_batch, const float *scratch, int N, int b);
// both trunks of a fusion model over N patches, ending at their taps (N, W, 32): one grid of (workgroups, 2), or two launches back to
// back under SMH_FUSION_TWO_LAUNCH=1 (read per call; A/B runs and tests -- the two forms are bit-identical).  fo: the input mode;
// xh / xp: each trunk's input, in the x0_one mode already advanced to its half
int launch_fusion_trunks(const smh_model *m, const float *xh, const float *xp, int N, float *tap_h, float *tap_p, ForwardOpts fo,
                         hipStream_t st);
// smh_model_cfg.block_variant = 1 (smh_tcn_v2.hip): the two-convolution residual block of keras-tcn >= 2.8, inference only
int launch_forward_v2(const smh_model *m, const float *d_x, int N, float *d_out, float *d_trunk, hipStream_t st);
}  // namespace smh_tcn
