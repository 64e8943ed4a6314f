// Launch plan of one TCN training step (smh_train.hip, smh_train_bf16.hip, smh_train_cascade.hip, smh_train_single.hip): which
// forward, which heads kernels in which form, which trunk backward on which grid with how much LDS, and the small kernels around
// it, decided here, once, as a plain value.  train_step, the heads launchers, the bf16 launcher, smh_fusion_train_step_f32,
// smh_internal_bwd_residency and the test query (smh_internal_train_plan) all take it from these functions.  Host arithmetic only,
// no HIP: a stand-alone host program can include this header by itself.  The constants of smh_model.h / smh_common.h that the
// arithmetic needs are restated in Dims; smh_train.hip holds the two together with static_asserts.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "../../include/smh.h"

namespace smh_tcn {

struct Dims {
    static constexpr int C = 32, SX = 36, PS = 80, Hidden = 16, MaxHeads = 4;  // smh_model.h: C, SX, kPS, kHidden, kMaxHeads
    static constexpr size_t LdsPerCU = 160 * 1024;                             // smh_common.h: kLdsBytesPerCU
    static constexpr size_t NetLdsLimit = LdsPerCU - 4 * 1024;                 // smh_model.h: kNetLdsLimit
};

// The implementation switches of the training step (A/B and tests), one getenv each: the only getenv of the step.  Read at the top of
// every step rather than once in smh_trainer_create: tests flip SMH_BWD_BF16, SMH_BWD_SPLIT and SMH_HEADS_GLOBAL between the steps
// of one trainer.  (SMH_BWD_PROBE makes results invalid and stays a probe_env read in the bf16 launcher.)
struct TrainSwitches {
    bool valu = false;         // SMH_TRAIN_VALU set: the scalar backward kernel (tcn_backward_kernel)
    bool bf16_bwd = true;      // SMH_BWD_BF16, default on: dtype 1's split-bf16 backward (0: the exact-f32 backward behind the bf16 forward)
    int split3 = 1;            // SMH_BWD_SPLIT, default 1: BwdArgs::split3
    int stamps = 0;            // SMH_BWD_STAMPS set: BwdArgs::stamps
    bool dwh_valu = false;     // SMH_DWH_VALU set: dwh_kernel instead of dwh_mfma_kernel
    bool heads_global = false;  // SMH_HEADS_GLOBAL set: heads_train_kernel reads global memory whatever the batch size
    int heads_stamps = 0;      // SMH_HEADS_STAMPS set: HeadsArgs::stamps
};
inline TrainSwitches read_train_switches() {
    TrainSwitches s;
    s.valu = getenv("SMH_TRAIN_VALU") != nullptr;
    const char *ev = getenv("SMH_BWD_BF16");
    s.bf16_bwd = !(ev && atoi(ev) == 0);
    ev = getenv("SMH_BWD_SPLIT");
    s.split3 = ev ? atoi(ev) != 0 : 1;
    s.stamps = getenv("SMH_BWD_STAMPS") ? 1 : 0;
    s.dwh_valu = getenv("SMH_DWH_VALU") != nullptr;
    s.heads_global = getenv("SMH_HEADS_GLOBAL") != nullptr;
    s.heads_stamps = getenv("SMH_HEADS_STAMPS") ? 1 : 0;
    return s;
}

struct Grid3 {
    int x, y, z;  // all zero: the kernel is not launched
};

// ---- heads ----------------------------------------------------------------------------------------------------------------------
// A heads kernel is STAGED when its tile of `pre` and of the targets fits the LDS beside the kernel's static arrays: the budget is
// the CU's 160 KB minus those.  heads_train_kernel holds 17 accumulator rows of kQ = 542 floats, two rows of 64 statistics and 64
// fixed-point sums, 37 880 bytes: 122 KB are left (3 classes: 232 bytes per patch, up to 538 patches; 5 classes: 320, up to 390).
// The cascaded kernels' static rows (9 of kA = 166 floats and the per-unit statistics) are far smaller; their budget was set to
// 120 KB when they were written and the plans that tests pin (136 and 76 bytes per patch: 903 and 1616 patches) follow from it.
constexpr size_t kHeadsStageBytes = Dims::LdsPerCU - 38 * 1024;
constexpr size_t kCascadeStageBytes = Dims::LdsPerCU - 40 * 1024;
constexpr int kHeadsThreadsMax = 512;  // heads_train_kernel: 512 threads up to this many patches (a sample per lane), 1024 beyond
constexpr int kSmallHeadThreads = 512;  // the cascaded and the single-task kernels (their kTh): one instantiation each

enum HeadsFamily { kHeadsFamilyMtl = 0, kHeadsFamilyCascaded = 1, kHeadsFamilySingle = 2 };
struct HeadsLaunch {
    int staged, threads, grid;
    size_t lds;  // dynamic LDS bytes of the launch: the staged tile, 0 for the global form
};
// MTL / fusion: k[0] = heads_train_kernel<staged, threads>.  Cascaded: k[0] = cascade_sm_kernel<staged>, k[1] = cascade_r_kernel<staged>.
// Single: k[0] = single_head_train_kernel (one instantiation, one workgroup that walks the batch in passes of its 512 lanes).
struct HeadsPlan {
    HeadsFamily family;
    int n_launch;
    HeadsLaunch k[2];
};
inline HeadsLaunch heads_launch(size_t tile_bytes, size_t budget, bool forced_global, int threads, int grid) {
    const bool staged = tile_bytes <= budget && !forced_global;
    return HeadsLaunch{staged ? 1 : 0, threads, grid, staged ? tile_bytes : 0};
}
inline HeadsPlan plan_heads(int heads, int n_classes, int n_heads, int out_dim, int N, const TrainSwitches &sw) {
    HeadsPlan p{};
    const size_t n = (size_t)N;
    if (heads == SMH_HEADS_SINGLE) {
        p.family = kHeadsFamilySingle, p.n_launch = 1;
        p.k[0] = HeadsLaunch{0, kSmallHeadThreads, 1, 0};
    } else if (heads == SMH_HEADS_CASCADED) {  // the staged columns of `pre` and the targets; no switch
        p.family = kHeadsFamilyCascaded, p.n_launch = 2;
        p.k[0] = heads_launch(sizeof(float) * (n * (2 * Dims::Hidden + 1) + n), kCascadeStageBytes, false, kSmallHeadThreads, 3);
        p.k[1] = heads_launch(sizeof(float) * (n * (Dims::Hidden + 1) + 2 * n), kCascadeStageBytes, false, kSmallHeadThreads, 1);
    } else {  // B3_MTL and intermediate fusion: rows of `pre` and of the targets at odd strides, one workgroup per head and one for '3C'
        p.family = kHeadsFamilyMtl, p.n_launch = 1;
        const int NHc = n_classes + n_heads * Dims::Hidden;
        p.k[0] = heads_launch(sizeof(float) * (n * (NHc | 1) + n * (out_dim | 1)), kHeadsStageBytes, sw.heads_global,
                              N <= kHeadsThreadsMax ? 512 : 1024, n_heads + 1);
    }
    return p;
}

// ---- trunk backward -------------------------------------------------------------------------------------------------------------
// scalar kernel (tcn_backward_kernel)
constexpr int kBG = 1;        // patches per workgroup
constexpr int kBS = 33;       // LDS row stride (floats) of its buffers
constexpr int kBThreads = 1024;
// f32 MFMA kernel (tcn_backward_mfma_kernel)
constexpr int kMG = 1;
constexpr int kWS = 36;  // row stride of the weight copies in LDS
constexpr int kMThreads = 512;
constexpr int kZW = 3 * Dims::SX + 4;  // zero words behind the images (tile_jobs)
constexpr int kMfmaMaxT = 128;   // short form: two float4 of saved activations per thread in the register prefetch; block kernels parked in LDS
constexpr int kMfmaLongT = 256;  // long form: four; kernels read from global memory (no LDS left)
// Dense-on-trunk weight gradient
constexpr int kDwhSlice = 16;  // dwh_kernel: patches per batch slice (grid.y)
constexpr int kDwhSplit = 8;   // dwh_mfma_kernel: batch slices (grid.z)
// split-bf16 kernel (tcn_backward_bf16_kernel): a block's operand slot (and its image in the packed buffer), in pieces of 1 KiB = 64
// lanes x 16 bytes: hi units 0..9, the 1x1 bias b2 as 32 raw floats, lo units 0..9.  Units: 0, 1 = W2 [mt] for dyn (canonical rows),
// 2..7 = W1 [tap][mt], 8, 9 = W2 [mt] in the forward's orientation (rows = output channel), for x_b = x_b+1 - W2 . y_b - b2.
constexpr int kDuRow = 80;  // bytes per row of the du images: 32 bf16 + 16 bytes of padding (smh_tcn_bf16.hip: kRS)
constexpr int kUnitsPerBlk = 10;
constexpr int kBiasPiece = kUnitsPerBlk, kLoPiece = kUnitsPerBlk + 1, kSlotPieces = 2 * kUnitsPerBlk + 1;
constexpr int kSlotLo = kLoPiece * 1024;  // byte offset of the lo units
constexpr int kSlotBytes = kSlotPieces * 1024;

// LDS plan of the split-bf16 kernel (a kernel argument: the layout is the kernel's)
struct BwdGeo {
    int G;        // patches per workgroup
    int units;    // 16-frame tiles per patch (<= 8: one per wave)
    int K32;      // k steps of 32 frames in the weight-gradient products
    int halo;     // zero frames in front of / behind the xT rows: 8 -- only dilations below 8 read across a chunk boundary
    int sxt, st;  // row strides in bytes of xT and of yT / gT / duT (16 x odd)
    int o_x, o_y, o_g, o_du_t, o_du;  // byte offsets of the image pairs inside a patch's region (hi, then lo at + the pair's half)
    int h_x, h_t, h_du;               // the halves: 32 * sxt, 32 * st, (T + 1) * kDuRow
    int per_patch;                    // bytes per patch
};
// false: the patch does not fit.  The kernel is instantiated for two patches per workgroup with K32 <= 3 and one with K32 = 4,
// which is what the arithmetic gives for every T <= 128 (K32 = 1, 2, 3, 4 up to 32, 64, 96, 128 frames; two patches up to 96).
inline bool bwd_geo(int T, BwdGeo *g) {
    if (T < 1 || T > 128) return false;
    g->units = (T + 15) / 16;
    g->K32 = (16 * g->units + 31) / 32;
    g->halo = 8;
    g->sxt = 2 * (2 * g->halo + 32 * g->K32) + 16;  // 16 x (3 + 4 K32): an odd multiple of 16 bytes
    g->st = 2 * 32 * g->K32 + 16;
    g->h_x = 32 * g->sxt, g->h_t = 32 * g->st, g->h_du = (T + 1) * kDuRow;
    g->o_x = 0;
    g->o_y = g->o_x + 2 * g->h_x;
    g->o_g = g->o_y + 2 * g->h_t;
    g->o_du_t = g->o_g + 2 * g->h_t;
    g->o_du = g->o_du_t + 2 * g->h_t;
    g->per_patch = g->o_du + 2 * g->h_du;
    g->per_patch = (g->per_patch + 15) / 16 * 16;
    if ((size_t)16 * g->units * Dims::SX * sizeof(float) > (size_t)g->per_patch) return false;  // the tail's f32 rows live on the patch's images
    g->G = (size_t)2 * g->per_patch + kSlotBytes <= Dims::LdsPerCU ? 2 : 1;
    if ((size_t)g->G * g->per_patch + kSlotBytes > Dims::LdsPerCU) return false;
    return (g->G == 2 && g->K32 <= 3) || (g->G == 1 && g->K32 == 4);
}

enum BwdRoute { kBwdBf16 = 0, kBwdMfmaShort = 1, kBwdMfmaLong = 2, kBwdScalar = 3, kBwdRefused = 4 };
enum DwhKind { kDwhNone = 0, kDwhMfma = 1, kDwhValu = 2 };
struct BackwardPlan {
    BwdRoute route;
    int grid, threads;
    size_t lds;
    int RPm;             // MFMA: LDS rows of a workgroup's images
    int use_wt;          // scalar: BwdArgs::use_wt, transposed LDS copies of the block kernels (0: patches so long that they do not fit)
    BwdGeo geo;          // bf16: G patches per workgroup, K32, the image offsets
    int acts_last_only;  // TrainIO::acts_last_only: the bf16 route rebuilds every block's input, so the forward saves the last slot alone
    Grid3 dtrunk;        // dtrunk_kernel (256 threads): d loss / d (trunk output) for the bf16 and MFMA routes of a one-input model
    DwhKind dwh;         // the Dense-on-trunk weight gradient behind those routes (the scalar kernel computes it itself, the fusion
    Grid3 dwh_grid;      // model's Dense layers are smh_fusion.hip's); 256 threads
    size_t gt_patch_floats;  // MFMA route of a one-input model: floats per patch of the trainer's d_gt
    size_t pack_slot_bytes, pack_bytes;  // bf16: the blocks' operand slots, and the whole pack [slots | gt (N, T, 32)]
};
// the f32 MFMA trunk backward at patch length T: the short form parks the block kernels in LDS, the long one reads them from the
// weight vector.  kBwdRefused beyond kMfmaLongT.
struct MfmaPlan {
    BwdRoute route;
    size_t lds;
    int RPm;
};
inline MfmaPlan plan_mfma(int T) {
    const int RPm = ((kMG * T + 15) / 16) * 16;
    const size_t lds_m = sizeof(float) * ((size_t)4 * RPm * Dims::SX + 4 * Dims::C * kWS + kMG * Dims::PS + Dims::C + kZW);
    const size_t lds_long = sizeof(float) * ((size_t)4 * RPm * Dims::SX + kMG * Dims::PS + Dims::C + kZW);
    const bool short_ok = lds_m <= Dims::NetLdsLimit && T <= kMfmaMaxT, long_ok = lds_long <= Dims::NetLdsLimit && T <= kMfmaLongT;
    return MfmaPlan{short_ok ? kBwdMfmaShort : long_ok ? kBwdMfmaLong : kBwdRefused, short_ok ? lds_m : lds_long, RPm};
}
// One trunk's backward of N patches of T frames.  fusion: each of the two trunks takes the MFMA route fed by smh_fusion.hip (no
// dtrunk, no dwh, no switch); it is refused beyond kMfmaLongT frames.  Else, in this order: dtype 1 takes the bf16 route where the
// geometry fits (T <= 128) unless SMH_BWD_BF16=0 or SMH_TRAIN_VALU; the MFMA route serves T <= 256 unless SMH_TRAIN_VALU; the
// scalar kernel serves the rest -- with transposed kernel copies while they fit (T <= 234), without up to 264 frames, refused beyond.
// Fields that belong to another route stay zero.
inline BackwardPlan plan_backward(int T, int n_blocks, int n_heads, int N, int dtype, bool fusion, const TrainSwitches &sw) {
    BackwardPlan p{};
    p.use_wt = 1;
    const int D = T * Dims::C;
    const MfmaPlan m = plan_mfma(T);
    BwdGeo geo;
    const bool bf16 = !fusion && dtype == 1 && !sw.valu && sw.bf16_bwd && bwd_geo(T, &geo);
    if (bf16) {
        p.route = kBwdBf16, p.geo = geo, p.acts_last_only = 1;
        p.grid = (N + geo.G - 1) / geo.G, p.threads = 512 * geo.G;
        p.lds = (size_t)geo.G * geo.per_patch + kSlotBytes;
        p.pack_slot_bytes = (size_t)n_blocks * kSlotBytes;
        p.pack_bytes = p.pack_slot_bytes + (size_t)N * D * sizeof(float);
    } else if (fusion || (m.route != kBwdRefused && !sw.valu)) {
        p.route = m.route, p.lds = m.lds, p.RPm = m.RPm;
        p.grid = (N + kMG - 1) / kMG, p.threads = kMThreads;
        if (fusion) return p;
        p.gt_patch_floats = (size_t)D;
    } else {
        const int RP = kBG * T;
        p.lds = sizeof(float) * ((size_t)4 * RP * kBS + 2 * (3 * Dims::C * Dims::C + Dims::C * Dims::C) + Dims::C + 3 * RP + kBG * Dims::PS);
        if (p.lds > Dims::NetLdsLimit) {  // long patches (the reference's W = 249): no room for the transposed kernel copies
            p.use_wt = 0;
            p.lds -= sizeof(float) * (3 * Dims::C * Dims::C + Dims::C * Dims::C);
        }
        p.route = p.lds <= Dims::NetLdsLimit ? kBwdScalar : kBwdRefused;
        p.grid = (N + kBG - 1) / kBG, p.threads = kBThreads;
        return p;
    }
    p.dtrunk = Grid3{D / 16, std::max(1, std::min(8, (N + 15) / 16 / 16)), 1};
    p.dwh = sw.dwh_valu ? kDwhValu : kDwhMfma;
    p.dwh_grid = sw.dwh_valu ? Grid3{(D * Dims::Hidden + 255) / 256, (N + kDwhSlice - 1) / kDwhSlice, 1 + n_heads}
                             : Grid3{(D / 16 + 3) / 4, 1 + n_heads, kDwhSplit};
    return p;
}

// ---- the step -------------------------------------------------------------------------------------------------------------------
// the training forward: launch_forward (f32), launch_forward_bf16_train (dtype 1), or the fusion model's two trunk-only f32 forwards
enum TrainForward { kTrainForwardF32 = 0, kTrainForwardBf16 = 1, kTrainForwardTrunkPair = 2 };
struct TrainShape {  // what of a model the plan depends on
    int heads, T, n_blocks, n_classes, n_heads, out_dim;
};
struct TrainPlan {
    TrainForward forward;
    HeadsPlan heads;
    BackwardPlan backward;
};
inline TrainPlan plan_train(const TrainShape &s, int N, int dtype, const TrainSwitches &sw) {
    const bool fusion = s.heads == SMH_HEADS_FUSION;
    TrainPlan p;
    p.forward = fusion ? kTrainForwardTrunkPair : dtype == 1 ? kTrainForwardBf16 : kTrainForwardF32;
    p.heads = plan_heads(s.heads, s.n_classes, s.n_heads, s.out_dim, N, sw);
    p.backward = plan_backward(s.T, s.n_blocks, s.n_heads, N, dtype, fusion, sw);
    return p;
}

// smh_internal_train_plan's answer, as ints in this order
enum TrainPlanInts {
    kTpForward, kTpHeadsFamily, kTpHeads0Staged, kTpHeads0Threads, kTpHeads0Grid, kTpHeads0Lds, kTpHeads1Staged, kTpHeads1Threads,
    kTpHeads1Grid, kTpHeads1Lds, kTpRoute, kTpGrid, kTpThreads, kTpLds, kTpG, kTpK32, kTpRPm, kTpUseWt, kTpActsLastOnly, kTpDtrunkX,
    kTpDtrunkY, kTpDwh, kTpDwhX, kTpDwhY, kTpDwhZ, kTpGtPatchFloats, kTpPackBytes, kTrainPlanInts
};
inline void train_plan_ints(const TrainPlan &p, int *out) {
    const HeadsLaunch *k = p.heads.k;
    const BackwardPlan &b = p.backward;
    const int v[kTrainPlanInts] = {p.forward, p.heads.family, k[0].staged, k[0].threads, k[0].grid, (int)k[0].lds, k[1].staged,
                                   k[1].threads, k[1].grid, (int)k[1].lds, b.route, b.grid, b.threads, (int)b.lds, b.geo.G,
                                   b.geo.K32, b.RPm, b.use_wt, b.acts_last_only, b.dtrunk.x, b.dtrunk.y, b.dwh,
                                   b.dwh_grid.x, b.dwh_grid.y, b.dwh_grid.z, (int)b.gt_patch_floats, (int)b.pack_bytes};
    std::copy(v, v + kTrainPlanInts, out);
}

}  // namespace smh_tcn
