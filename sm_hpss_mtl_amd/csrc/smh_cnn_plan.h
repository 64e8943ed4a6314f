// Launch plans of the Conv2D models (smh_cnn.hip, smh_cnn_train.hip): every split-K, tile and block count of a
// conv_gemm_kernel / colred_kernel / wgrad_smallk_kernel launch is decided here, once, as a plain value.  The launchers
// (launch_conv_gemm, col_reduce), the workspace sizing (carve, smh_cnn_trainer_create) and the test query
// (smh_internal_cnn_plan) all take it from these functions.  Host arithmetic only, no HIP: a stand-alone host program can
// include this header by itself.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "../../include/smh.h"

namespace {

constexpr int BM = 128, BK = 16;  // conv_gemm_kernel: rows per tile, k per step
constexpr int BKB = 32;           // conv_gemm_bf16_kernel: k per step
constexpr int kChunk = 64;        // images per pass through the layer list (bounds the activation workspace)
constexpr int kMaxRed = 1024;     // row chunks of a column reduction
constexpr int kSmallK = 32;       // deepest weight gradient of wgrad_smallk_kernel

enum Op { kConv, kPool, kLrnRelu, kMelCl };
struct Layer {
    Op op;
    int H, W, C, OH, OW, OC;            // input / output image geometry (Dense: H = W = 1)
    int kh, kw, sh, sw, pt, pl, act;
    int t_kernel = -1, t_bias = -1, t_bn = -1;  // parameter table indices (bn = gamma; beta, mean, var follow)
    size_t es_off = 0;                   // folded scale/shift in d_fold
    int K = 0, Kp = 0;
    size_t lut_off = 0;
    size_t wbf_off = 0;                  // this layer's transposed bf16 kernel [OC][Kp] in d_wbf (bf16 elements)
    float drop = 0.f;                    // Dropout rate behind this layer's activation (training only)
    int l2 = 0;                          // kernel_regularizer=l2() on this layer's kernel (Jang)
};

// the single-task baselines (lib/baseline_architectures.py): the trunk, then Dense(n_classes) + softmax, no S / M / R heads
inline bool cnn_single(int kind) {
    return kind == SMH_CNN_DOUKHAN_SINGLE || kind == SMH_CNN_PAPAKOSTAS_SINGLE || kind == SMH_CNN_JANG_SINGLE;
}
// Images the split-K plan of a forward pass of n images is made for.  The single-task kinds plan every pass as a full one: the order
// in which a row's products are summed then depends on the layer alone, so a row has the same bits in any batch and in any pass.
// (The MTL kinds keep the plan that follows the pass, and with it their bits.)
inline int plan_images(int kind, int n) { return cnn_single(kind) ? kChunk : n; }

// plan switches of the training step (tests and A/B runs), read once per step
struct CnnSwitches {
    bool pool_gather = false;  // SMH_CNN_POOL_GATHER: gather form of every pooling backward
    bool wgrad_mfma = false;   // SMH_CNN_WGRAD_MFMA: no VALU small-K weight gradient
    int wsplit = 0, dsplit = 0;  // SMH_CNN_WSPLIT / SMH_CNN_DSPLIT: forced slice count of the weight / data gradient (>= 1; 0: not set)
};
inline CnnSwitches read_cnn_switches() {
    CnnSwitches s;
    s.pool_gather = getenv("SMH_CNN_POOL_GATHER") != nullptr;
    s.wgrad_mfma = getenv("SMH_CNN_WGRAD_MFMA") != nullptr;
    if (const char *e = getenv("SMH_CNN_WSPLIT")) s.wsplit = std::max(1, atoi(e));
    if (const char *e = getenv("SMH_CNN_DSPLIT")) s.dsplit = std::max(1, atoi(e));
    return s;
}

inline int choose_split(int mtiles, int ntiles, int ksteps) {
    int s = 1;
    const int blocks = mtiles * ntiles;
    if (blocks >= 1 && blocks < 256 && ksteps >= 32) {
        s = (512 + blocks - 1) / blocks;
        if (s > 16) s = 16;
        if (s > ksteps / 8) s = ksteps / 8;
        if (s < 1) s = 1;
    }
    return s;
}
// fewer slices until their ordered partials (out_floats each) fit the partial buffer
inline int cap_split(int s, size_t out_floats, size_t cap_floats) {
    while (s > 1 && (size_t)s * out_floats > cap_floats) --s;
    return s;
}
inline int wgrad_split(int blocks, int ksteps, size_t out_floats, size_t cap_floats) {
    int s = 1;
    if (blocks < 1024 && ksteps >= 32) {
        s = (1024 + blocks - 1) / blocks;
        if (s > ksteps / 16) s = ksteps / 16;
        if (s > 256) s = 256;
        s = cap_split(s, out_floats, cap_floats);
        if (s < 1) s = 1;
    }
    return s;
}

// One conv_gemm_kernel launch: grid (mt, nt, ksplit) of the <bn> instantiation; slice z runs k-steps [z, z + 1) * ksteps_per.
struct GemmPlan {
    int bn, mt, nt;
    int ksteps, ksplit, ksteps_per;
    size_t partial_floats;  // ksplit * rows * cols of ordered partials; 0 when ksplit == 1
};
inline int col_tile(int cols) { return cols <= 64 ? 64 : 128; }
inline GemmPlan gemm_plan(int rows, int cols, int ksteps, int ksplit) {
    GemmPlan p{};
    p.bn = col_tile(cols);
    p.mt = (rows + BM - 1) / BM, p.nt = (cols + p.bn - 1) / p.bn;
    p.ksteps = ksteps, p.ksplit = ksplit, p.ksteps_per = (ksteps + ksplit - 1) / ksplit;
    p.partial_floats = ksplit > 1 ? (size_t)ksplit * rows * cols : 0;
    return p;
}

// Inference forward of one pass of n images.  The split is chosen on the f32 k-steps for both precisions (one workspace size), and on
// the rows of plan_images; the grid covers the n images that are there.
static_assert(BKB <= 8 * BK, "choose_split returns at most (Kp / BK) / 8 slices: no more than the bf16 kernel's Kp / BKB k-steps");
inline GemmPlan plan_forward(int kind, const Layer &L, int n, bool bf16) {
    const int rows_plan = plan_images(kind, n) * L.OH * L.OW;
    const int s = choose_split((rows_plan + BM - 1) / BM, (L.OC + col_tile(L.OC) - 1) / col_tile(L.OC), L.Kp / BK);
    return gemm_plan(n * L.OH * L.OW, L.OC, L.Kp / (bf16 ? BKB : BK), s);
}
// floats of split partials a forward of N images needs: the passes of kChunk images and the ragged last one, which may split K differently
inline size_t forward_partial_floats(int kind, const std::vector<Layer> &layers, int N) {
    const int full = N < 1 ? 1 : std::min(N, kChunk), last = N > kChunk ? N % kChunk : 0;
    size_t part = 0;
    for (int n : {full, last})
        for (const Layer &L : layers)
            if (n && L.op == kConv) part = std::max(part, plan_forward(kind, L, n, false).partial_floats);
    return part;
}

// Training forward of N images; cap_floats = the trainer's partial buffer.
inline GemmPlan plan_train_forward(const Layer &L, int N, size_t cap_floats) {
    const int rows = N * L.OH * L.OW, ksteps = L.Kp / BK;
    const GemmPlan g = gemm_plan(rows, L.OC, ksteps, 1);
    return gemm_plan(rows, L.OC, ksteps, cap_split(choose_split(g.mt, g.nt, ksteps), (size_t)rows * L.OC, cap_floats));
}

// Weight gradient dW[K x OC], reduction over the M = N * OH * OW output pixels.  Shallow layers (K <= kSmallK) take wgrad_smallk_kernel
// on a grid of (nb, ceil(OC / 64)) with rows_per_block pixels per block and nb ordered partials; the others the MODE-1 GEMM.
struct WgradPlan {
    bool smallk;
    GemmPlan gemm;           // !smallk: the MODE-1 GEMM
    int nb, rows_per_block;  // smallk: the block plan of wgrad_smallk_kernel
    size_t partial_floats;   // either way: floats of ordered partials (smallk: nb * K * OC, summed even when nb == 1)
};
inline WgradPlan plan_wgrad(const Layer &L, int N, size_t cap_floats, const CnnSwitches &sw) {
    const int M = N * L.OH * L.OW;
    const size_t outf = (size_t)L.K * L.OC;
    WgradPlan p{};
    if (L.K <= kSmallK && !sw.wgrad_mfma) {
        p.smallk = true;
        p.nb = cap_split(std::max(1, std::min(1024, M / 512)), outf, cap_floats);
        p.rows_per_block = ((M + p.nb - 1) / p.nb + 63) / 64 * 64;
        p.nb = (M + p.rows_per_block - 1) / p.rows_per_block;
        p.partial_floats = (size_t)p.nb * outf;
        return p;
    }
    const int ksteps = (M + BK - 1) / BK;
    const GemmPlan g = gemm_plan(L.K, L.OC, ksteps, 1);
    int s = wgrad_split(g.mt * g.nt, ksteps, outf, cap_floats);
    if (sw.wsplit) s = std::min(sw.wsplit, ksteps);
    s = cap_split(s, outf, cap_floats);  // a forced split too
    const int per = (ksteps + s - 1) / s;
    p.gemm = gemm_plan(L.K, L.OC, ksteps, (ksteps + per - 1) / per);  // no empty slices
    p.partial_floats = p.gemm.partial_floats;
    return p;
}

// Data gradient of a layer behind the first: dZ (zero-stuffed when strided) is the image, depth kh * kw * OC, columns = Cin padded to
// a multiple of 4.  A forced split is capped like the automatic one; empty slices stay (they write zeros to their partial block).
inline int dgrad_cols(const Layer &L) { return (L.C + 3) & ~3; }  // Jang conv1: 3 -> 4
inline GemmPlan plan_dgrad(const Layer &L, int N, size_t cap_floats, const CnnSwitches &sw) {
    const int ldc = dgrad_cols(L), rows = N * L.H * L.W, ksteps = (L.kh * L.kw * L.OC + BK - 1) / BK;
    const GemmPlan g = gemm_plan(rows, ldc, ksteps, 1);
    int s = choose_split(g.mt, g.nt, ksteps);
    if (sw.dsplit) s = std::min(sw.dsplit, ksteps);
    return gemm_plan(rows, ldc, ksteps, cap_split(s, (size_t)rows * ldc, cap_floats));
}

// Column sums of a row-major (M x C) matrix: colred_kernel on a grid of (blocks, slabs), rows_per_block rows each.
struct ColReducePlan {
    bool vec;  // four channels per thread: the kernel's own test
    unsigned slabs;
    size_t rows_per_pass, rows_per_block, blocks;
};
inline ColReducePlan plan_col_reduce(size_t M, int C) {
    ColReducePlan p{};
    const int cq = C >> 2;
    p.vec = (C & 3) == 0 && ((cq <= 256 && 256 % cq == 0) || cq % 256 == 0);
    p.rows_per_pass = p.vec ? (cq < 256 ? 256 / cq : 1) : 1;
    p.slabs = p.vec && cq > 256 ? cq / 256 : 1;
    p.rows_per_block = p.vec ? p.rows_per_pass * 16 : 64;
    p.blocks = (M + p.rows_per_block - 1) / p.rows_per_block;
    if (p.blocks > kMaxRed) {
        p.rows_per_block = (M + kMaxRed - 1) / kMaxRed;
        p.rows_per_block = (p.rows_per_block + p.rows_per_pass - 1) / p.rows_per_pass * p.rows_per_pass;
        p.blocks = (M + p.rows_per_block - 1) / p.rows_per_block;
    }
    return p;
}

// the trainer's partial buffer: 192 MB of split partials, or the forward split-K partials of the GEMMs at full batch if they need more
inline size_t trainer_partial_floats(const std::vector<Layer> &layers, int max_batch) {
    size_t p = (size_t)48 << 20;
    for (const Layer &L : layers)
        if (L.op == kConv) {
            const size_t M = (size_t)max_batch * L.OH * L.OW;
            p = std::max(p, (size_t)16 * std::min<size_t>(M, 4096) * L.OC);
        }
    return p;
}

}  // namespace
