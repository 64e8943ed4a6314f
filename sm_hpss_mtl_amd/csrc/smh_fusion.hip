// The intermediate-fusion MTL model (get_Lemaire_MTL_intermediate_fusion_model, lib/proposed_architectures.py:327-420): the layers
// behind its two TCN trunks.
//
//   x = BatchNormalization(concat[Flatten(trunk H), Flatten(trunk P)])      D = 2 W 32 features, H first, k = t * 32 + c per half
//   '3C' = softmax(Dense(n_classes)(x)),  heads = MTL_modifications(x)       (B3_MTL's heads on the fused vector)
//
// The trunks themselves run in the B3_MTL kernels (smh_tcn.hip forward with TcnArgs::trunk_only, smh_train.hip backward fed with
// d loss / d trunk output); this file holds what is new:
//   fusion_dense_kernel      the Dense layers on the fused features on the matrix cores (v_mfma_f32_16x16x4f32), the BatchNorm applied
//                            to the operand as it is loaded -- inference: moving statistics on the trunk taps, then the heads' tail of
//                            smh_tcn_heads.h; training: the normalised features xhat, `pre` out for the heads-training kernel
//   fusion_bn_*              batch statistics of the fused features (training), xhat
//   fusion_dwh_kernel        d loss / d Dense kernels over the fused features
//   fusion_dx_kernel         d loss / d x = dpre . Wh^T, with the per-slice sums the BatchNorm backward needs
//   fusion_bn_bwd_*          dgamma, dbeta and d loss / d (trunk output before its final relu) of both trunks
// No kernel here combines partial results with atomics: every sum runs in a fixed order, so a step is bit-reproducible.
// The BatchNorm is not folded into the Dense weights: the layers round where Keras rounds them.
#include "smh_model.h"
#include "smh_tcn_heads.h"

using namespace smh_tcn;

namespace {

constexpr int kFWaves = 16;      // waves of fusion_dense_kernel (they split the fused features)
constexpr int kMaxMt = kPS / 16;  // column tiles of the Dense-on-features outputs (3C + heads <= 80)

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// One workgroup = 16 patches (one MFMA row tile) x every output column; its 16 waves take the fused features in 16-wide chunks
// (chunk c goes to wave c % 16) and meet in LDS, summed in wave order.  Per chunk a lane loads four consecutive features of its patch
// (row = lane & 15, features k0 + 4 (lane >> 4) .. + 3) and the same four rows of the packed Dense kernel (WhA: [k / 4][ld][4]), so the
// four product steps u = 0..3 cover k0 + 4 q + u for q = 0..3 on both operands.
// TRAIN = false: A = BN(trunk tap) with the moving statistics, out = the heads' outputs.  TRAIN = true: A = xhat * gamma + beta
// (xhat: the batch-normalised features, (N, D)), out = pre (N, kPS) including the biases, for heads_train_kernel.
template <bool TRAIN>
__global__ void __launch_bounds__(64 * kFWaves) fusion_dense_kernel(TcnArgs ta, int N, int D, const float *__restrict__ xh,
                                                                 const float *__restrict__ xp, const float *__restrict__ bn,
                                                                 const float *__restrict__ WhA, const float *__restrict__ hp,
                                                                 float *__restrict__ out) {
    extern __shared__ float part[];  // [kFWaves][16][kPS], then pre[16][kPS]
    float *pre = part + (size_t)kFWaves * 16 * kPS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * 16, g_here = min(16, N - n0);
    const int half = D / 2, ld = 64 * ((ta.NH + 63) / 64), n_mt = (ta.NH + 15) / 16;
    const int nr = min(n0 + i, N - 1);  // rows past the batch repeat its last patch (their results are never stored)
    const float *gam = bn, *bet = bn + D, *mmean = bn + 2 * D, *mvar = bn + 3 * D;
    f32x4 acc[kMaxMt];
#pragma unroll
    for (int mt = 0; mt < kMaxMt; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = wave; c < D / 16; c += kFWaves) {
        const int k = c * 16 + 4 * q;
        f32x4 av;
        const f32x4 g = *reinterpret_cast<const f32x4 *>(gam + k), b = *reinterpret_cast<const f32x4 *>(bet + k);
        if constexpr (TRAIN) {
            const f32x4 xv = *reinterpret_cast<const f32x4 *>(xh + (size_t)nr * D + k);
#pragma unroll
            for (int u = 0; u < 4; ++u) av[u] = xv[u] * g[u] + b[u];
        } else {
            const float *src = k < half ? xh + (size_t)nr * half + k : xp + (size_t)nr * half + (k - half);
            const f32x4 xv = *reinterpret_cast<const f32x4 *>(src);
            const f32x4 mm = *reinterpret_cast<const f32x4 *>(mmean + k), mv = *reinterpret_cast<const f32x4 *>(mvar + k);
#pragma unroll
            for (int u = 0; u < 4; ++u) av[u] = (xv[u] - mm[u]) / sqrtf(mv[u] + kBnEps) * g[u] + b[u];
        }
        const f32x4 *wrow = reinterpret_cast<const f32x4 *>(WhA) + (size_t)(c * 4 + q) * ld + i;
#pragma unroll
        for (int mt = 0; mt < kMaxMt; ++mt) {
            if (mt < n_mt) {  // (uniform)
                const f32x4 bv = wrow[16 * mt];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[mt] = mfma4(av[u], bv[u], acc[mt]);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < kMaxMt; ++mt)
        if (mt < n_mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[((size_t)wave * 16 + 4 * q + r) * kPS + 16 * mt + i] = acc[mt][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * kPS; e += blockDim.x) {
        const int o = e % kPS;
        float v = 0.f;
        if (o < 16 * n_mt)
            for (int w = 0; w < kFWaves; ++w) v += part[(size_t)w * 16 * kPS + e];
        pre[e] = v;
    }
    __syncthreads();
    const float *bh = WhA + (size_t)D * ld;
    if constexpr (TRAIN) {
        for (int e = threadIdx.x; e < g_here * kPS; e += blockDim.x) {
            const int o = e % kPS;
            out[(size_t)n0 * kPS + e] = o < ta.NH ? pre[e] + bh[o] : 0.f;
        }
    } else {
        heads_tail(ta, pre, bh, hp, out, n0, g_here);
    }
}

// ---- batch statistics of the fused features (training) ----
// Feature k of patch n: relu of the saved pre-relu trunk output, acts (N, n_blocks + 1, W, 32) slot n_blocks, of trunk H (k < D / 2)
// or P.  Partial sums of x and x^2 per slice of kFSlice patches in float64, then summed over the slices in order.
constexpr int kFSlice = 32;
struct FusedAct {
    const float *acts[2];
    int nslot, half;
    __device__ __forceinline__ float pre_relu(int n, int k) const {
        const int b = k >= half, kk = k - b * half;
        return acts[b][((size_t)n * nslot + nslot - 1) * half + kk];
    }
};

__global__ void __launch_bounds__(256) fusion_bn_part_kernel(FusedAct fa, int N, int D, double *__restrict__ part) {
    const int k = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (k >= D) return;
    double s1 = 0.0, s2 = 0.0;
    for (int n = s * kFSlice; n < min(N, (s + 1) * kFSlice); ++n) {
        const double x = fmaxf(fa.pre_relu(n, k), 0.f);
        s1 += x, s2 += x * x;
    }
    part[((size_t)s * D + k) * 2] = s1;
    part[((size_t)s * D + k) * 2 + 1] = s2;
}

// bnstat: [mean (D) | population variance (D)] (the trainer's bucket); vec: [1 / sqrt(var + eps) (D) | ...]
__global__ void __launch_bounds__(256) fusion_bn_final_kernel(int N, int D, int n_slices, const double *__restrict__ part,
                                                              float *__restrict__ bnstat, float *__restrict__ vec) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= D) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < n_slices; ++s) s1 += part[((size_t)s * D + k) * 2], s2 += part[((size_t)s * D + k) * 2 + 1];
    const double mean = s1 / N, var = fmax(s2 / N - mean * mean, 0.0);
    bnstat[k] = (float)mean;
    bnstat[D + k] = (float)var;
    vec[k] = 1.0f / sqrtf((float)var + kBnEps);
}

__global__ void __launch_bounds__(256) fusion_bn_apply_kernel(FusedAct fa, int N, int D, const float *__restrict__ bnstat,
                                                              const float *__restrict__ vec, float *__restrict__ xhat) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * D) return;
    const int n = (int)(e / D), k = (int)(e - (size_t)n * D);
    xhat[e] = (fmaxf(fa.pre_relu(n, k), 0.f) - bnstat[k]) * vec[k];
}

// ---- backward ----
struct FusionHeadOffs {
    size_t head[kMaxHeads];
};
// dW[k][o] = sum_n y[n][k] dpre[n][col0 + o], y = xhat * gamma + beta: one wave = 16 features x the columns of one group ('3C', or the
// Dense(16) of one head) over the whole batch, in patch order; stored, not accumulated (nothing else writes these gradients).
__global__ void __launch_bounds__(256) fusion_dwh_kernel(int N, int D, int n_classes, const float *__restrict__ xhat,
                                                         const float *__restrict__ bn, const float *__restrict__ dpre,
                                                         float *__restrict__ grad, size_t off_c3, FusionHeadOffs offs) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = lane & 15, q = lane >> 4;
    const int k0 = (blockIdx.x * 4 + wave) * 16;
    if (k0 >= D) return;
    const int grp = blockIdx.y;
    const int ocount = grp == 0 ? n_classes : kHidden, col0 = grp == 0 ? 0 : n_classes + (grp - 1) * kHidden;
    const bool col_ok = i < ocount;
    const float g = bn[k0 + i], b = bn[D + k0 + i];
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    for (int n = 0; n < N; n += 8) {
        float av[2], bv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int nn = n + 4 * u + q;
            const bool ok = nn < N;
            const int nc = ok ? nn : 0;
            av[u] = ok ? xhat[(size_t)nc * D + k0 + i] * g + b : 0.f;
            bv[u] = (ok && col_ok) ? dpre[(size_t)nc * kPS + col0 + i] : 0.f;
        }
        acc0 = mfma4(av[0], bv[0], acc0);
        acc1 = mfma4(av[1], bv[1], acc1);
    }
    acc0 += acc1;
    if (col_ok) {
        const size_t base = (grp == 0 ? off_c3 : offs.head[grp - 1]) + (size_t)(k0 + 4 * q) * ocount + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) grad[base + (size_t)r * ocount] = acc0[r];
    }
}

// dy[n][k] = sum_o dpre[n][o] Wh[k][o] (d loss / d BN output), and per slice of kFSlice patches the sums of dy and dy * xhat
__global__ void __launch_bounds__(256) fusion_dx_kernel(int N, int D, int NH, const float *__restrict__ WhA,
                                                        const float *__restrict__ dpre, const float *__restrict__ xhat,
                                                        float *__restrict__ dy, double *__restrict__ part) {
    __shared__ float dp[kFSlice * kPS];
    const int k = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    const int nlo = s * kFSlice, nn = min(N, nlo + kFSlice) - nlo;
    for (int e = threadIdx.x; e < nn * kPS; e += 256) dp[e] = dpre[(size_t)nlo * kPS + e];
    __syncthreads();
    if (k >= D) return;
    const int ld = 64 * ((NH + 63) / 64);
    const float *w = WhA + (size_t)(k / 4) * ld * 4 + (k % 4);
    float acc[kFSlice];
#pragma unroll
    for (int r = 0; r < kFSlice; ++r) acc[r] = 0.f;
    for (int o = 0; o < NH; ++o) {
        const float wv = w[(size_t)o * 4];
#pragma unroll
        for (int r = 0; r < kFSlice; ++r) acc[r] = fmaf(dp[r * kPS + o], wv, acc[r]);
    }
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = 0; r < kFSlice; ++r)
        if (r < nn) {
            const size_t e = (size_t)(nlo + r) * D + k;
            dy[e] = acc[r];
            s1 += acc[r];
            s2 += (double)acc[r] * xhat[e];
        }
    part[((size_t)s * D + k) * 2] = s1;
    part[((size_t)s * D + k) * 2 + 1] = s2;
}

// dbeta = sum dy, dgamma = sum dy * xhat (stored into the gradient); vec[D ..]: mean(dy), vec[2 D ..]: mean(dy * xhat)
__global__ void __launch_bounds__(256) fusion_bn_bwd_final_kernel(int N, int D, int n_slices, const double *__restrict__ part,
                                                                  float *__restrict__ grad, size_t off_bn, float *__restrict__ vec) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= D) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < n_slices; ++s) s1 += part[((size_t)s * D + k) * 2], s2 += part[((size_t)s * D + k) * 2 + 1];
    grad[off_bn + k] = (float)s2;       // gamma
    grad[off_bn + D + k] = (float)s1;   // beta
    vec[D + k] = (float)(s1 / N);
    vec[2 * D + k] = (float)(s2 / N);
}

// d loss / d (trunk output before its final relu): dx = gamma / sqrt(var + eps) (dy - mean(dy) - xhat mean(dy xhat)), gated by the
// relu; gt: (2, N, W * 32) -- trunk H, then trunk P, each in the (N, T, 32) order the trunk backward reads
__global__ void __launch_bounds__(256) fusion_bn_bwd_apply_kernel(FusedAct fa, int N, int D, const float *__restrict__ bn,
                                                                  const float *__restrict__ vec, const float *__restrict__ dy,
                                                                  const float *__restrict__ xhat, float *__restrict__ gt) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * D) return;
    const int n = (int)(e / D), k = (int)(e - (size_t)n * D);
    const int b = k >= fa.half, kk = k - b * fa.half;
    const float g = bn[k] * vec[k] * (dy[e] - vec[D + k] - xhat[e] * vec[2 * D + k]);
    gt[((size_t)b * N + n) * fa.half + kk] = fa.pre_relu(n, k) > 0.f ? g : 0.f;
}

}  // namespace

namespace smh_tcn {

void fusion_tail_args(const smh_model *m, TcnArgs *a) {
    *a = TcnArgs{};
    a->D = m->D, a->NH = m->NH, a->n_mt = m->n_mt, a->n_classes = m->cfg.n_classes, a->n_heads = m->n_heads, a->out_dim = m->out_dim;
    for (int i = 0; i < kMaxHeads; ++i) a->head_odim[i] = m->head_odim[i], a->head_sigmoid[i] = m->head_sigmoid[i];
    a->cascade = 0;
}

static size_t dense_lds() { return sizeof(float) * (size_t)(kFWaves + 1) * 16 * kPS; }

int launch_fusion_dense(const smh_model *m, int N, const float *xh, const float *xp, float *out, bool train, hipStream_t st) {
    TcnArgs a;
    fusion_tail_args(m, &a);
    SMH_REQUIRE(m->NH <= kPS && (m->D % 64) == 0, "fusion: %d outputs / %d features outside the tail's tiling", m->NH, m->D);
    const float *bn = m->d_flat + offsets(m).fbn;
    const dim3 grid((N + 15) / 16), block(64 * kFWaves);
    if (train) {
        SMH_CHECK_HIP(hipFuncSetAttribute((const void *)fusion_dense_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dense_lds()));
        hipLaunchKernelGGL(fusion_dense_kernel<true>, grid, block, dense_lds(), st, a, N, m->D, xh, xp, bn, m->d_WhA, m->d_hp, out);
    } else {
        SMH_CHECK_HIP(hipFuncSetAttribute((const void *)fusion_dense_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dense_lds()));
        hipLaunchKernelGGL(fusion_dense_kernel<false>, grid, block, dense_lds(), st, a, N, m->D, xh, xp, bn, m->d_WhA, m->d_hp, out);
    }
    return smh::launch_status("fusion_dense_kernel");
}

size_t fusion_scratch_floats(const smh_model *m, int max_batch) {
    const size_t D = m->D, slices = (size_t)(max_batch + kFSlice - 1) / kFSlice;
    // xhat (N, D) | dy (N, D) | gt (2, N, D / 2) | vec (3 D) | partial sums (slices, D, 2) as doubles
    return 3 * (size_t)max_batch * D + 3 * D + 2 * (2 * slices * D);
}

int launch_fusion_train(const smh_model *m, int N, int max_batch, const float *acts_h, const float *acts_p, float *scratch,
                        float *bnstat, float *pd, float *grad, int phase, hipStream_t st) {
    const float *dpre = pd;
    const int D = m->D, half = D / 2;
    const Offsets off = offsets(m);
    const float *bn = m->d_flat + off.fbn;
    float *xhat = scratch, *dy = xhat + (size_t)max_batch * D, *gt = dy + (size_t)max_batch * D, *vec = gt + (size_t)max_batch * D;
    double *part = reinterpret_cast<double *>(vec + 3 * (size_t)D);  // (8-byte aligned: max_batch * D and D are even)
    FusedAct fa{{acts_h, acts_p}, m->n_blocks + 1, half};
    const int slices = (N + kFSlice - 1) / kFSlice;
    const dim3 gk((D + 255) / 256);
    const unsigned ge = (unsigned)(((size_t)N * D + 255) / 256);
    if (phase == 0) {  // forward: batch statistics, xhat, pre
        hipLaunchKernelGGL(fusion_bn_part_kernel, dim3(gk.x, slices), dim3(256), 0, st, fa, N, D, part);
        hipLaunchKernelGGL(fusion_bn_final_kernel, gk, dim3(256), 0, st, N, D, slices, (const double *)part, bnstat, vec);
        hipLaunchKernelGGL(fusion_bn_apply_kernel, dim3(ge), dim3(256), 0, st, fa, N, D, (const float *)bnstat, (const float *)vec, xhat);
        int rc = smh::launch_status("fusion_bn kernels");
        if (rc) return rc;
        return launch_fusion_dense(m, N, xhat, nullptr, pd, true, st);  // pd: the `pre` output of this phase
    }
    // backward: Dense kernels' gradient, dy, the BatchNorm backward, d loss / d trunk output (gt)
    FusionHeadOffs ho;
    for (int h = 0; h < kMaxHeads; ++h) ho.head[h] = off.head[h];
    hipLaunchKernelGGL(fusion_dwh_kernel, dim3((D / 16 + 3) / 4, 1 + m->n_heads), dim3(256), 0, st, N, D, m->cfg.n_classes,
                       (const float *)xhat, bn, dpre, grad, off.c3_k, ho);
    hipLaunchKernelGGL(fusion_dx_kernel, dim3(gk.x, slices), dim3(256), 0, st, N, D, m->NH, (const float *)m->d_WhA, dpre,
                       (const float *)xhat, dy, part);
    hipLaunchKernelGGL(fusion_bn_bwd_final_kernel, gk, dim3(256), 0, st, N, D, slices, (const double *)part, grad, off.fbn, vec);
    hipLaunchKernelGGL(fusion_bn_bwd_apply_kernel, dim3(ge), dim3(256), 0, st, fa, N, D, bn, (const float *)vec, (const float *)dy,
                       (const float *)xhat, gt);
    return smh::launch_status("fusion backward kernels");
}

const float *fusion_gt(const smh_model *m, int max_batch, const float *scratch, int N, int b) {
    return scratch + 2 * (size_t)max_batch * m->D + (size_t)b * N * (m->D / 2);
}

int launch_fusion_trunks(const smh_model *m, const float *xh, const float *xp, int N, float *tap_h, float *tap_p, ForwardOpts fo,
                         hipStream_t st) {
    fo.trunk_only = 1;
    const char *ev = getenv("SMH_FUSION_TWO_LAUNCH");
    if (ev && atoi(ev) != 0) {  // A/B runs and tests: one launch per trunk
        const int rc = launch_forward(m->trunk[0], xh, N, nullptr, tap_h, nullptr, st, fo);
        return rc ? rc : launch_forward(m->trunk[1], xp, N, nullptr, tap_p, nullptr, st, fo);
    }
    // one grid of (workgroups, 2): at the batch sizes of file-level inference with a hop above 1 and of the reference's own batches
    // (48 patches) one trunk fills 48 of 256 CUs.  Every workgroup does what it does in a launch of its own: same results
    fo.pair = m->trunk[1], fo.pair_x = xp, fo.pair_trunk = tap_p;
    return launch_forward(m->trunk[0], xh, N, nullptr, tap_h, nullptr, st, fo);
}

}  // namespace smh_tcn

extern "C" size_t smh_fusion_workspace_bytes(const smh_model *m, int N) {
    return (m && m->heads == SMH_HEADS_FUSION && N > 0) ? (size_t)N * m->D * sizeof(float) : 0;
}

extern "C" int smh_fusion_forward_f32(const smh_model *m, const float *d_xH, const float *d_xP, int N, float *d_out, void *d_work,
                                      size_t work_bytes, void *stream) {
    SMH_REQUIRE(m && d_xH && d_xP && d_out && d_work, "smh_fusion_forward_f32: null argument");
    SMH_REQUIRE(m->heads == SMH_HEADS_FUSION, "smh_fusion_forward_f32: the model is not an intermediate-fusion model");
    SMH_REQUIRE(N >= 0, "smh_fusion_forward_f32: N=%d", N);
    if (N == 0) return SMH_OK;
    SMH_REQUIRE(work_bytes >= smh_fusion_workspace_bytes(m, N), "smh_fusion_forward_f32: workspace of %zu bytes, %zu needed", work_bytes,
                smh_fusion_workspace_bytes(m, N));
    SMH_REQUIRE((reinterpret_cast<uintptr_t>(d_work) % 16) == 0, "smh_fusion_forward_f32: d_work must start on a 16-byte boundary");
    hipStream_t st = (hipStream_t)stream;
    float *tap[2] = {static_cast<float *>(d_work), static_cast<float *>(d_work) + (size_t)N * (m->D / 2)};
    const int rc = launch_fusion_trunks(m, d_xH, d_xP, N, tap[0], tap[1], ForwardOpts{}, st);
    if (rc) return rc;
    return launch_fusion_dense(m, N, tap[0], tap[1], d_out, false, st);
}

// ---- inference from the layer-0 partials: the fused pipeline from audio, and dense file-level inference ----
// The feature kernel (smh_features_l0_f32) and l0_frames_kernel write per featuregram half its share of a 1x1 convolution with
// rows [half * rows, + rows) of `w0`.  With w0 = smh_fusion_w0_ptr (trunk H's layer-0 kernel, then trunk P's) half 0 IS trunk H's
// complete layer 0 and half 1 trunk P's: the trunks read them in the x0_one mode, nothing is added up.
extern "C" const float *smh_fusion_w0_ptr(const smh_model *m) { return (m && m->heads == SMH_HEADS_FUSION) ? m->d_w0cat : nullptr; }

extern "C" size_t smh_fusion_x0_workspace_bytes(const smh_model *m, int N) { return smh_fusion_workspace_bytes(m, N); }

extern "C" int smh_fusion_forward_x0_f32(smh_model *m, const float *d_x0p, int N, void *d_work, size_t work_bytes, float *d_out,
                                         void *stream) {
    SMH_REQUIRE(m && d_x0p && d_out, "smh_fusion_forward_x0_f32: null argument");
    SMH_REQUIRE(m->heads == SMH_HEADS_FUSION, "smh_fusion_forward_x0_f32: the model is not an intermediate-fusion model; a B3_MTL or "
                "cascaded model takes smh_model_forward_x0_f32");
    SMH_REQUIRE(N >= 0, "smh_fusion_forward_x0_f32: N=%d", N);
    if (N == 0) return SMH_OK;
    SMH_REQUIRE(d_work, "smh_fusion_forward_x0_f32: null workspace");
    SMH_REQUIRE((reinterpret_cast<uintptr_t>(d_work) % 16) == 0 && (reinterpret_cast<uintptr_t>(d_x0p) % 16) == 0,
                "smh_fusion_forward_x0_f32: d_x0p and d_work are read / written with 16-byte accesses and must start on 16-byte boundaries");
    SMH_REQUIRE(work_bytes >= smh_fusion_x0_workspace_bytes(m, N), "smh_fusion_forward_x0_f32: workspace of %zu bytes, %zu needed",
                work_bytes, smh_fusion_x0_workspace_bytes(m, N));
    hipStream_t st = (hipStream_t)stream;
    const size_t half = (size_t)m->D / 2;  // W * 32: one trunk's tap per patch = one half of a patch's partials
    float *tap[2] = {static_cast<float *>(d_work), static_cast<float *>(d_work) + (size_t)N * half};
    ForwardOpts fo;
    fo.from_x0 = 1, fo.x0_one = 1;
    const int rc = launch_fusion_trunks(m, d_x0p, d_x0p + half, N, tap[0], tap[1], fo, st);
    if (rc) return rc;
    return launch_fusion_dense(m, N, tap[0], tap[1], d_out, false, st);
}

// Dense file-level inference: the patches go through the trunks and the tail in chunks of kFusionDenseChunk, so the workspace is
// [x0 (2, Tc, 32) | the two trunk taps of one chunk, (chunk, W, 32) each] whatever the length of the featuregram.
constexpr int kFusionDenseChunk = 2048;  // (a multiple of 16: every chunk but the last fills whole row tiles of fusion_dense_kernel)

extern "C" size_t smh_fusion_dense_workspace_bytes(const smh_model *m, int Tc, int shift) {
    if (!m || m->heads != SMH_HEADS_FUSION || Tc < m->cfg.patch_size || shift < 1) return 0;
    const int nP = smh_num_patches(Tc, m->cfg.patch_size, shift);
    const size_t chunk = (size_t)std::min(std::max(nP, 0), kFusionDenseChunk);
    return sizeof(float) * (2 * (size_t)Tc * C + chunk * m->D);
}

extern "C" int smh_fusion_forward_dense_f32(smh_model *m, const float *d_fv, int Tc, int shift, void *d_work, size_t work_bytes,
                                            float *d_out, void *stream) {
    int rc = dense_entry_ok("smh_fusion_forward_dense_f32", m, d_fv, Tc, shift, d_work, work_bytes, smh_fusion_dense_workspace_bytes(m, Tc, shift),
                            d_out, 4, "smh_fusion_forward_f32");
    if (rc) return rc;
    SMH_REQUIRE(m->heads == SMH_HEADS_FUSION, "smh_fusion_forward_dense_f32: the model is not an intermediate-fusion model; a B3_MTL or "
                "cascaded model takes smh_model_forward_dense_f32");
    const int W = m->cfg.patch_size, F = m->cfg.n_feat;
    const int nP = smh_num_patches(Tc, W, shift);
    if (nP <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float *x0 = static_cast<float *>(d_work);
    rc = launch_l0_frames(d_fv, m->d_w0cat, x0, F, Tc, st);
    if (rc) return rc;
    const size_t half = (size_t)m->D / 2;
    const int chunk = std::min(nP, kFusionDenseChunk);
    float *tap[2] = {x0 + 2 * (size_t)Tc * C, x0 + 2 * (size_t)Tc * C + (size_t)chunk * half};
    for (int p0 = 0; p0 < nP; p0 += chunk) {
        const int n = std::min(chunk, nP - p0);
        // patch p0 + i starts at min((p0 + i) shift, Tc - W): the window array advanced by p0 shift frames and shortened by as many
        // (p0 shift <= Tc - W: patch p0's centre lies inside the featuregram)
        const size_t adv = (size_t)p0 * shift;
        ForwardOpts fo;
        fo.from_x0 = 1, fo.x0_one = 1, fo.x0_shift = shift, fo.x0_T = Tc - (int)adv;
        rc = launch_fusion_trunks(m, x0 + adv * C, x0 + ((size_t)Tc + adv) * C, n, tap[0], tap[1], fo, st);
        if (rc) return rc;
        rc = launch_fusion_dense(m, n, tap[0], tap[1], d_out + (size_t)p0 * m->out_dim, false, st);
        if (rc) return rc;
    }
    return nP;
}
