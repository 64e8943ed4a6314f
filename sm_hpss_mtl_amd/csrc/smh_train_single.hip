// Head of one training step of the single-task Lemaire TCN baseline (SMH_HEADS_SINGLE; get_Lemaire_model,
// lib/baseline_architectures.py:196-300): Flatten -> Dense(n_classes) -> softmax behind B3_MTL's trunk.  From the logits the training
// forward of smh_tcn.hip leaves in `pre` (N, kPS; columns < n_classes, bias included):
//
//   p = softmax(logits)
//   n_classes == 2  loss = Keras binary_crossentropy on BOTH softmax outputs: pc = clip(p, 1e-7, 1 - 1e-7),
//                   -(y log(pc + 1e-7) + (1 - y) log(1 - pc + 1e-7)), mean over the two outputs, then over the batch;
//                   accuracy = binary accuracy, the mean over all N x 2 outputs of (p > 0.5) == y
//   n_classes 3, 5  loss = categorical cross-entropy -sum_c y_c log(clip(p_c)), accuracy = argmax p == argmax y
//
// The gradient with respect to the logits is the softmax Jacobian applied to d loss / d p of the CLIPPED expression (zero where the
// clip is active) -- dz_c = p_c (g_c - sum_k g_k p_k) --, not the p - y shortcut: for the two-output bce the two differ by the 1e-7
// terms and by the second output's own term.  It goes to `dpre` (the other kPS - n_classes columns zeroed), where the trunk
// backward, dtrunk_kernel and dwh_*_kernel (smh_train.hip, smh_train_bf16.hip) read it as they read the '3C' columns of the MTL
// models: with n_heads = 0 their head loops are empty and the Dense kernel's gradient and the gradient into the flattened trunk are
// the group-0 products they already compute.  The Dense bias gradient, the loss and the accuracy are batch sums: a wave sum (lanes
// = samples) into per-wave rows, totalled in wave order -- no atomics, so this head is bit-reproducible whatever
// smh_trainer_set_deterministic says.  One workgroup; batches beyond kTh samples take further passes over the same rows.
#include "smh_model.h"
#include "smh_train_plan.h"
#include "smh_wave.h"

using namespace smh_tcn;

namespace {

constexpr float kKerasEps = 1e-7f;
constexpr int kTh = 512;  // one sample per lane for the reference driver's batches (tests/single_task_plans.py restates the plan)
constexpr int kNW = kTh / 64;
constexpr int kMaxC = 5;
enum { A_DB = 0, A_LOSS = A_DB + kMaxC, A_HIT, kA };

__global__ void __launch_bounds__(kTh)
single_head_train_kernel(HeadsArgs a, const float *__restrict__ pre, const float *__restrict__ y, float *__restrict__ dpre,
                         float *__restrict__ grad, float *__restrict__ losses) {
    __shared__ float red[kNW][kA];
    const int tid = threadIdx.x, N = a.N, ncls = a.n_classes;
    float *row = red[tid >> 6];
    const bool bce = ncls == 2;
    const float scale = a.lw[0] / (float)N;
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        const int nc = on ? n : N - 1;
        const float *pr = pre + (size_t)nc * kPS, *yr = y + (size_t)nc * ncls;
        float p[kMaxC], t[kMaxC], g[kMaxC], mx = -INFINITY, den = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) {
            p[c] = c < ncls ? pr[c] : -INFINITY;
            t[c] = c < ncls ? yr[c] : 0.f;
            mx = fmaxf(mx, p[c]);
        }
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) den += (p[c] = c < ncls ? expf(p[c] - mx) : 0.f);
        float l = 0.f, hit = 0.f, gp = 0.f;
        int am = 0, at = 0;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) {
            p[c] /= den;
            g[c] = 0.f;
            if (c < ncls) {
                const float pc = fminf(fmaxf(p[c], kKerasEps), 1.0f - kKerasEps);
                const bool inside = p[c] > kKerasEps && p[c] < 1.0f - kKerasEps;  // the clip passes the gradient only inside
                if (bce) {
                    l -= 0.5f * (t[c] * logf(pc + kKerasEps) + (1.0f - t[c]) * logf(1.0f - pc + kKerasEps));
                    g[c] = inside ? -0.5f * (t[c] / (pc + kKerasEps) - (1.0f - t[c]) / (1.0f - pc + kKerasEps)) : 0.f;
                    hit += ((p[c] > 0.5f) == (t[c] > 0.5f)) ? 0.5f : 0.f;
                } else {
                    l -= t[c] * logf(pc);
                    g[c] = inside ? -t[c] / pc : 0.f;
                    if (p[c] > p[am]) am = c;
                    if (t[c] > t[at]) at = c;
                }
                gp = fmaf(g[c], p[c], gp);
            }
        }
        if (!bce) hit = am == at ? 1.0f : 0.f;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) {
            if (c < ncls) {  // (uniform)
                const float d = on ? p[c] * (g[c] - gp) * scale : 0.f;
                if (on) dpre[(size_t)n * kPS + c] = d;
                const float s = wave_sum_f(d);
                if ((tid & 63) == 0) row[A_DB + c] = n0 == 0 ? s : row[A_DB + c] + s;
            }
        }
        if (on)
            for (int c = ncls; c < kPS; ++c) dpre[(size_t)n * kPS + c] = 0.f;
        const float sl = wave_sum_f(on ? l : 0.f), sh = wave_sum_f(on ? hit : 0.f);
        if ((tid & 63) == 0) {
            row[A_LOSS] = n0 == 0 ? sl : row[A_LOSS] + sl;
            row[A_HIT] = n0 == 0 ? sh : row[A_HIT] + sh;
        }
    }
    __syncthreads();
    if (tid < kA) {  // every wave's row, in wave order
        float v = 0.f;
        for (int w = 0; w < kNW; ++w) v += red[w][tid];
        if (tid < ncls) grad[a.goff_c3b + tid] = v;
        if (tid == A_LOSS) {
            const float loss = v / (float)N;
            losses[0] = loss, losses[1] = a.lw[0] * loss;
            losses[3] = 0.f;  // no regularised kernel: the l2 slot of the MTL models' layout
        }
        if (tid == A_HIT) losses[2] = v / (float)N;
    }
}

}  // namespace

int smh_tcn::launch_single_head_train(const HeadsArgs &a, const float *pre, const float *y, float *dpre, float *grad, float *losses,
                                      hipStream_t st) {
    SMH_REQUIRE(a.n_heads == 0 && a.n_classes >= 2 && a.n_classes <= kMaxC && a.out_dim == a.n_classes,
                "single-task head: expected no heads and 2 .. %d classes", kMaxC);
    static_assert(kTh == kSmallHeadThreads, "smh_train_plan.h plans this kernel's workgroup");
    hipLaunchKernelGGL(single_head_train_kernel, dim3(1), dim3(kTh), 0, st, a, pre, y, dpre, grad, losses);
    return smh::launch_status("single_head_train_kernel");
}
