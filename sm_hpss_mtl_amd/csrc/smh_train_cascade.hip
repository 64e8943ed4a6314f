// Heads of one training step of the cascaded MTL model (get_Lemaire_Cascaded_MTL_model, lib/proposed_architectures.py:175-323):
// batch-statistics BatchNorms, Dropout, the four losses and d loss / d pre from the Dense-on-trunk outputs `pre` (N, kPS) =
// [3C logits | Dense(16) of S | of M | of R] that the training forward of smh_tcn.hip leaves.  The trunk backward kernels of
// smh_train.hip consume `dpre` exactly as they do for B3_MTL.
//
//   R:  r = Dense(2)(Dropout(relu(BN16(u_R))))
//   S:  z = concat[Dropout(relu(BN16(u_S))), r] (18);  s = sigmoid(Dense(1)(BN18(z)))   (M likewise, own weights)
//   3C: softmax(logits)
//
// In training BN18 normalises with the batch statistics of z, so d loss_S / d r (through BN18) flows into R's head on top of
// R's own MSE.  Two launches:
//   cascade_sm_kernel  (3 workgroups: S, M, 3C) -- S and M each recompute R's forward from `pre` (the same code on the same
//                      values: bit-identical r), run their own forward / backward and leave d loss / d r in `dr` (N x 2 each);
//   cascade_r_kernel   (1 workgroup: R) -- R's forward again, d loss / d r = its MSE term + both `dr`, R's backward, and the
//                      weighted total of the losses.
// Every sum over the batch is a wave sum (lanes = samples) added into per-wave rows that are totalled in wave order: no
// atomics, so the heads are bit-reproducible whatever smh_trainer_set_deterministic says.
#include "smh_model.h"
#include "smh_train_plan.h"
#include "smh_wave.h"

using namespace smh_tcn;

namespace {

constexpr float kKerasEps = 1e-7f;
constexpr int kTh = 512;  // threads per workgroup: one sample per lane for the reference driver's batches
constexpr int kNW = kTh / 64;
// accumulator slots (per wave, then totals)
enum { A_Z = 0, A_ZV = A_Z + kCat, A_DWO = A_ZV + kCat, A_DG2 = A_DWO + 2 * kHidden, A_DB2 = A_DG2 + kCat, A_DG = A_DB2 + kCat,
       A_DB = A_DG + kHidden, A_DBIAS = A_DB + kHidden, A_DBO = A_DBIAS + kHidden, A_LOSS = A_DBO + 2, A_ACC = A_LOSS + 1,
       A_C3 = A_ACC + 1, A_C3L = A_C3 + 8, A_C3A = A_C3L + 1, kA = A_C3A + 1 };

__device__ __forceinline__ void wave_add(float *row, int q, float v, bool first) {
    v = wave_sum_f(v);
    if ((threadIdx.x & 63) == 0) row[q] = first ? v : row[q] + v;
}

// every wave's row -> tot, in wave order; called by all threads
__device__ __forceinline__ void totals(float (*red)[kA], float *tot) {
    __syncthreads();
    for (int q = threadIdx.x; q < kA; q += blockDim.x) {
        float v = 0.f;
        for (int w = 0; w < kNW; ++w) v += red[w][q];
        tot[q] = v;
    }
    __syncthreads();
}

// batch mean / population variance of n_units columns, 16 lanes per unit (the order of heads_train_kernel's phase A)
template <typename PF>
__device__ __forceinline__ void batch_stats(int N, int n_units, PF P, float *s_mean, float *s_var, float *s_inv) {
    const int tid = threadIdx.x;
    for (int u0 = 0; u0 < n_units; u0 += kTh >> 4) {
        const int u = u0 + (tid >> 4), sub = tid & 15;
        const bool on = u < n_units;
        float s = 0.f;
        if (on)
            for (int n = sub; n < N; n += 16) s += P(n, u);
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s / (float)N;
        float q = 0.f;
        if (on)
            for (int n = sub; n < N; n += 16) {
                const float d = P(n, u) - mean;
                q += d * d;
            }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
        if (on && sub == 0) {
            const float var = q / (float)N;
            s_mean[u] = mean, s_var[u] = var, s_inv[u] = 1.0f / sqrtf(var + kBnEps);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void load_mask(const float *drop, int n, int h, float dm[kHidden]) {
    if (drop) {
        const float4 *dp = reinterpret_cast<const float4 *>(drop + ((size_t)n * 3 + h) * kHidden);
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            const float4 v = dp[i4];
            dm[4 * i4] = v.x, dm[4 * i4 + 1] = v.y, dm[4 * i4 + 2] = v.z, dm[4 * i4 + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kHidden; ++i) dm[i] = 1.0f;
    }
}

// training-mode Dense(16) -> BN -> relu -> Dropout of one sample; for R also its Dense(2) (wo != nullptr).  Shared by both kernels:
// S, M and R compute r with the same instructions on the same values.
__device__ __forceinline__ void hidden_fwd(const float u[kHidden], const float *mean, const float *inv, const float *gamma,
                                           const float *beta, const float dm[kHidden], float xh[kHidden], float bn[kHidden],
                                           float ad[kHidden]) {
#pragma unroll
    for (int i = 0; i < kHidden; ++i) {
        xh[i] = (u[i] - mean[i]) * inv[i];
        bn[i] = xh[i] * gamma[i] + beta[i];
        ad[i] = fmaxf(bn[i], 0.f) * dm[i];
    }
}
__device__ __forceinline__ void r_out(const float ad[kHidden], const float *wo, float r[2]) {
    r[0] = wo[2 * kHidden], r[1] = wo[2 * kHidden + 1];  // out bias behind the (16, 2) kernel
#pragma unroll
    for (int i = 0; i < kHidden; ++i) {
        r[0] = fmaf(ad[i], wo[2 * i], r[0]);
        r[1] = fmaf(ad[i], wo[2 * i + 1], r[1]);
    }
}

// Keras binary cross-entropy of one sigmoid output (heads_train_kernel's arithmetic): loss, hit, d loss / d logit (before lw)
__device__ __forceinline__ void bce(float zo, float t, int N, float &lsum, float &hit, float &dzo) {
    const float o = 1.0f / (1.0f + expf(-zo));
    hit = ((o > 0.5f) == (t > 0.5f)) ? 1.0f : 0.f;
    const float oc = fminf(fmaxf(o, kKerasEps), 1.0f - kKerasEps);
    lsum = -(t * logf(oc + kKerasEps) + (1.0f - t) * logf(1.0f - oc + kKerasEps));
    const bool inside = (o > kKerasEps) && (o < 1.0f - kKerasEps);
    const float doc = -(t / (oc + kKerasEps) - (1.0f - t) / (1.0f - oc + kKerasEps)) / (float)N;
    dzo = inside ? doc * o * (1.0f - o) : 0.f;
}

// blockIdx.x 0 / 1: head S / M; 2: the '3C' softmax
template <bool STAGED>
__global__ void __launch_bounds__(kTh)
cascade_sm_kernel(HeadsArgs a, const float *__restrict__ pre, const float *__restrict__ y, const float *__restrict__ hp,
                  const float *__restrict__ drop, float *__restrict__ dpre, float *__restrict__ dxh, float *__restrict__ dr,
                  float *__restrict__ grad, float *__restrict__ bnstat, float *__restrict__ losses) {
    extern __shared__ __attribute__((aligned(16))) float stage[];
    __shared__ float s_mean[2 * kHidden], s_var[2 * kHidden], s_inv[2 * kHidden];
    __shared__ float c_mean[kCat], c_var[kCat], c_inv[kCat];
    __shared__ float red[kNW][kA], tot[kA];
    const int tid = threadIdx.x, N = a.N, ncls = a.n_classes, nh = a.n_heads;
    float *row = red[tid >> 6];
    const int h = blockIdx.x;
    if (h == 2) {  // '3C': softmax + categorical cross-entropy, d loss / d logits, the zero padding columns of dpre
        for (int n0 = 0; n0 < N; n0 += kTh) {
            const int n = n0 + tid;
            const bool on = n < N;
            const int nc = on ? n : N - 1;
            const float *pr = pre + (size_t)nc * kPS;
            float mx = -INFINITY, p[8], t[8];
            for (int c = 0; c < ncls; ++c) mx = fmaxf(mx, pr[c]);
            float den = 0.f;
            for (int c = 0; c < ncls; ++c) den += (p[c] = expf(pr[c] - mx));
            int am = 0, at = 0;
            float l = 0.f;
            for (int c = 0; c < ncls; ++c) {
                p[c] /= den;
                t[c] = y[(size_t)nc * a.out_dim + (a.out_dim - ncls) + c];
                l -= t[c] * logf(fminf(fmaxf(p[c], kKerasEps), 1.0f - kKerasEps));
                if (p[c] > p[am]) am = c;
                if (t[c] > t[at]) at = c;
            }
            for (int c = 0; c < ncls; ++c) {
                const float d = on ? (p[c] - t[c]) / (float)N * a.lw[nh] : 0.f;
                if (on) dpre[(size_t)n * kPS + c] = d;
                wave_add(row, A_C3 + c, d, n0 == 0);
            }
            if (on)
                for (int c = ncls + nh * kHidden; c < kPS; ++c) dpre[(size_t)n * kPS + c] = 0.f;
            wave_add(row, A_C3L, on ? l / (float)N : 0.f, n0 == 0);
            wave_add(row, A_C3A, (on && am == at) ? 1.0f / (float)N : 0.f, n0 == 0);
        }
        totals(red, tot);
        if (tid < ncls) grad[a.goff_c3b + tid] = tot[A_C3 + tid];
        if (tid == 0) losses[nh] = tot[A_C3L], losses[nh + 2] = tot[A_C3A];
        return;
    }
    // local column c < 16: this head's Dense(16); 16 <= c < 32: R's
    constexpr int PST = 2 * kHidden + 1;
    auto gcol = [&](int c) { return ncls + (c < kHidden ? h * kHidden + c : 2 * kHidden + (c - kHidden)); };
    float *tile = stage, *ty = stage + (size_t)(STAGED ? N : 0) * PST;
    auto P = [&](int n, int c) -> float { return STAGED ? tile[n * PST + c] : pre[(size_t)n * kPS + gcol(c)]; };
    auto Y = [&](int n) -> float { return STAGED ? ty[n] : y[(size_t)n * a.out_dim + h]; };
    if constexpr (STAGED) {
        for (int i = tid; i < N * 2 * kHidden; i += kTh) {
            const int n = i / (2 * kHidden), c = i - n * 2 * kHidden;
            tile[n * PST + c] = pre[(size_t)n * kPS + gcol(c)];
        }
        for (int i = tid; i < N; i += kTh) ty[i] = y[(size_t)i * a.out_dim + h];
        __syncthreads();
    }
    batch_stats(N, 2 * kHidden, P, s_mean, s_var, s_inv);
    const float *ph = hp + a.hp_off[h], *pR = hp + a.hp_off[2];
    const float *gamma = ph, *beta = ph + 16;
    const float *cg = ph + 64, *cb = cg + kCat, *wo = cb + 3 * kCat, bo = wo[kCat];
    // forward of one sample up to the concatenation z (18)
    auto fwd = [&](int nc, float z[kCat], float xs[kHidden], float bs[kHidden], float dms[kHidden]) {
        float u[kHidden], uR[kHidden], dmR[kHidden], xr[kHidden], br[kHidden], ar[kHidden], r[2];
#pragma unroll
        for (int i = 0; i < kHidden; ++i) u[i] = P(nc, i), uR[i] = P(nc, kHidden + i);
        load_mask(drop, nc, 2, dmR);
        hidden_fwd(uR, s_mean + kHidden, s_inv + kHidden, pR, pR + 16, dmR, xr, br, ar);
        r_out(ar, pR + 64, r);
        load_mask(drop, nc, h, dms);
        hidden_fwd(u, s_mean, s_inv, gamma, beta, dms, xs, bs, z);
        z[kHidden] = r[0], z[kHidden + 1] = r[1];
    };
    // BN18 batch statistics (two passes over the samples)
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        float z[kCat], xs[kHidden], bs[kHidden], dms[kHidden];
        fwd(on ? n : N - 1, z, xs, bs, dms);
#pragma unroll
        for (int k = 0; k < kCat; ++k) wave_add(row, A_Z + k, on ? z[k] : 0.f, n0 == 0);
    }
    totals(red, tot);
    if (tid < kCat) c_mean[tid] = tot[A_Z + tid] / (float)N;
    __syncthreads();
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        float z[kCat], xs[kHidden], bs[kHidden], dms[kHidden];
        fwd(on ? n : N - 1, z, xs, bs, dms);
#pragma unroll
        for (int k = 0; k < kCat; ++k) {
            const float d = z[k] - c_mean[k];
            wave_add(row, A_ZV + k, on ? d * d : 0.f, n0 == 0);
        }
    }
    totals(red, tot);
    if (tid < kCat) {
        const float var = tot[A_ZV + tid] / (float)N;
        c_var[tid] = var, c_inv[tid] = 1.0f / sqrtf(var + kBnEps);
    }
    __syncthreads();
    // output, loss, the gradients of the output layer and of BN18's gamma / beta
    auto out_fwd = [&](const float z[kCat], float zh[kCat], float &zo) {
        zo = bo;
#pragma unroll
        for (int k = 0; k < kCat; ++k) {
            zh[k] = (z[k] - c_mean[k]) * c_inv[k];
            zo = fmaf(zh[k] * cg[k] + cb[k], wo[k], zo);
        }
    };
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        const int nc = on ? n : N - 1;
        float z[kCat], xs[kHidden], bs[kHidden], dms[kHidden], zh[kCat], zo, lsum, hit, dzo;
        fwd(nc, z, xs, bs, dms);
        out_fwd(z, zh, zo);
        bce(zo, Y(nc), N, lsum, hit, dzo);
        dzo = on ? dzo * a.lw[h] : 0.f;
        wave_add(row, A_DBO, dzo, n0 == 0);
        wave_add(row, A_LOSS, on ? lsum / (float)N : 0.f, n0 == 0);
        wave_add(row, A_ACC, on ? hit / (float)N : 0.f, n0 == 0);
#pragma unroll
        for (int k = 0; k < kCat; ++k) {
            const float db = dzo * wo[k];
            wave_add(row, A_DWO + k, (zh[k] * cg[k] + cb[k]) * dzo, n0 == 0);
            wave_add(row, A_DB2 + k, db, n0 == 0);
            wave_add(row, A_DG2 + k, db * zh[k], n0 == 0);
        }
    }
    totals(red, tot);
    // BN18 backward to z: d r leaves for cascade_r_kernel, d (Dropout output) goes on through relu / BN16
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        const int nc = on ? n : N - 1;
        float z[kCat], xs[kHidden], bs[kHidden], dms[kHidden], zh[kCat], zo, lsum, hit, dzo;
        fwd(nc, z, xs, bs, dms);
        out_fwd(z, zh, zo);
        bce(zo, Y(nc), N, lsum, hit, dzo);
        dzo = on ? dzo * a.lw[h] : 0.f;
        float dz[kCat];
#pragma unroll
        for (int k = 0; k < kCat; ++k)
            dz[k] = c_inv[k] / (float)N * ((float)N * (dzo * wo[k] * cg[k]) - cg[k] * tot[A_DB2 + k] - zh[k] * cg[k] * tot[A_DG2 + k]);
        if (on) dr[((size_t)h * N + n) * 2] = dz[kHidden], dr[((size_t)h * N + n) * 2 + 1] = dz[kHidden + 1];
#pragma unroll
        for (int i = 0; i < kHidden; ++i) {
            const float dbn = (on && bs[i] > 0.f) ? dz[i] * dms[i] : 0.f;
            if (on) dxh[(size_t)(h * kHidden + i) * N + n] = dbn * gamma[i];  // [unit][sample]
            wave_add(row, A_DG + i, dbn * xs[i], n0 == 0);
            wave_add(row, A_DB + i, dbn, n0 == 0);
        }
    }
    totals(red, tot);
    // BN16 backward to the Dense(16) pre-activations: d loss / d pre and the Dense bias gradient
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        const int nc = on ? n : N - 1;
#pragma unroll
        for (int i = 0; i < kHidden; ++i) {
            const float xhat = (P(nc, i) - s_mean[i]) * s_inv[i];
            const float s1 = gamma[i] * tot[A_DB + i], s2 = gamma[i] * tot[A_DG + i];
            float d = s_inv[i] / (float)N * ((float)N * dxh[(size_t)(h * kHidden + i) * N + nc] - s1 - xhat * s2);
            d = on ? d : 0.f;
            if (on) dpre[(size_t)n * kPS + ncls + h * kHidden + i] = d;
            wave_add(row, A_DBIAS + i, d, n0 == 0);
        }
    }
    totals(red, tot);
    // gradients of the small tensors, batch statistics, losses
    float *gh = grad + a.goff_head[h] + (size_t)a.D * kHidden;  // [bias, gamma, beta, mm, mv (16 each), cat gamma, beta, mm, mv (18 each), wo (18), bo]
    if (tid < kHidden) {
        gh[tid] = tot[A_DBIAS + tid];
        gh[16 + tid] = tot[A_DG + tid];
        gh[32 + tid] = tot[A_DB + tid];
        bnstat[h * 32 + tid] = s_mean[tid];
        bnstat[h * 32 + 16 + tid] = s_var[tid];
    }
    if (tid < kCat) {
        gh[4 * kHidden + 16 + tid] = tot[A_DG2 + tid];
        gh[4 * kHidden + 16 + kCat + tid] = tot[A_DB2 + tid];
        gh[4 * kHidden + 16 + 4 * kCat + tid] = tot[A_DWO + tid];
        bnstat[kBnStatFloats + h * 2 * kCat + tid] = c_mean[tid];
        bnstat[kBnStatFloats + h * 2 * kCat + kCat + tid] = c_var[tid];
    }
    if (tid == 0) {
        gh[4 * kHidden + 16 + 5 * kCat] = tot[A_DBO];
        losses[h] = tot[A_LOSS];
        if (a.ext_losses) losses[2 * nh + 4 + h] = tot[A_ACC];
    }
}

// head R: forward again, d loss / d r = MSE term + what S and M sent back, backward; then the weighted total loss
template <bool STAGED>
__global__ void __launch_bounds__(kTh)
cascade_r_kernel(HeadsArgs a, const float *__restrict__ pre, const float *__restrict__ y, const float *__restrict__ hp,
                 const float *__restrict__ drop, float *__restrict__ dpre, float *__restrict__ dxh, const float *__restrict__ dr,
                 float *__restrict__ grad, float *__restrict__ bnstat, float *__restrict__ losses) {
    extern __shared__ __attribute__((aligned(16))) float stage[];
    __shared__ float s_mean[kHidden], s_var[kHidden], s_inv[kHidden];
    __shared__ float red[kNW][kA], tot[kA];
    const int tid = threadIdx.x, N = a.N, ncls = a.n_classes, nh = a.n_heads;
    float *row = red[tid >> 6];
    constexpr int h = 2, PST = kHidden + 1;
    const int ycol = 2;  // R's columns of the targets: [S | M | R0 R1 | 3C]
    float *tile = stage, *ty = stage + (size_t)(STAGED ? N : 0) * PST;
    auto P = [&](int n, int c) -> float { return STAGED ? tile[n * PST + c] : pre[(size_t)n * kPS + ncls + 2 * kHidden + c]; };
    auto Y = [&](int n, int c) -> float { return STAGED ? ty[2 * n + c] : y[(size_t)n * a.out_dim + ycol + c]; };
    if constexpr (STAGED) {
        for (int i = tid; i < N * kHidden; i += kTh) {
            const int n = i / kHidden, c = i - n * kHidden;
            tile[n * PST + c] = pre[(size_t)n * kPS + ncls + 2 * kHidden + c];
        }
        for (int i = tid; i < 2 * N; i += kTh) ty[i] = y[(size_t)(i >> 1) * a.out_dim + ycol + (i & 1)];
        __syncthreads();
    }
    batch_stats(N, kHidden, P, s_mean, s_var, s_inv);
    const float *pR = hp + a.hp_off[h], *gamma = pR, *beta = pR + 16, *wo = pR + 64;
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        const int nc = on ? n : N - 1;
        float u[kHidden], dm[kHidden], xh[kHidden], bn[kHidden], ad[kHidden], r[2];
#pragma unroll
        for (int i = 0; i < kHidden; ++i) u[i] = P(nc, i);
        load_mask(drop, nc, h, dm);
        hidden_fwd(u, s_mean, s_inv, gamma, beta, dm, xh, bn, ad);
        r_out(ad, wo, r);
        float dzo[2], lsum = 0.f;
        for (int c = 0; c < 2; ++c) {
            const float d = r[c] - Y(nc, c);
            lsum += d * d;
            dzo[c] = 2.0f * d / (float)(N * 2) * a.lw[h] + dr[(size_t)nc * 2 + c] + dr[((size_t)N + nc) * 2 + c];
            dzo[c] = on ? dzo[c] : 0.f;
            wave_add(row, A_DBO + c, dzo[c], n0 == 0);
        }
        wave_add(row, A_LOSS, on ? lsum / (float)(N * 2) : 0.f, n0 == 0);
#pragma unroll
        for (int i = 0; i < kHidden; ++i) {
            float da = 0.f;
            for (int c = 0; c < 2; ++c) {
                da = fmaf(dzo[c], wo[i * 2 + c], da);
                wave_add(row, A_DWO + i * 2 + c, ad[i] * dzo[c], n0 == 0);
            }
            const float dbn = (on && bn[i] > 0.f) ? da * dm[i] : 0.f;
            if (on) dxh[(size_t)(h * kHidden + i) * N + n] = dbn * gamma[i];
            wave_add(row, A_DG + i, dbn * xh[i], n0 == 0);
            wave_add(row, A_DB + i, dbn, n0 == 0);
        }
    }
    totals(red, tot);
    for (int n0 = 0; n0 < N; n0 += kTh) {
        const int n = n0 + tid;
        const bool on = n < N;
        const int nc = on ? n : N - 1;
#pragma unroll
        for (int i = 0; i < kHidden; ++i) {
            const float xhat = (P(nc, i) - s_mean[i]) * s_inv[i];
            const float s1 = gamma[i] * tot[A_DB + i], s2 = gamma[i] * tot[A_DG + i];
            float d = s_inv[i] / (float)N * ((float)N * dxh[(size_t)(h * kHidden + i) * N + nc] - s1 - xhat * s2);
            d = on ? d : 0.f;
            if (on) dpre[(size_t)n * kPS + ncls + h * kHidden + i] = d;
            wave_add(row, A_DBIAS + i, d, n0 == 0);
        }
    }
    totals(red, tot);
    float *gh = grad + a.goff_head[h] + (size_t)a.D * kHidden;  // [bias, gamma, beta, mm, mv (16 each), wo (16, 2), bo (2)]
    if (tid < kHidden) {
        gh[tid] = tot[A_DBIAS + tid];
        gh[16 + tid] = tot[A_DG + tid];
        gh[32 + tid] = tot[A_DB + tid];
        gh[80 + 2 * tid] = tot[A_DWO + 2 * tid];
        gh[80 + 2 * tid + 1] = tot[A_DWO + 2 * tid + 1];
        bnstat[h * 32 + tid] = s_mean[tid];
        bnstat[h * 32 + 16 + tid] = s_var[tid];
    }
    if (tid < 2) gh[80 + 2 * kHidden + tid] = tot[A_DBO + tid];
    if (tid == 0) {
        losses[h] = tot[A_LOSS];
        if (a.ext_losses) losses[2 * nh + 4 + h] = 0.f;  // R is not a sigmoid head
        float total = 0.f;  // cascade_sm_kernel finished before this launch: its losses are in memory
        for (int k = 0; k <= nh; ++k) total += a.lw[k] * (k == h ? tot[A_LOSS] : losses[k]);
        losses[nh + 1] = total;  // without the l2 term (losses[nh + 3], l2_penalty_kernel)
    }
}

}  // namespace

static_assert(kTh == kSmallHeadThreads, "smh_train_plan.h plans these kernels' workgroups");
static auto pick_cascade_sm_kernel(bool staged) { return staged ? cascade_sm_kernel<true> : cascade_sm_kernel<false>; }
static auto pick_cascade_r_kernel(bool staged) { return staged ? cascade_r_kernel<true> : cascade_r_kernel<false>; }

int smh_tcn::launch_cascade_heads_train(const HeadsArgs &a, const HeadsPlan &p, const float *pre, const float *y, const float *hp,
                                        const float *drop, float *dpre, float *dxh, float *dr, float *grad, float *bnstat,
                                        float *losses, hipStream_t st) {
    SMH_REQUIRE(a.n_heads == 3 && a.head_odim[2] == 2, "cascaded heads: expected S, M, R[2]");
    const HeadsLaunch &sm = p.k[0], &r = p.k[1];
    const int rc = smh::launch_lds(pick_cascade_sm_kernel(sm.staged), "cascade_sm_kernel", dim3(sm.grid), dim3(sm.threads), sm.lds, sm.lds,
                                   st, a, pre, y, hp, drop, dpre, dxh, dr, grad, bnstat, losses);
    if (rc) return rc;
    return smh::launch_lds(pick_cascade_r_kernel(r.staged), "cascade_r_kernel", dim3(r.grid), dim3(r.threads), r.lds, r.lds, st, a, pre, y,
                           hp, drop, dpre, dxh, dr, grad, bnstat, losses);
}
