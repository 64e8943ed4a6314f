// HPSS audio separation: y_harm, y_perc = istft(D * softmask(harm, perc)), istft(D * softmask(perc, harm)) with D the complex STFT
// of the audio -- librosa.effects.hpss with this project's framing (center=False, periodic Hann zero-padded centrally to n_fft).
// The generator of the reference's hpss_audio/ listening demos.
//
// One kernel, hpss_resynth_kernel.  A workgroup owns a run of output samples (smh_resynth_plan.h: tile, halo, LDS budget) and, in
// passes of kPassFrames frames,
//   1  recomputes the frames' forward transform from the audio: the windowed real frame packed into M = n_fft / 2 complex points, the
//      mixed-radix Stockham FFT of smh_fft.h in LDS, the text the f32 STFT runs (smh_stft.hip: stft_mag_kernel);
//   2  per bin pair (k, M - k): untangles the two real-FFT bins X[k], X[M - k], multiplies each by its two masks (smh_softmask.h:
//      softmask_pair, the bits of smh_softmask_f32) and tangles the masked Hermitian spectra back into the packed form of an inverse real FFT,
//      Z'[k] = E[k] + i O[k], E[k] = (X[k] + conj X[M - k]) / 2, O[k] = (X[k] - conj X[M - k]) / 2 * conj w^k;
//   3  inverts both spectra with the same forward Stockham stages on conj Z' (ifft z = conj fft conj z / M): 2 * kPassFrames
//      independent transforms; even samples are the real parts, odd samples minus the imaginary parts;
//   4  adds w[n - t hop] * frame_t[n - t hop] to the sample's accumulator in LDS, each sample by ONE thread over the pass's frames in
//      ascending t: no atomics, and the sum's order depends on nothing but the sample.
// At the end every owned sample is divided by M * wss[n] (wss = sum of w^2 over the frames that reach n, summed per sample in
// ascending t; undivided where wss <= FLT_MIN, 0 behind the last frame) and stored, 16 bytes per lane where the tile's first
// output sample is 16-byte aligned in both outputs, 4 bytes per lane where it is not.  The complex spectrogram never leaves the CU.
// HBM traffic per one-second clip: 64 KB audio and 2 x 78.8 KB medians in (+ 12.5 % halo, served by L2), 2 x 64 KB out.
#include <cfloat>
#include <cstdint>

#include "smh_common.h"
#include "smh_fft.h"
#include "smh_resynth_plan.h"
#include "smh_softmask.h"

namespace {

using namespace smh_resynth;
using namespace smh_fft;

struct ResynthArgs {
    int n_samples, n_fft, hop, M, K, T;
    int tile, halo, pass, acc;  // acc: samples of one accumulator
    Stages st;
};

// the inverse of smh_fft.h's untangle: conj Z'[k] from xk = X[k], xm = X[M - k]; Z' = E + i O, E = (xk + conj xm) / 2, O = (xk - conj xm) / 2 * conj w
__device__ __forceinline__ float2 tangle_conj(float2 xk, float2 xm, float2 w) {
    const float2 e = make_float2(xk.x + xm.x, xk.y - xm.y), d = make_float2(xk.x - xm.x, xk.y + xm.y);
    const float2 o = make_float2(d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y);  // d conj w
    return make_float2(0.5f * (e.x - o.y), -0.5f * (e.y + o.x));
}

__global__ void __launch_bounds__(kThreads)
hpss_resynth_kernel(ResynthArgs a, const float *__restrict__ audio, const float *__restrict__ window,
                    const float2 *__restrict__ twM, const float2 *__restrict__ tw2M, const float *__restrict__ harm,
                    const float *__restrict__ perc, float *__restrict__ y_harm, float *__restrict__ y_perc) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int M = a.M, P = a.pass;
    const int MP = pad(M) + 2;  // padded frame stride (float2)
    float2 *tw = lds;           // M twiddles
    float2 *tw2 = lds + M;      // M + 1 (un)tangle twiddles
    float2 *R0 = tw2 + (M + 1);  // four regions of P frames: R0 / R1 forward and harmonic inverse, R2 / R3 percussive inverse
    float2 *R1 = R0 + P * MP, *R2 = R1 + P * MP, *R3 = R2 + P * MP;
    float *win = (float *)(R3 + P * MP);  // n_fft
    float *acc_h = win + a.n_fft, *acc_p = acc_h + a.acc;

    const int b = blockIdx.y, tile = blockIdx.x;
    const int t0 = tile * a.tile;            // first owned frame
    const int t1 = min(t0 + a.tile, a.T);    // behind the last
    const int tb = max(t0 - a.halo, 0);      // first frame that reaches an owned sample
    const int s0 = t0 * a.hop;               // first owned sample
    for (int i = threadIdx.x; i < M; i += blockDim.x) tw[i] = twM[i];
    for (int i = threadIdx.x; i <= M; i += blockDim.x) tw2[i] = tw2M[i];
    for (int i = threadIdx.x; i < a.n_fft; i += blockDim.x) win[i] = window[i];
    for (int i = threadIdx.x; i < 2 * a.acc; i += blockDim.x) acc_h[i] = 0.f;
    const float *clip = audio + (size_t)b * a.n_samples;
    const size_t spec = (size_t)b * a.K * a.T;
    const int npair = M / 2 + 1;  // pairs (k, M - k), k = 0 .. M / 2

    for (int p0 = tb; p0 < t1; p0 += P) {
        const int nf = min(P, t1 - p0);
        // 1: forward transform of the pass's frames
        float2 *src = R0, *dst = R1;
        int Ns = 1;
        for (int s = 0; s < a.st.n_stages; ++s) {
            const int R = a.st.radix[s];
            const int nb = M / R;
            __syncthreads();
            for (int it = threadIdx.x; it < nf * nb; it += blockDim.x) {
                const int f = fdiv(it, a.st.inv_nb[s]), j = it - f * nb;
                if (s == 0)
                    run_stage<true, float2>(nb, R, j, Ns, 1.f, 0, nullptr, dst + f * MP, tw, clip + (size_t)(p0 + f) * a.hop, win);
                else
                    run_stage<false, float2>(nb, R, j, Ns, a.st.inv_ns[s], a.st.tmul[s], src + f * MP, dst + f * MP, tw, nullptr, nullptr);
            }
            float2 *tmp = src;
            src = dst;
            dst = tmp;
            Ns *= R;
        }
        __syncthreads();
        // 2: bin pairs: untangle, mask, tangle.  The pair's item is the only reader and writer of Z[k] and Z[M - k] of its frame,
        // so the harmonic spectrum replaces the transform in place; the percussive one goes to R2.  Frames fastest.
        for (int it = threadIdx.x; it < nf * npair; it += blockDim.x) {
            const int k = it / nf, f = it - k * nf, k2 = M - k;
            float2 *Zh = src + f * MP, *Zp = R2 + f * MP;
            const float2 zk = Zh[pad(k)], zm = Zh[pad(k == 0 ? 0 : k2)];
            const float2 w1 = tw2[k], w2 = tw2[k2];
            const float2 x1 = untangle(zk, zm, w1), x2 = untangle(zm, zk, w2);
            const size_t o1 = spec + (size_t)k * a.T + (size_t)(p0 + f), o2 = spec + (size_t)k2 * a.T + (size_t)(p0 + f);
            float mh1, mp1, mh2, mp2;
            smh::softmask_pair(harm[o1], perc[o1], mh1, mp1);
            smh::softmask_pair(harm[o2], perc[o2], mh2, mp2);
            const float2 h1 = make_float2(x1.x * mh1, x1.y * mh1), h2 = make_float2(x2.x * mh2, x2.y * mh2);
            const float2 q1 = make_float2(x1.x * mp1, x1.y * mp1), q2 = make_float2(x2.x * mp2, x2.y * mp2);
            Zh[pad(k)] = tangle_conj(h1, h2, w1);
            Zp[pad(k)] = tangle_conj(q1, q2, w1);
            if (k != 0 && k2 != k) {
                Zh[pad(k2)] = tangle_conj(h2, h1, w2);
                Zp[pad(k2)] = tangle_conj(q2, q1, w2);
            }
        }
        // 3: both inverses as 2 * nf forward transforms of conj Z'
        float2 *hs = src, *hd = dst, *ps = R2, *pd = R3;
        Ns = 1;
        for (int s = 0; s < a.st.n_stages; ++s) {
            const int R = a.st.radix[s];
            const int nb = M / R;
            __syncthreads();
            for (int it = threadIdx.x; it < 2 * nf * nb; it += blockDim.x) {
                const int q = fdiv(it, a.st.inv_nb[s]), j = it - q * nb;
                const bool pc = q >= nf;
                const int f = pc ? q - nf : q;
                run_stage<false, float2>(nb, R, j, Ns, a.st.inv_ns[s], a.st.tmul[s], (pc ? ps : hs) + f * MP, (pc ? pd : hd) + f * MP, tw,
                                         nullptr, nullptr);
            }
            float2 *tmp = hs;
            hs = hd, hd = tmp;
            tmp = ps, ps = pd, pd = tmp;
            Ns *= R;
        }
        __syncthreads();
        // 4: overlap-add, one thread per sample, the pass's frames in ascending t (the next pass's first barrier separates these
        // reads from its writes)
        const int lo = max(p0 * a.hop, s0) - s0;
        const int hi = min((p0 + nf - 1) * a.hop + a.n_fft - s0, a.acc);
        for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
            float ah = acc_h[i], ap = acc_p[i];
            for (int f = 0; f < nf; ++f) {
                const int m = s0 + i - (p0 + f) * a.hop;
                if (m < 0 || m >= a.n_fft) continue;
                const float w = win[m];
                const float2 zh = hs[f * MP + pad(m >> 1)], zp = ps[f * MP + pad(m >> 1)];
                ah += w * ((m & 1) ? -zh.y : zh.x);
                ap += w * ((m & 1) ? -zp.y : zp.x);
            }
            acc_h[i] = ah, acc_p[i] = ap;
        }
    }
    __syncthreads();

    // owned samples: up to the next tile's first, the last tile up to the clip's end
    const int own = (t1 == a.T ? a.n_samples : s0 + a.tile * a.hop) - s0;
    const int cov_end = (a.T - 1) * a.hop + a.n_fft;  // behind the last frame's last sample
    const float fM = (float)M;
    auto value = [&](int i, float &vh, float &vp) {
        const int n = s0 + i;
        vh = vp = 0.f;
        if (n >= cov_end) return;
        const int tlo = n < a.n_fft ? 0 : (n - a.n_fft) / a.hop + 1, thi = min(a.T - 1, n / a.hop);
        float wss = 0.f;
        for (int t = tlo; t <= thi; ++t) {
            const float w = win[n - t * a.hop];
            wss += w * w;
        }
        const float den = wss > FLT_MIN ? wss * fM : fM;
        vh = acc_h[i] / den, vp = acc_p[i] / den;
    };
    float *oh = y_harm + (size_t)b * a.n_samples + s0, *op = y_perc + (size_t)b * a.n_samples + s0;
    const bool vec = ((uintptr_t)oh % 16 == 0) && ((uintptr_t)op % 16 == 0);
    const int nvec = vec ? own / 4 : 0;
    for (int g = threadIdx.x; g < nvec; g += blockDim.x) {
        float4 vh, vp;
        value(4 * g, vh.x, vp.x), value(4 * g + 1, vh.y, vp.y), value(4 * g + 2, vh.z, vp.z), value(4 * g + 3, vh.w, vp.w);
        reinterpret_cast<float4 *>(oh)[g] = vh;
        reinterpret_cast<float4 *>(op)[g] = vp;
    }
    for (int i = 4 * nvec + (int)threadIdx.x; i < own; i += blockDim.x) {
        float vh, vp;
        value(i, vh, vp);
        oh[i] = vh, op[i] = vp;
    }
}

Geom geom_of(const smh_ctx *ctx) { return Geom{ctx->cfg.n_fft, ctx->cfg.hop, ctx->M}; }

bool overlap(const void *p, size_t np, const void *q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace

extern "C" int smh_internal_resynth_plan(const smh_ctx *ctx, int n_samples, int *out) {
    SMH_REQUIRE(ctx && out, "smh_internal_resynth_plan: null argument");
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    const Plan p = plan(geom_of(ctx), T > 0 ? T : 1);
    SMH_REQUIRE(!p.refusal[0], "smh_hpss_resynth_f32: %s", p.refusal);
    out[0] = p.tile, out[1] = p.halo, out[2] = p.threads, out[3] = (int)p.lds;
    return SMH_OK;
}

extern "C" int smh_hpss_resynth_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, const float *d_harm,
                                    const float *d_perc, float *d_y_harm, float *d_y_perc, void *stream) {
    SMH_REQUIRE(ctx && d_audio && d_harm && d_perc && d_y_harm && d_y_perc, "smh_hpss_resynth_f32: null argument");
    SMH_REQUIRE(B >= 0, "smh_hpss_resynth_f32: B=%d is negative", B);
    SMH_REQUIRE((unsigned)B <= kMaxGridY, "smh_hpss_resynth_f32: B=%d exceeds the grid limit of %u clips per call", B, kMaxGridY);
    SMH_REQUIRE(n_samples >= ctx->cfg.n_fft, "smh_hpss_resynth_f32: n_samples=%d is shorter than n_fft=%d: no frame to invert", n_samples,
                ctx->cfg.n_fft);
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    const Plan p = plan(geom_of(ctx), T);
    SMH_REQUIRE(!p.refusal[0], "smh_hpss_resynth_f32: %s", p.refusal);
    if (B == 0) return SMH_OK;
    const size_t yb = (size_t)B * n_samples * sizeof(float), sb = (size_t)B * ctx->K * T * sizeof(float);
    SMH_REQUIRE(!overlap(d_y_harm, yb, d_y_perc, yb), "smh_hpss_resynth_f32: d_y_harm and d_y_perc overlap");
    for (float *y : {d_y_harm, d_y_perc})
        SMH_REQUIRE(!overlap(y, yb, d_audio, yb) && !overlap(y, yb, d_harm, sb) && !overlap(y, yb, d_perc, sb),
                    "smh_hpss_resynth_f32: an output overlaps an input");
    ResynthArgs a{};
    a.n_samples = n_samples, a.n_fft = ctx->cfg.n_fft, a.hop = ctx->cfg.hop, a.M = ctx->M, a.K = ctx->K, a.T = T;
    a.tile = p.tile, a.halo = p.halo, a.pass = p.pass, a.acc = (int)p.acc;
    fill_stages(ctx->radix, ctx->n_stages, a.M, a.st);
    return smh::launch_lds(hpss_resynth_kernel, "hpss_resynth_kernel", dim3((unsigned)p.tiles, (unsigned)B), dim3(p.threads), p.lds,
                           smh_resynth::kLdsLimit, (hipStream_t)stream, a, d_audio, ctx->d_window, ctx->d_twM, ctx->d_tw2M, d_harm, d_perc,
                           d_y_harm, d_y_perc);
}

// workspace of smh_hpss_audio_f32: S, harm and perc, (B, K, T) floats each, each on a 256-byte boundary
static size_t spec_bytes(const smh_ctx *ctx, int B, int n_samples) {
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    return ((size_t)B * ctx->K * (size_t)(T > 0 ? T : 0) * sizeof(float) + 255) / 256 * 256;
}

extern "C" size_t smh_hpss_audio_workspace_bytes(const smh_ctx *ctx, int B, int n_samples) {
    if (!ctx || B <= 0) return 0;
    return 3 * spec_bytes(ctx, B, n_samples);
}

extern "C" int smh_hpss_audio_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, float *d_y_harm, float *d_y_perc,
                                  void *d_work, size_t work_bytes, void *stream) {
    SMH_REQUIRE(ctx && d_audio && d_y_harm && d_y_perc, "smh_hpss_audio_f32: null argument");
    SMH_REQUIRE(B >= 0, "smh_hpss_audio_f32: B=%d is negative", B);
    SMH_REQUIRE((unsigned)B <= kMaxGridY, "smh_hpss_audio_f32: B=%d exceeds the grid limit of %u clips per call", B, kMaxGridY);
    SMH_REQUIRE(n_samples >= ctx->cfg.n_fft, "smh_hpss_audio_f32: n_samples=%d is shorter than n_fft=%d: no frame to invert", n_samples,
                ctx->cfg.n_fft);
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    const Plan p = plan(geom_of(ctx), T);
    SMH_REQUIRE(!p.refusal[0], "smh_hpss_audio_f32: %s", p.refusal);
    if (B == 0) return SMH_OK;
    const size_t need = smh_hpss_audio_workspace_bytes(ctx, B, n_samples), each = need / 3;
    SMH_REQUIRE(d_work, "smh_hpss_audio_f32: null workspace");
    if (work_bytes < need)
        return smh::set_error(SMH_E_WORKSPACE, "smh_hpss_audio_f32: workspace of %zu bytes, %zu needed", work_bytes, need);
    SMH_REQUIRE((uintptr_t)d_work % 16 == 0, "smh_hpss_audio_f32: workspace is not 16-byte aligned");
    const size_t yb = (size_t)B * n_samples * sizeof(float);
    SMH_REQUIRE(!overlap(d_y_harm, yb, d_y_perc, yb), "smh_hpss_audio_f32: d_y_harm and d_y_perc overlap");
    for (float *y : {d_y_harm, d_y_perc})
        SMH_REQUIRE(!overlap(y, yb, d_audio, yb) && !overlap(y, yb, d_work, need),
                    "smh_hpss_audio_f32: an output overlaps an input or the workspace");
    float *S = (float *)d_work, *harm = (float *)((char *)d_work + each), *perc = (float *)((char *)d_work + 2 * each);
    int rc = smh_stft_mag_f32(ctx, d_audio, B, n_samples, S, stream);
    if (rc == SMH_OK)
        rc = smh_hpss_median_f32(ctx, S, B, ctx->K, T, ctx->cfg.l_harm, ctx->cfg.l_perc, harm, perc, stream);
    if (rc == SMH_OK) rc = smh_hpss_resynth_f32(ctx, d_audio, B, n_samples, harm, perc, d_y_harm, d_y_perc, stream);
    return rc;
}
