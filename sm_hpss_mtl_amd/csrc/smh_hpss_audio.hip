// HPSS audio separation: y_harm, y_perc = istft(D * softmask(harm, perc)), istft(D * softmask(perc, harm)) with D the complex STFT
// of the audio -- librosa.effects.hpss with this project's framing (center=False, periodic Hann zero-padded centrally to n_fft).
// The generator of the reference's hpss_audio/ listening demos.
//
// One kernel, hpss_resynth_kernel, in two instantiations: B equal clips, and clips of different lengths in one launch (the ragged
// entries at the end of this file).  A workgroup owns a run of output samples (smh_resynth_plan.h: tile, halo, LDS budget) and, in
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
#include "smh_rag.h"
#include "smh_resynth_plan.h"
#include "smh_softmask.h"

namespace {

using namespace smh_resynth;
using namespace smh_fft;
using smh_rag::Clip;
using smh_rag::Item;

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

// what the ragged instantiation takes behind the equal-length kernel's arguments: the descriptors and the flat (clip, tile) list;
// this workgroup's item of the per-XCD grid (smh_xcd.h), false: none (a workgroup past the list)
__device__ __forceinline__ bool rag_item(const Clip *clips, const Item *items, int n_items, const Clip *&c, int &b, int &tile) {
    unsigned n;
    if (!smh::xcd_item(n_items, n)) return false;
    c = clips, b = items[n].clip, tile = items[n].tile;
    return true;
}

// One kernel body, two instantiations.  hpss_resynth_kernel<false>: B equal clips, workgroup (tile, clip) of the 2-D grid, everything
// per clip from `a` and blockIdx.y; harm (B, K, T); its arguments end with y_perc, as they always did.  hpss_resynth_kernel<true,
// const Clip *, const Item *, int>: clips of different lengths, workgroup = one (clip, tile) item of the flat list on the per-XCD grid
// (smh_xcd.h), everything per clip from its descriptor -- frames, samples, the offsets of its audio (both outputs start at the same
// offset), of its perc rows ((K, T), rows of exactly T floats) and of its harm, the 16-frame blocked image the medians of a ragged call
// write (smh_resynth_plan.h); a.T and a.n_samples are not read.  Nothing else differs: a clip's samples are the same bits from either.
template <bool RAG, class... Rag>
__global__ void __launch_bounds__(kThreads)
hpss_resynth_kernel(ResynthArgs a, const float *__restrict__ audio, const float *__restrict__ window,
                    const float2 *__restrict__ twM, const float2 *__restrict__ tw2M, const float *__restrict__ harm,
                    const float *__restrict__ perc, float *__restrict__ y_harm, float *__restrict__ y_perc, Rag... rag) {
    static_assert(sizeof...(Rag) == (RAG ? 3 : 0), "rag_item's first three arguments, or nothing");
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int M = a.M, P = a.pass;
    const int MP = pad(M) + 2;  // padded frame stride (float2)
    float2 *tw = lds;           // M twiddles
    float2 *tw2 = lds + M;      // M + 1 (un)tangle twiddles
    float2 *R0 = tw2 + (M + 1);  // four regions of P frames: R0 / R1 forward and harmonic inverse, R2 / R3 percussive inverse
    float2 *R1 = R0 + P * MP, *R2 = R1 + P * MP, *R3 = R2 + P * MP;
    float *win = (float *)(R3 + P * MP);  // n_fft
    float *acc_h = win + a.n_fft, *acc_p = acc_h + a.acc;

    int b, tile;
    const Clip *clips = nullptr;
    if constexpr (RAG) {
        if (!rag_item(rag..., clips, b, tile)) return;
    } else {
        b = blockIdx.y, tile = blockIdx.x;
    }
    // the clip's frames, samples and first sample, read where they are used (the equal-length form keeps the code it had)
    auto frames = [&]() { if constexpr (RAG) return clips[b].T; else return a.T; };
    auto samples = [&]() { if constexpr (RAG) return clips[b].n_samples; else return a.n_samples; };
    auto first = [&]() { if constexpr (RAG) return (size_t)clips[b].audio_off; else return (size_t)b * a.n_samples; };
    const int t0 = tile * a.tile;            // first owned frame
    const int t1 = min(t0 + a.tile, frames());  // behind the last
    const int tb = max(t0 - a.halo, 0);      // first frame that reaches an owned sample
    const int s0 = t0 * a.hop;               // first owned sample
    for (int i = threadIdx.x; i < M; i += blockDim.x) tw[i] = twM[i];
    for (int i = threadIdx.x; i <= M; i += blockDim.x) tw2[i] = tw2M[i];
    for (int i = threadIdx.x; i < a.n_fft; i += blockDim.x) win[i] = window[i];
    for (int i = threadIdx.x; i < 2 * a.acc; i += blockDim.x) acc_h[i] = 0.f;
    const float *clip = audio + first();
    size_t spec, hspec = 0;
    if constexpr (RAG) spec = (size_t)clips[b].spec_off, hspec = (size_t)clips[b].harm_off;
    else spec = (size_t)b * a.K * frames();
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
            const size_t o1 = spec + (size_t)k * frames() + (size_t)(p0 + f), o2 = spec + (size_t)k2 * frames() + (size_t)(p0 + f);
            size_t g1 = o1, g2 = o2;  // harm[k][t]: the (K, T) row, or the blocked image (t / 16, K, 16)
            if constexpr (RAG) {
                const int t = p0 + f, tb16 = (t >> 4) * a.K, tl = t & 15;
                g1 = hspec + (size_t)((tb16 + k) * 16 + tl), g2 = hspec + (size_t)((tb16 + k2) * 16 + tl);
            }
            float mh1, mp1, mh2, mp2;
            smh::softmask_pair(harm[g1], perc[o1], mh1, mp1);
            smh::softmask_pair(harm[g2], perc[o2], mh2, mp2);
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
    const int own = (t1 == frames() ? samples() : s0 + a.tile * a.hop) - s0;
    const int cov_end = (frames() - 1) * a.hop + a.n_fft;  // behind the last frame's last sample
    const float fM = (float)M;
    auto value = [&](int i, float &vh, float &vp) {
        const int n = s0 + i;
        vh = vp = 0.f;
        if (n >= cov_end) return;
        const int tlo = n < a.n_fft ? 0 : (n - a.n_fft) / a.hop + 1, thi = min(frames() - 1, n / a.hop);
        float wss = 0.f;
        for (int t = tlo; t <= thi; ++t) {
            const float w = win[n - t * a.hop];
            wss += w * w;
        }
        const float den = wss > FLT_MIN ? wss * fM : fM;
        vh = acc_h[i] / den, vp = acc_p[i] / den;
    };
    float *oh = y_harm + first() + s0, *op = y_perc + first() + s0;
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
    return smh::launch_lds(hpss_resynth_kernel<false>, "hpss_resynth_kernel", dim3((unsigned)p.tiles, (unsigned)B), dim3(p.threads), p.lds,
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

// ---- clips of different lengths in one call: the contract of smh_hpss_audio_ragged_sizes / _f32 (include/smh.h), on the planner of
// smh_rag.h.  STFT of every clip, both medians, the ragged resynthesis: one launch each per sub-batch.  Bits: an STFT frame does not
// depend on its tile, medians are selections, and the resynthesis runs resynth_tile either way, so a clip gets what smh_hpss_audio_f32
// gives it alone.  The clips the ragged STFT and median launches do not take (smh_rag.h: medians_ok, clip_ok, start_ok) go through
// smh_hpss_audio_f32 one by one on the same stream.
namespace {

using smh_rag::align_up;
using smh_rag::HostClip;
using smh_rag::Layout;

constexpr size_t kRagFixedBytes = 6 * 256;  // alignment slack between the regions of a sub-batch
const char kRagWho[] = "smh_hpss_audio_ragged_f32";

struct RagSwitches {  // read once per call: routing, table sizes and the launches agree
    smh_stft::StftSwitches stft = smh_stft::read_stft_switches();
    smh_median::MedianSwitches med = smh_median::read_median_switches();
};

// 0: the ragged kernels take clip b, -1: it goes alone (d_audio == nullptr: as if every clip started where the STFT can take it)
void rag_routes(const smh_ctx *ctx, const RagSwitches &sw, const float *d_audio, const long long *off, const Layout &p, int B,
                std::vector<int> &route) {
    route.assign(B, -1);
    if (!smh_rag::medians_ok(ctx, sw.med)) return;
    for (int b = 0; b < B; ++b)
        if (smh_rag::clip_ok(ctx, p.T[b]) && (!d_audio || smh_rag::start_ok(ctx, sw.stft, d_audio, off[b]))) route[b] = 0;
}

// what a sub-batch is sized with: the STFT's items counted at 16 frames (a lower bound of its tile), the medians' at their tile
size_t rag_estimate(const smh_ctx *ctx, const RagSwitches &sw, int T) {
    const int med = smh_median::rag_tile_frames(ctx->K, ctx->cfg.l_harm, ctx->cfg.l_perc, sw.med);
    return rag_clip_bytes(ctx->K, T, 16, med > 16 ? med : 16);
}

// the least workspace a call with these clips runs in: the largest clip alone, in a sub-batch or through smh_hpss_audio_f32
size_t rag_single_bytes(const smh_ctx *ctx, const RagSwitches &sw, const Layout &p, const int *len, const std::vector<int> &route, int B,
                        size_t *total) {
    size_t single = 0;
    *total = kRagFixedBytes;
    for (int b = 0; b < B; ++b) {
        single = std::max(single, smh_hpss_audio_workspace_bytes(ctx, 1, len[b]));
        if (route[b] < 0) continue;
        const size_t cb = rag_estimate(ctx, sw, p.T[b]);
        *total += cb;
        single = std::max(single, cb + kRagFixedBytes);
    }
    return single;
}

// one sub-batch: tables -> one upload -> one launch per stage
int audio_sub_batch(const smh_ctx *ctx, const RagSwitches &sw, const float *d_audio, const HostClip *hc, const int *len,
                    int n, float *d_y_harm, float *d_y_perc, char *d_work, size_t work_bytes, hipStream_t st) {
    std::vector<Clip> clips;
    const size_t spec = smh_rag::fill_clips(hc, n, ctx->K, false, clips);
    size_t harm = 0;
    for (int b = 0; b < n; ++b) {
        clips[b].harm_off = (long long)harm, clips[b].n_samples = len[b];
        harm += rag_harm_floats(ctx->K, hc[b].T);
    }
    // the tables: [clips][stft items][median items][resynthesis items]
    smh_rag::Tables t;
    int n_stft, n_med, n_syn;
    const int med_frames = smh_median::rag_tile_frames(ctx->K, ctx->cfg.l_harm, ctx->cfg.l_perc, sw.med);
    const size_t o_clips = t.add(clips.data(), clips.size() * sizeof(Clip));
    const size_t o_stft = t.add_items(hc, n, smh_stft::rag_frames(smh_stft::geom_of(ctx), sw.stft, true), -1, &n_stft);
    const size_t o_med = t.add_items(hc, n, med_frames, -1, &n_med);
    const size_t o_syn = t.add_items(hc, n, kTileFrames, -1, &n_syn);
    // device regions behind the tables, each on a 256-byte boundary: S, perc, harm
    const size_t sb = align_up(spec * sizeof(float), 256);
    int rc = t.upload(ctx, kRagWho, d_work, work_bytes, 2 * sb + harm * sizeof(float), st);
    if (rc) return rc;
    float *d_S = reinterpret_cast<float *>(t.behind()), *d_perc = reinterpret_cast<float *>(t.behind() + sb);
    float *d_harm = reinterpret_cast<float *>(t.behind() + 2 * sb);
    const Clip *d_clips = t.at<const Clip>(o_clips);
    rc = smh_stft::launch_rag(ctx, sw.stft, d_audio, d_S, d_clips, t.at<const Item>(o_stft), n_stft, true, st);
    if (rc) return rc;
    rc = smh_median::launch_rag(sw.med, d_S, d_harm, d_perc, ctx->K, ctx->cfg.l_harm, ctx->cfg.l_perc, d_clips, t.at<const Item>(o_med), n_med, st);
    if (rc) return rc;
    const RagPlan rp = plan_rag(geom_of(ctx), n_syn);
    ResynthArgs a{};
    a.n_fft = ctx->cfg.n_fft, a.hop = ctx->cfg.hop, a.M = ctx->M, a.K = ctx->K;
    a.tile = rp.tile, a.halo = rp.halo, a.pass = rp.pass, a.acc = (int)rp.acc;
    fill_stages(ctx->radix, ctx->n_stages, a.M, a.st);
    return smh::launch_lds(hpss_resynth_kernel<true, const Clip *, const Item *, int>, "hpss_resynth_kernel (ragged)", dim3(rp.grid_x, rp.grid_y), dim3(rp.threads), rp.lds,
                           smh_resynth::kLdsLimit, st, a, d_audio, ctx->d_window, ctx->d_twM, ctx->d_tw2M, (const float *)d_harm,
                           (const float *)d_perc, d_y_harm, d_y_perc, d_clips, t.at<const Item>(o_syn), n_syn);
}

// the arguments both entries and the route query share: the layout, or the refusal that names the clip at fault
int rag_layout(const smh_ctx *ctx, const char *who, const long long *off, const int *len, int B, Layout &p) {
    SMH_REQUIRE(B >= 0, "%s: B=%d is negative", who, B);
    SMH_REQUIRE(B == 0 || (off && len), "%s: null argument", who);
    return smh_rag::plan_layout(ctx, who, off, len, B, 0, 0, false, 0, p);
}

}  // namespace

extern "C" int smh_hpss_audio_ragged_sizes(const smh_ctx *ctx, const long long *h_offsets, const int *h_lengths, int B, int *h_T,
                                           size_t *work_bytes) {
    SMH_REQUIRE(ctx, "smh_hpss_audio_ragged_sizes: null argument");
    Layout p;
    int rc = rag_layout(ctx, "smh_hpss_audio_ragged_sizes", h_offsets, h_lengths, B, p);
    if (rc) return rc;
    smh_rag::export_layout(p, B, nullptr, nullptr, h_T, nullptr);
    if (work_bytes) {
        const RagSwitches sw;
        std::vector<int> route;
        rag_routes(ctx, sw, nullptr, h_offsets, p, B, route);  // (alignment is the call's business: sized as if every clip qualified)
        size_t total;
        const size_t single = rag_single_bytes(ctx, sw, p, h_lengths, route, B, &total);
        *work_bytes = smh_rag::work_size(B, single, total);
    }
    return SMH_OK;
}

extern "C" int smh_internal_hpss_audio_ragged_route(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets,
                                                    const int *h_lengths, int B, int *h_route) {
    SMH_REQUIRE(ctx && d_audio && h_route, "smh_internal_hpss_audio_ragged_route: null argument");
    Layout p;
    int rc = rag_layout(ctx, "smh_internal_hpss_audio_ragged_route", h_offsets, h_lengths, B, p);
    if (rc) return rc;
    std::vector<int> route;
    rag_routes(ctx, RagSwitches(), d_audio, h_offsets, p, B, route);
    for (int b = 0; b < B; ++b) h_route[b] = route[b];
    return SMH_OK;
}

extern "C" int smh_hpss_audio_ragged_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets, const int *h_lengths,
                                         int B, float *d_y_harm, float *d_y_perc, void *d_work, size_t work_bytes, void *stream) {
    SMH_REQUIRE(ctx && d_audio && h_offsets && h_lengths && d_y_harm && d_y_perc, "%s: null argument", kRagWho);
    Layout p;
    int rc = rag_layout(ctx, kRagWho, h_offsets, h_lengths, B, p);
    if (rc) return rc;
    const RagPlan rp = plan_rag(geom_of(ctx), 0);  // the refusals depend on the context alone: for the call as a whole, before any launch
    SMH_REQUIRE(!rp.refusal[0], "%s: %s", kRagWho, rp.refusal);
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(d_work, "%s: null workspace", kRagWho);
    // the clips in the order of their offsets: no two may share a sample, and the call's extent is first .. last
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return h_offsets[x] != h_offsets[y] ? h_offsets[x] < h_offsets[y] : x < y; });
    long long end = 0;
    for (int i = 0; i < B; ++i) {
        const int b = order[i];
        if (i > 0)
            SMH_REQUIRE(h_offsets[b] >= h_offsets[order[i - 1]] + h_lengths[order[i - 1]], "%s: clip %d and clip %d overlap", kRagWho,
                        order[i - 1], b);
        end = std::max(end, h_offsets[b] + h_lengths[b]);
    }
    const long long first = h_offsets[order[0]];
    const size_t yb = (size_t)(end - first) * sizeof(float);
    SMH_REQUIRE(!overlap(d_y_harm + first, yb, d_y_perc + first, yb), "%s: d_y_harm and d_y_perc overlap", kRagWho);
    for (float *y : {d_y_harm, d_y_perc})
        SMH_REQUIRE(!overlap(y + first, yb, d_audio + first, yb) && !overlap(y + first, yb, d_work, work_bytes),
                    "%s: an output overlaps the audio or the workspace", kRagWho);
    SMH_REQUIRE((uintptr_t)d_work % 16 == 0, "%s: workspace is not 16-byte aligned", kRagWho);
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SMH_REQUIRE(!(hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone),
                "%s uploads its tables from a staging buffer: it cannot be captured in a graph", kRagWho);
    const RagSwitches sw;
    std::vector<int> route;
    rag_routes(ctx, sw, d_audio, h_offsets, p, B, route);
    std::vector<int> sized(route);  // as smh_hpss_audio_ragged_sizes sizes: a clip sent alone for its start counts as taken
    if (smh_rag::medians_ok(ctx, sw.med))
        for (int b = 0; b < B; ++b)
            if (smh_rag::clip_ok(ctx, p.T[b])) sized[b] = 0;
    size_t total;
    const size_t least = align_up(rag_single_bytes(ctx, sw, p, h_lengths, sized, B, &total), 256);
    if (work_bytes < least)
        return smh::set_error(SMH_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed by the largest single clip", kRagWho, work_bytes, least);
    std::vector<HostClip> hc;
    std::vector<int> len;
    for (int b = 0; b < B; ++b)
        if (route[b] == 0) hc.push_back(smh_rag::host_clip(p, h_offsets, b, 1, 0)), len.push_back(h_lengths[b]);
    rc = smh_rag::run_sub_batches(
        hc.size(), kRagFixedBytes, work_bytes, st, [&](size_t b) { return rag_estimate(ctx, sw, hc[b].T); }, [&](size_t b0, size_t nb) {
            return audio_sub_batch(ctx, sw, d_audio, hc.data() + b0, len.data() + b0, (int)nb, d_y_harm, d_y_perc, (char *)d_work,
                                   work_bytes, st);
        });
    if (rc) return rc;
    // the clips no ragged kernel covers, one by one on the same stream (the workspace is free again in stream order)
    for (int b = 0; b < B; ++b) {
        if (route[b] == 0) continue;
        rc = smh_hpss_audio_f32(ctx, d_audio + h_offsets[b], 1, h_lengths[b], d_y_harm + h_offsets[b], d_y_perc + h_offsets[b], d_work,
                                work_bytes, stream);
        if (rc) return rc;
    }
    return SMH_OK;
}
