// a1 in f64 (stft_precision 1, smh_ctx_create_ex): |S| equal to np.abs(librosa.core.stft(...)) bit for bit.
//
// What the reference computes (librosa 0.8 stft, center=False): frame t = y[t*hop : t*hop + n_fft] (float32) times the periodic
// Hann window (float64) -> float64 products -> numpy's float64 rfft -> stored as complex64 -> np.abs of the complex64, a float32.
// Two facts make a bit-exact device form possible:
//   - the f64 transform's last bits do not survive the rounding to complex64: another f64 summation order (here a mixed-radix
//     Stockham FFT of the packed real frame, smh_fft.h in double2) gives the same complex64 on (practically) every bin;
//   - numpy's complex64 abs is not a correctly rounded hypot but  l = max(|re|, |im|), s = min(..), r = s / l,
//     |z| = l * sqrtf(fmaf(r, r, 1)), 0 when l = 0  (numpy's SIMD path; tests/test_stft_f64_pins.py pins it on the host).
// So: f64 window, f64 twiddles built on the host from exactly reduced angles (smh_ctx.hip), an f64 FFT in LDS, one rounding of
// Re and Im to f32 (v_cvt_f32_f64, nearest even), then the formula above with IEEE f32 division and square root (hipcc's default
// correctly rounded expansions; no fast-math forms) and an explicit fmaf.
//
// One kernel serves every call: equal-length batches (1-D grid of (clip, tile) items in 8 XCD-contiguous ranges, as
// stft_mag_kernel), ragged calls and the streaming route (the (clip, tile) item lists of smh_rag.h).  An item is up to F frames;
// the workgroup transforms them tt at a time (tt: the frames whose two f64 ping-pong buffers fit the LDS budget, chosen when the
// context is created).  A frame's bits do not depend on its tile, so a clip gets the same S in every kind of call.  Audio is read
// as single floats: no alignment requirement on the clip start or its length.
#include "smh_common.h"
#include "smh_fft.h"
#include "smh_rag.h"

namespace {

using smh_stft::kThreads;
using namespace smh_fft;

struct Stft64Args {
    int n_samples, hop, M, K, T;
    int F, tt;  // frames per item, frames per LDS pass (tt <= F)
    Stages st;
    int B, xcd_tiles;
};

typedef double2 c64;

// numpy's |complex64| (npy_cabsf on its SIMD path): not a correctly rounded hypot, and not sqrt(re^2 + im^2)
__device__ __forceinline__ float np_cabsf(float re, float im) {
    const float a = fabsf(re), b = fabsf(im);
    const float l = fmaxf(a, b), s = fminf(a, b);
    if (l == 0.f) return 0.f;
    const float r = s / l;
    return l * sqrtf(fmaf(r, r, 1.0f));
}

__global__ void __launch_bounds__(kThreads)
stft_f64_kernel(Stft64Args a, const float *__restrict__ audio, const double *__restrict__ window, const c64 *__restrict__ twM,
                const c64 *__restrict__ tw2M, float *__restrict__ S, const smh_rag::Clip *__restrict__ rag,
                const smh_rag::Item *__restrict__ items) {
    extern __shared__ __attribute__((aligned(16))) c64 lds[];
    const int M = a.M;
    const int MP = pad(M) + 2;  // padded frame stride (double2)
    c64 *tw = lds;               // M twiddles
    c64 *tw2 = tw + M;           // M + 1 untangle twiddles
    double *win = reinterpret_cast<double *>(tw2 + (M + 1));  // n_fft = 2M window values
    c64 *buf0 = tw2 + (M + 1) + M;
    c64 *buf1 = buf0 + a.tt * MP;
    int b = blockIdx.y, tile = blockIdx.x;
    size_t clip_off, spec_off;
    unsigned n;
    if (rag) {  // ragged call / streaming route (smh_rag.h): a.B items, one list range per XCD (smh_xcd.h)
        if (!smh::xcd_item(a.B, n)) return;
        const smh_rag::Item item = items[n];
        b = item.clip, tile = item.tile;
        a.T = rag[b].T;
        clip_off = (size_t)rag[b].audio_off, spec_off = (size_t)rag[b].spec_off;
    } else {
        if (a.xcd_tiles > 0) {  // the (clip, tile) items in clip-major order, one range per XCD
            if (!smh::xcd_item((unsigned)a.B * (unsigned)a.xcd_tiles, n)) return;
            b = (int)(n / (unsigned)a.xcd_tiles), tile = (int)(n - (unsigned)b * (unsigned)a.xcd_tiles);
        }
        clip_off = (size_t)b * a.n_samples, spec_off = (size_t)b * a.K * a.T;
    }
    const int t0 = tile * a.F;
    const int nitem = min(a.F, a.T - t0);
    for (int i = threadIdx.x; i < M; i += blockDim.x) tw[i] = twM[i];
    for (int i = threadIdx.x; i <= M; i += blockDim.x) tw2[i] = tw2M[i];
    for (int i = threadIdx.x; i < 2 * M; i += blockDim.x) win[i] = window[i];
    const float *clip = audio + clip_off;

    for (int c0 = 0; c0 < nitem; c0 += a.tt) {
        const int nf = min(a.tt, nitem - c0);
        c64 *src = buf0, *dst = buf1;
        int Ns = 1;
        for (int s = 0; s < a.st.n_stages; ++s) {
            const int R = a.st.radix[s];
            const int nb = M / R;
            __syncthreads();  // (also: the tables are in LDS, and the previous pass's untangle has read its frames)
            for (int it = threadIdx.x; it < nf * nb; it += blockDim.x) {
                const int f = fdiv(it, a.st.inv_nb[s]), j = it - f * nb;
                if (s == 0)
                    run_stage<true, c64>(nb, R, j, Ns, 1.f, 0, nullptr, dst + f * MP, tw, clip + (size_t)(t0 + c0 + f) * a.hop, win);
                else
                    run_stage<false, c64>(nb, R, j, Ns, a.st.inv_ns[s], a.st.tmul[s], src + f * MP, dst + f * MP, tw, nullptr, nullptr);
            }
            c64 *tmp = src;
            src = dst;
            dst = tmp;
            Ns *= R;
        }
        __syncthreads();
        // real-FFT untangle in f64, one rounding to complex64, numpy's magnitude; frames fastest -> contiguous stores along t
        float *Sb = S + spec_off + t0 + c0;
        const float inv_nf = 1.0f / (float)nf;
        for (int it = threadIdx.x; it < nf * a.K; it += blockDim.x) {
            const int k = fdiv(it, inv_nf), f = it - k * nf;
            const c64 *Z = src + f * MP;
            const c64 X = untangle(Z[pad(k == M ? 0 : k)], Z[pad(k == 0 ? 0 : M - k)], tw2[k]);
            Sb[(size_t)k * a.T + f] = np_cabsf((float)X.x, (float)X.y);
        }
    }
}

}  // namespace

int smh_stft::launch_f64(const smh_ctx *ctx, const StftPlan &p, const char *what, const float *d_audio, int n_items, int n_samples, int T,
                         float *d_S, const smh_rag::Clip *d_clips, const smh_rag::Item *d_items, hipStream_t st) {
    Stft64Args a;
    a.hop = ctx->cfg.hop, a.M = ctx->M, a.K = ctx->K;
    fill_stages(ctx->radix, ctx->n_stages, a.M, a.st);
    a.n_samples = n_samples, a.T = T, a.F = p.frames, a.tt = p.pass_frames, a.B = n_items, a.xcd_tiles = p.xcd_tiles;
    return smh::launch_lds(stft_f64_kernel, what, dim3(p.grid_x, p.grid_y), dim3(p.threads), p.lds, p.lds, st, a, d_audio, ctx->d_window64,
                           ctx->d_twM64, ctx->d_tw2M64, d_S, d_clips, d_items);
}
