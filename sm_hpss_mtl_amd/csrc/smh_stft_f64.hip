// a1 in f64 (stft_precision 1, smh_ctx_create_ex): |S| equal to np.abs(librosa.core.stft(...)) bit for bit.
//
// What the reference computes (librosa 0.8 stft, center=False): frame t = y[t*hop : t*hop + n_fft] (float32) times the periodic
// Hann window (float64) -> float64 products -> numpy's float64 rfft -> stored as complex64 -> np.abs of the complex64, a float32.
// Two facts make a bit-exact device form possible:
//   - the f64 transform's last bits do not survive the rounding to complex64: another f64 summation order (here a mixed-radix
//     Stockham FFT of the packed real frame, as in smh_stft.hip) gives the same complex64 on (practically) every bin;
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
#include "smh_rag.h"

namespace {

using smh_stft::kThreads;

struct Stft64Args {
    int n_samples, hop, M, K, T;
    int F, tt;  // frames per item, frames per LDS pass (tt <= F)
    int n_stages;
    int radix[smh::kMaxFftStages];
    float inv_nb[smh::kMaxFftStages];  // 1 / (M / radix)
    float inv_ns[smh::kMaxFftStages];  // 1 / Ns of the stage
    int tmul[smh::kMaxFftStages];      // M / (Ns * radix)
    int B, xcd_tiles;
};

typedef double2 c64;
__device__ __forceinline__ c64 cmul(c64 a, c64 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ c64 cadd(c64 a, c64 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ c64 csub(c64 a, c64 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ c64 mul_mi(c64 a) { return make_double2(a.y, -a.x); }  // * (-i)
__device__ __forceinline__ int pad(int i) { return i + (i >> 4); }
// exact floor(it / n) for 0 <= it < 2^20 given inv = 1/n (as smh_stft.hip)
__device__ __forceinline__ int fdiv(int it, float inv) { return (int)(((float)it + 0.5f) * inv); }

template <int R>
__device__ __forceinline__ void dft_generic(c64 *v) {
    c64 o[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        c64 acc = v[0];
#pragma unroll
        for (int r = 1; r < R; ++r) {
            const int e = (r * q) % R;
            const double ang = -6.283185307179586476925 * (double)e / (double)R;
            acc = cadd(acc, cmul(v[r], make_double2(__builtin_cos(ang), __builtin_sin(ang))));  // constant-folded
        }
        o[q] = acc;
    }
#pragma unroll
    for (int q = 0; q < R; ++q) v[q] = o[q];
}

__device__ __forceinline__ void dft4(c64 &a, c64 &b, c64 &c, c64 &d) {
    const c64 s0 = cadd(a, c), d0 = csub(a, c);
    const c64 s1 = cadd(b, d), d1 = mul_mi(csub(b, d));
    a = cadd(s0, s1);
    b = cadd(d0, d1);
    c = csub(s0, s1);
    d = csub(d0, d1);
}

template <int R>
__device__ __forceinline__ void dft(c64 *v) {
    if constexpr (R == 2) {
        const c64 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 4) {
        dft4(v[0], v[1], v[2], v[3]);
    } else if constexpr (R == 8) {
        c64 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
        c64 o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
        dft4(e0, e1, e2, e3);
        dft4(o0, o1, o2, o3);
        const double h = 0.70710678118654752440;
        o1 = make_double2(h * (o1.x + o1.y), h * (o1.y - o1.x));   // * (1 - i)/sqrt2
        o2 = mul_mi(o2);                                           // * (-i)
        o3 = make_double2(h * (o3.y - o3.x), -h * (o3.x + o3.y));  // * (-1 - i)/sqrt2
        v[0] = cadd(e0, o0), v[4] = csub(e0, o0);
        v[1] = cadd(e1, o1), v[5] = csub(e1, o1);
        v[2] = cadd(e2, o2), v[6] = csub(e2, o2);
        v[3] = cadd(e3, o3), v[7] = csub(e3, o3);
    } else if constexpr (R == 5) {
        const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;
        const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;
        const c64 t1 = cadd(v[1], v[4]), t2 = cadd(v[2], v[3]);
        const c64 t3 = csub(v[1], v[4]), t4 = csub(v[2], v[3]);
        const c64 a1 = make_double2(v[0].x + c1 * t1.x + c2 * t2.x, v[0].y + c1 * t1.y + c2 * t2.y);
        const c64 a2 = make_double2(v[0].x + c2 * t1.x + c1 * t2.x, v[0].y + c2 * t1.y + c1 * t2.y);
        const c64 b1 = make_double2(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y);
        const c64 b2 = make_double2(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y);
        v[0] = make_double2(v[0].x + t1.x + t2.x, v[0].y + t1.y + t2.y);
        v[1] = make_double2(a1.x + b1.y, a1.y - b1.x);  // a1 - i b1
        v[4] = make_double2(a1.x - b1.y, a1.y + b1.x);  // a1 + i b1
        v[2] = make_double2(a2.x + b2.y, a2.y - b2.x);
        v[3] = make_double2(a2.x - b2.y, a2.y + b2.x);
    } else {
        dft_generic<R>(v);
    }
}

// One Stockham stage for butterfly j of one frame (the formulation of smh_stft.hip's stage(), in f64)
template <int R, bool FIRST>
__device__ __forceinline__ void stage(int step, int j, int Ns, float inv_ns, int tmul, const c64 *__restrict__ src,
                                      c64 *__restrict__ dst, const c64 *__restrict__ tw, const float *__restrict__ audio,
                                      const double *__restrict__ win) {
    c64 v[R];
    if constexpr (FIRST) {  // the windowed real frame, packed: z[m] = (x[2m], x[2m+1]), x[n] = w64[n] * (double)y[n]
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int m = j + r * step;
            v[r] = make_double2(win[2 * m] * (double)audio[2 * m], win[2 * m + 1] * (double)audio[2 * m + 1]);
        }
    } else {
        const int k = j - fdiv(j, inv_ns) * Ns;
        const int tstep = k * tmul;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            c64 x = src[pad(j + r * step)];
            if (r > 0) x = cmul(x, tw[r * tstep]);
            v[r] = x;
        }
    }
    dft<R>(v);
    const int k = FIRST ? 0 : j - fdiv(j, inv_ns) * Ns;
    const int j0 = (j - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) dst[pad(j0 + r * Ns)] = v[r];
}

template <bool FIRST>
__device__ __forceinline__ void run_stage(int nb, int R, int j, int Ns, float inv_ns, int tmul, const c64 *src, c64 *dst,
                                          const c64 *tw, const float *audio, const double *win) {
    switch (R) {
        case 2: stage<2, FIRST>(nb, j, Ns, inv_ns, tmul, src, dst, tw, audio, win); break;
        case 3: stage<3, FIRST>(nb, j, Ns, inv_ns, tmul, src, dst, tw, audio, win); break;
        case 4: stage<4, FIRST>(nb, j, Ns, inv_ns, tmul, src, dst, tw, audio, win); break;
        case 5: stage<5, FIRST>(nb, j, Ns, inv_ns, tmul, src, dst, tw, audio, win); break;
        case 7: stage<7, FIRST>(nb, j, Ns, inv_ns, tmul, src, dst, tw, audio, win); break;
        case 8: stage<8, FIRST>(nb, j, Ns, inv_ns, tmul, src, dst, tw, audio, win); break;
        default: break;
    }
}

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
        for (int s = 0; s < a.n_stages; ++s) {
            const int R = a.radix[s];
            const int nb = M / R;
            __syncthreads();  // (also: the tables are in LDS, and the previous pass's untangle has read its frames)
            for (int it = threadIdx.x; it < nf * nb; it += blockDim.x) {
                const int f = fdiv(it, a.inv_nb[s]), j = it - f * nb;
                if (s == 0)
                    run_stage<true>(nb, R, j, Ns, 1.f, 0, nullptr, dst + f * MP, tw, clip + (size_t)(t0 + c0 + f) * a.hop, win);
                else
                    run_stage<false>(nb, R, j, Ns, a.inv_ns[s], a.tmul[s], src + f * MP, dst + f * MP, tw, nullptr, nullptr);
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
            const c64 zk = Z[pad(k == M ? 0 : k)];
            c64 zc = Z[pad(k == 0 ? 0 : M - k)];
            zc.y = -zc.y;
            const c64 e = cadd(zk, zc), d = csub(zk, zc);
            const c64 wd = cmul(tw2[k], d);  // X = 0.5 e - 0.5 i w d
            const double re = 0.5 * (e.x + wd.y);
            const double im = 0.5 * (e.y - wd.x);
            Sb[(size_t)k * a.T + f] = np_cabsf((float)re, (float)im);
        }
    }
}

}  // namespace

int smh_stft::launch_f64(const smh_ctx *ctx, const StftPlan &p, const char *what, const float *d_audio, int n_items, int n_samples, int T,
                         float *d_S, const smh_rag::Clip *d_clips, const smh_rag::Item *d_items, hipStream_t st) {
    Stft64Args a;
    a.hop = ctx->cfg.hop, a.M = ctx->M, a.K = ctx->K;
    fill_stages(ctx->radix, ctx->n_stages, a);
    a.n_samples = n_samples, a.T = T, a.F = p.frames, a.tt = p.pass_frames, a.B = n_items, a.xcd_tiles = p.xcd_tiles;
    return smh::launch_lds(stft_f64_kernel, what, dim3(p.grid_x, p.grid_y), dim3(p.threads), p.lds, p.lds, st, a, d_audio, ctx->d_window64,
                           ctx->d_twM64, ctx->d_tw2M64, d_S, d_clips, d_items);
}
