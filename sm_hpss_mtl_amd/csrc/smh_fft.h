// The mixed-radix Stockham autosort FFT of the packed real frame, in LDS: the one statement of it for the f32 STFT (smh_stft.hip),
// the f64 STFT (smh_stft_f64.hip) and the HPSS resynthesis (smh_hpss_audio.hip).  Everything is a template over the complex type C
// (float2 or double2; its real type is real_t<C>), so the three kernels run the same text in their own precision.
//
// A real frame of length n_fft is packed into M = n_fft / 2 complex points (z[m] = x[2m] + i x[2m+1]) and transformed in
// ping-pong buffers, one butterfly per thread and stage.  Butterflies: radix 8 (= 2 x 4 in registers), radix 4, radix 2, Winograd
// radix 5, generic 3 / 7.  LDS indices are padded (one element per 16) so that the strided Stockham writes spread over banks;
// work-item -> (frame, butterfly) maps use a reciprocal multiply instead of an integer division.
#pragma once
#include "smh_common.h"

namespace smh_fft {

// ---- the stage table: a kernel argument, filled on the host ---------------------------------------------------------------------
struct Stages {
    int n_stages;
    int radix[smh::kMaxFftStages];
    float inv_nb[smh::kMaxFftStages];  // 1 / (M / radix)
    float inv_ns[smh::kMaxFftStages];  // 1 / Ns of the stage
    int tmul[smh::kMaxFftStages];      // M / (Ns * radix)
};
inline void fill_stages(const int *radix, int n_stages, int M, Stages &st) {
    st.n_stages = n_stages;
    for (int i = 0, ns = 1; i < smh::kMaxFftStages; ++i) {
        st.radix[i] = i < n_stages ? radix[i] : 1;
        st.inv_nb[i] = (float)st.radix[i] / (float)M;
        st.inv_ns[i] = 1.0f / (float)ns;
        st.tmul[i] = M / (ns * st.radix[i]) > 0 ? M / (ns * st.radix[i]) : 0;
        ns *= st.radix[i];
        if (ns > M) ns = M;
    }
}

// ---- complex helpers ------------------------------------------------------------------------------------------------------------
template <class C>
using real_t = decltype(C::x);
template <class C>
__device__ __forceinline__ C cplx(real_t<C> x, real_t<C> y) {
    C c;
    c.x = x, c.y = y;
    return c;
}
template <class C>
__device__ __forceinline__ C cmul(C a, C b) { return cplx<C>(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <class C>
__device__ __forceinline__ C cadd(C a, C b) { return cplx<C>(a.x + b.x, a.y + b.y); }
template <class C>
__device__ __forceinline__ C csub(C a, C b) { return cplx<C>(a.x - b.x, a.y - b.y); }
template <class C>
__device__ __forceinline__ C mul_mi(C a) { return cplx<C>(a.y, -a.x); }  // * (-i)
__device__ __forceinline__ int pad(int i) { return i + (i >> 4); }
// exact floor(it / n) for 0 <= it < 2^20 given inv = 1/n
__device__ __forceinline__ int fdiv(int it, float inv) { return (int)(((float)it + 0.5f) * inv); }

// ---- butterflies ----------------------------------------------------------------------------------------------------------------
template <int R, class C>
__device__ __forceinline__ void dft_generic(C *v) {
    using T = real_t<C>;
    C o[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        C acc = v[0];
#pragma unroll
        for (int r = 1; r < R; ++r) {
            const int e = (r * q) % R;
            const double ang = -6.283185307179586476925 * (double)e / (double)R;
            const C w = cplx<C>((T)__builtin_cos(ang), (T)__builtin_sin(ang));  // constant-folded
            acc = cadd(acc, cmul(v[r], w));
        }
        o[q] = acc;
    }
#pragma unroll
    for (int q = 0; q < R; ++q) v[q] = o[q];
}

template <class C>
__device__ __forceinline__ void dft4(C &a, C &b, C &c, C &d) {
    const C s0 = cadd(a, c), d0 = csub(a, c);
    const C s1 = cadd(b, d), d1 = mul_mi(csub(b, d));
    a = cadd(s0, s1);
    b = cadd(d0, d1);
    c = csub(s0, s1);
    d = csub(d0, d1);
}

template <int R, class C>
__device__ __forceinline__ void dft(C *v) {
    using T = real_t<C>;
    if constexpr (R == 2) {
        const C a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 4) {
        dft4(v[0], v[1], v[2], v[3]);
    } else if constexpr (R == 8) {
        // 8 = 2 x 4: even/odd 4-point DFTs, odd outputs twisted by w8^k
        C e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
        C o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
        dft4(e0, e1, e2, e3);
        dft4(o0, o1, o2, o3);
        const T h = (T)0.70710678118654752440;
        o1 = cplx<C>(h * (o1.x + o1.y), h * (o1.y - o1.x));   // * (1 - i)/sqrt2
        o2 = mul_mi(o2);                                      // * (-i)
        o3 = cplx<C>(h * (o3.y - o3.x), -h * (o3.x + o3.y));  // * (-1 - i)/sqrt2
        v[0] = cadd(e0, o0), v[4] = csub(e0, o0);
        v[1] = cadd(e1, o1), v[5] = csub(e1, o1);
        v[2] = cadd(e2, o2), v[6] = csub(e2, o2);
        v[3] = cadd(e3, o3), v[7] = csub(e3, o3);
    } else if constexpr (R == 5) {
        // Winograd-style 5-point DFT: 34 real operations
        const T c1 = (T)0.30901699437494742410, c2 = (T)-0.80901699437494742410;
        const T s1 = (T)0.95105651629515357212, s2 = (T)0.58778525229247312917;
        const C t1 = cadd(v[1], v[4]), t2 = cadd(v[2], v[3]);
        const C t3 = csub(v[1], v[4]), t4 = csub(v[2], v[3]);
        const C a1 = cplx<C>(v[0].x + c1 * t1.x + c2 * t2.x, v[0].y + c1 * t1.y + c2 * t2.y);
        const C a2 = cplx<C>(v[0].x + c2 * t1.x + c1 * t2.x, v[0].y + c2 * t1.y + c1 * t2.y);
        const C b1 = cplx<C>(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y);
        const C b2 = cplx<C>(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y);
        v[0] = cplx<C>(v[0].x + t1.x + t2.x, v[0].y + t1.y + t2.y);
        v[1] = cplx<C>(a1.x + b1.y, a1.y - b1.x);  // a1 - i b1
        v[4] = cplx<C>(a1.x - b1.y, a1.y + b1.x);  // a1 + i b1
        v[2] = cplx<C>(a2.x + b2.y, a2.y - b2.x);
        v[3] = cplx<C>(a2.x - b2.y, a2.y + b2.x);
    } else {
        dft_generic<R>(v);
    }
}

// ---- stages ---------------------------------------------------------------------------------------------------------------------
// One sample of the windowed frame in the transform's precision.  f64 is the reference's product, float64 window times the float32
// sample widened (smh_stft_f64.hip); each type keeps its operand order.
__device__ __forceinline__ float windowed(const float *y, const float *w, int n) { return y[n] * w[n]; }
__device__ __forceinline__ double windowed(const float *y, const double *w, int n) { return w[n] * (double)y[n]; }

// One Stockham stage for butterfly j of one frame (Govindaraju et al. formulation).  FIRST: the inputs are the windowed real frame
// read straight from global memory, z[m] = (x[2m], x[2m+1]).
template <int R, bool FIRST, class C>
__device__ __forceinline__ void stage(int step, int j, int Ns, float inv_ns, int tmul, const C *__restrict__ src, C *__restrict__ dst,
                                      const C *__restrict__ tw, const float *__restrict__ audio, const real_t<C> *__restrict__ win) {
    C v[R];
    if constexpr (FIRST) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int m = j + r * step;
            v[r] = cplx<C>(windowed(audio, win, 2 * m), windowed(audio, win, 2 * m + 1));
        }
    } else {
        const int k = j - fdiv(j, inv_ns) * Ns;
        const int tstep = k * tmul;  // exp(-2 pi i k r / (Ns R)) = twM[k r M/(Ns R)]
#pragma unroll
        for (int r = 0; r < R; ++r) {
            C x = src[pad(j + r * step)];
            if (r > 0) x = cmul(x, tw[r * tstep]);
            v[r] = x;
        }
    }
    dft<R>(v);
    const int k = FIRST ? 0 : j - fdiv(j, inv_ns) * Ns;
    const int j0 = (j - k) * R + k;  // (j / Ns) * Ns * R + k
#pragma unroll
    for (int r = 0; r < R; ++r) dst[pad(j0 + r * Ns)] = v[r];
}

template <bool FIRST, class C>
__device__ __forceinline__ void run_stage(int nb, int R, int j, int Ns, float inv_ns, int tmul, const C *src, C *dst, const C *tw,
                                          const float *audio, const real_t<C> *win) {
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

// The loop over the stages -- barrier, item -> (frame, butterfly) by fdiv, run_stage<s == 0>, swap the ping-pong buffers, Ns *= R --
// stays with each kernel.  As a function of this header that takes the stage table by reference it compiled to other loops in all
// three kernels (the table is a kernel argument, and behind a reference the optimiser no longer treats it as one), and the kernels'
// machine code is not to change for tidiness.

// ---- the real-FFT bin -----------------------------------------------------------------------------------------------------------
// X[k] of the real frame from the packed transform: zk = Z[k], zm = Z[M - k], w = exp(-2 pi i k / n_fft);
// X = (e - i w d) / 2 with e = zk + conj zm, d = zk - conj zm
template <class C>
__device__ __forceinline__ C untangle(C zk, C zm, C w) {
    using T = real_t<C>;
    const C e = cplx<C>(zk.x + zm.x, zk.y - zm.y), d = cplx<C>(zk.x - zm.x, zk.y + zm.y);
    const C wd = cmul(w, d);
    return cplx<C>((T)0.5 * (e.x + wd.y), (T)0.5 * (e.y - wd.x));
}

}  // namespace smh_fft
