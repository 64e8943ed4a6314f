// a1: S = |STFT|  --  np.abs(librosa.core.stft(y, n_fft, win_length, hop_length, center=False))
// (call sites /root/reference/lib/preprocessing.py:407,417,429,439).
//
// Frame t = y[t*hop : t*hop + n_fft] * periodic-Hann.  The real frame of length n_fft is packed into a
// complex sequence of length M = n_fft/2 (z[m] = x[2m] + i x[2m+1]), transformed by a mixed-radix
// Stockham autosort FFT that lives entirely in LDS (ping-pong buffers, one butterfly per thread),
// un-tangled into the n_fft/2+1 real-FFT bins and written as magnitudes, frame-fastest, so that the
// (K, T) freq-major layout librosa returns is produced directly.  n_fft = 400 -> M = 200 = 8*5*5.
// The FFT itself (stage table, butterflies, stages, the untangle) is smh_fft.h's.
// HBM traffic per clip: 64,000 B audio in (re-reads of the 2.5x frame overlap are served by L2),
// 78,792 B magnitudes out.
#include "smh_common.h"
#include "smh_fft.h"
#include "smh_rag.h"

namespace {

using namespace smh_stft;  // the plan's constants (kThreads, kMP400: stft400_kernel's float2 frame stride) and functions
using namespace smh_fft;

struct StftArgs {
    int n_samples, n_fft, hop, M, K, T, tt;  // tt = frames per workgroup
    Stages st;
    float inv_tt;
    int B, xcd_tiles;  // xcd_tiles > 0: 1-D grid, neighbouring tiles on one XCD (smh_xcd.h); the value is the tiles per clip
};

// |re + i im| on the hardware square root (v_sqrt_f32, 1 ulp): the correctly rounded expansion of sqrtf costs ~12 more
// instructions per bin and the STFT kernels are VALU-bound; the parity bound on |S| is 1e-5 of its maximum
__device__ __forceinline__ float mag(float re, float im) { return __builtin_amdgcn_sqrtf(re * re + im * im); }

__global__ void __launch_bounds__(kThreads)
stft_mag_kernel(StftArgs a, const float *__restrict__ audio, const float *__restrict__ window,
                const float2 *__restrict__ twM, const float2 *__restrict__ tw2M, float *__restrict__ S,
                const smh_rag::Clip *__restrict__ rag, const smh_rag::Item *__restrict__ items) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int M = a.M;
    const int MP = pad(M) + 2;  // padded frame stride (float2)
    float2 *tw = lds;           // M twiddles
    float2 *tw2 = lds + M;      // M + 1 untangle twiddles
    float2 *buf0 = tw2 + (M + 1);
    float2 *buf1 = buf0 + a.tt * MP;
    int b = blockIdx.y, tile = blockIdx.x;
    size_t clip_off, spec_off;
    unsigned n;
    if (rag) {  // ragged call (smh_rag.h): a.B items of clips of different lengths, one list range per XCD (smh_xcd.h)
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
    const int t0 = tile * a.tt;
    const int nf = min(a.tt, a.T - t0);
    for (int i = threadIdx.x; i < M; i += blockDim.x) tw[i] = twM[i];
    for (int i = threadIdx.x; i <= M; i += blockDim.x) tw2[i] = tw2M[i];
    const float *clip = audio + clip_off;

    float2 *src = buf0, *dst = buf1;
    int Ns = 1;
    for (int s = 0; s < a.st.n_stages; ++s) {
        const int R = a.st.radix[s];
        const int nb = M / R;
        __syncthreads();
        for (int it = threadIdx.x; it < nf * nb; it += blockDim.x) {
            const int f = fdiv(it, a.st.inv_nb[s]), j = it - f * nb;
            if (s == 0)
                run_stage<true, float2>(nb, R, j, Ns, 1.f, 0, nullptr, dst + f * MP, tw, clip + (size_t)(t0 + f) * a.hop, window);
            else
                run_stage<false, float2>(nb, R, j, Ns, a.st.inv_ns[s], a.st.tmul[s], src + f * MP, dst + f * MP, tw, nullptr, nullptr);
        }
        float2 *tmp = src;
        src = dst;
        dst = tmp;
        Ns *= R;
    }
    __syncthreads();
    // real-FFT untangle + magnitude; frames fastest -> contiguous stores along t
    float *Sb = S + spec_off + t0;
    const float inv_nf = nf == a.tt ? a.inv_tt : 1.0f / (float)nf;
    for (int it = threadIdx.x; it < nf * a.K; it += blockDim.x) {
        const int k = fdiv(it, inv_nf), f = it - k * nf;
        const float2 *Z = src + f * MP;
        // smh_fft.h's untangle(), written out: called as that function, one multiply of this loop comes out with its operands swapped
        const float2 zk = Z[pad(k == M ? 0 : k)];
        float2 zc = Z[pad(k == 0 ? 0 : M - k)];
        zc.y = -zc.y;
        const float2 e = cadd(zk, zc), d = csub(zk, zc);
        const float2 wd = cmul(tw2[k], d);  // X = 0.5*e - 0.5*i*w*d
        const float re = 0.5f * (e.x + wd.y);
        const float im = 0.5f * (e.y - wd.x);
        Sb[(size_t)k * a.T + f] = mag(re, im);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// n_fft = 400 (the reference's only STFT size besides Jang's 512): M = 200 = 8 x 25 as a two-phase Cooley-Tukey
// with ONE exchange through LDS instead of two Stockham passes, and the real-FFT untangle done per pair (k, M-k):
//   phase 1  item (frame, n2 < 25): radix-8 DFT over n1 of z[25 n1 + n2] read straight from the windowed audio,
//            twiddle W_200^(n2 k1), store Y[k1][n2];
//   phase 2  item (frame, k1 < 8): 25-point DFT (5 x 5 Winograd butterflies in registers, constant twiddles) over
//            n2 of Y[k1][.], store Z[k1 + 8 k2];
//   phase 3  item (k <= 100, frame): |X[k]| and |X[200 - k]| from the pair Z[k], Z[200 - k]; frames fastest, so the
//            (K, T) stores are contiguous along t.
// Where the tile allows, phase 1 keeps one column n2 per thread (its window and twiddles in registers instead of LDS tables)
// and phase 3 takes two neighbouring frames per item (one 8-byte store per bin): same operations in the same order per
// element, see the kernel.
// ~225 wave-instructions per frame instead of ~510 in the generic kernel.  Frame stride 201 float2 (odd) keeps the
// frame-strided phase-3 reads and the 25-strided phase-2 reads conflict-free.

// Complex arithmetic on (re, im) register PAIRS for stft400_kernel.  hipcc packs float2 math into v_pk_* instructions but
// builds every swapped / negated operand ((-i) b, conj b, the cross terms of a complex product) with v_mov / v_pk_mov into a new
// pair first: 333 of the kernel's 1000 VALU instructions were such moves (round 2), and a VALU instruction costs the SIMD four
// cycles whatever it does.  The VOP3P encoding selects and negates the halves of each source itself (op_sel, op_sel_hi,
// neg_lo, neg_hi), so these patterns are single instructions -- spelled out here because the compiler does not form them:
typedef float v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2 sub_i(v2 a, v2 b) {  // a - i b = (a.x + b.y, a.y - b.x)
    v2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ v2 add_i(v2 a, v2 b) {  // a + i b = (a.x - b.y, a.y + b.x)
    v2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ v2 add_conj(v2 a, v2 b) {  // a + conj(b) = (a.x + b.x, a.y - b.y)
    v2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ v2 sub_conj(v2 a, v2 b) {  // a - conj(b) = (a.x - b.x, a.y + b.y)
    v2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ v2 cmulp(v2 a, v2 w) {  // a w: (a.x w.x, a.x w.y) then (- a.y w.y, + a.y w.x) on top
    v2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(w));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(a), "v"(w), "v"(t));
    return r;
}
// the same with a compile-time twiddle kept in a scalar register pair (one constant-bus operand per instruction)
__device__ __forceinline__ v2 cmulp_s(v2 a, v2 w) {
    v2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "s"(w));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(a), "s"(w), "v"(t));
    return r;
}

__device__ __forceinline__ void pk_dft4(v2 &a, v2 &b, v2 &c, v2 &d) {
    const v2 s0 = a + c, d0 = a - c, s1 = b + d, bd = b - d;
    a = s0 + s1;
    b = sub_i(d0, bd);  // d0 + (-i)(b - d)
    c = s0 - s1;
    d = add_i(d0, bd);
}
__device__ __forceinline__ void pk_dft8(v2 *v) {  // 8 = 2 x 4: even / odd 4-point DFTs, odd outputs twisted by w8^k
    v2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    v2 o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    pk_dft4(e0, e1, e2, e3);
    pk_dft4(o0, o1, o2, o3);
    const float h = 0.70710678118654752440f;
    const v2 u1 = sub_i(o1, o1);  // o1 (1 - i)
    const v2 u3 = add_i(o3, o3);  // o3 (1 + i): w8^3 o3 = -h u3
    v[0] = e0 + o0, v[4] = e0 - o0;
    v[1] = e1 + h * u1, v[5] = e1 - h * u1;
    v[2] = sub_i(e2, o2), v[6] = add_i(e2, o2);  // w8^2 = -i
    v[3] = e3 - h * u3, v[7] = e3 + h * u3;
}
__device__ __forceinline__ void pk_dft5(v2 *v) {  // Winograd-style 5-point DFT
    const float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;
    const float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
    const v2 t1 = v[1] + v[4], t2 = v[2] + v[3], t3 = v[1] - v[4], t4 = v[2] - v[3];
    const v2 a1 = v[0] + c1 * t1 + c2 * t2, a2 = v[0] + c2 * t1 + c1 * t2;
    const v2 b1 = s1 * t3 + s2 * t4, b2 = s2 * t3 - s1 * t4;
    v[0] = v[0] + t1 + t2;
    v[1] = sub_i(a1, b1), v[4] = add_i(a1, b1);
    v[2] = sub_i(a2, b2), v[3] = add_i(a2, b2);
}
__device__ __forceinline__ void pk_dft25(v2 *x) {
    // x[5a + b] -> X[c + 5d]:  inner DFT over a (output c), twiddle W_25^(b c), outer DFT over b (output d)
    v2 t[5][5];  // t[c][b]
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        v2 u[5] = {x[b], x[5 + b], x[10 + b], x[15 + b], x[20 + b]};
        pk_dft5(u);
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            if (b * c == 0) {
                t[c][b] = u[c];
            } else {
                const double ang = -6.283185307179586476925 * (double)(b * c) / 25.0;
                t[c][b] = cmulp_s(u[c], v2{(float)__builtin_cos(ang), (float)__builtin_sin(ang)});
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        pk_dft5(t[c]);
#pragma unroll
        for (int d = 0; d < 5; ++d) x[c + 5 * d] = t[c][d];
    }
}

__device__ __forceinline__ void dft25(float2 *x) {
    // x[5a + b] -> X[c + 5d]:  inner DFT over a (output c), twiddle W_25^(b c), outer DFT over b (output d)
    float2 t[5][5];  // t[c][b]
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        float2 u[5] = {x[b], x[5 + b], x[10 + b], x[15 + b], x[20 + b]};
        dft<5>(u);
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            if (b * c == 0) {
                t[c][b] = u[c];
            } else {
                const double ang = -6.283185307179586476925 * (double)(b * c) / 25.0;
                t[c][b] = cmul(u[c], make_float2((float)__builtin_cos(ang), (float)__builtin_sin(ang)));
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        dft<5>(t[c]);
#pragma unroll
        for (int d = 0; d < 5; ++d) x[c + 5 * d] = t[c][d];
    }
}

// (at least four waves per SIMD: 128 VGPRs -- at 129 a fourth 256-thread workgroup per CU did not fit)
template <int ROW>  // float2 pitch of a phase-1 table row: 25, or 40 = the 25 entries and the first 15 again (below)
__global__ void __launch_bounds__(512, 4)
stft400_kernel(const float *__restrict__ audio, const float *__restrict__ window, const float2 *__restrict__ twM,
               const float2 *__restrict__ tw2M, float *__restrict__ S, int n_samples, int hop, int T, int F, int probe, int B,
               int ntiles, int pairs, const smh_rag::Clip *__restrict__ rag, const smh_rag::Item *__restrict__ items) {
    // pairs (SMH_STFT_PAIRS, default 1): phase 1 with a fixed column per thread and phase 3 in frame pairs where the tile allows; 0: the
    // round-robin phase 1 with its LDS tables and one frame per phase-3 item on every tile (A/B runs, the bit-equality test)
    // probe (SMH_STFT_PROBE_NOSTORE, tools/gpu/r2_fusion_bound.sh): magnitudes computed but not stored -- the cost of S's trip to HBM
    constexpr int M = 200, K = 201;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    v2 *tw = reinterpret_cast<v2 *>(lds);  // 8 rows of twiddles
    v2 *tw2 = tw + 8 * ROW;   // M + 1 untangle twiddles
    v2 *win2 = tw2 + (M + 2); // 8 rows: window as (w[2m], w[2m+1])
    v2 *Z = win2 + 8 * ROW;   // F frames of kMP400
    // (ROW == 40) table column of item `it` (= 25 f + n2): n2, + 25 behind a frame change inside the item's 16-lane group
    auto column = [&](int it, int f, int n2) { return ROW == 25 ? n2 : n2 + 25 * (f - (it & ~15) / 25); };
    // Workgroup -> (clip, frame tile).  ntiles > 0: a 1-D grid decoded so that NEIGHBOURING TILES RUN ON ONE XCD (smh_xcd.h has the
    // reasoning): the B * ntiles (clip, tile) items in clip-major order, one contiguous range per XCD.  ntiles == 0: the plain grid.
    // rag != nullptr (smh_rag.h): B work items of clips of DIFFERENT lengths, item n = (clip, tile) from the list, clip shapes and
    // offsets from the descriptor table; the items are in clip-major order and cut into the same 8 ranges.
    int b = blockIdx.y, tile = blockIdx.x;
    size_t clip_off, spec_off;
    unsigned n;
    if (rag) {
        if (!smh::xcd_item(B, n)) return;
        const smh_rag::Item item = items[n];
        b = item.clip, tile = item.tile;
        T = rag[b].T;
        clip_off = (size_t)rag[b].audio_off, spec_off = (size_t)rag[b].spec_off;
    } else {
        if (ntiles > 0) {
            if (!smh::xcd_item((unsigned)B * (unsigned)ntiles, n)) return;  // (the plan keeps B * ntiles below 2^31)
            b = (int)(n / (unsigned)ntiles), tile = (int)(n - (unsigned)b * (unsigned)ntiles);
        }
        clip_off = (size_t)b * n_samples, spec_off = (size_t)b * K * T;
    }
    const int t0 = tile * F, tid = threadIdx.x;
    const int nf = min(F, T - t0);
    const int nthr = blockDim.x;  // 256 or 512
    const float *clip = audio + clip_off + (size_t)t0 * hop;
    float *Sb = S + spec_off + t0;
    const int dq1 = nthr / 25, dr1 = nthr - dq1 * 25;
    // Phase 3 in FRAME PAIRS (below) wants the two frames of a pair in two conflict-free sets of LDS slots: frame f of the tile
    // lives in slot (f >> 1) + (f & 1) * (nf / 2).  Phases 1 and 2 only ever need the slot number.  A tile takes the pair form
    // when its two magnitudes are one aligned 8-byte store: nf, t0 and T even and the clip's S on an 8-byte boundary; any other
    // tile (odd T in a ragged call, T = 1, an odd tile under SMH_STFT_FRAMES) keeps slot = frame and one frame per item.
    const int nh = nf >> 1;
    const bool pair3 = pairs && ((nf | t0 | T) & 1) == 0 && (reinterpret_cast<uintptr_t>(Sb) & 7) == 0;
    auto slot_frame = [&](int s) { return pair3 ? (s < nh ? 2 * s : 2 * (s - nh) + 1) : s; };
    auto frame_slot = [&](int f) { return pair3 ? (f >> 1) + (f & 1) * nh : f; };
    // Phase 1, FIXED COLUMN form (pairs != 0 and the tile's slots fit kRounds1 rounds of nthr / 25 frame groups: nf <= 30 at 256
    // threads): thread tid owns column n2 = tid % 25 and frame group fg = tid / 25 and transforms the slots fg + r * (nthr / 25).
    // Its column of the window (8 pairs) and of the twiddles W_200^(n2 k1) (7) is the same in every round, so it comes straight
    // from memory into registers, requested together with the audio: no table in LDS, no staging loop, no barrier in front of
    // phase 1, and none of the 15 ds_read per item.  (The round-robin item map below gives a thread another column every round.)
    // Banks of the Z writes (ds_write_b64: groups of 16 lanes over 16 bank pairs, float2 offset 201 s + 25 k1 + n2): a group inside
    // one frame group holds 16 consecutive n2; one that straddles two holds n2 = a .. 24 of slot s and 0 .. a - 10 of slot s + 1,
    // i.e. a .. 24 and 201 + (0 .. a - 10) = 9 .. a - 1 (mod 16): 16 distinct pairs again.
    // Otherwise the audio is requested FIRST, for all of this thread's items at once (up to kRounds1 rounds of (frame, n2) items,
    // 8 float2 each), then the twiddle / window tables travel to LDS: one trip to memory per workgroup where there were
    // one for the tables and one per round (a round's loads used to be issued when the previous round's butterflies were done).
    constexpr int kRounds1 = 3;
    const bool fixed = pairs && nf <= kRounds1 * dq1;
    const bool ahead = !fixed && 25 * nf <= kRounds1 * nthr;
    v2 au[kRounds1][8];
    int fr_[kRounds1], n2_[kRounds1], col_[kRounds1];
    v2 wr[8], tr[8];
    if (fixed) {
        const int fg = tid / 25, n2 = tid - fg * 25;  // (fg == nthr / 25: the threads past the last whole group, idle in phase 1)
#pragma unroll
        for (int r = 0; r < kRounds1; ++r) {
            const int f = slot_frame(min(fg + r * dq1, nf - 1));
            const v2 *fr = reinterpret_cast<const v2 *>(clip + (unsigned)(f * hop));
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) au[r][n1] = fr[25 * n1 + n2];
        }
#pragma unroll
        for (int n1 = 0; n1 < 8; ++n1) wr[n1] = reinterpret_cast<const v2 *>(window)[25 * n1 + n2];
#pragma unroll
        for (int k1 = 1; k1 < 8; ++k1) tr[k1] = reinterpret_cast<const v2 *>(twM)[n2 * k1];
    } else if (ahead) {
        int f = tid / 25, n2 = tid - (tid / 25) * 25;
#pragma unroll
        for (int r = 0; r < kRounds1; ++r) {
            fr_[r] = f, n2_[r] = n2, col_[r] = column(tid + r * nthr, f, n2);
            const v2 *fr = reinterpret_cast<const v2 *>(clip + (unsigned)(min(f, nf - 1) * hop));
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) au[r][n1] = fr[25 * n1 + n2];
            n2 += dr1;
            const int carry = n2 >= 25 ? 1 : 0;
            n2 -= 25 * carry;
            f += dq1 + carry;
        }
    }
    // the untangle twiddles are first read in phase 3: one entry per thread (M + 1 <= nthr), written behind phase 1
    const v2 t2 = reinterpret_cast<const v2 *>(tw2M)[min(tid, M)];
    if (fixed) {
#pragma unroll
        for (int r = 0; r < kRounds1; ++r) {
            const int fg = tid / 25, s = fg + r * dq1;
            if (fg < dq1 && s < nf) {
#pragma unroll
                for (int n1 = 0; n1 < 8; ++n1) au[r][n1] = au[r][n1] * wr[n1];
                pk_dft8(au[r]);
                v2 *zf = Z + s * kMP400 + (tid - fg * 25);
                zf[0] = au[r][0];
#pragma unroll
                for (int k1 = 1; k1 < 8; ++k1) zf[k1 * 25] = cmulp(au[r][k1], tr[k1]);
            }
        }
    } else {
        // tw is stored by output index: tw[25 * k1 + n2] = W_200^(n2 k1), so that phase 1's lanes (n2 fastest) read consecutive
        // entries (indexed n2 * k1 the reads were strided by k1: up to 4 lanes per bank)
        // ROW == 40: a row holds its 25 entries and the first 15 again.  The table reads are ds_read2_b64, served in groups of 16
        // lanes over 32 banks, and a group in which the frame changes (n2 = a .. 24, 0 .. a - 10) meets itself in up to 7 banks --
        // 270 of the kernel's 720 conflict cycles per workgroup (simulated per phase; matches SQ_LDS_BANK_CONFLICT / 5120); with the
        // longer rows such a group reads entries a .. a + 15.
        for (int i = tid; i < 8 * ROW; i += nthr) {
            const int k1 = i / ROW, j = i - ROW * k1, n2 = j < 25 ? j : j - 25;
            tw[i] = reinterpret_cast<const v2 *>(twM)[n2 * k1];
            win2[i] = reinterpret_cast<const v2 *>(window)[25 * k1 + n2];
        }
        __syncthreads();
        auto butterfly1 = [&](v2 (&v)[8], int f, int n2, int j) {  // j: the item's table column
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) v[n1] = v[n1] * win2[ROW * n1 + j];
            pk_dft8(v);
            v2 *zf = Z + frame_slot(f) * kMP400 + n2;
            zf[0] = v[0];
#pragma unroll
            for (int k1 = 1; k1 < 8; ++k1) zf[k1 * 25] = cmulp(v[k1], tw[ROW * k1 + j]);
        };
        if (ahead) {
#pragma unroll
            for (int r = 0; r < kRounds1; ++r)
                if (fr_[r] < nf) butterfly1(au[r], fr_[r], n2_[r], col_[r]);
        } else {
            int it = tid;
            for (int f = tid / 25, n2 = tid - (tid / 25) * 25; f < nf; it += nthr) {
                const v2 *fr = reinterpret_cast<const v2 *>(clip + (unsigned)(f * hop));
                v2 v[8];
#pragma unroll
                for (int n1 = 0; n1 < 8; ++n1) v[n1] = fr[25 * n1 + n2];
                butterfly1(v, f, n2, column(it, f, n2));
                n2 += dr1;
                const int carry = n2 >= 25 ? 1 : 0;
                n2 -= 25 * carry;
                f += dq1 + carry;
            }
        }
    }
    if (tid <= M) tw2[tid] = t2;
    __syncthreads();
    // phase 2: read, barrier, compute, write in place (natural order); 8 * F <= blockDim.x items, one per (k1, SLOT).
    // Banks: the 25 reads of an item compile to ds_read2_b64, which LDS serves in groups of 16 consecutive lanes over 32
    // dword banks.  Items are laid out FRAMES FASTEST (item = k1 * nf + f): a 16-lane group then holds 16 frames of one k1, float2
    // offsets 201 f + 25 k1 + n2, and 201 = 9 (mod 16) is odd -- 16 distinct bank pairs.  (Round 2 had k1 fastest: 2 frames x 8 k1
    // per group, offsets 9 f + 9 k1 (mod 16), the two frames' sets meeting in 6 of 8 -- two-way conflicts on every access, and no
    // frame stride serves that layout and phase 3's frame-fastest lanes at once: 8 (mod 16) here against odd there.)  Only the
    // groups that straddle two k1 (nf is not a multiple of 16) still meet, in at most 3 of their 16 lanes.
    {
        const int k1 = tid / nf, f = tid - k1 * nf;
        const bool live = k1 < 8;
        v2 x[25];
        if (live) {
            const v2 *zf = Z + f * kMP400 + k1 * 25;
#pragma unroll
            for (int n2 = 0; n2 < 25; ++n2) x[n2] = zf[n2];
        }
        __syncthreads();
        if (live) {
            pk_dft25(x);
            v2 *zo = Z + f * kMP400 + k1;
#pragma unroll
            for (int k2 = 0; k2 < 25; ++k2) zo[8 * k2] = x[k2];
        }
    }
    __syncthreads();
    // phase 3: untangle + magnitude, one pair of bins (k, M - k) per item.
    // X[k] = (e - i g) / 2 and X[M-k] = conj(e + i g) / 2 with e = A + conj(B), g = tw2[k] (A - conj(B)):
    // one twiddle product serves both bins of the pair; the halving is exact, so it is taken on the magnitude
    auto untangle = [](v2 A, v2 Bz, v2 w, float &lo, float &hi) {
        const v2 e = add_conj(A, Bz), d = sub_conj(A, Bz);
        const v2 g = cmulp(d, w);
        const v2 x = sub_i(e, g);  // (e.x + g.y, e.y - g.x)
        lo = 0.5f * mag(x.x, x.y);
        const v2 y = add_i(e, g);  // (e.x - g.y, e.y + g.x)
        hi = 0.5f * mag(y.x, y.y);
    };
    if (pair3) {
        // Item it = k * (nf / 2) + fp: the frames 2 fp and 2 fp + 1 (slots fp and fp + nf / 2, both at the odd stride 201) share
        // the (k, fp) carry arithmetic, the tw2[k] read and the store offsets, and their magnitudes leave as one 8-byte store
        // per bin.  Frame pairs fastest, so the (K, T) stores stay contiguous along t.
        const int dq = nthr / nh, dr = nthr - dq * nh;
        int k = tid / nh, fp = tid - k * nh;
        for (; k <= M / 2;) {
            const v2 *z0 = Z + fp * kMP400, *z1 = z0 + nh * kMP400;
            const int kb = k == 0 ? 0 : M - k;
            const v2 w = tw2[k];
            float2 lo, hi;
            untangle(z0[k], z0[kb], w, lo.x, hi.x);
            untangle(z1[k], z1[kb], w, lo.y, hi.y);
            if (!probe || lo.x == -1.f) *reinterpret_cast<float2 *>(Sb + (unsigned)(k * T + 2 * fp)) = lo;
            if (k != M / 2 && (!probe || hi.x == -1.f)) *reinterpret_cast<float2 *>(Sb + (unsigned)((M - k) * T + 2 * fp)) = hi;
            fp += dr;
            const int carry = fp >= nh ? 1 : 0;
            fp -= carry * nh;
            k += dq + carry;
        }
        return;
    }
    // One frame per item, it = k * nf + f, frames fastest (contiguous stores);
    // (k, f) advance by (nthr / nf, nthr % nf) with a carry instead of a division per item, and every address is a 32-bit
    // offset from a uniform base: the item used to spend more instructions on 64-bit index arithmetic than on the butterfly.
    const int dq = nthr / nf, dr = nthr - dq * nf;
    int k = tid / nf, f = tid - k * nf;
    for (; k <= M / 2; ) {
        const v2 *zf = Z + f * kMP400;
        float lo, hi;
        untangle(zf[k], zf[k == 0 ? 0 : M - k], tw2[k], lo, hi);
        if (!probe || lo == -1.f) Sb[(unsigned)(k * T + f)] = lo;
        if (k != M / 2 && (!probe || hi == -1.f)) Sb[(unsigned)((M - k) * T + f)] = hi;
        f += dr;
        const int carry = f >= nf ? 1 : 0;
        f -= carry * nf;
        k += dq + carry;
    }
}

// the plan of smh_stft_mag_f32 for B clips of T >= 1 frames
StftPlan equal_plan(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int T) {
    return plan_equal(geom_of(ctx), read_stft_switches(), frames_aligned8(reinterpret_cast<uintptr_t>(d_audio), B, n_samples), B, T);
}
// plan p onto the stream: n_items items of a ragged call (d_clips != nullptr), else B = n_items clips of n_samples samples, T frames
int launch(const smh_ctx *ctx, const StftPlan &p, const float *d_audio, int n_items, int n_samples, int T, float *d_S,
           const smh_rag::Clip *d_clips, const smh_rag::Item *d_items, hipStream_t st) {
    SMH_REQUIRE(!p.refusal[0], "%s", p.refusal);
    const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
    if (p.kernel == kF64)
        return launch_f64(ctx, p, d_clips ? "stft_f64_kernel (ragged)" : "stft_f64_kernel", d_audio, n_items, n_samples, T, d_S, d_clips, d_items, st);
    if (p.kernel == kGeneric) {
        StftArgs a;
        a.n_fft = ctx->cfg.n_fft, a.hop = ctx->cfg.hop, a.M = ctx->M, a.K = ctx->K;
        fill_stages(ctx->radix, ctx->n_stages, a.M, a.st);
        a.n_samples = n_samples, a.T = T, a.tt = p.frames, a.inv_tt = 1.0f / (float)a.tt, a.B = n_items, a.xcd_tiles = p.xcd_tiles;
        return smh::launch_lds(stft_mag_kernel, d_clips ? "stft_mag_kernel (ragged)" : "stft_mag_kernel", grid, block, p.lds, p.lds, st, a, d_audio,
                               ctx->d_window, ctx->d_twM, ctx->d_tw2M, d_S, d_clips, d_items);
    }
    int row = 25, probe = 0;
    if (!d_clips) {  // the probes of an equal-length call: outputs invalid
        if (const char *ev = smh::probe_env("SMH_STFT_ROW")) row = atoi(ev) == 40 ? 40 : 25;
        probe = smh::probe_env("SMH_STFT_PROBE_NOSTORE") ? 1 : 0;  // timing experiment, S is not written
    }
    const size_t lds = lds400_bytes(row, p.frames);
    return smh::launch_lds(row == 25 ? stft400_kernel<25> : stft400_kernel<40>, d_clips ? "stft400_kernel (ragged)" : "stft400_kernel", grid, block,
                           lds, lds, st, d_audio, ctx->d_window, ctx->d_twM, ctx->d_tw2M, d_S, n_samples, ctx->cfg.hop, T, p.frames, probe, n_items,
                           p.xcd_tiles, p.pairs, d_clips, d_items);
}
}  // namespace

// One launch for clips of different lengths (smh_rag.h).  A frame's transform does not depend on the frames it shares a workgroup
// with, so every clip gets the bits smh_stft_mag_f32 gives it alone.
int smh_stft::launch_rag(const smh_ctx *ctx, const StftSwitches &sw, const float *d_audio, float *d_S, const smh_rag::Clip *d_clips,
                         const smh_rag::Item *d_items, int n_items, bool aligned8, hipStream_t st) {
    if (n_items <= 0) return SMH_OK;
    return launch(ctx, plan_rag(geom_of(ctx), sw, aligned8, n_items), d_audio, n_items, 0, 0, d_S, d_clips, d_items, st);
}

// tests: the kernel smh_stft_mag_f32 runs for this call (smh_stft_plan.h: Kernel; it does not depend on T), -1 for a null context
extern "C" int smh_internal_stft_route(const smh_ctx *ctx, const float *d_audio, int B, int n_samples) {
    return ctx ? equal_plan(ctx, d_audio, B, n_samples, 1).kernel : -1;
}
// tests: the plan (stft_plan_ints) of this smh_stft_mag_f32 call, or (ragged != 0) of launch_rag(aligned8, n_items), or its refusal
extern "C" int smh_internal_stft_plan(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int ragged, int aligned8, int n_items,
                                      int *out) {
    SMH_REQUIRE(ctx && out, "smh_internal_stft_plan: null argument");
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    SMH_REQUIRE(ragged || (B >= 1 && T >= 1), "smh_internal_stft_plan: bad shape");
    const StftPlan p = ragged ? plan_rag(geom_of(ctx), read_stft_switches(), aligned8 != 0, n_items) : equal_plan(ctx, d_audio, B, n_samples, T);
    SMH_REQUIRE(!p.refusal[0], "%s", p.refusal);
    stft_plan_ints(p, out);
    return SMH_OK;
}

extern "C" int smh_stft_mag_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, float *d_S, void *stream) {
    SMH_REQUIRE(ctx && (d_audio || B == 0) && (d_S || B == 0), "smh_stft_mag_f32: null argument");
    SMH_REQUIRE(B >= 0 && B <= 65535, "smh_stft_mag_f32: B=%d out of range", B);
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    SMH_REQUIRE(T >= 1, "smh_stft_mag_f32: clip of %d samples is shorter than n_fft=%d", n_samples, ctx->cfg.n_fft);
    if (B == 0) return SMH_OK;
    return launch(ctx, equal_plan(ctx, d_audio, B, n_samples, T), d_audio, B, n_samples, T, d_S, nullptr, nullptr, (hipStream_t)stream);
}
