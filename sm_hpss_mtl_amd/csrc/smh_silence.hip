// The step in front of the hot path: lib/preprocessing.py:330-350 load_and_preprocess_signal
// after the decode -- normalise, librosa.feature.rms, tools.removeSilence (lib/cython_impl/tools.pyx:42-134),
// normalise again -- batched over B equal-length clips that stay resident in HBM.
//
// All of it is streaming / integer work (a few passes over N samples per clip): the kernels are written for
// coalesced float loads and deterministic reductions, not for arithmetic.  The run detection is the reference's
// literal while-loop executed by one thread per clip (nFrames iterations of byte reads); everything around it is
// parallel over samples.
//
// Layout of this file: the host plan (frame arithmetic, route, workspace), the reference's rules as device functions,
// then the two routes that call them -- the stand-alone kernels of the multi-pass route and preprocess_fused_kernel,
// the clip-in-LDS route -- and the entries.  A rule is stated once; a kernel keeps where its tables live (HBM or LDS),
// how partial results cross waves and workgroups, its optional outputs and its summation order.
#include "smh_common.h"
#include "smh_wave.h"

#include <cstdlib>

namespace {

constexpr int kChunk = 8192;   // samples per workgroup in the streaming passes
constexpr int kThreads = 256;
constexpr int kFusedThreads = 1024;
constexpr int kFusedWaves = kFusedThreads / 64;
constexpr int kFusedMaxN = 36000;            // 144 KB of samples + tables within the 160 KB of one CU
constexpr size_t kFusedMaxLds = 155 * 1024;  // samples + tables of the clip-in-LDS kernel (short hops grow the tables)

// ---- the host plan: what the entries derive from (N, fs, Tw, Ts) or (N, frame_length, hop), stated once ----------
// tools.pyx:88-89: int((T*fs)/1000) -- true division, truncated
inline int ms_to_samples(int T_ms, int fs) { return (int)((double)T_ms * fs / 1000.0); }
// frames of librosa.feature.rms (centre=True): util.frame of the signal padded by frame/2 on both sides
inline int frame_count(int N, int frame, int hop) { return 1 + (N + 2 * (frame / 2) - frame) / hop; }
// An upper BOUND of frame_count for every frame >= 1 (equal for an even frame): the workspace is sized from (B, N, hop)
// alone, so its tables are sized by this, and smh_remove_silence_f32 accepts any nFrames up to it.
inline int frame_bound(int N, int hop) { return hop > 0 ? 1 + N / hop : 1; }
// runs that `frames` frames can hold (a run needs a silent and a loud frame), plus slack: rows of a run table
inline int max_runs(int frames) { return frames / 2 + 2; }

enum Reject { kAccepted = 0, kBadParams, kZeroFrame, kShortClip };

struct CondPlan {
    int frame, hop;   // frame size and shift in samples
    int nF;           // frame_count; 0 where the arguments are rejected
    int nF_bound;     // frame_bound >= nF
    int maxrun;       // max_runs(nF): the clip-in-LDS kernel's run table (the workspace's has max_runs(nF_bound) rows)
    size_t lds;       // dynamic LDS of preprocess_fused_kernel: samples, energies, run table, raw and filtered markers
    bool fused;       // the route of smh_preprocess_signal_f32: clip-in-LDS kernel, else multi-pass
    bool from_ms;     // built from (fs, Tw, Ts): words the messages
    Reject reject;
};

CondPlan plan_frames(int N, int frame, int hop, bool from_ms = false) {
    CondPlan p{};
    p.frame = frame, p.hop = hop, p.from_ms = from_ms;
    p.nF_bound = frame_bound(N, hop);
    if (frame < 1 || hop < 1) return p.reject = kZeroFrame, p;
    if (N <= frame / 2) return p.reject = kShortClip, p;  // reflect padding
    p.nF = frame_count(N, frame, hop);
    p.maxrun = max_runs(p.nF);
    p.lds = (size_t)((N + 3) & ~3) * 4 + (size_t)p.nF * 4 + (size_t)p.maxrun * 12 + 2 * (size_t)p.nF;
    // SMH_SILENCE_MULTIPASS (test hook) forces the general path; read on every call, the tests flip it within one process
    p.fused = N <= kFusedMaxN && getenv("SMH_SILENCE_MULTIPASS") == nullptr && p.lds <= kFusedMaxLds;
    return p;
}

CondPlan plan_ms(int N, int fs, int Tw, int Ts) {
    if (fs < 1 || Tw < 1 || Ts < 1) {
        CondPlan p{};
        return p.from_ms = true, p.reject = kBadParams, p;
    }
    return plan_frames(N, ms_to_samples(Tw, fs), ms_to_samples(Ts, fs), true);
}

int report(const char *fn, const CondPlan &p, int N) {
    switch (p.reject) {
    case kBadParams: return smh::set_error(SMH_E_INVALID, "%s: bad frame parameters", fn);
    case kZeroFrame:
        return smh::set_error(SMH_E_INVALID, p.from_ms ? "%s: frame size/shift round to zero samples"
                                                       : "%s: frame_length and hop must be >= 1", fn);
    case kShortClip:
        return smh::set_error(SMH_E_INVALID, "%s: reflect padding needs N > %s/2 (N=%d)", fn,
                              p.from_ms ? "frameSize" : "frame_length", N);
    default: return SMH_OK;
    }
}

struct SilWork {  // carved out of the caller's workspace
    double *psum;          // (B, R, nchunk) ordered partial sums of R rows per clip: normalise 1, mix_signals 2 (sized for 2)
    float *mean;           // (B)
    unsigned *absmax;      // (B) float bits of max|x-mean|   (max is order independent -> atomics are deterministic)
    unsigned *emax;        // (B) float bits of max(energy)
    int *nrun;             // (B)
    int *nkeep;            // (B)
    int *runs;             // (B, maxrun, 3): k, l, samples removed before this run
    float *fac;            // (B, 2) mixing factors of mix_signals, in the run table's slot (mix_signals finds no runs)
    unsigned char *raw;    // (B, nF) energy >= threshold
    unsigned char *fmark;  // (B, nF) after medfilt(., 5)
    float *energy;         // (B, nF)
    float *xn;             // (B, N) normalised signal of the fused entry point
    int nchunk, nF, maxrun;  // nF: the frame BOUND of (N, hop)
    size_t bytes;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// `hop` = N where the caller has no frames (normalise, mix_signals): the tables shrink to two frames.
SilWork carve(void *base, int B, int N, int hop, bool with_signal = true) {
    SilWork w{};
    w.nchunk = (N + kChunk - 1) / kChunk;
    if (w.nchunk < 1) w.nchunk = 1;
    w.nF = frame_bound(N, hop);
    w.maxrun = max_runs(w.nF);
    size_t off = 0;
    char *p = (char *)base;
    auto take = [&](size_t n) {
        char *q = p ? p + off : nullptr;
        off += align256(n);
        return (void *)q;
    };
    const size_t b = (size_t)(B > 0 ? B : 1);
    w.psum = (double *)take(2 * b * w.nchunk * sizeof(double));
    w.mean = (float *)take(b * sizeof(float));
    w.absmax = (unsigned *)take(b * sizeof(unsigned));
    w.emax = (unsigned *)take(b * sizeof(unsigned));
    w.nrun = (int *)take(b * sizeof(int));
    w.nkeep = (int *)take(b * sizeof(int));
    // one slot under two names: max_runs() >= 2 rows of three ints hold the two floats of a clip
    void *runs_or_fac = take(b * w.maxrun * 3 * sizeof(int));
    w.runs = (int *)runs_or_fac;
    w.fac = (float *)runs_or_fac;
    w.raw = (unsigned char *)take(b * w.nF);
    w.fmark = (unsigned char *)take(b * w.nF);
    w.energy = (float *)take(b * w.nF * sizeof(float));
    w.xn = with_signal ? (float *)take(b * (size_t)N * sizeof(float)) : nullptr;
    w.bytes = off;
    return w;
}

// carve, check the caller's size, report under the entry's name
int take_work(const char *fn, void *d_work, size_t work_bytes, int B, int N, int hop, bool with_signal, SilWork &w) {
    w = carve(d_work, B, N, hop, with_signal);
    if (work_bytes < w.bytes)
        return smh::set_error(SMH_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", fn, work_bytes, w.bytes);
    return SMH_OK;
}

// ---- wave reductions (smh_wave.h: the xor-tree f64 sum; the DPP wave_sum_f adds in another order and is not used here) --
using smh::wave_sum;
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- the rules, each called from both routes ------------------------------------------------------------------------
// Table parameters are plain pointers; every call is inlined, and the clip-in-LDS kernel still reads its tables with ds_
// instructions, none with flat_ ones (profiles/r20_silence_rules.txt).

// np.max(|x - mean|) of the values one lane walks: max with NaN propagation.  How lanes, waves and workgroups are
// combined is the kernel's (wave_max + atomics on the bits, or block_absmax); nan_max() is the one NaN rule.
__device__ __forceinline__ bool absmax_take(float d, float &m) {  // m = max(m, |d|); true if d is NaN (fmaxf drops it)
    const float a = fabsf(d);
    m = fmaxf(m, a);
    return a != a;
}
__device__ __forceinline__ float nan_max(float m, bool any_nan) { return any_nan ? __uint_as_float(0x7fc00000u) : m; }

// np.max(energy) on bit patterns: bit pattern order == value order for the non-negative energies; NaN sorts highest
__device__ __forceinline__ unsigned energy_bits(float e) { return __float_as_uint(e) & 0x7fffffffu; }

// librosa.feature.rms, one frame by one wave (centre=True, reflect padding): lane-strided fmaf, xor-tree sum; the energy in
// every lane
__device__ __forceinline__ float frame_rms(const float *y, int N, int t, int frame, int hop, int lane) {
    const int base = t * hop - frame / 2;
    float s = 0.f;
    for (int i = lane; i < frame; i += 64) {
        int src = base + i;
        if (src < 0) src = -src;
        if (src >= N) src = 2 * (N - 1) - src;
        const float v = y[src];
        s = fmaf(v, v, s);
    }
    return sqrtf(wave_sum(s) / (float)frame);
}

// tools.pyx:93 `cdef float energyThresh = alpha * np.max(energy)`: double product (numpy 1.19 promotes the
// float32 scalar times a Python float to float64) stored into a C float
__device__ __forceinline__ float energy_thresh(double alpha, unsigned emax_bits) {
    return (float)(alpha * (double)__uint_as_float(emax_bits));
}
__device__ __forceinline__ unsigned char raw_mark(float e, float thresh) { return e >= thresh ? 1 : 0; }
// medfilt(marker, 5) with zero padding, frame i: the median of five 0/1 values
__device__ __forceinline__ unsigned char mark_frame(const unsigned char *raw, int nF, int i) {
    int c = 0;
#pragma unroll
    for (int d = -2; d <= 2; ++d) {
        const int j = i + d;
        c += (j >= 0 && j < nF) ? raw[j] : 0;
    }
    return c >= 3 ? 1 : 0;
}

// tools.pyx:126: with fewer than two runs nothing is removed and the input is returned as is
__device__ __forceinline__ bool runs_remove(int n) { return n > 1; }

// The reference's run loop, by one thread: (k, l, samples removed before this run) per run that passes beta, at most
// maxrun of them.
struct Runs {
    int n, n_keep;
};
__device__ __forceinline__ Runs find_runs(const unsigned char *fm, int nF, int N, int frameSize, int frameShift, int fs,
                                          double beta, int maxrun, int *runs) {
    int n = 0, removed = 0;
    int i = 0;
    while (i < nF) {  // tools.pyx:101-123, literally
        while (fm[i] == 1) {
            if (i == nF - 1) break;
            ++i;
        }
        int j = i;
        while (fm[j] == 0) {
            if (j == nF - 1) break;
            ++j;
        }
        const int k = max(frameShift * (i - 1) + frameSize, 1);
        const int l = min(frameShift * (j - 1) + frameSize, N);
        if ((double)(l - k) / (double)fs > beta && n < maxrun) {
            runs[3 * n] = k;
            runs[3 * n + 1] = l;
            runs[3 * n + 2] = removed;
            removed += l - k;
            ++n;
        }
        i = j + 1;
    }
    return Runs{n, runs_remove(n) ? N - removed : N};
}

// Where sample s goes when the first n runs are cut out (kept samples move left by the number of removed samples before
// them), or -1 if it lies in one of them.
__device__ __forceinline__ int compacted_index(const int *runs, int n, int s) {
    int a = -1, z = n - 1;  // last run with k <= s
    while (a < z) {
        const int mid = (a + z + 1) >> 1;
        if (runs[3 * mid] <= s) a = mid; else z = mid - 1;
    }
    if (a < 0) return s;
    const int k = runs[3 * a], l = runs[3 * a + 1];
    const bool in_run = s < l;
    const int before = runs[3 * a + 2] + (in_run ? 0 : l - k);
    return in_run ? -1 : s - before;
}

// Ordered two-level f64 sum of R rows per clip (fixed tree -> bit-reproducible from run to run).  Level 1: a workgroup of
// kThreads folds its threads' sums of one chunk into psum[b][r][c]; level 2: one wave folds a clip's chunks, every lane gets
// the sums.
template <int R>
__device__ __forceinline__ void chunk_sums(double (&s)[R], int b, int c, int nchunk, double *psum) {
    __shared__ double sh[R][kThreads / 64];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        s[r] = wave_sum(s[r]);
        if ((threadIdx.x & 63) == 0) sh[r][threadIdx.x >> 6] = s[r];
    }
    __syncthreads();
    if (threadIdx.x < R) {
        double t = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) t += sh[threadIdx.x][w];
        psum[((size_t)b * R + threadIdx.x) * nchunk + c] = t;
    }
}
template <int R>
__device__ __forceinline__ void fold_chunks(const double *psum, int b, int nchunk, double (&s)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = 0.0;
    for (int c = threadIdx.x; c < nchunk; c += 64) {
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += psum[((size_t)b * R + r) * nchunk + c];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = wave_sum(s[r]);
}

// ---- normalise: x -= mean(x); x /= max|x|  (preprocessing.py:332-333, 348-349) ---------------------------------
// pass 1: ordered f64 partial sums per chunk
__global__ __launch_bounds__(kThreads) void sum_chunks_kernel(const float *__restrict__ x, int N, int nchunk,
                                                              double *__restrict__ psum) {
    const int b = blockIdx.y, c = blockIdx.x;
    const float *xb = x + (size_t)b * N;
    const int lo = c * kChunk, hi = min(N, lo + kChunk);
    double s[1] = {0.0};
    for (int i = lo + threadIdx.x; i < hi; i += kThreads) s[0] += (double)xb[i];
    chunk_sums<1>(s, b, c, nchunk, psum);
}

// pass 1b: one wave per clip folds the partials in a fixed order; also resets the max accumulators
__global__ __launch_bounds__(64) void mean_kernel(const double *__restrict__ psum, int N, int nchunk,
                                                  float *__restrict__ mean, unsigned *__restrict__ absmax) {
    const int b = blockIdx.x;
    double s[1];
    fold_chunks<1>(psum, b, nchunk, s);
    if (threadIdx.x == 0) {
        mean[b] = (float)(s[0] / (double)N);
        absmax[b] = 0u;
    }
}

// pass 2: max |x - mean| (float bits of a non-negative float order like unsigned integers)
__global__ __launch_bounds__(kThreads) void absmax_kernel(const float *__restrict__ x, int N,
                                                          const float *__restrict__ mean,
                                                          unsigned *__restrict__ absmax) {
    const int b = blockIdx.y;
    const float *xb = x + (size_t)b * N;
    const float mu = mean[b];
    const int lo = blockIdx.x * kChunk, hi = min(N, lo + kChunk);
    float m = 0.f;
    bool nan = false;
    for (int i = lo + threadIdx.x; i < hi; i += kThreads) nan |= absmax_take(xb[i] - mu, m);
    m = wave_max(m);
    m = nan_max(m, __any(nan));
    if ((threadIdx.x & 63) == 0) atomicMax(&absmax[b], __float_as_uint(m));
}

// pass 3: write (x - mean) / max  (IEEE division, like numpy)
__global__ __launch_bounds__(kThreads) void normalize_write_kernel(const float *__restrict__ x, int N,
                                                                   const float *__restrict__ mean,
                                                                   const unsigned *__restrict__ absmax,
                                                                   float *__restrict__ out) {
    const int b = blockIdx.y;
    const float *xb = x + (size_t)b * N;
    float *ob = out + (size_t)b * N;
    const float mu = mean[b];
    const float m = __uint_as_float(absmax[b]);
    const int lo = blockIdx.x * kChunk, hi = min(N, lo + kChunk);
    for (int i = lo + threadIdx.x; i < hi; i += kThreads) ob[i] = __fdiv_rn(xb[i] - mu, m);
}

// ---- librosa.feature.rms(y, frame_length, hop_length) ------------------------------------------------------------
// One wave per frame; the clip maximum of the energy (tools.pyx:93) is folded in.
__global__ __launch_bounds__(kThreads) void rms_kernel(const float *__restrict__ y, int N, int frame_length, int hop,
                                                       int nF, float *__restrict__ energy,
                                                       unsigned *__restrict__ emax) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (t >= nF) return;
    const int lane = threadIdx.x & 63;
    const float e = frame_rms(y + (size_t)b * N, N, t, frame_length, hop, lane);
    if (lane == 0) {
        energy[(size_t)b * nF + t] = e;
        if (emax) atomicMax(&emax[b], energy_bits(e));
    }
}

__global__ void zero_u32_kernel(unsigned *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0u;
}

__global__ __launch_bounds__(kThreads) void energy_max_kernel(const float *__restrict__ energy, int nF,
                                                              unsigned *__restrict__ emax) {
    const int b = blockIdx.x;
    unsigned m = 0u;
    for (int i = threadIdx.x; i < nF; i += kThreads) m = max(m, energy_bits(energy[(size_t)b * nF + i]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&emax[b], m);
}

// ---- tools.removeSilence ------------------------------------------------------------------------------------
// One workgroup per clip: threshold marker, medfilt(marker, 5), then the run loop; tables in HBM.
__global__ __launch_bounds__(kThreads) void silence_runs_kernel(const float *__restrict__ energy, int nF, int N,
                                                                const unsigned *__restrict__ emax, double alpha,
                                                                double beta, int fs, int frameSize, int frameShift,
                                                                int maxrun, unsigned char *__restrict__ raw,
                                                                unsigned char *__restrict__ fmark,
                                                                int *__restrict__ frame_marker_out,
                                                                int *__restrict__ runs, int *__restrict__ nrun,
                                                                int *__restrict__ nkeep) {
    const int b = blockIdx.x;
    const float *e = energy + (size_t)b * nF;
    unsigned char *rw = raw + (size_t)b * nF;
    unsigned char *fm = fmark + (size_t)b * nF;
    const float thresh = energy_thresh(alpha, emax[b]);
    for (int i = threadIdx.x; i < nF; i += kThreads) rw[i] = raw_mark(e[i], thresh);
    __syncthreads();
    for (int i = threadIdx.x; i < nF; i += kThreads) {
        const unsigned char m = mark_frame(rw, nF, i);
        fm[i] = m;
        if (frame_marker_out) frame_marker_out[(size_t)b * nF + i] = m;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const Runs r = find_runs(fm, nF, N, frameSize, frameShift, fs, beta, maxrun, runs + (size_t)b * maxrun * 3);
    nrun[b] = r.n;
    nkeep[b] = r.n_keep;
}

// Compaction: the tail keeps the 1.0 of the reference's np.ones() initialisation (tools.pyx:126-131).  The sample marker
// shows every run, also where nothing is removed.
__global__ __launch_bounds__(kThreads) void silence_compact_kernel(const float *__restrict__ x, int N, int maxrun,
                                                                   const int *__restrict__ runs,
                                                                   const int *__restrict__ nrun,
                                                                   const int *__restrict__ nkeep,
                                                                   float *__restrict__ out,
                                                                   unsigned char *__restrict__ sample_marker) {
    const int b = blockIdx.y;
    const int *rb = runs + (size_t)b * maxrun * 3;
    const int n = nrun[b];
    const int keep = nkeep[b];
    const float *xb = x + (size_t)b * N;
    float *ob = out + (size_t)b * N;
    const int lo = blockIdx.x * kChunk, hi = min(N, lo + kChunk);
    for (int s = lo + threadIdx.x; s < hi; s += kThreads) {
        const int dst = compacted_index(rb, n, s);
        if (sample_marker) sample_marker[(size_t)b * N + s] = dst < 0 ? 0 : 1;
        if (runs_remove(n)) {
            if (dst >= 0) ob[dst] = xb[s];
            if (s >= keep) ob[s] = 1.0f;
        } else {
            ob[s] = xb[s];
        }
    }
}

// ---- fused form of preprocessing.py:332-349 for clips that fit in LDS (CondPlan::fused) --------------------------
// One workgroup per clip: the clip is read from HBM once into LDS, every later pass (mean, max, rms frames, marker,
// run loop, compaction, second normalisation) works out of LDS, and the result is written once: 8 bytes of HBM
// traffic per sample instead of the ~40 of the multi-pass path.  The rules are the functions above; its own are the tables
// in LDS, the float4 load, the block reductions (its f64 block sum is another order than the chunked sum, on purpose) and
// the second normalisation taken over the samples where they lie, before they move.
struct BlockScratch {
    double d[kFusedWaves];
    float f[kFusedWaves];
    int flag[kFusedWaves];
    float bcast_f[2];
    double bcast_d;
    int nrun, nkeep;
};

__device__ __forceinline__ double block_sum(double v, BlockScratch &sc) {
    v = wave_sum(v);
    __syncthreads();  // scratch reuse
    if ((threadIdx.x & 63) == 0) sc.d[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kFusedWaves; ++w) t += sc.d[w];  // every thread folds in the same fixed order
    return t;
}

// absmax_take's pair across the workgroup: NaN if any lane saw one
__device__ __forceinline__ float block_absmax(float m, bool nan, BlockScratch &sc) {
    m = wave_max(m);
    const int anynan = __any(nan) ? 1 : 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sc.f[threadIdx.x >> 6] = m;
        sc.flag[threadIdx.x >> 6] = anynan;
    }
    __syncthreads();
    float t = 0.f;
    int fl = 0;
#pragma unroll
    for (int w = 0; w < kFusedWaves; ++w) {
        t = fmaxf(t, sc.f[w]);
        fl |= sc.flag[w];
    }
    return nan_max(t, fl != 0);
}

__global__ __launch_bounds__(kFusedThreads) void preprocess_fused_kernel(const float *__restrict__ x, int N,
                                                                         int frameSize, int frameShift, int nF,
                                                                         int maxrun, int fs, double alpha, double beta,
                                                                         float *__restrict__ out,
                                                                         int *__restrict__ n_keep) {
    extern __shared__ __align__(16) unsigned char lds_raw[];  // CondPlan::lds
    float *xs = (float *)lds_raw;                       // (N) rounded up to a multiple of 4
    const int Np = (N + 3) & ~3;
    float *en = xs + Np;                                // (nF)
    int *runs = (int *)(en + nF);                       // (maxrun, 3)
    unsigned char *raw = (unsigned char *)(runs + 3 * maxrun);  // (nF)
    unsigned char *fm = raw + nF;                       // (nF)
    __shared__ BlockScratch sc;

    const int b = blockIdx.x, tid = threadIdx.x;
    const float *xb = x + (size_t)b * N;
    float *ob = out + (size_t)b * N;

    // 1. HBM -> LDS, f64 sum
    double s = 0.0;
    if ((N & 3) == 0) {
        const float4 *x4 = (const float4 *)xb;
        for (int i = tid; i < N / 4; i += kFusedThreads) {
            const float4 v = x4[i];
            ((float4 *)xs)[i] = v;
            s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        }
    } else {
        for (int i = tid; i < N; i += kFusedThreads) {
            const float v = xb[i];
            xs[i] = v;
            s += (double)v;
        }
    }
    const float mu = (float)(block_sum(s, sc) / (double)N);
    // 2. x - mean, max |.|
    float m = 0.f;
    bool nan = false;
    for (int i = tid; i < N; i += kFusedThreads) {
        const float d = xs[i] - mu;
        xs[i] = d;
        nan |= absmax_take(d, m);
    }
    const float mx = block_absmax(m, nan, sc);
    for (int i = tid; i < N; i += kFusedThreads) xs[i] = __fdiv_rn(xs[i], mx);
    __syncthreads();
    // 3. rms frames, one wave per frame; the maximum crosses the waves through the scratch
    const int lane = tid & 63, wave = tid >> 6;
    unsigned emax_bits = 0u;
    for (int t = wave; t < nF; t += kFusedWaves) {
        const float e = frame_rms(xs, N, t, frameSize, frameShift, lane);
        if (lane == 0) en[t] = e;
        emax_bits = max(emax_bits, energy_bits(e));
    }
    __syncthreads();
    if (lane == 0) sc.flag[wave] = (int)emax_bits;
    __syncthreads();
    unsigned eb = 0u;
#pragma unroll
    for (int w = 0; w < kFusedWaves; ++w) eb = max(eb, (unsigned)sc.flag[w]);
    const float thresh = energy_thresh(alpha, eb);
    // 4. marker, medfilt(., 5), run loop
    for (int i = tid; i < nF; i += kFusedThreads) raw[i] = raw_mark(en[i], thresh);
    __syncthreads();
    for (int i = tid; i < nF; i += kFusedThreads) fm[i] = mark_frame(raw, nF, i);
    __syncthreads();
    if (tid == 0) {
        const Runs r = find_runs(fm, nF, N, frameSize, frameShift, fs, beta, maxrun, runs);
        sc.nrun = r.n;
        sc.nkeep = r.n_keep;
    }
    __syncthreads();
    const int n = runs_remove(sc.nrun) ? sc.nrun : 0;
    const int keep = sc.nkeep;
    if (tid == 0 && n_keep) n_keep[b] = keep;
    // 5. second normalisation over [retained samples..., 1.0 tail]
    double s2 = 0.0;
    for (int i = tid; i < N; i += kFusedThreads)
        if (compacted_index(runs, n, i) >= 0) s2 += (double)xs[i];
    const double tail = (double)(N - keep);
    const float mu2 = (float)((block_sum(s2, sc) + tail) / (double)N);
    float m2 = 0.f;
    bool nan2 = false;
    for (int i = tid; i < N; i += kFusedThreads)
        if (compacted_index(runs, n, i) >= 0) nan2 |= absmax_take(xs[i] - mu2, m2);
    if (keep < N) m2 = fmaxf(m2, fabsf(1.0f - mu2));
    const float mx2 = block_absmax(m2, nan2, sc);
    const float tailv = __fdiv_rn(1.0f - mu2, mx2);
    for (int i = tid; i < N; i += kFusedThreads) {
        const int dsti = compacted_index(runs, n, i);
        if (dsti >= 0) ob[dsti] = __fdiv_rn(xs[i] - mu2, mx2);
        if (i >= keep) ob[i] = tailv;
    }
}

// ---- mix_signals (preprocessing.py:297-325): music looped to the speech length, scaled to the target SMR --------
// pass 1: ordered f64 partial sums of sp^2 and (looped mu)^2 per chunk
__global__ __launch_bounds__(kThreads) void mix_energy_kernel(const float *__restrict__ sp, const float *__restrict__ mu,
                                                              int N, int Nmu, int nchunk, double *__restrict__ psum) {
    const int b = blockIdx.y, c = blockIdx.x;
    const float *s = sp + (size_t)b * N, *m = mu + (size_t)b * Nmu;
    const int lo = c * kChunk, hi = min(N, lo + kChunk);
    double e[2] = {0.0, 0.0};  // speech, music
    for (int i = lo + threadIdx.x; i < hi; i += kThreads) {
        const double a = s[i], v = m[i % Nmu];
        e[0] += a * a;
        e[1] += v * v;
    }
    chunk_sums<2>(e, b, c, nchunk, psum);
}

// pass 2: the two mixing factors per clip (float32, like the float32 audio of the reference)
__global__ __launch_bounds__(64) void mix_factor_kernel(const double *__restrict__ psum, int N, int nchunk,
                                                        const float *__restrict__ target_db, float *__restrict__ fac) {
    const int b = blockIdx.x;
    double e[2];
    fold_chunks<2>(psum, b, nchunk, e);
    if (threadIdx.x == 0) {
        const double e_sp = e[0] / N, e_mu = e[1] / N;
        const double req = e_sp / pow(10.0, (double)target_db[b] / 10.0);
        double f_mu = sqrt(req / e_mu), f_sp = 1.0;
        const double sum = f_mu + f_sp;
        f_mu /= sum, f_sp /= sum;
        fac[2 * b] = (float)f_sp;
        fac[2 * b + 1] = (float)f_mu;
    }
}

// pass 3: mix = f_sp * sp + f_mu * mu  (two roundings, as numpy evaluates it)
__global__ __launch_bounds__(kThreads) void mix_write_kernel(const float *__restrict__ sp, const float *__restrict__ mu,
                                                             int N, int Nmu, const float *__restrict__ fac,
                                                             float *__restrict__ out) {
    const int b = blockIdx.y;
    const float *s = sp + (size_t)b * N, *m = mu + (size_t)b * Nmu;
    float *o = out + (size_t)b * N;
    const float fs = fac[2 * b], fm = fac[2 * b + 1];
    const int lo = blockIdx.x * kChunk, hi = min(N, lo + kChunk);
    for (int i = lo + threadIdx.x; i < hi; i += kThreads) o[i] = __fadd_rn(__fmul_rn(fs, s[i]), __fmul_rn(fm, m[i % Nmu]));
}

int check_common(const char *fn, const void *d_x, int B, int N) {
    SMH_REQUIRE(B >= 0 && B <= 65535, "%s: B must be in [0, 65535]", fn);
    SMH_REQUIRE(N >= 1, "%s: N must be >= 1", fn);
    SMH_REQUIRE(d_x || B == 0, "%s: null input", fn);
    return SMH_OK;
}

int launch_normalize(const float *d_x, int B, int N, float *d_out, const SilWork &w, hipStream_t st) {
    const dim3 grid(w.nchunk, B);
    hipLaunchKernelGGL(sum_chunks_kernel, grid, dim3(kThreads), 0, st, d_x, N, w.nchunk, w.psum);
    hipLaunchKernelGGL(mean_kernel, dim3(B), dim3(64), 0, st, w.psum, N, w.nchunk, w.mean, w.absmax);
    hipLaunchKernelGGL(absmax_kernel, grid, dim3(kThreads), 0, st, d_x, N, w.mean, w.absmax);
    hipLaunchKernelGGL(normalize_write_kernel, grid, dim3(kThreads), 0, st, d_x, N, w.mean, w.absmax, d_out);
    return smh::launch_status("normalize kernels");
}

int launch_rms(const float *d_y, int B, int N, const CondPlan &p, float *d_energy, unsigned *emax, hipStream_t st) {
    if (emax) hipLaunchKernelGGL(zero_u32_kernel, dim3((B + 255) / 256), dim3(256), 0, st, emax, B);
    hipLaunchKernelGGL(rms_kernel, dim3((p.nF + 3) / 4, B), dim3(kThreads), 0, st, d_y, N, p.frame, p.hop, p.nF, d_energy,
                       emax);
    return smh::launch_status("rms_kernel");
}

// nF: the caller's frame count (any up to the workspace's bound), not necessarily the plan's
int launch_remove(const float *d_x, int B, int N, const float *d_energy, int nF, int fs, const CondPlan &p, double alpha,
                  double beta, float *d_out, unsigned char *d_sample_marker, int *d_frame_marker, int *d_n_keep,
                  const SilWork &w, bool emax_ready, hipStream_t st) {
    if (!emax_ready) {
        hipLaunchKernelGGL(zero_u32_kernel, dim3((B + 255) / 256), dim3(256), 0, st, w.emax, B);
        hipLaunchKernelGGL(energy_max_kernel, dim3(B), dim3(kThreads), 0, st, d_energy, nF, w.emax);
    }
    hipLaunchKernelGGL(silence_runs_kernel, dim3(B), dim3(kThreads), 0, st, d_energy, nF, N, w.emax, alpha, beta, fs,
                       p.frame, p.hop, w.maxrun, w.raw, w.fmark, d_frame_marker, w.runs, w.nrun, w.nkeep);
    hipLaunchKernelGGL(silence_compact_kernel, dim3(w.nchunk, B), dim3(kThreads), 0, st, d_x, N, w.maxrun, w.runs,
                       w.nrun, w.nkeep, d_out, d_sample_marker);
    if (d_n_keep)
        (void)hipMemcpyAsync(d_n_keep, w.nkeep, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, st);
    return smh::launch_status("remove-silence kernels");
}

}  // namespace

extern "C" size_t smh_silence_workspace_bytes(int B, int N, int hop) {
    if (B < 0 || N < 1 || hop < 1) return 0;
    return carve(nullptr, B, N, hop).bytes;
}

extern "C" size_t smh_normalize_workspace_bytes(int B, int N) {
    if (B < 0 || N < 1) return 0;
    return carve(nullptr, B, N, N, false).bytes;
}

extern "C" int smh_normalize_f32(const float *d_x, int B, int N, float *d_out, void *d_work, size_t work_bytes,
                                 void *stream) {
    if (int rc = check_common("smh_normalize_f32", d_x, B, N)) return rc;
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(d_out && d_work, "smh_normalize_f32: null output or workspace");
    SilWork w;
    if (int rc = take_work("smh_normalize_f32", d_work, work_bytes, B, N, N, false, w)) return rc;
    return launch_normalize(d_x, B, N, d_out, w, (hipStream_t)stream);
}

extern "C" int smh_rms_f32(const float *d_y, int B, int N, int frame_length, int hop, float *d_energy, void *stream) {
    if (int rc = check_common("smh_rms_f32", d_y, B, N)) return rc;
    const CondPlan p = plan_frames(N, frame_length, hop);
    if (int rc = report("smh_rms_f32", p, N)) return rc;
    if (B == 0) return p.nF;
    SMH_REQUIRE(d_energy, "smh_rms_f32: null output");
    if (int rc = launch_rms(d_y, B, N, p, d_energy, nullptr, (hipStream_t)stream)) return rc;
    return p.nF;
}

extern "C" int smh_remove_silence_f32(const float *d_x, int B, int N, const float *d_energy, int nFrames, int fs,
                                      int Tw, int Ts, double alpha, double beta, float *d_out,
                                      unsigned char *d_sample_marker, int *d_frame_marker, int *d_n_keep,
                                      void *d_work, size_t work_bytes, void *stream) {
    const char *fn = "smh_remove_silence_f32";
    if (int rc = check_common(fn, d_x, B, N)) return rc;
    // the energy is the caller's: of the plan's checks only the parameters and the shift concern this entry (a frame size
    // of zero samples and a clip too short for rms are accepted, as they were)
    const CondPlan p = plan_ms(N, fs, Tw, Ts);
    SMH_REQUIRE(nFrames >= 1 && p.reject != kBadParams, "%s: bad frame parameters", fn);
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(d_energy && d_out && d_work, "%s: null argument", fn);
    SMH_REQUIRE(d_out != d_x, "%s: in-place operation is not supported", fn);
    SMH_REQUIRE(p.hop >= 1, "%s: frame shift rounds to zero samples", fn);
    SMH_REQUIRE(nFrames <= p.nF_bound, "%s: nFrames=%d exceeds 1 + N/hop = %d", fn, nFrames, p.nF_bound);
    SilWork w;
    if (int rc = take_work(fn, d_work, work_bytes, B, N, p.hop, true, w)) return rc;
    return launch_remove(d_x, B, N, d_energy, nFrames, fs, p, alpha, beta, d_out, d_sample_marker, d_frame_marker, d_n_keep,
                         w, false, (hipStream_t)stream);
}

extern "C" int smh_preprocess_signal_f32(const float *d_x, int B, int N, int fs, int Tw, int Ts, float *d_out,
                                         int *d_n_keep, void *d_work, size_t work_bytes, void *stream) {
    const char *fn = "smh_preprocess_signal_f32";
    if (int rc = check_common(fn, d_x, B, N)) return rc;
    const CondPlan p = plan_ms(N, fs, Tw, Ts);
    if (int rc = report(fn, p, N)) return rc;
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(d_out && d_work, "%s: null output or workspace", fn);
    SMH_REQUIRE(d_out != d_x, "%s: in-place operation is not supported", fn);
    hipStream_t st = (hipStream_t)stream;
    if (p.fused) {  // clip fits in LDS: one read, one write
        SMH_CHECK_HIP(hipFuncSetAttribute((const void *)preprocess_fused_kernel,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        hipLaunchKernelGGL(preprocess_fused_kernel, dim3(B), dim3(kFusedThreads), p.lds, st, d_x, N, p.frame, p.hop, p.nF,
                           p.maxrun, fs, 0.025, 0.075, d_out, d_n_keep);
        return smh::launch_status("preprocess_fused_kernel");
    }
    SilWork w;
    if (int rc = take_work(fn, d_work, work_bytes, B, N, p.hop, true, w)) return rc;
    SMH_REQUIRE(p.nF <= w.nF, "%s: internal frame count mismatch", fn);
    if (int rc = launch_normalize(d_x, B, N, w.xn, w, st)) return rc;                 // :332-333
    if (int rc = launch_rms(w.xn, B, N, p, w.energy, w.emax, st)) return rc;          // :338
    if (int rc = launch_remove(w.xn, B, N, w.energy, p.nF, fs, p, 0.025, 0.075, d_out, nullptr, nullptr, d_n_keep, w, true,
                               st))
        return rc;                                                                    // :339
    return launch_normalize(d_out, B, N, d_out, w, st);                               // :348-349
}

// Test-only (not in include/smh.h): the route smh_preprocess_signal_f32 takes for these arguments in this process --
// 1 = clip-in-LDS kernel, 0 = multi-pass, -1 = arguments the call itself rejects.
extern "C" int smh_internal_preprocess_route(int N, int fs, int Tw, int Ts) {
    if (N < 1) return -1;
    const CondPlan p = plan_ms(N, fs, Tw, Ts);
    return p.reject ? -1 : p.fused ? 1 : 0;
}

extern "C" int smh_mix_signals_f32(const float *d_sp, const float *d_mu, int B, int N, int N_mu, const float *d_target_db,
                                   float *d_out, void *d_work, size_t work_bytes, void *stream) {
    if (int rc = check_common("smh_mix_signals_f32", d_sp, B, N)) return rc;
    SMH_REQUIRE(N_mu >= 1, "smh_mix_signals_f32: empty music signal");
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(d_mu && d_target_db && d_out && d_work, "smh_mix_signals_f32: null argument");
    SilWork w;
    if (int rc = take_work("smh_mix_signals_f32", d_work, work_bytes, B, N, N, false, w)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(w.nchunk, B);
    hipLaunchKernelGGL(mix_energy_kernel, grid, dim3(kThreads), 0, st, d_sp, d_mu, N, N_mu, w.nchunk, w.psum);
    hipLaunchKernelGGL(mix_factor_kernel, dim3(B), dim3(64), 0, st, w.psum, N, w.nchunk, d_target_db, w.fac);
    hipLaunchKernelGGL(mix_write_kernel, grid, dim3(kThreads), 0, st, d_sp, d_mu, N, N_mu, w.fac, d_out);
    if (int rc = smh::launch_status("mix kernels")) return rc;
    return launch_normalize(d_out, B, N, d_out, w, st);  // preprocessing.py:323 normalize_signal(Xin_mix)
}
