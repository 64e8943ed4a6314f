// The skewness-vector feed (PARAMS['skewness_vector'] = 'Row' / 'Col', Proposed_Work_Results.py:97-113, 475-481): the statistic
// tools.get_data_statistics (lib/cython_impl/tools.pyx:169-215) takes of every patch, computed straight from featuregrams that are
// ALREADY on the device -- (rows, T_b) float32, dense, as run_ragged(W = None) and the device featuregram cache hold them (the table
// of smh_fvtable.h).  No patch is ever written: a call reads the featuregrams and writes nP * rows (axis 1) or nP * W (axis 0) numbers.
//
// The value under the statistic is the patch element the existing entries write, bit for bit: without statistics the per-file
// StandardScaler value of smh_standardize_rows_f32 (row_stats + standardize of smh_feat.h, over the file's own T frames), with
// d_mean / d_stdev smh_scaled_patches_f32's (float)(((double)x - mean[r]) / (stdev[r] + 1e-10)).  The statistic itself is float64
// and two-pass, statistic() of smh_tools.hip restated: the mean first, then the central moments of x - mean, every sum in index
// order.  No running sums slide from one patch to the next, and the order of the additions depends on W (axis 1) or rows (axis 0)
// alone: a file's vectors are the same bits alone and in any batch.
//
//   patch_stats_rows_kernel (axis 1, 'Row': over the W frames of a patch -> (nP, rows)).  One workgroup of eight waves per (clip, block
//       of R rows).  A wave takes a row at a time for the file statistics (two reads of the row, the second from L2), then the block's
//       rows are walked ONCE more in segments: the standardised float32 values go into a ring of `cap` frames per row in LDS (index
//       = tiled frame & (cap - 1), row stride cap + 1 words), each tiled frame exactly once, and a thread takes one (row, patch) of
//       the patches that lie wholly in the ring -- 2 W LDS reads per output, whatever the overlap W / shift.  Rows are the fast index
//       of the items: the R lanes of a patch read R different rows, R banks (stride = 1 mod 32), and the stores are runs of R values.
//       cap = 512 and R = 16 up to W = 256 (32.8 KB: four workgroups, 32 waves, per CU -- the row walks are chains of memory latency,
//       which only other waves hide: with two waves per workgroup the call took 2.0 to 2.3 times as long, profiles/r15_skew_feed.txt);
//       a longer W doubles cap and halves R down to one row of 8192 frames, the longest W this kernel takes.
//   row_scalers_kernel + patch_stats_frames_kernel (axis 0, 'Col': over the rows of a frame -> (nP, W)).  The statistic of frame t
//       over the rows does not depend on the patch: c[t] is computed once per file and every patch is a window of it.  The prepass
//       leaves every (clip, row)'s (mean, scale) in the workspace (a wave per row); then one workgroup per (clip, 64 frames), a lane
//       per frame, so every row is read in 256-byte runs; the four waves take a quarter of the rows each -- the split depends on rows
//       alone -- and their partial sums meet in LDS in the order of the waves.  Wave 0 stores c[t] at every place (patch, j) that
//       holds frame t (modulo T for a tiled clip): runs along j.
//
// 30 to 40 VGPRs and no scratch in every kernel ("The skewness-vector feed", has what was measured).  All offsets into the
// featuregrams and the output are 64-bit; a clip without a patch (nP = 0) returns before it reads or writes anything.
#include <cmath>
#include <cstdint>
#include <vector>

#include "smh_common.h"
#include "smh_feat.h"
#include "smh_fvtable.h"
#include "smh_rag.h"

namespace {

using smh_fvtable::fill_table;
using smh_fvtable::FvClip;
using smh_fvtable::kMaxClips;

constexpr int kRowThreads = 512;   // axis 1: eight waves, two rows each at R = 16
constexpr int kRingFloats = 8192;  // axis 1: R * cap, the ring of one workgroup (+ R words of padding)
constexpr int kMinCap = 512;
constexpr int kFrameWaves = 4;     // axis 0: the rows in four parts
constexpr int kScalerRows = 16;    // axis 0 prepass: rows per workgroup, four per wave

// get_data_statistics' result from the mean and the central moments' sums over len values (smh_tools.hip: statistic())
__device__ __forceinline__ double result_of(int stat, int len, double m2, double m3, double m4) {
    m2 /= len, m3 /= len, m4 /= len;
    if (stat == 1) return m2;                                      // np.var (population)
    if (stat == 2) return m2 == 0.0 ? 0.0 : m3 / (m2 * sqrt(m2));  // scipy.stats.skew (bias=True); constant input -> 0
    return m2 == 0.0 ? -3.0 : m4 / (m2 * m2) - 3.0;                // scipy.stats.kurtosis (fisher=True, bias=True)
}

template <typename At>
__device__ __forceinline__ double statistic(int len, int stat, At &&at) {
    double s = 0.0;
    for (int i = 0; i < len; ++i) s += at(i);
    const double mean = s / len;
    if (stat == 0) return mean;
    double m2 = 0.0, m3 = 0.0, m4 = 0.0;
    for (int i = 0; i < len; ++i) {
        const double d = at(i) - mean, d2 = d * d;
        m2 += d2;
        m3 += d2 * d;
        m4 += d2 * d2;
    }
    return result_of(stat, len, m2, m3, m4);
}

// the patch element of row r: per-file StandardScaler (fold == false: a = mean, b = scale) or the fold's statistics (a = mean[r],
// b = stdev[r] + 1e-10)
__device__ __forceinline__ float element(float x, bool fold, double a, double b) {
    return fold ? (float)(((double)x - a) / b) : smh_feat::standardize(x, a, b);
}

template <typename Out>
__global__ void __launch_bounds__(kRowThreads)
patch_stats_rows_kernel(const FvClip *__restrict__ clips, int rows, int nrb, const double *__restrict__ mean,
                        const double *__restrict__ stdev, int W, int shift, int stat, int cap, int rshift, Out *__restrict__ out) {
    extern __shared__ float ring[];  // [R][cap + 1]
    __shared__ double s_a[16], s_b[16];
    const int clip = blockIdx.x / nrb, rb = blockIdx.x - clip * nrb;
    const FvClip c = clips[clip];
    const int T = c.T, nP = c.nP;
    if (nP <= 0) return;  // (uniform: before any barrier)
    const int R = 1 << rshift, stride = cap + 1, mask = cap - 1;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r0 = rb * R, nr = min(R, rows - r0);
    const bool fold = mean != nullptr;
    for (int rl = wave; rl < nr; rl += kRowThreads / 64) {
        const float *x = c.fv + (size_t)(r0 + rl) * T;
        double a, b;
        if (fold) a = mean[r0 + rl], b = stdev[r0 + rl] + 1e-10;
        else smh_feat::row_stats(T, lane, [&](int t) { return x[t]; }, a, b);
        if (lane == 0) s_a[rl] = a, s_b[rl] = b;
    }
    __syncthreads();
    const int per_seg = (cap - W) / shift + 1;  // patches whose frames fit the ring together
    int loaded = 0;                             // tiled frames below this one have been in the ring
    for (int p0 = 0; p0 < nP; p0 += per_seg) {
        const int np = min(per_seg, nP - p0);
        const int u0 = max(loaded, p0 * shift), u1 = (p0 + np - 1) * shift + W;  // u1 <= Ttiled: patch starts are never clamped
        for (int rl = wave; rl < nr; rl += kRowThreads / 64) {
            const float *x = c.fv + (size_t)(r0 + rl) * T;
            const double a = s_a[rl], b = s_b[rl];
            float *z = ring + rl * stride;
            for (int u = u0 + lane; u < u1; u += 64) z[u & mask] = element(x[u < T ? u : u % T], fold, a, b);
        }
        loaded = u1;
        __syncthreads();
        for (int item = threadIdx.x; item < (np << rshift); item += kRowThreads) {
            const int rl = item & (R - 1), p = p0 + (item >> rshift);
            if (rl < nr) {
                const float *z = ring + rl * stride;
                const int base = p * shift;
                const double v = statistic(W, stat, [&](int i) { return (double)z[(base + i) & mask]; });
                out[((size_t)c.patch_off + (size_t)p) * rows + r0 + rl] = (Out)v;
            }
        }
        __syncthreads();  // the next segment overwrites the frames in front of its first patch
    }
}

__global__ void __launch_bounds__(256)
row_scalers_kernel(const FvClip *__restrict__ clips, int rows, int nrb, double *__restrict__ scalers) {
    const int clip = blockIdx.x / nrb, rb = blockIdx.x - clip * nrb;
    const FvClip c = clips[clip];
    if (c.nP <= 0) return;
    const int T = c.T;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r1 = min(rows, (rb + 1) * kScalerRows);
    for (int r = rb * kScalerRows + wave; r < r1; r += 4) {
        const float *x = c.fv + (size_t)r * T;
        double a, b;
        smh_feat::row_stats(T, lane, [&](int t) { return x[t]; }, a, b);
        if (lane == 0) {
            const size_t o = (size_t)clip * rows + r;
            scalers[2 * o] = a, scalers[2 * o + 1] = b;
        }
    }
}

template <typename Out>
__global__ void __launch_bounds__(64 * kFrameWaves)
patch_stats_frames_kernel(const FvClip *__restrict__ clips, int rows, const double *__restrict__ mean, const double *__restrict__ stdev,
                          const double *__restrict__ scalers, int W, int shift, int stat, Out *__restrict__ out) {
    __shared__ double part[4][kFrameWaves][64];
    const int clip = blockIdx.x;
    const FvClip c = clips[clip];
    const int T = c.T, nP = c.nP, Tt = c.Ttiled;
    const int t0 = blockIdx.y * 64;
    if (t0 >= T || nP <= 0) return;  // (uniform: before any barrier)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int t = t0 + lane;
    const float *x = c.fv + min(t, T - 1);  // lanes beyond the clip's last frame read that frame again and store nothing
    const bool fold = mean != nullptr;
    const double *sc = fold ? nullptr : scalers + (size_t)clip * rows * 2;
    const int per = (rows + kFrameWaves - 1) / kFrameWaves;
    const int ra = min(rows, wave * per), rb = min(rows, ra + per);
    auto value = [&](int r) -> double {
        const float v = x[(size_t)r * T];
        return (double)(fold ? element(v, true, mean[r], stdev[r] + 1e-10) : element(v, false, sc[2 * r], sc[2 * r + 1]));
    };
    double s = 0.0;
#pragma unroll 4
    for (int r = ra; r < rb; ++r) s += value(r);
    part[0][wave][lane] = s;
    __syncthreads();
    s = ((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane];
    const double mu = s / rows;
    double v = mu;
    if (stat != 0) {
        double m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll 4
        for (int r = ra; r < rb; ++r) {
            const double d = value(r) - mu, d2 = d * d;
            m2 += d2;
            m3 += d2 * d;
            m4 += d2 * d2;
        }
        part[1][wave][lane] = m2, part[2][wave][lane] = m3, part[3][wave][lane] = m4;
        __syncthreads();
        if (wave != 0) return;
        m2 = ((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane];
        m3 = ((part[2][0][lane] + part[2][1][lane]) + part[2][2][lane]) + part[2][3][lane];
        m4 = ((part[3][0][lane] + part[3][1][lane]) + part[3][2][lane]) + part[3][3][lane];
        v = result_of(stat, rows, m2, m3, m4);
    }
    if (wave != 0 || t >= T) return;
    const size_t patch_off = (size_t)c.patch_off;
    for (int u = t; u < Tt; u += T) {  // the frame's positions in the tiled featuregram (one unless T < W)
        int p_lo, p_hi;
        smh_feat::patch_range(u, W, shift, nP, p_lo, p_hi);
        for (int p = p_lo; p <= p_hi; ++p) out[(patch_off + (size_t)p) * W + (u - p * shift)] = (Out)v;
    }
}

// axis 1: the ring's frames per row and log2 of the rows per workgroup for patches of W frames; false beyond the longest W
bool ring_plan(int W, int &cap, int &rshift) {
    cap = kMinCap;
    while (cap < 2 * W && cap < kRingFloats) cap *= 2;
    if (cap < W) return false;
    rshift = 0;
    while ((cap << (rshift + 1)) <= kRingFloats) ++rshift;
    return true;
}

}  // namespace

extern "C" size_t smh_patch_statistics_workspace_bytes(int B, int rows, int axis, int with_stats) {
    if (B <= 0 || rows <= 0 || axis != 0 || with_stats) return 0;
    return (size_t)B * rows * 2 * sizeof(double);
}

extern "C" int smh_patch_statistics(const smh_ctx *ctx, const float *const *h_fv, const int *h_T, int B, int rows, const double *d_mean,
                                    const double *d_stdev, int W, int shift, int stat, int axis, int out_f32, void *d_out, void *d_work,
                                    size_t work_bytes, void *stream) {
    SMH_REQUIRE(ctx && B >= 0 && rows >= 1, "smh_patch_statistics: bad argument (B=%d rows=%d)", B, rows);
    SMH_REQUIRE(W >= 1 && shift >= 1, "smh_patch_statistics: bad patch geometry W=%d shift=%d", W, shift);
    SMH_REQUIRE(stat >= 0 && stat <= 3, "smh_patch_statistics: stat must be 0 (mean), 1 (variance), 2 (skew) or 3 (kurtosis), got %d", stat);
    SMH_REQUIRE(axis == 0 || axis == 1, "smh_patch_statistics: axis must be 0 or 1, got %d", axis);
    SMH_REQUIRE((d_mean == nullptr) == (d_stdev == nullptr), "smh_patch_statistics: d_mean and d_stdev come together or not at all");
    int cap = 0, rshift = 0;
    if (axis == 1)
        SMH_REQUIRE(ring_plan(W, cap, rshift), "smh_patch_statistics: axis 1 takes patches of up to %d frames, got W=%d", kRingFloats, W);
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(h_fv && h_T && d_out, "smh_patch_statistics: null argument");
    const bool fold = d_mean != nullptr;
    const size_t need = smh_patch_statistics_workspace_bytes(B, rows, axis, fold ? 1 : 0);
    if (need > 0 && (!d_work || work_bytes < need || (reinterpret_cast<uintptr_t>(d_work) % 8) != 0))
        return smh::set_error(SMH_E_WORKSPACE, "smh_patch_statistics: the workspace must be %zu bytes, 8-byte aligned (got %zu)", need, work_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int R = axis == 1 ? 1 << rshift : kScalerRows;
    const int nrb = (rows + R - 1) / R;
    const int per = std::max(1, std::min(kMaxClips, (int)(((1ll << 31) - 1) / nrb)));
    std::vector<FvClip> t;
    long long patch_off = 0;
    for (int b0 = 0; b0 < B; b0 += per) {
        const int n = std::min(per, B - b0);
        int max_T = 0;
        int rc = fill_table("smh_patch_statistics", h_fv, h_T, b0, n, W, shift, patch_off, max_T, t);
        if (rc) return rc;
        const int segs = (max_T + 63) / 64;
        SMH_REQUIRE(axis == 1 || segs <= 65535, "smh_patch_statistics: a featuregram of %d frames is beyond %d segments of 64", max_T, 65535);
        double *scalers = need > 0 ? static_cast<double *>(d_work) + (size_t)b0 * rows * 2 : nullptr;
        rc = smh_rag::launch_with_table(ctx, "smh_patch_statistics", t.data(), t.size() * sizeof(FvClip), st, [&](const void *d_table) -> int {
            const FvClip *clips = static_cast<const FvClip *>(d_table);
            if (axis == 1) {
                const size_t lds = sizeof(float) * ((size_t)R * (cap + 1));
                const dim3 grid((unsigned)n * (unsigned)nrb), block(kRowThreads);
                if (out_f32)
                    hipLaunchKernelGGL(patch_stats_rows_kernel<float>, grid, block, lds, st, clips, rows, nrb, d_mean, d_stdev, W, shift, stat,
                                       cap, rshift, static_cast<float *>(d_out));
                else
                    hipLaunchKernelGGL(patch_stats_rows_kernel<double>, grid, block, lds, st, clips, rows, nrb, d_mean, d_stdev, W, shift, stat,
                                       cap, rshift, static_cast<double *>(d_out));
                return smh::launch_status("patch_stats_rows_kernel");
            }
            if (!fold) {
                hipLaunchKernelGGL(row_scalers_kernel, dim3((unsigned)n * (unsigned)nrb), dim3(256), 0, st, clips, rows, nrb, scalers);
                const int rc2 = smh::launch_status("row_scalers_kernel");
                if (rc2) return rc2;
            }
            const dim3 grid((unsigned)n, (unsigned)segs), block(64 * kFrameWaves);
            if (out_f32)
                hipLaunchKernelGGL(patch_stats_frames_kernel<float>, grid, block, 0, st, clips, rows, d_mean, d_stdev, scalers, W, shift, stat,
                                   static_cast<float *>(d_out));
            else
                hipLaunchKernelGGL(patch_stats_frames_kernel<double>, grid, block, 0, st, clips, rows, d_mean, d_stdev, scalers, W, shift, stat,
                                   static_cast<double *>(d_out));
            return smh::launch_status("patch_stats_frames_kernel");
        });
        if (rc) return rc;
    }
    return SMH_OK;
}
