// Frame-level scaling on the device (PARAMS['frame_level_scaling']): the statistics of a training fold and the scaled patch feed.
//
// With the switch on, the reference replaces get_feature_patches' per-file StandardScaler by ONE mean and ONE standard deviation
// per feature row over the whole training fold (lib/preprocessing.py:461-586, get_data_stats) and applies them to every file's
// featuregram before the patches are cut (lib/cython_impl/tools.pyx:138-165, scale_data).  Both halves work here on featuregrams
// that are ALREADY on the device -- (rows, T_b) float32, dense, rows of exactly T_b floats, as run_ragged(W = None), the
// equal-length entries and the device featuregram cache hold them -- described by a small per-clip table (FvClip) that goes through
// smh_rag::launch_with_table: separately allocated tensors and views of one buffer share a launch.
//
//   row_moments_kernel     one workgroup per (clip, block of 16 rows), 4 waves, a wave per row at a time.  Pass 1: lanes stride the
//       row's frames by 64 with ONE f64 partial sum each, then a fixed xor-shuffle tree -> sum(x); values that are not finite are
//       counted on the way.  Pass 2 re-reads the row (40 KB at 10 000 frames: L2) for M2 = sum((x - sum / T)^2) the same way.  The
//       order of every addition depends on T alone and there are no atomics, so a clip's moments are the same bits alone and in any
//       batch.  The host needs nothing else: around ANY mean mu, sum((x - mu)^2) = M2 + T (sum / T - mu)^2 exactly.
//   scaled_patches_kernel  one workgroup per (clip, block of 32 rows, segment of 256 frames), 4 waves of 8 rows.  A lane holds one
//       frame of a row: (float)(((double)x - mean[r]) / (stdev[r] + 1e-10)), tools.pyx's arithmetic rounded ONCE to the float32 every
//       device feed delivers (the division is IEEE f64: no reciprocal).  Time-major (nP, W, rows): through a [32][65] LDS tile and out
//       transposed, as 128-byte runs of 32 rows in every patch that holds the frame -- plain_finish_kernel's pass 2 (smh_plain.hip),
//       whose bank reasoning holds here: ds_write_b32 and ds_read_b32 count conflicts per 32-lane half on (word mod 32); a wave
//       writes one row, words 65 r + lane (bank lane + r: all 32), and a half reads 32 rows of one frame, words 65 f + t (bank
//       f + t: all 32).  Image (nP, rows, W): straight from the registers as runs of up to 256 bytes
//       along the patch's time axis, no LDS, no barrier.  No row-statistics pass and no second read of the featuregram; a frame
//       outside every patch is read and dropped.  Patches lie on the grid of smh_tiled_frames / smh_num_patches / smh_patch_start,
//       tile-if-short wrapping included (a frame of a clip with T < W has several positions in the tiled featuregram).
//
// 256 threads per workgroup, 34 to 54 VGPRs and no scratch; the time-major instantiation's 8.3 KB tile is the only LDS, so the wave
// limit, not LDS, decides the residency (no second launch-bounds argument: nothing here needs a register cap).  Both kernels are
// bound by the featuregram read and the patch write.  All offsets into the featuregrams and the patch buffer are 64-bit.
#include <cmath>
#include <cstdint>
#include <vector>

#include "smh_common.h"
#include "smh_feat.h"
#include "smh_fvtable.h"
#include "smh_rag.h"

namespace {

constexpr int kWaves = 4;
constexpr int kMomRows = 16;    // rows per moments workgroup: four per wave, one at a time
constexpr int kTile = 64;       // frames per chunk: one lane per frame
constexpr int kRowBlock = 32;   // rows per patch workgroup: 128-byte runs in the time-major patches
constexpr int kRowsPerWave = kRowBlock / kWaves;
constexpr int kSegFrames = 4 * kTile;  // frames per patch workgroup

using smh_fvtable::fill_table;
using smh_fvtable::FvClip;
using smh_fvtable::kMaxClips;

using smh::wave_sum;  // smh_wave.h: the xor-tree order

__global__ void __launch_bounds__(64 * kWaves)
row_moments_kernel(const FvClip *__restrict__ clips, int rows, int nrb, double *__restrict__ moments, int *__restrict__ nonfinite) {
    const int clip = blockIdx.x / nrb, rb = blockIdx.x - clip * nrb;
    const FvClip c = clips[clip];
    const int T = c.T;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r1 = min(rows, (rb + 1) * kMomRows);
    for (int r = rb * kMomRows + wave; r < r1; r += kWaves) {
        const float *x = c.fv + (size_t)r * T;
        double s = 0.0;
        int bad = 0;
#pragma unroll 4
        for (int t = lane; t < T; t += 64) {
            const float v = x[t];
            s += (double)v;
            bad += (__builtin_fabsf(v) <= 3.4028234663852886e38f) ? 0 : 1;  // NaN compares false
        }
        s = wave_sum(s);
        for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
        const double m = s / (double)T;
        double q = 0.0;
#pragma unroll 4
        for (int t = lane; t < T; t += 64) {
            const double d = (double)x[t] - m;
            q += d * d;
        }
        q = wave_sum(q);
        if (lane == 0) {
            const size_t o = (size_t)clip * rows + r;
            moments[2 * o] = s, moments[2 * o + 1] = q;
            nonfinite[o] = bad;
        }
    }
}

template <bool IMAGE>
__global__ void __launch_bounds__(64 * kWaves)
scaled_patches_kernel(const FvClip *__restrict__ clips, int rows, int nrb, const double *__restrict__ mean,
                      const double *__restrict__ stdev, int W, int shift, float *__restrict__ patches) {
    float *tile = nullptr;  // the transposing LDS tile: time-major only
    if constexpr (!IMAGE) {
        __shared__ float tile_lds[kRowBlock * (kTile + 1)];
        tile = tile_lds;
    }
    const int clip = blockIdx.x / nrb, rb = blockIdx.x - clip * nrb;
    const FvClip c = clips[clip];
    const int T = c.T, nP = c.nP, Tt = c.Ttiled;
    const int s0 = blockIdx.y * kSegFrames;
    if (s0 >= T || nP <= 0) return;  // (uniform: before any barrier)
    const int s1 = min(T, s0 + kSegFrames);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r0 = rb * kRowBlock, nr = min(kRowBlock, rows - r0);
    const size_t patch_off = (size_t)c.patch_off;
    const float *x[kRowsPerWave];  // this wave's rows: r0 + 4 q + wave; rows beyond the block repeat its last one and are never written
    double mu[kRowsPerWave], den[kRowsPerWave];
#pragma unroll
    for (int q = 0; q < kRowsPerWave; ++q) {
        const int r = r0 + min(q * kWaves + wave, nr - 1);
        x[q] = c.fv + (size_t)r * T;
        mu[q] = mean[r], den[q] = stdev[r] + 1e-10;
    }
    const int f = threadIdx.x & (kRowBlock - 1), tl0 = threadIdx.x >> 5;
    for (int c0 = s0; c0 < s1; c0 += kTile) {
        const int nt = min(kTile, T - c0);
        const int tc = c0 + min(lane, nt - 1);  // lanes beyond the clip's last frame read that frame again and store nothing
        float v[kRowsPerWave];
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) v[q] = x[q][tc];
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) {
            const int rl = q * kWaves + wave;
            if (rl < nr) {
                const float z = (float)(((double)v[q] - mu[q]) / den[q]);
                if constexpr (IMAGE) v[q] = z;
                else tile[rl * (kTile + 1) + lane] = z;
            }
        }
        if constexpr (IMAGE) {
            for (int u = lane < nt ? c0 + lane : Tt; u < Tt; u += T) {  // the frame's positions in the tiled featuregram (one unless T < W)
                int p_lo, p_hi;
                smh_feat::patch_range(u, W, shift, nP, p_lo, p_hi);
                for (int p = p_lo; p <= p_hi; ++p) {
                    float *dst = patches + ((patch_off + (size_t)p) * rows + r0 + wave) * W + (u - p * shift);
#pragma unroll
                    for (int q = 0; q < kRowsPerWave; ++q)
                        if (q * kWaves + wave < nr) dst[(size_t)q * kWaves * W] = v[q];
                }
            }
        } else {
            __syncthreads();
            for (int tl = tl0; tl < nt; tl += (64 * kWaves) / kRowBlock) {
                for (int u = c0 + tl; u < Tt; u += T) {
                    int p_lo, p_hi;
                    smh_feat::patch_range(u, W, shift, nP, p_lo, p_hi);
                    for (int p = p_lo; p <= p_hi; ++p) {
                        const int j = u - p * shift;
                        if (f < nr) patches[((patch_off + (size_t)p) * W + j) * rows + r0 + f] = tile[f * (kTile + 1) + tl];
                    }
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" int smh_row_moments_f64(const smh_ctx *ctx, const float *const *h_fv, const int *h_T, int B, int rows, double *d_moments,
                                   int32_t *d_nonfinite, void *stream) {
    SMH_REQUIRE(ctx && B >= 0 && rows >= 1, "smh_row_moments_f64: bad argument (B=%d rows=%d)", B, rows);
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(h_fv && h_T && d_moments && d_nonfinite, "smh_row_moments_f64: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int nrb = (rows + kMomRows - 1) / kMomRows;
    const int per = std::max(1, std::min(kMaxClips, (int)(((1ll << 31) - 1) / nrb)));
    std::vector<FvClip> t;
    long long none = 0;
    for (int b0 = 0; b0 < B; b0 += per) {
        const int n = std::min(per, B - b0);
        int max_T = 0;
        int rc = fill_table("smh_row_moments_f64", h_fv, h_T, b0, n, 0, 0, none, max_T, t);
        if (rc) return rc;
        double *mom = d_moments + (size_t)b0 * rows * 2;
        int *bad = (int *)d_nonfinite + (size_t)b0 * rows;
        rc = smh_rag::launch_with_table(ctx, "smh_row_moments_f64", t.data(), t.size() * sizeof(FvClip), st, [&](const void *d_table) -> int {
            hipLaunchKernelGGL(row_moments_kernel, dim3((unsigned)n * (unsigned)nrb), dim3(64 * kWaves), 0, st,
                               static_cast<const FvClip *>(d_table), rows, nrb, mom, bad);
            return smh::launch_status("row_moments_kernel");
        });
        if (rc) return rc;
    }
    return SMH_OK;
}

extern "C" long long smh_scaled_patches_count(const int *h_T, int B, int W, int shift, long long *h_patch_off) {
    if (B < 0 || W < 1 || shift < 1 || (B > 0 && !h_T)) return smh::set_error(SMH_E_INVALID, "smh_scaled_patches_count: bad argument");
    long long total = 0;
    for (int b = 0; b < B; ++b) {
        if (h_T[b] < 1) return smh::set_error(SMH_E_INVALID, "smh_scaled_patches_count: featuregram %d has T=%d frames", b, h_T[b]);
        if (h_patch_off) h_patch_off[b] = total;
        total += smh_num_patches(smh_tiled_frames(h_T[b], W), W, shift);
    }
    if (h_patch_off) h_patch_off[B] = total;
    return total;
}

extern "C" int smh_scaled_patches_f32(const smh_ctx *ctx, const float *const *h_fv, const int *h_T, int B, int rows, const double *d_mean,
                                      const double *d_stdev, int W, int shift, int patch_layout, float *d_patches, void *stream) {
    SMH_REQUIRE(patch_layout == smh_feat::kLayoutImage || patch_layout == smh_feat::kLayoutTimeMajor,
                "smh_scaled_patches_f32: patch_layout must be 0 (image) or 1 (time-major), got %d", patch_layout);
    SMH_REQUIRE(ctx && B >= 0 && rows >= 1, "smh_scaled_patches_f32: bad argument (B=%d rows=%d)", B, rows);
    SMH_REQUIRE(W >= 1 && shift >= 1, "smh_scaled_patches_f32: bad patch geometry W=%d shift=%d", W, shift);
    if (B == 0) return SMH_OK;
    SMH_REQUIRE(h_fv && h_T && d_mean && d_stdev && d_patches, "smh_scaled_patches_f32: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int nrb = (rows + kRowBlock - 1) / kRowBlock;
    const int per = std::max(1, std::min(kMaxClips, (int)(((1ll << 31) - 1) / nrb)));
    std::vector<FvClip> t;
    long long patch_off = 0;
    for (int b0 = 0; b0 < B; b0 += per) {
        const int n = std::min(per, B - b0);
        int max_T = 0;
        int rc = fill_table("smh_scaled_patches_f32", h_fv, h_T, b0, n, W, shift, patch_off, max_T, t);
        if (rc) return rc;
        const int segs = (max_T + kSegFrames - 1) / kSegFrames;
        SMH_REQUIRE(segs <= 65535, "smh_scaled_patches_f32: a featuregram of %d frames is beyond %d segments of %d", max_T, 65535, kSegFrames);
        rc = smh_rag::launch_with_table(ctx, "smh_scaled_patches_f32", t.data(), t.size() * sizeof(FvClip), st, [&](const void *d_table) -> int {
            const auto kernel = patch_layout == smh_feat::kLayoutImage ? scaled_patches_kernel<true> : scaled_patches_kernel<false>;
            hipLaunchKernelGGL(kernel, dim3((unsigned)n * (unsigned)nrb, (unsigned)segs), dim3(64 * kWaves), 0, st,
                               static_cast<const FvClip *>(d_table), rows, nrb, d_mean, d_stdev, W, shift, d_patches);
            return smh::launch_status("scaled_patches_kernel");
        });
        if (rc) return rc;
    }
    return SMH_OK;
}
