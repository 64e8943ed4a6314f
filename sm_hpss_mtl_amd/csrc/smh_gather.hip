// Window gather of the fine-tuning feed (gfx950): one launch builds a whole training batch from a RESIDENT featuregram.
//
// The reference's segmentation driver (DAFx12_Speech_Music_Detection_B3_MTL_v2.py: generator, :346-436) cuts "parts" out of the
// standardised featuregram of the whole training set, materialises every patch of a part on the host (get_feature_patches,
// :260-294) and queues them; a batch is the head of two such queues, transposed for the TCN (:422-424) and noise-augmented
// (:427-430).  Here the featuregram (F, T) stays on the device, the queues hold integer descriptors (sm_hpss_mtl_amd/dafx.py) and
// a batch of N patches is
//
//     out[n] = FV[:, base[n] + (first[n] + t) % period[n]],  t < W          (+ N(0, noise_scale) per element)
//
// -- the periodic form is get_feature_patches' tile-if-short rule (:262-265): a part shorter than W is repeated, so a window of it
// wraps inside [base, base + period); with period >= first + W it is a plain window.
//
// gather_windows_kernel: one workgroup (256 threads) per (patch, 64-feature tile, 64-frame tile).
//   read : a wave reads 64 consecutive frames of one row of FV -- 4-byte loads, coalesced along time (window starts are arbitrary,
//          so nothing wider is aligned); the frame's column, the only modulo, is computed once per lane.
//   image layout (n, f, t): the value goes straight out, 4-byte stores coalesced along t (a patch row starts at any element).
//   time-major (n, t, f): through an LDS tile [64 f][64 + 1 t].  Written row-wise (bank = t + f mod 32: a 32-lane half covers all
//          banks), read transposed: with F % 4 == 0 a lane reads four features of one frame (words 65 (4 q + j) + t: 4 q + t mod 32
//          over q < 8, t < 4 is every bank once per half) and stores them as 16 bytes; any other F takes the scalar path, lanes
//          along f (words 65 f + t: f mod 32).
//   noise: smh_rng.h's draw of the element's position in d_out, added to the value on its way out -- the 16-byte store is exactly
//          one Philox group; noise_scale == 0 skips the draw and the output is a bit copy.
// All offsets into FV and out are 64-bit.  Bandwidth-bound at best and latency-bound at the driver's 32-patch batch (one workgroup
// per CU at W = 99, F = 240): its job is one launch per batch.
#include <cstdint>
#include <vector>

#include "smh_rag.h"
#include "smh_rng.h"

namespace {

constexpr int kTT = 64;           // frames per tile = lanes of a wave
constexpr int kFT = 64;           // features per tile
constexpr int kStride = kTT + 1;  // LDS row of a feature, padded by one word
constexpr int kThreads = 256;

struct Desc {
    int base, period, first;
};

// LAYOUT 0: image (n, f, t); 1: time-major (n, t, f), VEC4: F % 4 == 0
template <int LAYOUT, bool VEC4>
__global__ void __launch_bounds__(kThreads) gather_windows_kernel(const float *__restrict__ FV, long long T, int F, int W,
                                                                  const Desc *__restrict__ desc, float scale,
                                                                  unsigned long long seed, unsigned long long offset,
                                                                  float *__restrict__ out) {
    const int n = blockIdx.x, f0 = blockIdx.y * kFT, t0 = blockIdx.z * kTT;
    const Desc d = desc[n];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t patch = (size_t)n * W * F;
    const bool noisy = scale != 0.f;

    const int t = t0 + lane;
    const bool t_ok = t < W;
    // the frame's column: inside [base, base + period), which the host checked against [0, T)
    const long long col = d.base + ((long long)d.first + (t_ok ? t : 0)) % d.period;

    if constexpr (LAYOUT == 0) {
        for (int r = wave; r < kFT; r += kThreads / 64) {
            const int f = f0 + r;
            if (f >= F) break;
            if (t_ok) {
                const float v = FV[(long long)f * T + col];
                const size_t i = patch + (size_t)f * W + t;
                out[i] = noisy ? smh_rng::noise_one(v, i, scale, seed, offset) : v;
            }
        }
    } else {
        __shared__ float tile[kFT * kStride];
        for (int r = wave; r < kFT; r += kThreads / 64) {
            const int f = f0 + r;
            if (f < F && t_ok) tile[r * kStride + lane] = FV[(long long)f * T + col];
        }
        __syncthreads();
        if constexpr (VEC4) {
            // a 32-lane half: 8 feature quads x 4 frames; the halves take quads 0..7 and 8..15 of the same frames
            const int q = (lane & 7) | ((lane >> 5) << 3), tq = (lane >> 3) & 3;
            const int f = f0 + 4 * q;
            if (f < F) {  // F % 4 == 0: f + 3 < F as well
                for (int tl = tq + 4 * wave; tl < kTT; tl += 16) {
                    const int tt = t0 + tl;
                    if (tt >= W) break;
                    const float *src = tile + 4 * q * kStride + tl;
                    float4 v = make_float4(src[0], src[kStride], src[2 * kStride], src[3 * kStride]);
                    const size_t i = patch + (size_t)tt * F + f;  // a multiple of 4: one Philox group
                    if (noisy) {
                        float z[4];
                        smh_rng::normals_of_group(i / 4, seed, offset, z);
                        v.x = smh_rng::add_noise(v.x, scale, z[0]), v.y = smh_rng::add_noise(v.y, scale, z[1]);
                        v.z = smh_rng::add_noise(v.z, scale, z[2]), v.w = smh_rng::add_noise(v.w, scale, z[3]);
                    }
                    *reinterpret_cast<float4 *>(out + i) = v;
                }
            }
        } else {
            const int f = f0 + lane;
            if (f < F) {
                for (int tl = wave; tl < kTT; tl += kThreads / 64) {
                    const int tt = t0 + tl;
                    if (tt >= W) break;
                    const float v = tile[lane * kStride + tl];
                    const size_t i = patch + (size_t)tt * F + f;
                    out[i] = noisy ? smh_rng::noise_one(v, i, scale, seed, offset) : v;
                }
            }
        }
    }
}

}  // namespace

extern "C" int smh_gather_windows_f32(const smh_ctx *ctx, const float *d_FV, int F, long long T, const int *h_desc, int N, int W,
                                      int patch_layout, float noise_scale, unsigned long long seed, unsigned long long offset,
                                      float *d_out, void *stream) {
    SMH_REQUIRE(ctx && d_FV && h_desc && d_out, "smh_gather_windows_f32: null argument");
    SMH_REQUIRE(N >= 0 && W >= 1 && F >= 1, "smh_gather_windows_f32: bad shape N=%d W=%d F=%d", N, W, F);
    SMH_REQUIRE(patch_layout == 0 || patch_layout == 1,
                "smh_gather_windows_f32: patch_layout=%d (0 = image (N, F, W), 1 = time-major (N, W, F))", patch_layout);
    SMH_REQUIRE(noise_scale >= 0.f, "smh_gather_windows_f32: noise_scale=%g is negative", (double)noise_scale);  // (a NaN fails too)
    SMH_REQUIRE((reinterpret_cast<uintptr_t>(d_out) % 16) == 0, "smh_gather_windows_f32: d_out must be 16-byte aligned");
    for (int n = 0; n < N; ++n) {
        const long long base = h_desc[3 * n], period = h_desc[3 * n + 1], first = h_desc[3 * n + 2];
        SMH_REQUIRE(base >= 0 && period >= 1 && first >= 0 && base + period <= T,
                    "smh_gather_windows_f32: row %d (base=%lld, period=%lld, first=%lld) is outside the %lld frames", n, base, period,
                    first, T);
    }
    if (N == 0) return SMH_OK;
    const int f_tiles = (F + kFT - 1) / kFT, t_tiles = (W + kTT - 1) / kTT;
    SMH_REQUIRE(f_tiles <= 65535 && t_tiles <= 65535, "smh_gather_windows_f32: F=%d or W=%d beyond %d tiles of 64", F, W, 65535);
    hipStream_t st = (hipStream_t)stream;
    return smh_rag::launch_with_table(
        ctx, "smh_gather_windows_f32", h_desc, (size_t)N * sizeof(Desc), st, [&](const void *d_table) -> int {
            const Desc *d_desc = static_cast<const Desc *>(d_table);
            const dim3 grid(N, f_tiles, t_tiles), block(kThreads);
            if (patch_layout == 0)
                hipLaunchKernelGGL((gather_windows_kernel<0, false>), grid, block, 0, st, d_FV, T, F, W, d_desc, noise_scale, seed,
                                   offset, d_out);
            else if (F % 4 == 0)
                hipLaunchKernelGGL((gather_windows_kernel<1, true>), grid, block, 0, st, d_FV, T, F, W, d_desc, noise_scale, seed,
                                   offset, d_out);
            else
                hipLaunchKernelGGL((gather_windows_kernel<1, false>), grid, block, 0, st, d_FV, T, F, W, d_desc, noise_scale, seed,
                                   offset, d_out);
            return smh::launch_status("gather_windows_kernel");
        });
}
