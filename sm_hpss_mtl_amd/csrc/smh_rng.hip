// Random draws of the training step, on the device and in ONE pass each (gfx950).
//   smh_noise_augment_f32 : batchData + N(0, scale)     -- Proposed_Work_Results.py:239-242 (np.random.normal + np.add)
//   smh_dropout_masks_f32 : the SpatialDropout1D / Dropout keep masks of one step, 0 or 1 / keep, two rates in one launch
//                           (lib/proposed_architectures.py: tcn.TCN(dropout_rate=...), Dropout(0.4) of the heads)
// Until round 3 these were torch kernels on the step's stream (normal_ 15.8 + add 15.1 + bernoulli 5.0 + mul 5.2 us per 510-clip
// step): two full passes over the 33 MB patch tensor where one does.  The generator is Philox4x32-10 (counter = element group,
// key = seed, second counter word = the caller's offset: a (seed, offset) pair never repeats a stream), normals by Box-Muller on
// v_log_f32 / v_sin_f32 / v_cos_f32 (the latter two take revolutions: no 2 pi product).  Both kernels are HBM-bound: 16 bytes in
// and 16 bytes out per lane and ~150 VALU instructions per four values.  The generator itself is smh_rng.h (shared with the window
// gather of smh_gather.hip, which adds the same draws on its way out).
#include "smh_rng.h"

namespace {

using smh_rng::add_noise;
using smh_rng::normals_of_group;
using smh_rng::philox4x32_10;

__global__ void __launch_bounds__(256) noise_augment_kernel(const float *__restrict__ x, float *__restrict__ out, size_t n,
                                                            float scale, unsigned long long seed, unsigned long long offset) {
    const size_t groups = (n + 3) / 4;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        float z[4];
        normals_of_group(g, seed, offset, z);
        const size_t i = 4 * g;
        if (i + 4 <= n) {
            float4 v = *reinterpret_cast<const float4 *>(x + i);
            v.x = add_noise(v.x, scale, z[0]), v.y = add_noise(v.y, scale, z[1]);
            v.z = add_noise(v.z, scale, z[2]), v.w = add_noise(v.w, scale, z[3]);
            *reinterpret_cast<float4 *>(out + i) = v;
        } else {
            for (size_t j = i; j < n; ++j) out[j] = add_noise(x[j], scale, z[j - i]);
        }
    }
}

__global__ void __launch_bounds__(256) dropout_masks_kernel(float *__restrict__ out, size_t n_a, float keep_a, size_t n_b,
                                                            float keep_b, unsigned long long seed, unsigned long long offset) {
    const size_t n = n_a + n_b, groups = (n + 3) / 4;
    const float inv_a = 1.0f / keep_a, inv_b = 1.0f / keep_b;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        unsigned r[4];
        philox4x32_10(g, offset, seed, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = 4 * g + j;
            if (i < n) {
                const float u = (float)(r[j] >> 8) * 5.9604644775390625e-8f;  // [0, 1)
                const bool a = i < n_a;
                out[i] = u < (a ? keep_a : keep_b) ? (a ? inv_a : inv_b) : 0.f;
            }
        }
    }
}

int grid_for(size_t groups) {
    const size_t blocks = (groups + 255) / 256;
    return (int)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks));  // grid-stride: 32 workgroups per CU at most
}

}  // namespace

extern "C" int smh_noise_augment_f32(const float *d_x, float *d_out, size_t n, float scale, unsigned long long seed,
                                     unsigned long long offset, void *stream) {
    SMH_REQUIRE((d_x && d_out) || n == 0, "smh_noise_augment_f32: null argument");
    SMH_REQUIRE(scale >= 0.f, "smh_noise_augment_f32: scale=%g is negative", (double)scale);
    SMH_REQUIRE((reinterpret_cast<uintptr_t>(d_x) % 16) == 0 && (reinterpret_cast<uintptr_t>(d_out) % 16) == 0,
                "smh_noise_augment_f32: buffers must be 16-byte aligned");
    if (n == 0) return SMH_OK;
    hipLaunchKernelGGL(noise_augment_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_x, d_out, n, scale,
                       seed, offset);
    return smh::launch_status("noise_augment_kernel");
}

extern "C" int smh_dropout_masks_f32(float *d_out, size_t n_a, float keep_a, size_t n_b, float keep_b, unsigned long long seed,
                                     unsigned long long offset, void *stream) {
    SMH_REQUIRE(d_out || n_a + n_b == 0, "smh_dropout_masks_f32: null argument");
    SMH_REQUIRE(keep_a > 0.f && keep_a <= 1.f && keep_b > 0.f && keep_b <= 1.f,
                "smh_dropout_masks_f32: keep probabilities %g, %g outside (0, 1]", (double)keep_a, (double)keep_b);
    if (n_a + n_b == 0) return SMH_OK;
    hipLaunchKernelGGL(dropout_masks_kernel, dim3(grid_for((n_a + n_b + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_out, n_a,
                       keep_a, n_b, keep_b, seed, offset);
    return smh::launch_status("dropout_masks_kernel");
}
