// The device half of the training step's random draws (smh_rng.hip), shared with the kernels that fuse a draw into their own
// store (smh_gather.hip): Philox4x32-10 (counter = element group of four, key = seed, second counter word = the caller's offset),
// normals by Box-Muller on v_log_f32 / v_sin_f32 / v_cos_f32, and the one expression that adds a draw to a value.  A kernel that
// calls normals_of_group + add_noise (a whole group of four) or noise_one (one element) with the position in the array gets the
// bits smh_noise_augment_f32 gives that element.
#pragma once
#include "smh_common.h"

namespace smh_rng {

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): four 32-bit words per (counter, key)
__device__ __forceinline__ void philox4x32_10(unsigned long long group, unsigned long long offset, unsigned long long seed,
                                              unsigned (&r)[4]) {
    r[0] = (unsigned)group, r[1] = (unsigned)(group >> 32), r[2] = (unsigned)offset, r[3] = (unsigned)(offset >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(r, k0, k1);
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// two standard normals from two 32-bit words: u1 in (0, 1], u2 in [0, 1) revolutions
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float &n0, float &n1) {
    const float u1 = ((float)(a >> 8) + 1.0f) * 5.9604644775390625e-8f;  // (k + 1) / 2^24: never 0, log finite
    const float u2 = (float)(b >> 8) * 5.9604644775390625e-8f;
    // -2 ln u1 = -2 ln2 * log2(u1)
    const float rad = __builtin_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    n0 = rad * __builtin_amdgcn_cosf(u2), n1 = rad * __builtin_amdgcn_sinf(u2);
}

// the four standard normals of element group g (elements 4 g .. 4 g + 3 of the array)
__device__ __forceinline__ void normals_of_group(size_t g, unsigned long long seed, unsigned long long offset, float (&z)[4]) {
    unsigned r[4];
    philox4x32_10(g, offset, seed, r);
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
}

// x + N(0, scale): THE expression of the augmentation (one place, so that every kernel contracts it alike)
__device__ __forceinline__ float add_noise(float x, float scale, float z) { return x + scale * z; }

// the draw of the single element i (the pair of its group it belongs to: half the Box-Muller work of the whole group)
__device__ __forceinline__ float noise_one(float x, size_t i, float scale, unsigned long long seed, unsigned long long offset) {
    unsigned r[4];
    philox4x32_10(i / 4, offset, seed, r);
    const bool hi = (i & 2) != 0;
    float n0, n1;
    box_muller(hi ? r[2] : r[0], hi ? r[3] : r[1], n0, n1);
    return add_noise(x, scale, (i & 1) ? n1 : n0);
}

}  // namespace smh_rng
