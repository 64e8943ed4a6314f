// Wave-level sums: the DPP float sum of the heads-training kernels (smh_train.hip, smh_train_cascade.hip,
// smh_train_single.hip) and the xor-tree f64 sum of the f64 statistics (smh_silence.hip, smh_feat.h, smh_scale.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace smh {

// Sum over the 64 lanes, result in every lane, as a butterfly: lane i adds lane i ^ 32, then ^ 16, ... ^ 1.  Results that
// are compared bit for bit (the per-file StandardScaler, the normalisation means, the mixing energies) were fixed on this
// order.  smh_tcn::wave_sum_f below adds in ANOTHER order (rows of 16 first) and must not replace it.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
}  // namespace smh

namespace smh_tcn {

// Sum over the 64 lanes, result in every lane, on the VALU's lane-permute paths: four DPP steps inside each row of 16 lanes
// (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror), then gfx950's v_permlane32_swap / v_permlane16_swap
// across the rows.  (__shfl_xor is a ds_bpermute per step -- an LDS round trip, six of them in a dependent chain: the
// heads kernel makes ~350 of these sums per step and spent most of its time in them.)
__device__ __forceinline__ float wave_sum_f(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xF, 0xF, false));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
    v += dpp(v, std::integral_constant<int, 0x141>{});  // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>{});  // row_mirror: every lane holds the sum of its row of 16
    const unsigned u = __float_as_uint(v);
    const auto r32 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
    const unsigned u2 = __float_as_uint(v);
    const auto r16 = __builtin_amdgcn_permlane16_swap(u2, u2, false, false);
    return __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
}
}  // namespace smh_tcn
