// librosa.util.softmask(X, X_ref, power=2, split_zeros=True) for both orientations at once, as librosa.decompose.hpss calls it with
// margin 1: mh = softmask(h, p), mp = softmask(p, h).  The one statement of the mask pair for the feature stage (smh_feat.hip), the
// ragged feature walk (smh_ragged.hip) and the resynthesis (smh_hpss_audio.hip).
// numpy's float32 operation order: Z = max(h, p); bad = Z < tiny -> Z = 1; (h / Z)^2 and (p / Z)^2, each rounded; m / (m + r);
// bad -> 0.5 for both.
#pragma once
#include <cfloat>

#include <hip/hip_runtime.h>

namespace smh {

// numpy's bits: IEEE divisions, and no FMA contraction (numpy rounds the squares and their sum)
__device__ __forceinline__ void softmask_pair(float h, float p, float &mh, float &mp) {
    float Z = fmaxf(h, p);
    const bool bad = Z < FLT_MIN;
    Z = bad ? 1.0f : Z;
    const float a = h / Z, b = p / Z;
    const float m = __fmul_rn(a, a), r = __fmul_rn(b, b);
    const float den = __fadd_rn(m, r);
    mh = m / den, mp = r / den;
    mh = bad ? 0.5f : mh;
    mp = bad ? 0.5f : mp;
}

// The same masks for the FUSED paths: hardware reciprocals (1 ulp) instead of IEEE divisions.  The masked spectra are not outputs
// there; the dB features they feed are compared at 1e-3 dB (SURVEY 8d').
__device__ __forceinline__ void softmask_pair_fast(float h, float p, float &mh, float &mp) {
    float Z = fmaxf(h, p);
    const bool bad = Z < FLT_MIN;
    Z = bad ? 1.0f : Z;
    const float iz = __builtin_amdgcn_rcpf(Z);
    const float a = h * iz, b = p * iz;
    const float m = a * a, r = b * b;
    const float id = __builtin_amdgcn_rcpf(m + r);
    mh = m * id, mp = r * id;
    mh = bad ? 0.5f : mh;
    mp = bad ? 0.5f : mp;
}

}  // namespace smh
