// The per-clip table of the entries that work on featuregrams ALREADY on the device (smh_scale.hip, smh_skew.hip): B dense (rows, T_b)
// float32 featuregrams, separate allocations or views of one buffer, described by one 32-byte record each and uploaded through
// smh_rag::launch_with_table.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "smh_common.h"

namespace smh_fvtable {

constexpr size_t kTableBytes = 64 * 1024;  // one launch's table: what a staging slot holds without growing

// one featuregram of a call (32 bytes)
struct FvClip {
    const float *fv;      // (rows, T), dense
    long long patch_off;  // patches in front of this clip's
    int T, Ttiled, nP, pad_;
};
static_assert(sizeof(FvClip) == 32, "FvClip is a 32-byte table entry");
constexpr int kMaxClips = (int)(kTableBytes / sizeof(FvClip));

// the table of clips [b0, b0 + n); W < 1: no patch geometry (the moments).  patch_off runs on over the whole call.
inline int fill_table(const char *who, const float *const *h_fv, const int *h_T, int b0, int n, int W, int shift, long long &patch_off,
                      int &max_T, std::vector<FvClip> &t) {
    t.resize(n);
    for (int i = 0; i < n; ++i) {
        const int b = b0 + i, T = h_T[b];
        SMH_REQUIRE(h_fv[b] && T >= 1, "%s: featuregram %d is null or has T=%d frames", who, b, T);
        SMH_REQUIRE((reinterpret_cast<uintptr_t>(h_fv[b]) % 4) == 0, "%s: featuregram %d is not float-aligned", who, b);
        FvClip &c = t[i];
        c.fv = h_fv[b], c.T = T, c.pad_ = 0;
        c.Ttiled = W >= 1 ? smh_tiled_frames(T, W) : T;
        c.nP = W >= 1 ? smh_num_patches(c.Ttiled, W, shift) : 0;
        c.patch_off = patch_off;
        patch_off += c.nP;
        max_T = std::max(max_T, T);
    }
    return SMH_OK;
}

}  // namespace smh_fvtable
