// Length-array ("ragged") form of the front end: what the kernels read when clips of DIFFERENT lengths share one launch.
// The reference's callers feed one file at a time (Proposed_Work_Results.py:92-95, 131-134, 189-192, 465-474 -> get_featuregram,
// lib/preprocessing.py:355-457, and get_feature_patches, :137-292); here the files of a batch are one launch per stage: every
// kernel takes a per-clip descriptor table and a flat (clip, tile) work list built on the host by smh_frontend_ragged_f32
// (smh_ragged.hip) and uploaded once per call.  The host half -- the planner below -- is shared by every front end with a ragged
// entry ("Ragged batches": what a front end supplies); its implementation lives in smh_ragged.hip.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "smh_common.h"
#include "smh_median_plan.h"
#include "smh_stft_plan.h"

namespace smh_feat {
struct PatchOut;  // smh_feat.h: where a call's patches go
}

namespace smh_rag {

// one clip of a ragged call (64 bytes; offsets in floats from the call's base pointers)
struct Clip {
    long long audio_off;  // d_audio
    long long spec_off;   // workspace S and perc: (K, T) each, rows of exactly T floats as in the equal-length layout; multiple of 4
    long long harm_off;   // workspace harm: the 16-frame blocked image (ceil(T/16), K, 16); multiple of 4
    long long fv_off;     // d_fv: (2*rows, T)
    long long patch_off;  // d_patches: patches in front of this clip's
    int T;                // frames, 1 + (n_samples - n_fft) / hop
    int Ttiled;           // frames after tile-if-short (lib/preprocessing.py:139-142)
    int nP;               // patches (0: none asked for)
    int row0;             // first row of this clip in the per-row statistics table (long clips only)
    int n_samples;        // samples of the clip: set and read by the ragged HPSS audio separation only (smh_hpss_audio.hip), else 0
    int pad_;
};
static_assert(sizeof(Clip) == 64, "smh_rag::Clip is read with 16-byte scalar loads");

// one workgroup's share of a stage: tile / chunk `tile` of clip `clip`
struct Item {
    int clip, tile;
};

// The feature path of a clip of T frames when no taps are asked for, decided once for smh_frontend_f32 and the ragged planner
// (and reported by smh_internal_frontend_route):
//   0  the LDS image, even T: features_half_kernel      1  the LDS image, odd T (or SMH_FEAT_NOPAIR): features_clip_kernel
//   2  the streaming kernels of smh_ragged.hip           3  neither: launch_hp_feat + launch_std_patch on the whole clip
int feature_route(const smh_ctx *ctx, const smh_median::MedianSwitches &msw, int T);
// smh_frontend_f32's route 2 for B equal clips: the streaming kernels of smh_ragged.hip on the tables of B equal clips (returns 1 if
// it ran, 0 if this context or shape has no ragged kernels, < 0 on error), and what that adds to the workspace
size_t equal_overhead_bytes(const smh_ctx *ctx, int B, int T);
int run_equal(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int T, const smh_feat::PatchOut &po, float *d_fv, void *d_work,
              size_t work_bytes, const smh_median::MedianSwitches &msw, bool stft_aligned8, hipStream_t st);

// Which clips the ragged STFT and median launches take, decided once for every entry that chains them (smh_frontend_ragged_*,
// smh_hpss_audio_ragged_f32); a clip they do not take goes alone through the entry's equal-length form, with the same bits.
//   medians_ok   the context has a block-split median kernel (rag_tile_frames > 0) and SMH_RAGGED_PERFILE is not set
//   clip_ok      both medians fold once per side (fast_ok) and the clip's rows fit 32-bit offsets
//   start_ok     the clip starts where the STFT kernel of an aligned call can take it: on 8 bytes where the f32 STFT reads float2
bool medians_ok(const smh_ctx *ctx, const smh_median::MedianSwitches &msw);
bool clip_ok(const smh_ctx *ctx, int T);
bool start_ok(const smh_ctx *ctx, const smh_stft::StftSwitches &sw, const float *d_audio, long long off);

// ---- the host-side planner of a ragged entry (smh_frontend_ragged_*, smh_plain_frontend_ragged_*, smh_hpss_audio_ragged_*) ------
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// where every clip of a call lies in the caller's buffers: frames, patches, and the floats / patches in front of clip b (B + 1 sums);
// fv_rows: featuregram rows per clip (2 * feat_rows with the H || P pair); `who` prefixes the error texts
struct Layout {
    std::vector<int> T, nP;
    std::vector<long long> fv_off, patch_off;
};
int plan_layout(const smh_ctx *ctx, const char *who, const long long *off, const int *len, int B, int W, int shift, bool patches,
                int fv_rows, Layout &p);
// the layout into the arrays of a *_ragged_sizes call (any of them may be null)
void export_layout(const Layout &p, int B, long long *h_fv_off, long long *h_patch_off, int *h_T, int *h_nP);
// what a *_ragged_sizes call asks for: every clip at once (total) up to 8 GiB, never less than the largest single clip needs (single)
size_t work_size(int B, size_t single, size_t total);

struct HostClip {  // one clip a sub-batch takes
    long long audio_off, fv_off, patch_off;
    int T, Ttiled, nP;
    int cls;  // the front end's own class of the clip (smh_ragged.hip: the feature route; unused by smh_plain.hip)
};
HostClip host_clip(const Layout &p, const long long *off, int b, int W /* >= 1: PatchOut's */, int cls);
// the descriptors of a sub-batch (harm_off and row0 stay 0); returns the floats of S: the sum of K * T, each rounded up to 4
size_t fill_clips(const HostClip *hc, int n, int K, bool patches, std::vector<Clip> &clips);

// The tables of one sub-batch as ONE blob at the start of the workspace: every add() places its region on the next 16-byte
// boundary, in the order of the calls, and returns the region's offset -- the handle at<>() turns into a device pointer.
class Tables {
  public:
    size_t add(const void *src, size_t bytes);  // src == nullptr: zeros (the max keys)
    // the (clip, tile) work list of a stage of `frames` frames per item over the clips of class cls (-1: all of them)
    size_t add_items(const HostClip *hc, int n, int frames, int cls, int *count);
    // one copy through a pinned slot of the context, stream-ordered on st; before it, the sub-batch's true extent -- the tables and
    // `behind` bytes of device regions behind them -- is checked against the workspace (SMH_E_WORKSPACE, `who` in the text)
    int upload(const smh_ctx *ctx, const char *who, char *d_work, size_t work_bytes, size_t behind, hipStream_t st);
    template <class T>
    T *at(size_t off) const { return reinterpret_cast<T *>(d_ + off); }
    char *behind() const { return d_ + align_up(blob_.size(), 256); }  // the first device region behind the tables

  private:
    std::vector<char> blob_;
    char *d_ = nullptr;
};

// clips [0, n) in as few sub-batches as the workspace allows by the front end's estimate: `fixed` bytes plus bytes(b) per clip;
// run(first, count) enqueues one.  A clip the estimate finds too large even alone is tried alone: Tables::upload decides by its true
// extent.  Refuses a capturing stream before anything is enqueued (the tables come from a staging buffer).
int run_sub_batches(size_t n, size_t fixed, size_t work_bytes, hipStream_t st,
                    const std::function<size_t(size_t)> &bytes, const std::function<int(size_t, size_t)> &run);
// the clips no sub-batch took (!taken(b)), one by one through the equal-length entry on the same stream:
// alone(b, W, shift, fv, patches) with W = shift = 0 and patches = nullptr for a clip without patches
int run_alone(const Layout &p, int B, int W, int shift, int fv_rows, float *d_fv, float *d_patches,
              const std::function<bool(int)> &taken, const std::function<int(int, int, int, float *, float *)> &alone);

// An entry WITHOUT a workspace argument that needs a small host table on the device (smh_gather.hip): the table goes through a
// pinned slot of the context into the slot's own device twin, stream-ordered on st, and launch(d_table) enqueues the kernel that
// reads it; the slot is reused only after that kernel has finished.  Refuses a capturing stream before anything is enqueued.
int launch_with_table(const smh_ctx *ctx, const char *who, const void *src, size_t bytes, hipStream_t st,
                      const std::function<int(const void *)> &launch);

}  // namespace smh_rag

namespace smh_stft {  // the launches of a plan of smh_stft_plan.h
inline Geom geom_of(const smh_ctx *c) { return Geom{c->cfg.n_fft, c->cfg.win_length, c->cfg.hop, c->M, c->K, c->stft_f64, c->stft64_frames}; }
// |STFT| of every (clip, frame tile) item into the workspace; items of rag_frames(geom, sw, aligned8) frames: sw as the tables were sized
int launch_rag(const smh_ctx *ctx, const StftSwitches &sw, const float *d_audio, float *d_S, const smh_rag::Clip *d_clips,
               const smh_rag::Item *d_items, int n_items, bool aligned8, hipStream_t st);
// the f64 STFT of smh_stft_f64.hip under plan p: n_items items of a ragged call (d_clips != nullptr), else B = n_items clips of n_samples
int launch_f64(const smh_ctx *ctx, const StftPlan &p, const char *what, const float *d_audio, int n_items, int n_samples, int T, float *d_S,
               const smh_rag::Clip *d_clips, const smh_rag::Item *d_items, hipStream_t st);
}  // namespace smh_stft

namespace smh_median {  // the launches of a plan of smh_median_plan.h; sw: as the caller routed and sized its tables
// both HPSS medians of every (clip, frame tile) item of rag_tile_frames(K, lh, lp, sw) frames; harm in the 16-frame blocked layout
int launch_rag(const MedianSwitches &sw, const float *d_S, float *d_harm, float *d_perc, int K, int lh, int lp, const smh_rag::Clip *d_clips,
               const smh_rag::Item *d_items, int n_items, hipStream_t st);
// both HPSS medians of B equal clips in one launch where the pair is fused; returns the harm layout written -- want_layout where the
// kernel has it (2: blocked_harm_ok(K, T, lh, lp, sw)), else 1 or 0 --, < 0 on error
int launch_hpss(const MedianSwitches &sw, const float *S, int B, int K, int T, int lh, int lp, float *harm, float *perc, int want_layout,
                hipStream_t st);
}  // namespace smh_median
