// Launch plan of the HPSS audio resynthesis (smh_hpss_audio.hip: masked complex STFT and overlap-add ISTFT): the tile of frames a
// workgroup owns, its halo, the frames per LDS pass, the LDS bytes and the refusals -- decided here, once, as a plain value.
// smh_hpss_resynth_f32, smh_hpss_audio_f32 and the test query smh_internal_resynth_plan all take it from plan(); the ragged entry
// smh_hpss_audio_ragged_f32 takes the same plan for its refusals and LDS and, for clips of different lengths in one launch, plan_rag()
// and the per-clip sizes below it.  Host arithmetic only, no HIP: a stand-alone host program can include this header by itself.
//
// Tile.  A workgroup owns the kTileFrames * hop output samples that start at frame t0's first sample (the last tile of a clip owns
// the rest of the clip too: the last frame's tail and the zeros behind it).  Frame t reaches the samples t * hop .. t * hop +
// n_fft - 1, so the owned samples are reached by the tile's own frames and by the halo = ceil(n_fft / hop) - 1 frames in front of
// t0; the same number of frames behind the tile reach into the NEXT tile's samples and are that tile's halo.  A workgroup therefore
// transforms tile + halo frames (16 + 2 at (400, 160): 12.5 % recomputed; 16 + 3 at (512, 160)) and needs no exchange with its
// neighbours: no atomics, and a sample is the sum of its frames in ascending frame order whatever the tile, the batch or the run.
//
// LDS budget (bytes, M = n_fft / 2, MP = M + M / 16 + 2 the padded float2 stride of a frame as in the STFT's Stockham kernel):
//   tables        8 M + 8 (M + 1) + 4 n_fft        FFT twiddles, real-FFT (un)tangle twiddles, window
//   pass buffers  4 * kPassFrames * 8 MP           forward ping-pong pair = harmonic inverse pair, percussive inverse pair
//   accumulators  2 * 4 ((tile - 1) hop + n_fft)   overlap-add numerators of y_harm and y_perc
//   (400, 400, 160): 4,808 + 27,392 + 22,400 = 54,600      (512, 400, 160): 6,152 + 35,072 + 23,296 = 64,520
// Either way two 256-thread workgroups per CU (160 KB).  kPassFrames = 4: the inverse runs the harmonic and the percussive spectrum of
// the pass as 8 independent length-M transforms, 8 * M / radix = 200..256 butterflies per stage for 256 threads; 8 frames per pass
// would be one workgroup per CU at n_fft = 512.  kTileFrames = 16: one second (T = 98) is 7 tiles per clip, 7168 workgroups per
// 1024 clips; 32 would halve the recomputation (6 %) and double the accumulators (one workgroup per CU at 512).
#pragma once
#include <cstddef>
#include <cstdio>

#include "smh_xcd.h"

namespace smh_resynth {

struct Geom { int n_fft, hop, M; };

constexpr int kThreads = 256;
constexpr int kTileFrames = 16;  // frames whose first hop samples a workgroup owns
constexpr int kPassFrames = 4;   // frames transformed per LDS pass
constexpr int kMaxHalo = kTileFrames;        // n_fft <= (kMaxHalo + 1) * hop: at most as many halo frames as tile frames
constexpr size_t kLdsLimit = 150 * 1024;     // dynamic LDS a launch may ask for
constexpr unsigned kMaxGridY = 65535;        // clips per launch (grid.y)

inline int halo_frames(const Geom &g) { return (g.n_fft + g.hop - 1) / g.hop - 1; }
inline size_t padded_frame(int M) { return (size_t)M + (M >> 4) + 2; }  // float2 stride of one frame, as smh_stft::padded_frame
inline size_t acc_samples(const Geom &g) { return (size_t)(kTileFrames - 1) * g.hop + g.n_fft; }
inline size_t lds_bytes(const Geom &g) {
    return 8 * ((size_t)g.M + (g.M + 1)) + 4 * (size_t)g.n_fft + 4 * (size_t)kPassFrames * 8 * padded_frame(g.M) + 2 * 4 * acc_samples(g);
}

struct Plan {
    int tile, halo, pass, threads;
    int tiles;         // per clip
    size_t lds;        // dynamic LDS bytes
    size_t acc;        // samples of one accumulator
    char refusal[96];  // non-empty: the launch is refused (SMH_E_INVALID) with this text
};

// a clip of T >= 1 frames
inline Plan plan(const Geom &g, int T) {
    Plan p{};
    p.tile = kTileFrames, p.pass = kPassFrames, p.threads = kThreads;
    p.halo = g.hop > 0 ? halo_frames(g) : 0;
    p.tiles = (T + p.tile - 1) / p.tile;
    p.lds = lds_bytes(g), p.acc = acc_samples(g);
    if (g.hop > g.n_fft)
        snprintf(p.refusal, sizeof p.refusal, "hop=%d > n_fft=%d: frames that do not touch cannot be overlap-added", g.hop, g.n_fft);
    else if (p.halo > kMaxHalo)
        snprintf(p.refusal, sizeof p.refusal, "n_fft=%d > %d * hop=%d: more than %d overlapping frames per sample", g.n_fft, kMaxHalo + 1,
                 g.hop, kMaxHalo + 1);
    else if (p.lds > kLdsLimit)
        snprintf(p.refusal, sizeof p.refusal, "n_fft=%d, hop=%d need %zu bytes of LDS, the limit is %zu", g.n_fft, g.hop, p.lds, kLdsLimit);
    return p;
}

// ---- clips of different lengths in one launch (hpss_resynth_rag_kernel) --------------------------------------------------------
// The work list is flat: one (clip, tile) item per kTileFrames frames of every clip, clip-major, on the 1-D per-XCD grid (smh_xcd.h);
// a workgroup takes T, the sample count and every offset from its clip's descriptor.  The medians of a ragged call write harm in
// 16-frame blocks, (ceil(T / 16), K, 16): element (k, t) at ((t >> 4) * K + k) * 16 + (t & 15).  A resynthesis tile starts on a
// multiple of kTileFrames = 16 frames, so its own frames are one block and its halo frames (at most kMaxHalo = 16) lie in the block
// before.  S and perc are (K, T) rows of exactly T floats, each clip's rounded up to 4 floats so that the next starts on 16 bytes.
constexpr int kHarmBlock = 16;  // frames per block of the blocked harm image (smh_median_plan.h: layout 2)
static_assert(kTileFrames % kHarmBlock == 0 && kMaxHalo <= kHarmBlock, "a tile starts on a harm block, its halo lies in the block before");

inline int rag_items(int T) { return (T + kTileFrames - 1) / kTileFrames; }  // items of a clip of T frames
inline size_t rag_spec_floats(int K, int T) { return ((size_t)K * T + 3) / 4 * 4; }  // S, and perc, of a clip in the workspace
inline size_t rag_harm_floats(int K, int T) { return (size_t)((T + kHarmBlock - 1) / kHarmBlock) * K * kHarmBlock; }  // blocked harm
// workspace bytes a clip adds to a ragged call: S, perc, blocked harm, its descriptor (64 bytes) and its 8-byte (clip, tile) items
// of the three stages -- the STFT's and the medians' tiles of stft_frames and med_frames frames, the resynthesis tiles
inline size_t rag_clip_bytes(int K, int T, int stft_frames, int med_frames) {
    const size_t items = (size_t)(T + stft_frames - 1) / stft_frames + (size_t)(T + med_frames - 1) / med_frames + (size_t)rag_items(T);
    return 4 * (2 * rag_spec_floats(K, T) + rag_harm_floats(K, T)) + 64 + 8 * items;
}

struct RagPlan {
    int tile, halo, pass, threads;
    unsigned grid_x, grid_y;  // the per-XCD grid of n_items items
    size_t lds, acc;
    char refusal[96];  // plan()'s: it depends on the context alone, so it holds for the ragged call as a whole
};
inline RagPlan plan_rag(const Geom &g, long long n_items) {
    const Plan q = plan(g, 1);
    RagPlan p{};
    p.tile = q.tile, p.halo = q.halo, p.pass = q.pass, p.threads = q.threads, p.lds = q.lds, p.acc = q.acc;
    p.grid_x = smh::xcd_grid(n_items), p.grid_y = 1;
    snprintf(p.refusal, sizeof p.refusal, "%s", q.refusal);
    return p;
}

}  // namespace smh_resynth
