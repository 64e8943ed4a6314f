// Launch plan of the HPSS audio resynthesis (smh_hpss_audio.hip: masked complex STFT and overlap-add ISTFT): the tile of frames a
// workgroup owns, its halo, the frames per LDS pass, the LDS bytes and the refusals -- decided here, once, as a plain value.
// smh_hpss_resynth_f32, smh_hpss_audio_f32 and the test query smh_internal_resynth_plan all take it from plan().  Host arithmetic
// only, no HIP: a stand-alone host program can include this header by itself.
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

}  // namespace smh_resynth
