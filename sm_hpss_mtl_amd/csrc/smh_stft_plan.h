// Launch plan of the STFT (smh_stft.hip, smh_stft_f64.hip): which kernel, how many frames per work item, how many tiles per clip, on
// which grid with how much LDS -- decided here, once, as a plain value.  smh_stft_mag_f32, the ragged launch, the routers of the front
// ends (smh_frontend.hip, smh_ragged.hip, smh_plain.hip), smh_ctx.hip and the test queries (smh_internal_stft_route, _plan) all take
// it from these functions.  Host arithmetic only, no HIP: a stand-alone host program can include this header by itself.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "smh_xcd.h"

namespace smh_stft {

// what of a context the plan depends on (smh_rag.h: geom_of); f64: stft_precision 1, f64_pass: its frames per LDS pass (f64_frames)
struct Geom { int n_fft, win_length, hop, M, K, f64, f64_pass; };

// The implementation switches of the STFT launches (A/B runs, tuning, tests), the only getenv of these launches.  Read once per call:
// tests flip them between calls.  (SMH_STFT_ROW and SMH_STFT_PROBE_NOSTORE make outputs invalid: probe_env reads in the launcher.)
struct StftSwitches {
    bool generic = false;          // SMH_STFT_GENERIC set: never the specialised kernel
    int pairs = 1;                 // SMH_STFT_PAIRS=0: stft400_kernel's round-robin phase 1 and one-frame phase 3 on every tile; same bits
    int maxf = 20, threads = 256;  // SMH_STFT_FRAMES=maxf,threads: the specialised equal-length plan (tools/gpu/r2_stft_tune.sh)
    bool xcd = true;               // SMH_STFT_XCD=0: the plain (tile, clip) grid of an equal-length launch
};
inline StftSwitches read_stft_switches() {
    StftSwitches s;
    s.generic = getenv("SMH_STFT_GENERIC") != nullptr;
    const char *ev = getenv("SMH_STFT_PAIRS");
    s.pairs = ev && atoi(ev) == 0 ? 0 : 1;
    if ((ev = getenv("SMH_STFT_FRAMES"))) sscanf(ev, "%d,%d", &s.maxf, &s.threads);
    if (s.threads != 512) s.threads = 256;
    s.maxf = s.maxf < 1 ? 1 : s.maxf > s.threads / 8 ? s.threads / 8 : s.maxf;  // phase 2 has 8 items per frame, one per thread
    ev = getenv("SMH_STFT_XCD");
    s.xcd = !ev || atoi(ev) != 0;
    return s;
}

// ---- kernel choice, numbered as smh_internal_stft_route answers ----------------------------------------------------------------
enum Kernel { kGeneric = 0, kSpecialised = 1, kF64 = 2 };  // stft_mag_kernel, stft400_kernel (8 x 25), stft_f64_kernel
// frames per work item at most, by kernel.  Specialised: 20 frames are 37 KB of LDS and, at 128 VGPRs, FOUR 256-thread workgroups per
// CU, T = 98 -> 5 tiles; 25 frames (45 KB: three per CU) measured 69-71 us against 64.6, 16 and fewer leave half of phase 2's threads
// idle.  The ragged planners size their item tables from these (rag_frames).
constexpr int kItemFrames[3] = {16, 20, 16};
constexpr int kThreads = 256;  // the generic and f64 kernels, and the specialised one in a ragged call
constexpr size_t kLdsLimit = 150 * 1024;     // dynamic LDS a launch may ask for
constexpr size_t kF64PairLimit = 64 * 1024;  // f64: two workgroups per CU below it

// the specialised kernel reads the audio as float2: n_fft = 400 with an even hop, and every frame on an 8-byte boundary (aligned8)
inline bool rag_needs_aligned8(const Geom &g, const StftSwitches &sw) {
    return !g.f64 && g.n_fft == 400 && g.M == 200 && g.win_length <= 400 && g.hop % 2 == 0 && !sw.generic;
}
inline bool clip_aligned8(uintptr_t address) { return address % 8 == 0; }
// an equal-length batch: an odd clip length only matters for where the NEXT clip starts, so a single clip keeps the kernel
inline bool frames_aligned8(uintptr_t first_clip, int B, int n_samples) { return (n_samples % 2 == 0 || B == 1) && clip_aligned8(first_clip); }
inline Kernel stft_kernel(const Geom &g, const StftSwitches &sw, bool aligned8) {
    return g.f64 ? kF64 : rag_needs_aligned8(g, sw) && aligned8 ? kSpecialised : kGeneric;
}
inline int rag_frames(const Geom &g, const StftSwitches &sw, bool aligned8) { return kItemFrames[stft_kernel(g, sw, aligned8)]; }

// ---- LDS of the three kernels, from their layouts ------------------------------------------------------------------------------
constexpr int kMP400 = 201;  // stft400_kernel: float2 stride of one frame (odd: conflict-free phase-2 and phase-3 reads)
// stft400_kernel<row>: 8 rows of twiddles, M + 2 untangle twiddles, 8 rows of window pairs, F frames; float2 each
inline size_t lds400_bytes(int row, int F) { return 8 * ((size_t)8 * row + 202 + 8 * row + (size_t)F * kMP400); }
inline size_t padded_frame(int M) { return (size_t)M + (M >> 4) + 2; }  // frame stride of the Stockham kernels: one pad per 16, + 2
// stft_mag_kernel: M twiddles, M + 1 untangle twiddles, two buffers of tt padded frames; float2 each
inline size_t generic_lds_bytes(int M, int tt) { return 8 * ((size_t)M + (M + 1) + 2 * (size_t)tt * padded_frame(M)); }
// stft_f64_kernel: the same and the n_fft = 2 M window values; double2 each
inline size_t f64_lds_bytes(int M, int tt) { return 16 * ((size_t)M + (M + 1) + M + 2 * (size_t)tt * padded_frame(M)); }
// f64 frames per LDS pass: up to 8 (two workgroups per CU at n_fft = 400: 63 KB each), fewer for a large n_fft; 0: not one frame fits
inline int f64_frames(int M) {
    for (int tt = 8; tt >= 1; --tt)
        if (f64_lds_bytes(M, tt) <= kF64PairLimit || (tt == 1 && f64_lds_bytes(M, 1) <= kLdsLimit)) return tt;
    return 0;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
struct StftPlan {
    Kernel kernel;
    int frames, pass_frames;  // frames per work item, and for f64 per LDS pass (else 0)
    int tiles, threads;       // tiles per clip (0 in a ragged call)
    size_t lds;               // dynamic LDS bytes
    unsigned grid_x, grid_y;
    int xcd_tiles;     // > 0: the 1-D per-XCD grid of an equal-length launch (smh_xcd.h), = tiles; 0: the plain (tile, clip) grid
    int pairs;         // specialised: StftSwitches::pairs; else 0
    char refusal[80];  // non-empty: the launch is refused (SMH_E_INVALID) with this text
};
inline void size_lds(const Geom &g, const char *who, StftPlan &p) {  // (row 25; the probe SMH_STFT_ROW sizes its own)
    p.pass_frames = p.kernel == kF64 ? g.f64_pass : 0;
    p.lds = p.kernel == kSpecialised ? lds400_bytes(25, p.frames)
            : p.kernel == kF64       ? f64_lds_bytes(g.M, g.f64_pass) : generic_lds_bytes(g.M, p.frames);
    if (p.kernel != kGeneric) return;
    if (p.lds > kLdsLimit)
        snprintf(p.refusal, sizeof p.refusal, "%s: n_fft=%d too large for the LDS FFT", who, g.n_fft);
    else if ((size_t)p.frames * g.K >= (1u << 20))  // fdiv's exact range (K >= 65536: behind the LDS refusal on either path)
        snprintf(p.refusal, sizeof p.refusal, "%s: tile too large", who);
}
// B equal clips of T >= 1 frames.  T is split evenly into tiles of at most maxf frames (98 -> 5 x 20, the last with 18; generic and
// f64 7 x 14); the specialised plan rounds an odd tile up for an even T so that every tile can take phase 3 in frame pairs.
inline StftPlan plan_equal(const Geom &g, const StftSwitches &sw, bool aligned8, int B, int T) {
    StftPlan p{};
    p.kernel = stft_kernel(g, sw, aligned8);
    const bool spec = p.kernel == kSpecialised;
    const int maxf = spec ? sw.maxf : kItemFrames[p.kernel];
    p.threads = spec ? sw.threads : kThreads, p.pairs = spec ? sw.pairs : 0;
    p.tiles = (T + maxf - 1) / maxf;
    p.frames = (T + p.tiles - 1) / p.tiles;
    if (p.pairs && T % 2 == 0 && p.frames % 2 != 0 && p.frames < maxf) ++p.frames;
    p.tiles = (T + p.frames - 1) / p.frames;
    size_lds(g, "smh_stft_mag_f32", p);
    const long long items = (long long)B * p.tiles;
    const bool xcd = sw.xcd && smh::xcd_fits(items);
    p.xcd_tiles = xcd ? p.tiles : 0;
    p.grid_x = xcd ? smh::xcd_grid(items) : (unsigned)p.tiles, p.grid_y = xcd ? 1u : (unsigned)B;
    return p;
}
// n_items (clip, tile) items of clips of different lengths: always the per-XCD grid, the item size of rag_frames, 256 threads
inline StftPlan plan_rag(const Geom &g, const StftSwitches &sw, bool aligned8, int n_items) {
    StftPlan p{};
    p.kernel = stft_kernel(g, sw, aligned8);
    p.frames = kItemFrames[p.kernel], p.threads = kThreads, p.pairs = p.kernel == kSpecialised ? sw.pairs : 0;
    size_lds(g, "ragged STFT", p);
    p.grid_x = smh::xcd_grid(n_items), p.grid_y = 1;
    return p;
}

// smh_internal_stft_plan's answer: ten ints, in the order of StftPlan's members
inline void stft_plan_ints(const StftPlan &p, int *out) {
    const int v[10] = {p.kernel,   p.frames,      p.pass_frames, p.tiles,     p.threads,
                       (int)p.lds, (int)p.grid_x, (int)p.grid_y, p.xcd_tiles, p.pairs};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}

}  // namespace smh_stft
