"""Python restatement of the STFT's launch plan (sm_hpss_mtl_amd/csrc/smh_stft_plan.h: plan_equal, plan_rag; smh_xcd.h) -- TEST
INFRASTRUCTURE.  It computes no numbers: it says which kernel an STFT call runs, with how many frames per work item, how many tiles
per clip, how many threads, how much dynamic LDS and on which grid.

Written from the kernels' LDS layouts (smh_stft.hip, smh_stft_f64.hip), not from the header.  tests/test_stft_plans.py pins the
boundaries by hand; tests/test_stft_plan_gpu.py holds every value to the library's own answer (smh_internal_stft_plan), so a
constant that moves in the header without moving here fails there.
"""
from __future__ import annotations

import re

LDS_LIMIT = 150 * 1024        # the dynamic LDS a launch may ask for: beyond it the generic kernel's launch is refused
F64_PAIR_LIMIT = 64 * 1024    # f64: two workgroups share a CU below it
GENERIC, SPECIALISED, F64 = 0, 1, 2                  # smh_internal_stft_route's numbers
ITEM_FRAMES = {GENERIC: 16, SPECIALISED: 20, F64: 16}
SWITCHES = ("SMH_STFT_GENERIC", "SMH_STFT_PAIRS", "SMH_STFT_FRAMES", "SMH_STFT_XCD")
# the order of smh_internal_stft_plan's ints (stft_plan_ints)
FIELDS = ("kernel", "frames", "pass_frames", "tiles", "threads", "lds", "grid_x", "grid_y", "xcd_tiles", "pairs")


class Refused(Exception):
    pass


def _atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def switches(env=None):
    """(generic, pairs, maxf, threads, xcd) under the switches that are set (read_stft_switches)."""
    env = env or {}
    maxf, threads = 20, 256
    if "SMH_STFT_FRAMES" in env:                      # sscanf("%d,%d"): what does not parse keeps its default
        m = re.match(r"\s*([+-]?\d+)(?:,\s*([+-]?\d+))?", env["SMH_STFT_FRAMES"])
        if m:
            maxf = int(m.group(1))
            threads = int(m.group(2)) if m.group(2) else threads
    threads = 512 if threads == 512 else 256
    maxf = max(1, min(maxf, threads // 8))            # phase 2 of the specialised kernel: 8 items per frame, one per thread
    pairs = 0 if "SMH_STFT_PAIRS" in env and _atoi(env["SMH_STFT_PAIRS"]) == 0 else 1
    xcd = "SMH_STFT_XCD" not in env or _atoi(env["SMH_STFT_XCD"]) != 0
    return "SMH_STFT_GENERIC" in env, pairs, maxf, threads, xcd


def rag_needs_aligned8(geom, f64=False, env=None):
    """Whether the specialised kernel is reachable in this context: n_fft = 400 with an even hop, f32, not forced generic.  It reads
    the audio as float2, so every clip of a ragged call must then start on an 8-byte boundary."""
    n_fft, wl, hop = geom
    return not f64 and n_fft == 400 and wl <= 400 and hop % 2 == 0 and not switches(env)[0]


def frames_aligned8(address, B, n_samples):
    """An equal-length batch: every frame of every clip on an 8-byte boundary (an odd length moves the NEXT clip only)."""
    return address % 8 == 0 and (n_samples % 2 == 0 or B == 1)


def route(geom, f64, aligned8, env=None):
    return F64 if f64 else SPECIALISED if rag_needs_aligned8(geom, f64, env) and aligned8 else GENERIC


def _padded(M):
    return M + (M >> 4) + 2                            # frame stride of the Stockham kernels: one pad per 16 elements, + 2


def lds_specialised(F, row=25):
    """stft400_kernel: 8 rows of twiddles, 202 untangle twiddles, 8 rows of window pairs, F frames at stride 201; float2."""
    return 8 * (8 * row + 202 + 8 * row + F * 201)


def lds_generic(n_fft, tt):
    """stft_mag_kernel: M twiddles, M + 1 untangle twiddles, two buffers of tt padded frames; float2."""
    M = n_fft // 2
    return 8 * (M + (M + 1) + 2 * tt * _padded(M))


def lds_f64(n_fft, tt):
    """stft_f64_kernel: the same and n_fft = 2 M window values (M double2); double2."""
    M = n_fft // 2
    return 16 * (M + (M + 1) + M + 2 * tt * _padded(M))


def f64_pass_frames(n_fft):
    """Frames per LDS pass of an f64 context: the most, up to 8, under 64 KB; one if only that fits 150 KB; 0: the context is refused."""
    for tt in range(8, 0, -1):
        if lds_f64(n_fft, tt) <= F64_PAIR_LIMIT:
            return tt
    return 1 if lds_f64(n_fft, 1) <= LDS_LIMIT else 0


def xcd_grid(n):
    return 8 * ((n + 7) // 8)


def _lds(kernel, geom, frames, who):
    n_fft = geom[0]
    if kernel == SPECIALISED:
        return 0, lds_specialised(frames)
    if kernel == F64:
        tt = f64_pass_frames(n_fft)
        return tt, lds_f64(n_fft, tt)
    lds = lds_generic(n_fft, frames)
    if lds > LDS_LIMIT:
        raise Refused("%s: n_fft=%d too large for the LDS FFT" % (who, n_fft))
    if frames * (1 + n_fft // 2) >= 1 << 20:
        raise Refused("%s: tile too large" % who)
    return 0, lds


def plan_equal(geom, f64, aligned8, B, T, env=None):
    """The plan of B equal clips of T frames as a dict over FIELDS, or Refused."""
    _, pairs, maxf, threads, xcd = switches(env)
    kernel = route(geom, f64, aligned8, env)
    if kernel != SPECIALISED:
        pairs, maxf, threads = 0, ITEM_FRAMES[kernel], 256
    tiles = -(-T // maxf)
    frames = -(-T // tiles)                            # T split evenly
    if pairs and T % 2 == 0 and frames % 2 and frames < maxf:
        frames += 1                                    # even tiles for an even T: phase 3 in frame pairs on every tile
    tiles = -(-T // frames)
    pass_frames, lds = _lds(kernel, geom, frames, "smh_stft_mag_f32")
    xcd = xcd and B * tiles < 2 ** 31 - 8
    return dict(kernel=kernel, frames=frames, pass_frames=pass_frames, tiles=tiles, threads=threads, lds=lds,
                grid_x=xcd_grid(B * tiles) if xcd else tiles, grid_y=1 if xcd else B, xcd_tiles=tiles if xcd else 0, pairs=pairs)


def plan_rag(geom, f64, aligned8, n_items, env=None):
    """The plan of a ragged launch of n_items (clip, tile) items."""
    kernel = route(geom, f64, aligned8, env)
    frames = ITEM_FRAMES[kernel]
    pass_frames, lds = _lds(kernel, geom, frames, "ragged STFT")
    return dict(kernel=kernel, frames=frames, pass_frames=pass_frames, tiles=0, threads=256, lds=lds, grid_x=xcd_grid(n_items), grid_y=1,
                xcd_tiles=0, pairs=switches(env)[1] if kernel == SPECIALISED else 0)


def ints(p):
    return tuple(int(p[f]) for f in FIELDS)


def ask_library(lib, ctx, address, B, n_samples, ragged=False, aligned8=False, n_items=0):
    """The library's own plan under the switches set now, as the ints of `ints`, or None where the library refuses the launch.
    smh_internal_stft_plan is a test-only export, not in include/smh.h; it launches nothing.  Needs the GPU."""
    import ctypes as C
    got = (C.c_int * len(FIELDS))()
    rc = lib.smh_internal_stft_plan(ctx, C.c_void_p(address), B, n_samples, int(ragged), int(aligned8), n_items, got)
    return tuple(got) if rc == 0 else None
