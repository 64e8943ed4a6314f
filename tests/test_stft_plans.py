"""No GPU: the STFT's launch plan (tests/stft_plans.py) at the default context and at its boundaries, worked out by hand from the
kernels' LDS layouts."""
import pytest

from tests import stft_plans as P

G400 = (400, 400, 160)


def _eq(T, B=3, geom=G400, f64=False, aligned8=True, env=None):
    return P.plan_equal(geom, f64, aligned8, B, T, env)


def test_default_context_one_second_clips():
    """T = 98.  Specialised: 5 tiles of 20 frames, 8 (200 + 202 + 200 + 20 x 201) bytes.  Generic: 7 tiles of 14, stride
    200 + 12 + 2 = 214: 8 (200 + 201 + 2 x 14 x 214).  f64: 7 tiles of 14 in passes of 8: 16 (601 + 2 x 8 x 214), under the 64 KB that
    put two workgroups on a CU."""
    p = _eq(98, B=1024)
    assert P.ints(p) == (P.SPECIALISED, 20, 0, 5, 256, 36976, 5120, 1, 5, 1)
    assert 8 * (200 + 202 + 200 + 20 * 201) == 36976
    r = P.plan_rag(G400, False, True, 9)
    assert (r["lds"], r["frames"], r["threads"], r["grid_x"], r["grid_y"], r["tiles"], r["xcd_tiles"]) == (36976, 20, 256, 16, 1, 0, 0)
    p = _eq(98, aligned8=False)
    assert P.ints(p) == (P.GENERIC, 14, 0, 7, 256, 51144, 24, 1, 7, 0) and 8 * (200 + 201 + 2 * 14 * 214) == 51144
    p = _eq(98, f64=True)
    assert P.ints(p) == (P.F64, 14, 8, 7, 256, 64400, 24, 1, 7, 0) and 16 * (601 + 2 * 8 * 214) == 64400 <= P.F64_PAIR_LIMIT
    assert P.lds_f64(400, 9) > P.F64_PAIR_LIMIT and P.plan_rag(G400, True, True, 8)["frames"] == 16


def test_specialised_tiles_are_even_for_an_even_T():
    got = {T: (_eq(T)["tiles"], _eq(T)["frames"]) for T in (50, 22, 38, 41, 1, 20, 21)}
    assert got == {50: (3, 18), 22: (2, 12), 38: (2, 20), 41: (3, 14), 1: (1, 1), 20: (1, 20), 21: (2, 11)}
    off = {"SMH_STFT_PAIRS": "0"}
    assert (_eq(50, env=off)["tiles"], _eq(50, env=off)["frames"], _eq(50, env=off)["pairs"]) == (3, 17, 0)
    assert _eq(50, env={"SMH_STFT_PAIRS": "1"})["frames"] == 18
    # the other kernels never round: 50 -> 4 tiles of 13
    assert (_eq(50, aligned8=False)["tiles"], _eq(50, aligned8=False)["frames"]) == (4, 13) == (_eq(50, f64=True)["tiles"], _eq(50, f64=True)["frames"])


def test_frames_override_and_its_clamp():
    env = {"SMH_STFT_FRAMES": "32,256"}
    assert [(_eq(T, env=env)["tiles"], _eq(T, env=env)["frames"]) for T in (30, 31, 32, 63)] == [(1, 30), (1, 31), (1, 32), (2, 32)]
    assert _eq(32, env=env)["lds"] == 8 * (602 + 32 * 201) == 56272 and _eq(32, env=env)["threads"] == 256
    # maxf <= threads / 8: phase 2 has 8 items per frame and one per thread; threads is 512 or 256
    for text, want in (("40,256", (32, 256)), ("100,512", (64, 512)), ("64,512", (64, 512)), ("40,300", (32, 256)), ("0,256", (1, 256)),
                       ("-3", (1, 256)), ("16", (16, 256)), ("x", (20, 256))):
        assert P.switches({"SMH_STFT_FRAMES": text})[2:4] == want, text
    assert (_eq(100, env={"SMH_STFT_FRAMES": "100,512"})["tiles"], _eq(100, env={"SMH_STFT_FRAMES": "100,512"})["frames"]) == (2, 50)
    # the override is the specialised plan's alone
    assert _eq(63, aligned8=False, env=env)["frames"] == 16 and _eq(63, f64=True, env=env)["frames"] == 16
    assert P.plan_rag(G400, False, True, 8, env)["frames"] == 20


def test_plain_grid():
    for kw in (dict(), dict(aligned8=False), dict(f64=True)):
        tiles = _eq(98, B=1024, **kw)["tiles"]
        p = _eq(98, B=1024, env={"SMH_STFT_XCD": "0"}, **kw)
        assert (p["grid_x"], p["grid_y"], p["xcd_tiles"]) == (tiles, 1024, 0), kw
        p = _eq(98, B=1024, env={"SMH_STFT_XCD": "1"}, **kw)
        assert (p["grid_x"], p["grid_y"], p["xcd_tiles"]) == (8 * ((1024 * tiles + 7) // 8), 1, tiles), kw
    # the 1-D grid and its 32-bit decode hold fewer than 2^31 - 8 items
    B = (2 ** 31 - 8) // 5
    assert 5 * B == 2 ** 31 - 8
    p = _eq(98, B=B)
    assert (p["grid_x"], p["grid_y"], p["xcd_tiles"]) == (5, B, 0)
    p = _eq(98, B=B - 1)
    assert (p["grid_x"], p["grid_y"], p["xcd_tiles"]) == (2 ** 31 - 8, 1, 5)
    assert [P.xcd_grid(n) for n in (1, 7, 8, 9)] == [8, 8, 8, 16]


def test_route_table():
    """Route 1 needs n_fft = 400, an even hop and every frame on an 8-byte boundary; rag_needs_aligned8 is true exactly where it is
    reachable.  (win_length <= n_fft holds in every context, so no context of n_fft = 400 fails the kernel's win_length <= 400.)"""
    n = 400 + 40 * 160
    assert P.rag_needs_aligned8(G400) and P.route(G400, False, P.frames_aligned8(512, 3, n)) == P.SPECIALISED
    assert not P.rag_needs_aligned8((400, 400, 161)) and P.route((400, 400, 161), False, True) == P.GENERIC
    assert P.frames_aligned8(512, 1, n + 1) and not P.frames_aligned8(512, 3, n + 1)
    assert not P.frames_aligned8(516, 1, n) and not P.frames_aligned8(516, 3, n)
    assert P.route(G400, False, False) == P.GENERIC and P.plan_rag(G400, False, False, 8)["frames"] == 16
    forced = {"SMH_STFT_GENERIC": "1"}
    assert not P.rag_needs_aligned8(G400, env=forced) and P.route(G400, False, True, forced) == P.GENERIC
    assert not P.rag_needs_aligned8(G400, f64=True) and P.route(G400, True, True) == P.F64 == P.route(G400, True, False, forced)
    for geom in ((512, 400, 160), (8, 8, 3), (1024, 1000, 256)):
        assert not P.rag_needs_aligned8(geom) and P.route(geom, False, True) == P.GENERIC
    assert P.rag_needs_aligned8((400, 1, 2))


def test_generic_refusal_at_the_first_n_fft_beyond_the_limit():
    """16 frames: 8 (2 M + 1 + 32 (M + M / 16 + 2)) <= 153 600 up to M = 531."""
    assert P.lds_generic(1062, 16) == 153400 <= P.LDS_LIMIT == 153600 < P.lds_generic(1064, 16) == 153672
    assert _eq(16, geom=(1062, 1062, 256))["lds"] == 153400 and P.plan_rag((1062, 1062, 256), False, True, 3)["lds"] == 153400
    with pytest.raises(P.Refused, match="smh_stft_mag_f32: n_fft=1064 too large for the LDS FFT"):
        _eq(16, geom=(1064, 1064, 256))
    with pytest.raises(P.Refused, match="ragged STFT: n_fft=1064 too large for the LDS FFT"):
        P.plan_rag((1064, 1064, 256), False, True, 3)
    # by the clip's frame count: n_fft = 2048 runs up to 7 frames per tile (tests/test_stft_f32_shapes_gpu.py runs 3 and 40)
    assert _eq(7, geom=(2048, 1600, 400))["lds"] == P.lds_generic(2048, 7) <= P.LDS_LIMIT
    for T in (8, 40):
        with pytest.raises(P.Refused):
            _eq(T, geom=(2048, 1600, 400))


def test_f64_frames_per_pass():
    """16 (3 M + 1 + 2 tt (M + M / 16 + 2)) <= 65 536: 8 frames up to M = 203; a single frame may take up to 150 KB: M <= 1872."""
    assert [P.f64_pass_frames(n) for n in (400, 406, 408, 512, 1024, 2048)] == [8, 8, 7, 6, 2, 1]
    assert P.lds_f64(406, 8) == 16 * 4082 <= P.F64_PAIR_LIMIT < P.lds_f64(408, 8) == 16 * 4101
    assert P.lds_f64(2048, 1) > P.F64_PAIR_LIMIT                       # alone above 64 KB: one workgroup per CU
    assert P.f64_pass_frames(3744) == 1 and P.lds_f64(3744, 1) == 16 * 9599 <= P.LDS_LIMIT
    assert P.f64_pass_frames(3746) == 0 and P.lds_f64(3746, 1) == 16 * 9604 > P.LDS_LIMIT
    p = _eq(40, geom=(2048, 1600, 400), f64=True)                      # f64 is never refused at launch: the item is walked in passes
    assert (p["frames"], p["pass_frames"], p["lds"]) == (14, 1, P.lds_f64(2048, 1))
