"""GPU (contexts are created, nothing is launched): the library's own STFT launch plan (smh_internal_stft_plan: plan_equal / plan_rag
of smh_stft_plan.h under the switches the launches read) equals the restatement of tests/stft_plans.py on every integer -- six
geometries in both precisions, frame counts on both sides of every tile boundary, one clip and three, even and odd lengths, a first
clip on and 4 bytes off an 8-byte boundary, under no switch and each forced one, and the ragged form.  A launch the library refuses is
refused by the restatement, and the other way round.  The address is only ever looked at, so a made-up one serves."""
import ctypes as C

import pytest

from tests import stft_plans as P

pytestmark = pytest.mark.gpu

GEOMS = [(400, 400, 160), (400, 400, 161), (512, 400, 160), (8, 8, 3), (1024, 1000, 256), (2048, 1600, 400)]
FRAMES = (1, 2, 15, 16, 17, 19, 20, 21, 22, 38, 40, 41, 50, 98, 99)
FORCED = (None, ("SMH_STFT_GENERIC", "1"), ("SMH_STFT_PAIRS", "0"), ("SMH_STFT_FRAMES", "32,256"), ("SMH_STFT_XCD", "0"))
ON8, OFF8 = 1 << 20, (1 << 20) + 4
_FES = {}


def _fe(geom, f64):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    if (geom, f64) not in _FES:
        n_fft, wl, hop = geom
        _FES[geom, f64] = Frontend(FrontendConfig(n_fft=n_fft, win_length=wl, hop=hop, n_mels=0, stft_precision="f64" if f64 else "f32"))
    return _FES[geom, f64]


def _route(fe, address, B, n):
    f = fe.lib.smh_internal_stft_route  # test-only export, not in include/smh.h
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return f(fe._h, C.c_void_p(address), B, n)


def _want(fn, *args):
    try:
        return P.ints(fn(*args))
    except P.Refused:
        return None


def _clean(monkeypatch):
    for var in P.SWITCHES:
        monkeypatch.delenv(var, raising=False)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "-".join(map(str, g)))
def test_library_plan_equals_the_restatement(geom, f64, monkeypatch):
    _clean(monkeypatch)
    fe = _fe(geom, f64)
    n_fft, _, hop = geom
    refused = kernels = 0
    for switch in FORCED:
        if switch:
            monkeypatch.setenv(*switch)
        env = dict([switch]) if switch else {}
        for T in FRAMES:
            for r in (0, 1):
                n = n_fft + (T - 1) * hop + r
                for B in (1, 3):
                    for address in (ON8, OFF8):
                        got = P.ask_library(fe.lib, fe._h, address, B, n)
                        want = _want(P.plan_equal, geom, f64, P.frames_aligned8(address, B, n), B, T, env)
                        assert got == want, (geom, f64, switch, T, n, B, address % 8,
                                             [(f, g, w) for f, g, w in zip(P.FIELDS, got or (), want or ()) if g != w])
                        refused += got is None
                        if got:  # smh_internal_stft_route answers from the same plan
                            kernels |= 1 << got[0]
                            assert _route(fe, address, B, n) == got[0]
        for aligned8 in (False, True):
            for n_items in (1, 7, 8, 9):
                got = P.ask_library(fe.lib, fe._h, 0, 0, 0, ragged=True, aligned8=aligned8, n_items=n_items)
                want = _want(P.plan_rag, geom, f64, aligned8, n_items, env)
                assert got == want, (geom, f64, switch, "ragged", aligned8, n_items)
                refused += got is None
        if switch:
            monkeypatch.delenv(switch[0])
    # what each context reaches: both f32 kernels at (400, 400, 160) alone; refusals at n_fft = 2048 in f32 alone (every ragged launch,
    # and the equal-length ones beyond 7 frames per tile)
    assert kernels == (1 << P.F64 if f64 else 3 if geom == (400, 400, 160) else 1 << P.GENERIC)
    assert (refused > 0) == (geom[0] == 2048 and not f64)


def test_the_query_follows_the_switches_between_calls(monkeypatch):
    """The switches are read per query, as they are per launch: one context, a switch flipped between two calls."""
    _clean(monkeypatch)
    fe = _fe((400, 400, 160), False)
    n = 400 + 49 * 160
    ask = lambda: dict(zip(P.FIELDS, P.ask_library(fe.lib, fe._h, ON8, 3, n)))
    assert (ask()["kernel"], ask()["frames"], ask()["xcd_tiles"]) == (P.SPECIALISED, 18, 3)
    monkeypatch.setenv("SMH_STFT_PAIRS", "0")
    assert (ask()["frames"], ask()["pairs"]) == (17, 0)
    monkeypatch.setenv("SMH_STFT_XCD", "0")
    assert (ask()["grid_x"], ask()["grid_y"], ask()["xcd_tiles"]) == (3, 3, 0)
    monkeypatch.setenv("SMH_STFT_GENERIC", "1")
    assert (ask()["kernel"], ask()["frames"], ask()["tiles"]) == (P.GENERIC, 13, 4)
    _clean(monkeypatch)
    assert (ask()["kernel"], ask()["frames"], ask()["pairs"], ask()["grid_x"]) == (P.SPECIALISED, 18, 1, 16)
