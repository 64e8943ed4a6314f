"""GPU: the median filters' launch plan (csrc/smh_median_plan.h) where it meets the device.

(a) The CU count is an argument of the plan; smh_internal_median_plan asks the device only when it is given 0.  For this device's own
count both forms give the same plan on the shapes around the persistent kernel's threshold B = 2 n_cu, and that plan is the
restatement's (tests/median_plans.py).

(b) The block-split kernel's two stagings at the boundaries tests/test_median_plans.py pins by hand, through real launches: the query,
given the alignment class of the pointer the launch is given, reports the staging; every value equals oracle.frontend.median_time /
median_freq (np.array_equal), and the 64 sentinel floats around the input and every output are untouched.
  smh_median_time_ex_f32, K = 2, T = 34, l_harm = 11, B = 3: a clip is 272 bytes, the tile 2 x 35 x 4 = 280.  Input on a 16-byte
  boundary: LDS-DMA (272 <= 280).  8 bytes past one: the copy would run from the boundary below to the one above, 288 > 280: registers.
  smh_hpss_median_ex_f32, K = 24, (17, 17), SMH_MEDIAN_PERSIST=0, input on a 16-byte boundary: T = 34 (3264 bytes <= 24 x 35 x 4) DMA;
  T = 33 (3168 = 198 x 16 bytes, exactly the tile of stride 33) DMA; T = 36 (gcd(36, 64) = 4) registers.

(c) SMH_MEDIAN_NOSPLIT is read on every call: flipped in-process between launches of one (17, 17) call it moves the call from the
block-split to the delete/insert kernel and back, with the same bits.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import median_cases as M
from tests import median_plans as P

pytestmark = pytest.mark.gpu

GUARD = 64       # floats: 256 bytes, so the input behind it keeps the allocation's alignment
SENTINEL = -7.0  # no median of a magnitude spectrogram


@pytest.fixture(scope="module")
def lib():
    from sm_hpss_mtl_amd import _lib
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in P.SWITCHES + ("SMH_MEDIAN_PROBE_NOLOAD",):
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _oracle(K, T, w, along_t):
    f = ofe.median_time if along_t else ofe.median_freq
    out = np.stack([f(s, w) for s in M.clips(K, T)])
    out.setflags(write=False)
    return out


def _align_class(ptr, clip_bytes):
    """The class the launcher derives: the largest of 16 / 8 / 4 that divides the pointer and K T 4; 0 off a 4-byte boundary."""
    return next((a for a in (16, 8, 4) if ptr % a == 0 and clip_bytes % a == 0), 0)


def _launch(lib, entry, K, T, lh, lp, B, lay, offset_floats=0):
    """One call on clips(K, T) placed `offset_floats` behind a 16-byte boundary -> (alignment class of the input pointer, layout
    returned, harm (B, K, T), perc (B, K, T) or None); asserts every guard."""
    n = B * K * T
    src = torch.full((GUARD + offset_floats + n + GUARD,), SENTINEL, device="cuda")
    lo = GUARD + offset_floats
    src[lo:lo + n] = torch.from_numpy(M.clips(K, T)[M.clip_index(B)]).cuda().reshape(-1)
    ptr = src.data_ptr() + 4 * lo
    assert (ptr - 4 * offset_floats) % 16 == 0
    harm = torch.full((GUARD + P.owned_floats(2, B, K, T) + GUARD,), SENTINEL, device="cuda")
    perc = torch.full((GUARD + n + GUARD,), SENTINEL, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, p = C.c_void_p(harm.data_ptr() + 4 * GUARD), C.c_void_p(perc.data_ptr() + 4 * GUARD)
    if entry == "time_ex":
        got = lib.smh_median_time_ex_f32(None, C.c_void_p(ptr), B, K, T, lh, h, lay, st)
    else:
        got = lib.smh_hpss_median_ex_f32(None, C.c_void_p(ptr), B, K, T, lh, lp, h, p, lay, st)
    torch.cuda.synchronize()
    assert got in (0, 1, 2), got
    owned = P.owned_floats(got, B, K, T)
    assert bool((harm[:GUARD] == SENTINEL).all()) and bool((harm[GUARD + owned:] == SENTINEL).all()), "harm: a guard was touched"
    wrote_perc = n if entry == "hpss_ex" else 0
    assert bool((perc[:GUARD] == SENTINEL).all()) and bool((perc[GUARD + wrote_perc:] == SENTINEL).all()), "perc: a guard was touched"
    assert bool((src[:lo] == SENTINEL).all()) and bool((src[lo + n:] == SENTINEL).all()), "the input's guards were written"
    hd = P.decode_harm(harm[GUARD:GUARD + owned].cpu().numpy(), got, B, K, T)
    pd = perc[GUARD:GUARD + n].cpu().numpy().reshape(B, K, T) if wrote_perc else None
    return _align_class(ptr, K * T * 4), got, hd, pd


def test_the_devices_cu_count_as_an_argument_and_asked_for_give_the_same_plan(lib, n_cu):
    seen = set()
    for K, T, lh, lp in ((25, 33, 21, 11), (24, 34, 21, 21), (24, 36, 21, 11), (201, 98, 21, 11), (201, 98, 17, 17)):
        for B in (2 * n_cu - 1, 2 * n_cu, 2 * n_cu + 3):
            for lay in (0, 2):
                a = ("hpss_ex", K, T, lh, lp, B, lay)
                asked, given = M.library_route(lib, *a, n_cu=0), M.library_route(lib, *a, n_cu=n_cu)
                assert asked == given == P.route(*a, n_cu), a
                seen.add((given["family"], B - 2 * n_cu))
    assert {("persist", 0), ("persist", 3), ("split", -1), ("split", 0)} <= seen and ("persist", -1) not in seen


@pytest.mark.parametrize("lay", [1, 2])
@pytest.mark.parametrize("offset_floats,dma", [(0, 1), (2, 0)])
def test_single_filter_at_the_dma_boundary_by_alignment(lib, n_cu, lay, offset_floats, dma):
    K, T, lh, B = 2, 34, 11, 3
    align, got, h, _ = _launch(lib, "time_ex", K, T, lh, 0, B, lay, offset_floats)
    assert align == (16 if offset_floats == 0 else 8)
    plan = M.library_route(lib, "time_ex", K, T, lh, 0, B, lay, n_cu=n_cu, align=align)
    assert plan == P.route("time_ex", K, T, lh, 0, B, lay, n_cu, align=align)
    assert (plan["family"], plan["layout"], plan["ntiles"], plan["lds"], plan["dma"]) == ("split", lay, 1, 280, dma) and got == lay
    ref = _oracle(K, T, lh, True)[M.clip_index(B)]
    assert np.array_equal(h, ref), "harm differs at (clip, bin, frame) %s" % np.argwhere(h != ref)[:4].tolist()


@pytest.mark.parametrize("lay", [1, 2])
@pytest.mark.parametrize("T,dma", [(34, 1), (33, 1), (36, 0)])
def test_pair_at_the_dma_boundary_by_clip_length(lib, n_cu, lay, T, dma, monkeypatch):
    monkeypatch.setenv("SMH_MEDIAN_PERSIST", "0")
    K, lh, lp, B = 24, 17, 17, 3
    align, got, h, p = _launch(lib, "hpss_ex", K, T, lh, lp, B, lay)
    assert align == 16
    plan = M.library_route(lib, "hpss_ex", K, T, lh, lp, B, lay, n_cu=n_cu, align=align)
    assert plan == P.route("hpss_ex", K, T, lh, lp, B, lay, n_cu, persist="0", align=align)
    assert (plan["family"], plan["layout"], plan["ntiles"], plan["dma"]) == ("split", lay, 1, dma) and got == lay
    idx = M.clip_index(B)
    ref_h, ref_p = _oracle(K, T, lh, True)[idx], _oracle(K, T, lp, False)[idx]
    assert np.array_equal(h, ref_h), "harm differs at (clip, bin, frame) %s" % np.argwhere(h != ref_h)[:4].tolist()
    assert np.array_equal(p, ref_p), "perc differs at (clip, bin, frame) %s" % np.argwhere(p != ref_p)[:4].tolist()


def test_nosplit_flipped_between_launches_moves_the_family_and_keeps_the_bits(lib, n_cu, monkeypatch):
    K, T, lh, lp, B, lay = 24, 34, 17, 17, 3, 2
    runs = []
    for nosplit, family, wrote in ((False, "split", 2), (True, "delete_insert", 1), (False, "split", 2)):
        if nosplit:
            monkeypatch.setenv("SMH_MEDIAN_NOSPLIT", "1")
        else:
            monkeypatch.delenv("SMH_MEDIAN_NOSPLIT", raising=False)
        plan = M.library_route(lib, "hpss_ex", K, T, lh, lp, B, lay, n_cu=n_cu)
        assert (plan["family"], plan["layout"]) == (family, wrote)
        _, got, h, p = _launch(lib, "hpss_ex", K, T, lh, lp, B, lay)
        assert got == wrote
        runs.append((h, p))
    idx = M.clip_index(B)
    for h, p in runs:
        assert np.array_equal(h, _oracle(K, T, lh, True)[idx]) and np.array_equal(p, _oracle(K, T, lp, False)[idx])
