"""No GPU: the restatement of the median filters' routing (tests/median_plans.py) against boundaries worked out by hand from the
C++, every case of tests/test_median_layouts_gpu.py (the table of tests/median_cases.py) on the kernel family and the harm layout
it is named for, the table against every (family, requested layout, entry point) that exists, and the decoders of harm layouts
1 and 2 against an encoder of the documented layouts."""
import os

import numpy as np
import pytest

from tests import median_cases as M
from tests import median_plans as P
from tests.median_cases import CASES, CROSS_ENTRY, N_CU_MI355X, REFUSED, batch, case_id

N_CU = N_CU_MI355X


def _route(c, n_cu=N_CU):
    return P.route(c["entry"], c["K"], c["T"], c["lh"], c["lp"], batch(c["B"], n_cu), c["lay"], n_cu, c["persist"])


# ---- hand-computed pins ---------------------------------------------------------------------------------------------------------
def test_hand_computed_tiles():
    """make_plan: two workgroups per CU leave (160 KiB / 2 - 1 KiB) / 4 = 20 224 words for a tile of K rows at an odd stride.
    K = 201: 201 x 99 = 19 899 fits (T = 98, one tile); 201 x 101 = 20 301 does not, 20 224 // 201 = 100 -> 99 columns, less the
    halo of 2 x 10 frames -> TT = 79, T = 101 is two tiles and T = 180 three (0, 79, 158).  l_harm = 17: TT = 99 - 16 = 83.
    K = 257: 20 224 // 257 = 78 -> 77 columns: one tile up to T = 77, then TT = 57 (l_harm = 21) or 61 (17)."""
    assert P.make_plan(201, 98, 21, 11)["ntiles"] == 1 and P.make_plan(201, 98, 21, 11)["stride"] == 99
    p = P.make_plan(201, 101, 21, 11)
    assert (p["TT"], p["ntiles"], p["stride"], p["tall"]) == (79, 2, 99, False)
    assert P.make_plan(201, 100, 21, 11)["ntiles"] == 2 and P.make_plan(201, 99, 21, 11)["ntiles"] == 1
    assert P.make_plan(201, 180, 21, 11)["ntiles"] == 3 and P.segment_starts(180, 79, 1) == [0, 79, 158]
    p = P.make_plan(201, 333, 17, 17)
    assert (p["TT"], p["ntiles"]) == (83, 5) and 333 - 4 * 83 == 1
    assert P.make_plan(257, 77, 21, 11)["ntiles"] == 1
    assert [P.make_plan(257, 78, lh, 11)["TT"] for lh in (21, 17)] == [57, 61]
    p = P.make_plan(257, 130, 21, 11)
    assert (p["TT"], p["ntiles"], p["stride"]) == (57, 3, 77)


def _first(pred, lo, hi):
    return next(K for K in range(lo, hi) if pred(K))


def _refusal(*a):
    try:
        P.route(*a)
    except P.Refused as e:
        return str(e)
    return None


def test_hand_computed_tall_branch_and_refusals():
    """l_harm = 21.  The tile shrinks below 8 frames when the odd column count drops to 27, i.e. 20 224 // K <= 28: K >= 698
    (20 224 / 29 = 697.4).  There the whole 160 KiB less 1 KiB = 40 704 words go to one workgroup: 40 704 // 698 = 58 -> 57 columns,
    TT = 37.  That branch refuses once 40 704 // K <= 20, K >= 1939 (40 704 / 21 = 1938.3) -- but the 16 waves of a workgroup run out
    first: one harmonic lane per bin is ceil(K / 64) waves, so a pair (one percussive wave more) is refused from K = 961 and a single
    harmonic filter from K = 1025, both with the wave message."""
    tall = lambda K: P.make_plan(K, 200, 21, 11)["tall"]  # noqa: E731
    assert _first(tall, 1, 960) == 698 and P.make_plan(697, 200, 21, 11)["TT"] == 9 and P.make_plan(698, 200, 21, 11)["TT"] == 37
    assert P.make_plan(698, 77, 21, 11)["ntiles"] == 3
    pair = lambda K: _refusal("hpss_ex", K, 200, 21, 11, 1, 2, N_CU)  # noqa: E731
    single = lambda K: _refusal("time_ex", K, 200, 21, 0, 1, 2, N_CU)  # noqa: E731
    assert _first(pair, 1, 3000) == 961 and pair(961) == "tile 961x21 needs more than 16 waves per workgroup"
    assert _first(single, 1, 3000) == 1025 and single(1025) == "tile 1025x19 needs more than 16 waves per workgroup"
    lds = lambda K: (pair(K) or "").startswith("K=")  # noqa: E731
    assert _first(lds, 1, 3000) == 1939 and pair(1939) == "K=1939 too large for an LDS tile with l_harm=21"
    assert all(pair(K) for K in range(961, 2100)) and all(single(K) for K in range(1025, 2100))
    # the last accepted shapes run the delete/insert kernel with all 16 waves, and write layout 1 for a requested 2
    for r in (P.route("hpss_ex", 960, 45, 21, 11, 1, 2, N_CU), P.route("time_ex", 1024, 41, 21, 0, 1, 2, N_CU)):
        assert (r["family"], r["layout"], r["ntiles"]) == ("delete_insert", 1, 3)


def test_hand_computed_roles():
    """make_split_roles.  K = 201, T = 98: the harmonic lanes are 4 waves (7 in two segments).  (17, 17), 8 waves: two harmonic
    segments never fit, and 4 + ceil(98 nsp / 64) <= 8 allows nsp <= 2; the cost max((98 + 17) 23, (ceil(201 / nsp) + 17) 23) falls
    from 5014 to 2714 -> (1, 2).  (21, 11), 6 waves: only (1, 1).  K = 24, T = 98, (11, 11): the percussive cost (24 + 11) 17 = 595
    is fixed (K < 44), the harmonic cost (ceil(98 / nsh) + 11) 17 stays above it up to nsh = 4 (36 x 17) -> (4, 1), segments of 25."""
    assert P.make_split_roles(201, 98, 17, 17, 8) == (1, 2, 4, 4)
    assert P.make_split_roles(201, 98, 21, 11, 6) == (1, 1, 4, 2)
    assert P.make_split_roles(24, 98, 11, 11, 8) == (4, 1, 2, 2) and P.segment_starts(98, 98, 4) == [0, 25, 50, 75]
    assert P.make_split_roles(1024, 19, 21, 0, 6) is None and P.make_split_roles(698, 37, 21, 11, 6) is None
    assert P.split_threads(17, 17) == 512 and P.split_threads(21, 11) == 384 and P.split_threads(11, 21) == 384


def test_hand_computed_persistent_kernel_thresholds():
    """Two clips per CU (B >= 2 n_cu), one tile, gcd(T, 64) <= 2 (T odd, or T = 2 mod 4: 34 yes, 36 no), two tiles of
    persist_tile_bytes in 160 KiB; windows above 17 ask for it, SMH_MEDIAN_PERSIST forces either way."""
    assert P.conflict_free(33) and P.conflict_free(34) and not P.conflict_free(36) and P.conflict_free(98) and not P.conflict_free(64)
    assert P.persist_tile_bytes(201, 98) == 78848 and P.persist_tile_bytes(24, 33) == 4096  # 78 792 + 16 and 3 168 + 16, up to 1 KiB
    fam = lambda B, T=33, w=(21, 11), persist=None, n_cu=N_CU: P.route("hpss_ex", 25, T, w[0], w[1], B, 2, n_cu, persist)["family"]  # noqa: E731
    assert fam(2 * N_CU) == "persist" and fam(2 * N_CU - 1) == "split" and fam(2 * N_CU + 3) == "persist"
    assert fam(208, n_cu=104) == "persist" and fam(207, n_cu=104) == "split"
    assert fam(512, T=34) == "persist" and fam(512, T=36) == "split"
    assert fam(512, w=(17, 17)) == "split" and fam(512, w=(17, 17), persist="1") == "persist" and fam(512, persist="0") == "split"
    assert fam(512, w=(31, 31)) == "delete_insert"  # no persistent build of that pair
    assert P.route("hpss_ex", 201, 98, 21, 11, 512, 2, N_CU)["family"] == "persist"   # the headline shape at 17 x 17 is split:
    assert P.route("hpss_ex", 201, 98, 17, 17, 1024, 2, N_CU)["family"] == "split"
    assert P.route("hpss_ex", 201, 100, 21, 11, 512, 2, N_CU)["family"] == "split"    # two tiles
    assert P.route("time_ex", 25, 33, 21, 0, 512, 2, N_CU)["family"] == "split"       # a single filter never


def test_hand_computed_tables_and_fallbacks():
    assert len(P.PAIRS) == 26 and len(P.SINGLES) == 62 and len(P.SPLIT) == 25 and len(P.PERSIST) == 11
    assert (31, 31) in P.PAIRS and (31, 31) not in P.SPLIT and (5, 31) not in P.PAIRS and (13, 7) not in P.PAIRS
    assert (23, 0) in P.SINGLES and (23, 0) not in P.SPLIT and (21, 0) in P.SPLIT and (63, 0) in P.SINGLES
    assert P.fast_ok(15, 21) and not P.fast_ok(14, 21) and not P.fast_ok(33, 1) and P.fast_ok(10, 11) and not P.fast_ok(9, 11)
    r = lambda *a: (lambda d: (d["family"], d["layout"]))(P.route(*a, N_CU))  # noqa: E731
    assert r("hpss_ex", 40, 33, 31, 31, 3, 2) == ("delete_insert", 1) and r("hpss_ex", 40, 33, 31, 31, 3, 1) == ("delete_insert", 1)
    assert r("time_ex", 24, 33, 21, 0, 3, 2) == ("split", 2) and r("time_ex", 24, 33, 23, 0, 3, 2) == ("delete_insert", 1)
    assert r("hpss_ex", 40, 33, 13, 7, 3, 2) == ("two_singles", 0) and r("hpss_ex", 24, 14, 21, 11, 3, 2) == ("two_singles", 0)
    assert r("time_ex", 24, 14, 21, 0, 3, 2) == ("small", 0) and r("time_ex", 24, 33, 1, 0, 3, 2) == ("copy", 0)
    assert r("time_ex", 24, 33, 21, 0, 3, 0) == ("split", 0) and r("hpss_ex", 24, 33, 21, 11, 0, 2) == (None, 2)
    assert _refusal("hpss_ex", 24, 33, 4, 11, 1, 0, N_CU) == "smh_hpss_median_ex_f32: window must be odd in [1,63], got 4"
    assert _refusal("time_ex", 24, 33, 21, 0, 1, 3, N_CU) == "smh_median_time_ex_f32: harm_layout must be 0, 1 or 2"
    assert _refusal("hpss_ex", 10, 2000, 21, 3, 1, 0, N_CU) == "tile 10x2000 needs more than 16 waves per workgroup"


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_gpu_cases_reach_the_route_they_are_named_for(c):
    r = _route(c)
    assert (r["family"], r["layout"]) == (c["family"], c["wrote"])
    if isinstance(c["B"], str):  # named in compute units: the same route on a device with another count
        r2 = _route(c, n_cu=304)
        assert (r2["family"], r2["layout"]) == (c["family"], c["wrote"])
    # a few seconds per case: no buffer above 1 M floats
    assert batch(c["B"], 304) * P.harm_buffer_floats(c["K"], c["T"]) <= 1 << 20


@pytest.mark.parametrize("entry,K,T,lh,lp,lay,msg", REFUSED)
def test_refused_cases_are_refused_with_their_message(entry, K, T, lh, lp, lay, msg):
    assert _refusal(entry, K, T, lh, lp, 1, lay, N_CU) == msg
    if msg.startswith("tile") and K < 1938:  # ... and it is the first such K: one bin fewer runs
        assert _refusal(entry, K - 1, T, lh, lp, 1, lay, N_CU) is None


def test_cross_entry_cases_write_the_same_layout():
    for K, T, lh, lp, B, lay, wrote in CROSS_ENTRY:
        assert P.route("hpss_ex", K, T, lh, lp, B, lay, N_CU)["layout"] == wrote
        assert P.route("time_ex", K, T, lh, 0, B, lay, N_CU)["layout"] == wrote
    assert len(CROSS_ENTRY) == 3 and {w for *_, w in CROSS_ENTRY} == {1, 2}


def _existing_cells():
    """Every (entry, family) a sweep over shapes, windows, batches and the switch reaches, times the layouts the entry can be asked
    for."""
    seen = set()
    for entry in P.ENTRIES:
        for K in (9, 24, 201, 698):
            for T in (5, 14, 33, 36, 180):
                for lh in (1, 3, 13, 21, 31, 63):
                    for lp in (1, 7, 11, 31):
                        for B in (3, 2 * N_CU):
                            for persist in (None, "1"):
                                try:
                                    seen.add((entry, P.route(entry, K, T, lh, lp, B, 2, N_CU, persist)["family"]))
                                except P.Refused:
                                    pass
    return {(e, f, lay) for e, f in seen for lay in ((0, 1, 2) if e.endswith("_ex") else (0,))}


def test_the_table_covers_every_family_layout_and_entry_point_that_exists():
    """hpss_ex: split, persist, delete_insert, two_singles; time_ex: copy, small, split, delete_insert (a single filter has no
    persistent build and nothing to split into); each at requested layouts 0, 1 and 2.  The entries without a layout argument:
    the same families at layout 0."""
    by_hand = {("hpss_ex", f, lay) for f in ("split", "persist", "delete_insert", "two_singles") for lay in (0, 1, 2)}
    by_hand |= {("time_ex", f, lay) for f in ("copy", "small", "split", "delete_insert") for lay in (0, 1, 2)}
    by_hand |= {("hpss", f, 0) for f in ("split", "persist", "delete_insert", "two_singles")}
    by_hand |= {("time", f, 0) for f in ("copy", "small", "split", "delete_insert")}
    assert _existing_cells() == by_hand
    have = {(c["entry"], c["family"], c["lay"]) for c in CASES if c["family"]}
    assert have == by_hand, by_hand ^ have
    # B == 0 on both layout-taking entries at both non-reference layouts
    assert {(c["entry"], c["lay"]) for c in CASES if c["B"] == 0} == {(e, lay) for e in ("hpss_ex", "time_ex") for lay in (1, 2)}


def test_the_table_covers_the_store_edges():
    """What the shapes were chosen for: layout 2 with every T mod 16 class of the issue's list, 1 .. 4 harmonic segments, a segment
    length that is no multiple of 4 and one that is a multiple of 16, tile starts that are multiples of neither 4 nor 16, a
    one-frame last tile, the demotion on pairs and singles, both persistent thresholds, and a multi-tile clip at B = 1 and 3."""
    l2 = [(c, _route(c)) for c in CASES if c["family"] in ("split", "persist") and c["lay"] == 2]
    for fam in ("split", "persist"):
        seg = {r["nsh"] for c, r in l2 if c["family"] == fam}
        assert seg >= ({1, 2, 3, 4} if fam == "split" else {1, 2}), (fam, seg)
    assert {c["T"] for c, r in l2 if c["family"] == "split" and c["K"] == 24} >= {16, 17, 31, 33, 47, 98}
    assert {c["entry"] for c, r in l2} == {"hpss_ex", "time_ex"}
    seglens = {P.segment_starts(c["T"], r["TT"], r["nsh"])[1] for c, r in l2 if r["ntiles"] == 1 and r["nsh"] > 1}
    assert any(n % 4 for n in seglens) and any(n % 16 == 0 for n in seglens), seglens
    tiles = {(c["K"], c["T"], r["TT"], r["ntiles"]) for c, r in l2 if r["ntiles"] > 1}
    assert {(201, 101, 79, 2), (201, 180, 79, 3), (201, 333, 83, 5), (257, 130, 57, 3)} <= tiles
    assert all(TT % 4 for _, _, TT, _ in tiles)
    for K, T in ((201, 101), (201, 180), (201, 333), (257, 130)):
        assert {(c["B"], c["lay"]) for c in CASES if (c["K"], c["T"], c["entry"]) == (K, T, "hpss_ex") and c["family"] == "split"} \
            >= {(1, 1), (1, 2), (3, 1), (3, 2)}
    demoted = {(c["entry"], c["lh"], c["lp"]) for c in CASES if c["lay"] == 2 and c["wrote"] == 1}
    assert demoted >= {("hpss_ex", 31, 31), ("hpss_ex", 11, 51), ("time_ex", 23, 0), ("time_ex", 63, 0)}
    assert {(c["entry"], c["lh"], c["lp"]) for c in CASES if c["lay"] == 1 and c["family"] == "delete_insert"} >= demoted
    pers = {(c["lh"], c["lp"], c["persist"], c["B"], c["T"], c["lay"]) for c in CASES if c["family"] == "persist"}
    for lh, lp, sw in ((21, 11, None), (21, 21, None), (17, 17, "1"), (11, 11, "1")):
        for lay in (0, 1, 2):
            assert (lh, lp, sw, "2cu", 34, lay) in pers and (lh, lp, sw, "2cu+3", 33, lay) in pers
    assert {(c["B"], c["T"]) for c in CASES if c["why"] == "persist" and c["family"] == "split"} >= {("2cu-1", 33), ("2cu", 36)}
    tall = [(c, _route(c)) for c in CASES if c["why"] == "tall"]
    assert all(P.make_plan(c["K"], c["T"], c["lh"], c["lp"])["tall"] and r["ntiles"] == 3 for c, r in tall)
    assert {c["K"] for c, r in tall} == {698, 960, 1024}


# ---- the plan's launch fields, pinned by hand ---------------------------------------------------------------------------------------
def test_hand_computed_ragged_tile():
    """rag_tile_frames: K = 201 leaves 20 224 // 201 = 100 -> 99 columns; less the halo of 2 x 10 frames (l_harm = 21) 79, down to a
    multiple of 4: 76 frames, 96 columns, stride 97, 201 x 97 x 4 bytes of LDS.  (21, 11) is a 384-thread build: 6 waves, 4 of them
    the 201 harmonic lanes, so one segment each.  The grid is the item count rounded up to a multiple of 8 (one range per XCD)."""
    r = P.route("rag", 201, 0, 21, 11, 1001, 2, N_CU)
    assert (r["family"], r["layout"], r["ntiles"], r["TT"], r["stride"], r["lds"]) == ("split", 2, 0, 76, 97, 201 * 97 * 4)
    assert (r["nsh"], r["nsp"], r["nwh"], r["nwp"], r["threads"], r["grid_x"], r["grid_y"], r["dma"]) == (1, 1, 4, 2, 384, 1008, 1, 0)
    assert P.rag_tile(201, 17, 17) == (80, 97) and P.rag_tile(201, 31, 31) is None and P.rag_tile(201, 21, 0) is None
    # the tile must hold 2 hh + 8 = 28 frames: 48 columns, so 49 odd ones, 20 224 // K >= 49 -> K <= 412 (20 224 / 49 = 412.7;
    # K = 413 -> 48 -> 47 columns -> 27 -> 24 frames)
    assert P.rag_tile(412, 21, 11) == (28, 49) and P.rag_tile(413, 21, 11) is None
    assert _refusal("rag", 413, 0, 21, 11, 5, 2, N_CU) == "ragged medians: no block-split kernel for (l_harm,l_perc)=(21,11), K=413"
    assert P.route("rag", 201, 0, 21, 11, 0, 2, N_CU)["family"] is None


def test_hand_computed_dma_staging_boundary():
    """dma_staged.  time_ex, K = 2, T = 34, l_harm = 11: one tile, odd stride 35, 2 x 35 x 4 = 280 bytes of LDS; the clip is
    2 x 34 x 4 = 272 bytes, a multiple of 16.  On a 16-byte boundary the copy is the clip, 272 <= 280: DMA, the kernel is given the
    flat image's stride 34.  Known only to 8 bytes it may start 8 bytes behind a boundary: 272 + 8 = 280, rounded out to 288 > 280:
    registers, stride 35.  T = 33 (odd: the tile has no spare column, 2 x 33 x 4 = 264 -> 272 > 264) and T = 36 (gcd(36, 64) = 4)
    never; K = 201, T = 98 (78 792 bytes, + 12 -> 78 816 <= 201 x 99 x 4 = 79 596) at all three alignments; a pointer off a 4-byte
    boundary, a clip of several tiles and SMH_MEDIAN_DMA_STAGE=0 never."""
    r = lambda T, align, K=2, env=None: P.route("time_ex", K, T, 11, 0, 3, 1, N_CU, env=env, align=align)  # noqa: E731
    a = r(34, 16)
    assert (a["family"], a["ntiles"], a["lds"], a["dma"], a["stride"], a["threads"], a["grid_x"], a["grid_y"]) == ("split", 1, 280, 1, 34, 512, 1, 3)
    b = r(34, 8)
    assert (b["dma"], b["stride"], b["lds"]) == (0, 35, 280) and r(34, 4)["dma"] == 0 and r(34, 0)["dma"] == 0
    assert P.dma_stage_bytes(272, 16) == 272 and P.dma_stage_bytes(272, 8) == 288 and P.dma_stage_bytes(78792, 4) == 78816
    assert [r(33, al)["dma"] for al in (16, 8, 4)] == [0, 0, 0] and [r(36, al)["dma"] for al in (16, 8, 4)] == [0, 0, 0]
    assert [r(98, al, K=201)["dma"] for al in (16, 8, 4, 0)] == [1, 1, 1, 0]
    assert r(34, 16, env={"SMH_MEDIAN_DMA_STAGE": "0"})["dma"] == 0 and r(34, 16, env={"SMH_MEDIAN_DMA_STAGE": "1"})["dma"] == 1
    two = P.route("hpss_ex", 201, 102, 21, 11, 3, 2, N_CU, align=16)  # gcd(102, 64) = 2, but two tiles
    assert (two["family"], two["ntiles"], two["dma"], two["stride"]) == ("split", 2, 0, 99)
    # the other families never stage by DMA; the persistent kernel's rows are T, its LDS two tiles, its grid the CUs
    pers = P.route("hpss_ex", 201, 98, 21, 11, 512, 2, N_CU)
    assert (pers["family"], pers["dma"], pers["stride"], pers["lds"], pers["grid_x"], pers["grid_y"], pers["threads"]) \
        == ("persist", 0, 98, 2 * 78848, N_CU, 1, 512) and (pers["nwh"], pers["nwp"]) == (4, 4)
    di = P.route("hpss_ex", 40, 34, 31, 31, 3, 2, N_CU)
    assert (di["family"], di["dma"], di["stride"], di["threads"], di["grid_x"], di["grid_y"]) == ("delete_insert", 0, 35, 1024, 1, 3)


# ---- the library's own plan: no device is asked when the CU count is given ----------------------------------------------------------
def _env():
    """The switches the library reads in this process, for the restatement."""
    return {n: os.environ[n] for n in P.SWITCHES if n in os.environ}


def _same(lib, entry, K, T, lh, lp, B, lay, n_cu, align):
    """The library's plan (or refusal) of one call equals the restatement's, field by field."""
    a = (entry, K, T, lh, lp, B, lay)
    try:
        want = P.route(*a, n_cu, env=_env(), align=align)
    except P.Refused as e:
        with pytest.raises(P.Refused) as got:
            M.library_route(lib, *a, n_cu=n_cu, align=align)
        assert str(got.value) == str(e), a
    else:
        assert M.library_route(lib, *a, n_cu=n_cu, align=align) == want, (a, n_cu, align)


@pytest.fixture(scope="module")
def lib():
    from sm_hpss_mtl_amd import _lib
    return _lib.load()


def test_library_route_equals_the_restatement_on_a_sweep_of_shapes(lib):
    """The export reports the plan the launchers execute, and the CU count is its argument: the restatement is held against the C++
    without a device over tile, segment, table, fallback and staging boundaries, on a device of 256 and one of 104 CUs, at all three
    alignment classes, under whatever switches are set."""
    n = 0
    for entry in P.ALL_ENTRIES[:5]:
        for K in (1, 9, 10, 24, 44, 66, 201, 257, 697, 698, 960, 961, 1024, 1025, 1938, 1939):
            for T in (1, 14, 15, 33, 43, 44, 67, 88, 98, 100, 101, 180, 333, 2000):
                for lh in ((0,) if entry == "freq" else (1, 3, 11, 13, 17, 21, 23, 31, 63, 4, 65)):
                    for lp in ((0,) if entry.startswith("time") else (1, 7, 11, 17, 21, 51, 6) if entry == "freq" else (1, 7, 11, 17, 21, 51)):
                        for lay in ((0, 1, 2, 3) if entry.endswith("_ex") else (0,)):
                            n_cu, align = ((256, 16), (104, 8), (256, 4), (104, 16), (256, 8), (104, 4))[n % 6]
                            _same(lib, entry, K, T, lh, lp, 3, lay, n_cu, align)
                            n += 1
    assert n > 20000
    assert M.library_route(lib, "hpss_ex", 24, 33, 21, 11, 0, 2, n_cu=N_CU) == P.route("hpss_ex", 24, 33, 21, 11, 0, 2, N_CU)
    with pytest.raises(P.Refused, match="exceeds the grid limit"):
        M.library_route(lib, "time_ex", 24, 33, 21, 0, 65536, 1, n_cu=N_CU)
    for K in (1, 24, 201, 257, 412, 413, 697, 2100):
        for lh, lp in ((21, 11), (17, 17), (11, 11), (11, 21), (21, 21), (31, 31), (21, 0), (13, 7)):
            for n_items in (0, 1, 8, 9, 1001):
                _same(lib, "rag", K, 0, lh, lp, n_items, 2, N_CU, 16)


def test_library_plan_holds_the_persistent_threshold_on_both_sides_without_a_device(lib):
    """B >= 2 n_cu with n_cu an argument: 256 and 104 CUs, one clip short, exact and three over, every layout and alignment class, on
    the shapes the sweep above used to skip (a persistent build exists and the pair is fused)."""
    n = {"persist": 0, "split": 0, "delete_insert": 0}
    for n_cu in (256, 104):
        for entry in ("hpss_ex", "hpss"):
            for K, T in ((25, 33), (24, 34), (24, 36), (201, 98), (201, 97), (201, 100), (410, 98)):
                for lh, lp in ((21, 11), (21, 21), (11, 21), (17, 17), (11, 11), (31, 31)):
                    for B in (2 * n_cu - 1, 2 * n_cu, 2 * n_cu + 3):
                        for lay in ((0, 1, 2) if entry == "hpss_ex" else (0,)):
                            for align in (16, 8, 4):
                                _same(lib, entry, K, T, lh, lp, B, lay, n_cu, align)
                    if not _env():
                        fam = [P.route(entry, K, T, lh, lp, B, 0, n_cu)["family"] for B in (2 * n_cu - 1, 2 * n_cu)]
                        assert fam[0] != "persist"
                        n[fam[1]] += 1
                        if fam[1] == "persist":
                            assert M.library_route(lib, entry, K, T, lh, lp, 2 * n_cu - 1, 0, n_cu=n_cu)["family"] == "split"
                            assert M.library_route(lib, entry, K, T, lh, lp, 2 * n_cu, 0, n_cu=n_cu)["family"] == "persist"
    assert _env() or min(n.values()) >= 8, n


def test_library_reads_every_switch_on_every_call(lib, monkeypatch):
    """Each SMH_MEDIAN_* variable set in-process between two calls of the query moves the plan, and unset moves it back; the
    restatement under the same `env` agrees each time.  SMH_MEDIAN_NOSPLIT is no longer frozen at first use."""
    for name in P.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    a17, a21 = ("hpss_ex", 201, 98, 17, 17, 512, 2), ("hpss_ex", 201, 98, 21, 11, 512, 2)

    def both(a, align=16):
        got = M.library_route(lib, *a, n_cu=N_CU, align=align)
        assert got == P.route(*a, N_CU, env=_env(), align=align), (a, _env())
        return got

    base17, base21 = both(a17), both(a21)
    assert (base17["family"], base17["layout"], base17["dma"], base17["nsh"], base17["nsp"]) == ("split", 2, 1, 1, 2)
    assert (base21["family"], base21["threads"]) == ("persist", 512)
    monkeypatch.setenv("SMH_MEDIAN_NOSPLIT", "1")
    r = both(a17)
    assert (r["family"], r["layout"], r["threads"], r["dma"]) == ("delete_insert", 1, 1024, 0) and both(a21)["family"] == "delete_insert"
    with pytest.raises(P.Refused, match="ragged medians"):
        M.library_route(lib, "rag", 201, 0, 21, 11, 9, 2, n_cu=N_CU)
    monkeypatch.delenv("SMH_MEDIAN_NOSPLIT")
    assert both(a17) == base17 and both(a21) == base21 and both(("rag", 201, 0, 21, 11, 9, 2))["TT"] == 76
    monkeypatch.setenv("SMH_MEDIAN_PERSIST", "1")
    assert both(a17)["family"] == "persist"
    monkeypatch.setenv("SMH_MEDIAN_PERSIST", "0")
    assert both(a17) == base17 and both(a21)["family"] == "split"
    monkeypatch.delenv("SMH_MEDIAN_PERSIST")
    monkeypatch.setenv("SMH_MEDIAN_PTHREADS", "768")
    r = both(a21)
    assert (r["family"], r["threads"], r["lds"]) == ("persist", 768, base21["lds"]) and r["nwh"] + r["nwp"] > 8
    monkeypatch.setenv("SMH_MEDIAN_PTHREADS", "640")  # no such build
    assert both(a21)["family"] == "split"
    monkeypatch.delenv("SMH_MEDIAN_PTHREADS")
    monkeypatch.setenv("SMH_MEDIAN_SEG", "1,1")
    r = both(a17)
    assert (r["family"], r["nsh"], r["nsp"], r["nwh"], r["nwp"]) == ("split", 1, 1, 4, 2)
    monkeypatch.setenv("SMH_MEDIAN_SEG", "2,9")  # 7 + 14 waves do not fit 8: the plan's own counts stay
    assert both(a17) == base17
    monkeypatch.setenv("SMH_MEDIAN_SEG", "1")   # not "nsh,nsp": ignored
    assert both(a17) == base17
    monkeypatch.delenv("SMH_MEDIAN_SEG")
    monkeypatch.setenv("SMH_MEDIAN_DMA_STAGE", "0")
    r = both(a17)
    assert (r["dma"], r["stride"]) == (0, 99) and {k: v for k, v in r.items() if k not in ("dma", "stride")} \
        == {k: v for k, v in base17.items() if k not in ("dma", "stride")}
    monkeypatch.delenv("SMH_MEDIAN_DMA_STAGE")
    assert both(a17) == base17 and both(a21) == base21


# ---- the decoders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T", [(5, 16), (7, 17), (3, 31), (24, 33), (6, 98), (1, 1)])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_decoders_round_trip_the_documented_layouts_and_see_a_shifted_frame(layout, K, T):
    """include/smh.h: 0 = (B, K, T), 1 = (B, T, K), 2 = (B, ceil(T / 16), K, 16).  The encoder here writes those index formulas
    element by element, without the decoder's reshapes; an encoder one frame off must not decode to the same image."""
    B = 3
    h = np.random.default_rng(T).standard_normal((B, K, T)).astype(np.float32)
    nb = (T + 15) // 16
    flat = np.full(P.owned_floats(layout, B, K, T), np.float32(-7.0))
    for b in range(B):
        for k in range(K):
            for t in range(T):
                i = ((b * K + k) * T + t, (b * T + t) * K + k, ((b * nb + t // 16) * K + k) * 16 + t % 16)[layout]
                flat[i] = h[b, k, t]
    assert P.owned_floats(layout, B, K, T) == (B * nb * 16 * K if layout == 2 else B * K * T)
    assert np.array_equal(P.decode_harm(flat, layout, B, K, T), h)
    assert np.array_equal(P.encode_harm(h, layout, pad=-7.0), flat)
    if T > 1:
        for shift in (1, -1):
            assert not np.array_equal(P.decode_harm(P.encode_harm(h, layout, shift=shift), layout, B, K, T), h)


def test_input_clips_hold_what_they_are_there_for():
    """|Gaussian| noise, a clip of multiples of 1/4, and a clip with zero rows, f32 subnormals and values near 1e30; nothing negative,
    no -0.0, nothing that is not finite."""
    S = M.clips(24, 33)
    assert S.shape == (3, 24, 33) and S.dtype == np.float32 and np.isfinite(S).all() and not np.signbit(S).any()
    assert np.array_equal(S[1] * 4, np.round(S[1] * 4)) and len(np.unique(S[1])) < 24
    tiny = np.finfo(np.float32).tiny
    sub = S[2][(S[2] > 0) & (S[2] < tiny)]
    assert len(sub) > 100 and sub.min() >= 1e-41 and sub.max() <= 1.0001e-39 and len(np.unique(sub)) > 50
    assert (S[2] >= 1e30).sum() > 100 and not S[2, :8].any() and S[2, 8:].all()
    assert np.array_equal(M.clip_index(5), [0, 1, 2, 0, 1])
