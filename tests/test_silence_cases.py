"""Host-only test of the case table tests/silence_cases.py: with oracle/silence.py alone, every crafted case does what its claim
says, every audio case keeps its silence decision out of reach of float32 summation order, and the route arithmetic restated in
the table gives the figures worked out from smh_silence.hip.  (The GPU tests of tests/test_silence_edges_gpu.py then compare the
kernels with the same oracle on cases that are known to reach the branch they name.)  The last two tests ask the library itself,
which loads without a GPU: what callers allocate (the workspace sizes) and what the route query rejects."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import silence as osil
from tests import silence_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "silence_runs_golden.npz"))


def test_table_is_well_formed():
    names = [c.name for c in sc.CRAFTED]
    assert len(set(names)) == len(names)
    for required in ("straddle_8192", "many_runs", "k_clamped_to_1", "k_not_clamped", "l_clamped_to_N", "ends_in_sound",
                     "starts_in_sound", "beta_exact", "beta_above", "thresh_tie", "medfilt_ends", "one_of_many", "all_loud",
                     "all_zero_energy", "alpha_beta", "fewer_frames"):
        assert required in names
    for c in sc.CRAFTED:
        assert c.energy.dtype == np.float32
        full = sc.n_frames(c.N, c.fs, c.Tw, c.Ts)
        assert len(c.energy) == (full - 1 if c.name.startswith("fewer_frames") else full)
        assert len(sc.neighbours(c)) == 2 and c not in sc.neighbours(c)
    assert np.array_equal(sc.CRAFTED_BY_NAME["k_clamped_to_1"].energy, sc.CRAFTED_BY_NAME["k_not_clamped"].energy)


@pytest.mark.parametrize("c", sc.CRAFTED, ids=lambda c: c.name)
def test_crafted_case_does_what_it_claims(c):
    x, out, sm, fm, _ = sc.oracle_remove(c)
    runs = osil.silence_runs(fm, c.N, c.fs, c.Tw, c.Ts, c.beta)
    claim = c.claim
    assert "runs" in claim or "n_runs" in claim
    if "runs" in claim:
        assert runs == claim["runs"]
    if "n_runs" in claim:
        assert len(runs) == claim["n_runs"]
    for k, l in runs:  # the sample marker shows every run that passes beta, also when nothing is removed
        assert not sm[k:l].any()
    assert int((sm == 0).sum()) == sum(l - k for k, l in runs)
    if claim.get("untouched"):
        assert len(runs) < 2 and out is x
    else:
        assert len(runs) >= 2 and out is not x
        kept = int(sm.sum())
        assert kept == claim["kept"]
        assert np.array_equal(out[:kept], x[sm == 1]) and np.all(out[kept:] == 1.0)
    if "straddles" in claim:
        assert any(k < claim["straddles"] < l for k, l in runs)
    if "moves" in claim:
        src, dst = claim["moves"]
        assert sm[src] == 1 and int(sm[:src].sum()) == dst and src // sc.KCHUNK != dst // sc.KCHUNK
    for frame, v in claim.get("fmark", {}).items():
        assert fm[frame] == v


def test_named_edges():
    """The arithmetic behind the claims, where a claim alone does not show it."""
    by = sc.CRAFTED_BY_NAME
    # straddle_8192: one run over sample 8192, the next behind 16384
    (k0, l0), (k1, _) = by["straddle_8192"].claim["runs"]
    assert k0 < 8192 < l0 and k1 > 16384
    # frame size below the shift: 160 * (0 - 1) + 80 < 1
    assert sc.frame_params(16000, 5, 10) == (80, 160) and by["k_clamped_to_1"].claim["runs"][0] == (1, 1840)
    assert by["k_not_clamped"].claim["runs"][0] == (240, 2160)
    assert by["l_clamped_to_N"].claim["runs"][-1] == (14640, 16000) and 160 * 99 + 400 > 16000
    # beta: 15 frames of 80 samples are 1200 samples, and 1200 / 16000 > 0.075 is false in float64
    assert sc.frame_params(16000, 25, 5) == (400, 80) and not (1200 / 16000 > 0.075) and 1280 / 16000 > 0.075
    c = by["beta_exact"]
    cand = osil.silence_runs(sc.oracle_remove(c)[3], c.N, c.fs, c.Tw, c.Ts, -np.inf)
    assert [l - k for k, l in cand if l - k > 0] == [1200, 1200]
    # threshold tie: the float threshold of a clip whose largest energy is 1.0
    c = by["thresh_tie"]
    thresh = np.float32(float(c.alpha) * float(np.max(c.energy)))
    assert thresh == sc.THRESH and (c.energy == thresh).sum() == 15 and (c.energy == sc.BELOW).sum() == 15 and sc.BELOW < thresh
    # many_runs: dozens of runs, 9 silent frames of every 12
    c = by["many_runs"]
    assert len(c.energy) == 1001 and int((c.energy == sc.QUIET).sum()) == 9 * 83 + 5
    # one_of_many: three silent stretches, one run
    c = by["one_of_many"]
    cand = osil.silence_runs(sc.oracle_remove(c)[3], c.N, c.fs, c.Tw, c.Ts, -np.inf)
    assert len([1 for k, l in cand if l - k > 0]) == 3 and len(c.claim["runs"]) == 1
    # alpha_beta: at the default alpha the 0.05 stretches would be loud
    c = by["alpha_beta"]
    assert (c.alpha, c.beta) == (0.1, 0.2) and not osil.silence_runs(
        osil.remove_silence(sc.crafted_signal(c), c.energy, c.fs, c.Tw, c.Ts)[2], c.N, c.fs, c.Tw, c.Ts)


@pytest.mark.parametrize("c", sc.CRAFTED, ids=lambda c: c.name)
def test_golden_matches_table_and_oracle(golden, c):
    """The committed results of the compiled reference belong to THIS table, and the oracle reproduces them."""
    x, out, sm, fm, tot = sc.oracle_remove(c)
    assert np.array_equal(golden[c.name + "_x_sha"], sc.sha(x)) and np.array_equal(golden[c.name + "_energy_sha"], sc.sha(c.energy))
    assert np.array_equal(golden[c.name + "_frame_marker"], fm)
    assert np.array_equal(golden[c.name + "_sample_marker"], np.packbits(sm.astype(np.uint8)))
    assert np.array_equal(golden[c.name + "_out_sha"], sc.sha(out))
    assert list(golden[c.name + "_meta"]) == [c.N, int(sm.sum()), int(out is x), tot]


def test_golden_holds_exactly_the_table(golden):
    assert {k.rsplit("_", 2)[0] if k.endswith("_sha") or k.endswith("_marker") else k[:-len("_meta")] for k in golden.files} \
        == {c.name for c in sc.CRAFTED}


@pytest.mark.parametrize("p", sc.AUDIO_PARAMS, ids=sc.audio_id)
def test_audio_case_margins(p):
    a, n = p
    f = sc.audio_facts(sc.audio_clip(a, n), a.fs, a.Tw, a.Ts)
    assert f["energy_margin"] >= sc.ENERGY_MARGIN_MIN
    assert f["beta_margin_hops"] >= sc.BETA_MARGIN_MIN_HOPS


def test_audio_gap_sets_cover_their_outcomes():
    seen = {}
    for a, n in sc.AUDIO_PARAMS:
        if n < 8000:
            continue  # the 201-sample clips are shorter than any run
        f = sc.audio_facts(sc.audio_clip(a, n), a.fs, a.Tw, a.Ts)
        seen.setdefault(a.gaps, []).append(n)
        frame, hop = sc.frame_params(a.fs, a.Tw, a.Ts)
        if a.gaps == "two_runs":
            assert f["n_runs"] == 2 and f["n_keep"] < n
        elif a.gaps == "one_run":
            assert f["n_runs"] == 1 and f["n_keep"] == n
        elif a.gaps == "both_ends":
            assert f["n_runs"] == 3 and f["runs"][0][0] == max(frame - hop, 1) and f["runs"][-1][1] >= n - hop
        else:
            assert a.gaps == "ends_in_silence" and f["n_runs"] == 2 and f["runs"][-1] == f["candidates"][-1] and f["runs"][-1][1] >= n - hop
    assert all(len(set(v)) >= 3 for v in seen.values()) and set(seen) == {"two_runs", "one_run", "both_ends", "ends_in_silence"}


def test_mixed_batch_outcomes():
    x = sc.mixed_batch()
    assert x.shape == (8, 16000) and x.dtype == np.float32 and 8 * sc.MIXED_REPEAT == 136
    for row, (outcome, _) in zip(x, sc.MIXED_BATCH):
        f = sc.audio_facts(row, sc.MIXED_FS, sc.MIXED_TW, sc.MIXED_TS)
        assert f["energy_margin"] >= sc.ENERGY_MARGIN_MIN and f["beta_margin_hops"] >= sc.BETA_MARGIN_MIN_HOPS
        if outcome == "removed":
            assert f["n_runs"] == 2 and f["n_keep"] < 16000
        elif outcome == "untouched":
            assert f["n_runs"] == 1 and f["n_keep"] == 16000
        elif outcome == "none":
            assert f["n_runs"] == 0 and f["n_keep"] == 16000
        else:
            assert outcome == "both ends" and f["n_runs"] == 3 and f["runs"][0][0] == 240 and f["runs"][-1][1] == 16000
    assert [o for o, _ in sc.MIXED_BATCH] == ["removed", "untouched", "none", "removed", "both ends", "untouched", "removed", "none"]


def test_route_arithmetic():
    assert sc.lds_bytes(36000, 400, 160) == 146736
    assert sc.lds_bytes(36000, 400, 16) == 171030
    assert sc.lds_bytes(33408, 400, 16) <= 155 * 1024 < sc.lds_bytes(33409, 400, 16)
    assert all(sc.lds_bytes(n, 400, 16) > 155 * 1024 for n in range(33409, 36001))  # 33408 is the LAST length inside
    assert sc.route(36000, 16000, 25, 10) == 1 and sc.route(36001, 16000, 25, 10) == 0
    assert sc.route(33408, 16000, 25, 1) == 1 and sc.route(33409, 16000, 25, 1) == 0
    assert sc.route(36000, 16000, 25, 10, multipass=True) == 0
    # frame 551 at fs = 22050: the kernel's frame count is one below the workspace's 1 + N // hop when hop divides N
    assert sc.frame_params(22050, 25, 10) == (551, 220) and sc.n_frames(22000, 22050, 25, 10) == 1 + 21999 // 220 == 22000 // 220
    # both routes are in the table on both sides of both conditions, and every remainder of N % 4 on the LDS route
    routes = {(n, sc.route(n, a.fs, a.Tw, a.Ts)) for a, n in sc.AUDIO_PARAMS}
    assert {(36000, 1), (36001, 0), (33408, 1), (33409, 0), (44101, 0)} <= routes
    assert {n % 4 for n, r in routes if r == 1} == {0, 1, 2, 3}


# ---- the library's host plan (smh_silence.hip: CondPlan, carve), no GPU ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sm_hpss_mtl_amd import _lib
    lib = _lib.load()
    lib.smh_internal_preprocess_route.restype = C.c_int  # test-only export, not in include/smh.h
    lib.smh_internal_preprocess_route.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    return lib


def test_workspace_sizes_are_the_recorded_ones(lib):
    """Bytes that smh_silence_workspace_bytes(B, N, hop) and smh_normalize_workspace_bytes(B, N) returned before the plan struct
    existed: callers allocate by them, so they are pinned as literals."""
    recorded = {(1, 201, 160): (3584, 2560), (3, 16000, 160): (197888, 2560), (8, 36001, 16): (1371136, 3328),
                (136, 160000, 160): (88723968, 54784)}
    for (B, N, hop), (silence, normalize) in recorded.items():
        assert lib.smh_silence_workspace_bytes(B, N, hop) == silence, (B, N, hop)
        assert lib.smh_normalize_workspace_bytes(B, N) == normalize, (B, N)
    # (1, 201, 160) by hand: ten regions of at most 256 bytes (sums, mean, two maxima, two counts, run table, two markers,
    # energies) and 201 floats rounded up to 1024 bytes
    assert 10 * 256 + 1024 == 3584
    for B, N, hop in ((-1, 201, 160), (1, 0, 160), (1, 201, 0), (1, 201, -3)):  # rejected arguments: 0 bytes
        assert lib.smh_silence_workspace_bytes(B, N, hop) == 0
    assert lib.smh_normalize_workspace_bytes(-1, 201) == 0 and lib.smh_normalize_workspace_bytes(1, 0) == 0


def test_route_query_rejects_what_the_entry_rejects(lib, monkeypatch):
    monkeypatch.delenv("SMH_SILENCE_MULTIPASS", raising=False)
    route = lib.smh_internal_preprocess_route
    for N, fs, Tw, Ts in ((0, 16000, 25, 10), (16000, 0, 25, 10), (16000, 16000, 0, 10), (16000, 16000, 25, 0),  # bad parameters
                          (16000, 20, 25, 10),   # frame 0.5 and shift 0.2 samples: both round to zero
                          (16000, 30, 40, 25),   # frame 1 sample, shift 0.75: the shift rounds to zero
                          (16000, 30, 25, 40),   # shift 1 sample, frame 0.75: the frame size rounds to zero
                          (200, 16000, 25, 10),  # N <= frame / 2 = 200: no reflect padding
                          (1, 1000, 2, 1)):      # the smallest such: frame 2, N = 1
        frame, hop = sc.frame_params(fs, Tw, Ts)
        assert min(N, fs, Tw, Ts) < 1 or frame < 1 or hop < 1 or N <= frame // 2  # the case is what its comment says
        assert route(N, fs, Tw, Ts) == -1, (N, fs, Tw, Ts)
    # the first accepted neighbours
    assert route(201, 16000, 25, 10) == 1 and route(2, 1000, 2, 1) == 1 and route(1, 1000, 1, 1) == 1
    assert route(36001, 16000, 25, 10) == 0
    assert route(16000, 1000, 1, 1) == sc.route(16000, 1000, 1, 1) == 0  # frame and shift of one sample: the tables outgrow LDS
    monkeypatch.setenv("SMH_SILENCE_MULTIPASS", "1")  # read on every call
    assert route(201, 16000, 25, 10) == 0 and route(200, 16000, 25, 10) == -1
