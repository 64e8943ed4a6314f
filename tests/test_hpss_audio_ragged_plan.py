"""No GPU: the ragged launch plan of the HPSS resynthesis (tests/hpss_audio_ragged_plan.py restates smh_resynth_plan.h) against
values worked out by hand: items per clip, the blocked-harm and S / perc floats of a clip in the workspace, the blocked index, the
bytes a clip adds, the grid and the LDS at the two reference configurations."""
import pytest

from tests import hpss_audio_ragged_plan as P

K400, K512 = 201, 257


def test_items_per_clip():
    """ceil(T / 16): a clip of 16 frames is one tile, 17 frames add a one-frame tile."""
    assert {T: P.rag_items(T) for T in (1, 15, 16, 17, 33, 98, 153)} == {1: 1, 15: 1, 16: 1, 17: 2, 33: 3, 98: 7, 153: 10}


def test_blocked_harm_floats():
    """ceil(T / 16) * K * 16: whole 16-frame blocks, the last one padded."""
    want = {1: 3216, 15: 3216, 16: 3216, 17: 6432, 33: 9648, 98: 22512, 153: 32160}
    assert {T: P.rag_harm_floats(K400, T) for T in want} == want
    assert 201 * 16 == 3216 and 7 * 3216 == 22512 and 10 * 3216 == 32160
    assert P.rag_harm_floats(K512, 17) == 2 * 257 * 16 == 8224


def test_spec_floats_rounded_up_to_4():
    """(K, T) rows of exactly T floats, the clip's total rounded up to 4 so that the next clip starts on 16 bytes."""
    want = {1: 204, 15: 3016, 16: 3216, 17: 3420, 33: 6636, 98: 19700, 153: 30756}
    assert {T: P.rag_spec_floats(K400, T) for T in want} == want
    assert (201 * 1, 201 * 15, 201 * 17, 201 * 33, 201 * 98, 201 * 153) == (201, 3015, 3417, 6633, 19698, 30753)
    assert P.rag_spec_floats(K512, 1) == 260 and P.rag_spec_floats(K512, 4) == 1028


def test_blocked_index():
    """element (k, t) at ((t >> 4) * K + k) * 16 + (t & 15): a tile's own frames are one block, its halo frames lie in the block before."""
    assert P.harm_index(K400, 0, 0) == 0 and P.harm_index(K400, 0, 15) == 15 and P.harm_index(K400, 1, 0) == 16
    assert P.harm_index(K400, 200, 15) == 3215 and P.harm_index(K400, 0, 16) == 3216
    # tile 2 (frames 32 .. 47) at (400, 160): halo frames 30, 31 are the last two columns of block 1
    assert P.harm_index(K400, 7, 30) == (201 + 7) * 16 + 14 == 3342 and P.harm_index(K400, 7, 32) == (402 + 7) * 16 == 6544
    for T in (1, 17, 153):  # every element inside the clip's floats, no two alike
        idx = {P.harm_index(K400, k, t) for k in range(K400) for t in range(T)}
        assert len(idx) == K400 * T and max(idx) < P.rag_harm_floats(K400, T)


def test_clip_bytes():
    """T = 98, K = 201, STFT tiles of 16, median tiles of 76: 4 (2 x 19700 + 22512) + 64 + 8 (7 + 2 + 7) = 247840."""
    assert P.rag_clip_bytes(K400, 98, 16, 76) == 4 * (39400 + 22512) + 64 + 128 == 247840
    assert P.rag_clip_bytes(K400, 1, 16, 76) == 4 * (408 + 3216) + 64 + 24 == 14584


@pytest.mark.parametrize("geom,lds,halo", [((400, 160), 54600, 2), ((512, 160), 64520, 3)])
def test_plan_rag(geom, lds, halo):
    """The LDS budget is the equal-length kernel's; the grid is the per-XCD one: the items rounded up to 8."""
    p = P.plan_rag(*geom, n_items=37)
    assert (p["tile"], p["halo"], p["threads"], p["lds"], p["grid_x"], p["grid_y"], p["refusal"]) == (16, halo, 256, lds, 40, 1, "")
    assert P.plan_rag(*geom, n_items=8)["grid_x"] == 8 and P.plan_rag(*geom, n_items=9)["grid_x"] == 16


def test_plan_rag_refusals():
    assert "hop=65 > n_fft=64" in P.plan_rag(64, 65, 1)["refusal"]
    assert "more than 17" in P.plan_rag(400, 16, 1)["refusal"]
    assert "LDS" in P.plan_rag(2048, 512, 1)["refusal"]


def test_header_states_the_same_constants():
    """The restatement's constants are the header's."""
    import os
    import re
    from tests.conftest import ROOT
    hdr = open(os.path.join(ROOT, "sm_hpss_mtl_amd", "csrc", "smh_resynth_plan.h")).read()
    assert int(re.search(r"constexpr int kTileFrames = (\d+);", hdr).group(1)) == P.TILE_FRAMES
    assert int(re.search(r"constexpr int kHarmBlock = (\d+);", hdr).group(1)) == P.HARM_BLOCK
    assert "inline RagPlan plan_rag(" in hdr and "inline size_t rag_clip_bytes(" in hdr
