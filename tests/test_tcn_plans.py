"""No GPU: the restatement of the network forward's launch plan (tests/tcn_plans.py) against plans worked out by hand from the C++
(fill_args / launch_forward as they stood before plan_forward existed), the two LDS boundaries, and the plan branch that every
case of the existing GPU tests of the forward reaches -- read from those tests' own parameter lists."""
import pytest

from tests import tcn_plans as P
from tests.tcn_plans import ONE_SET, PREFETCH, SKEW, SKEW16, Refused, plan

F, NB = 240, 24  # n_feat 240, 3 x 8 blocks unless said


# ---- hand-computed pins ---------------------------------------------------------------------------------------------------------
def test_hand_computed_plans():
    """W = 68, N = 1024: ceil(1024 / 256) = 4 patches per workgroup, 272 rows, 17 tiles: the skew schedule (8 x 3 - 17 = 7 >= 3) on 8
    waves, no split; LDS = 8 x 273 x 36 = 78 624 for x and y, + 2 x 4160 x 4 = 33 280 for the weight slots, + 2 064 exchange area.
    N = 510: two patches, 136 -> 144 rows, raised to ceil(5376 / 36) = 150 by the head scratch (8 x 4 x 128 + 16 x 80 floats) and to
    ceil(60 x 128 / 36) = 214 by the layer-0 staging, rounded to 224; 9 tiles: barrier schedule, two register sets, 9 % 8 == 1: split.
    N = 768 (three patches) and W = 99 at N = 510 (two): 13 tiles, which the skew schedule leaves to the barrier schedule.
    One patch of 68 frames: 5 tiles.  W = 249: 256 rows, 16 tiles = two full rounds (8 x 2 - 16 < 3): prefetch, nothing to split.
    W = 500: 512 rows, 8 x 513 x 36 = 147 744 bytes leave no room for the slots; 32 tiles: ceil(32 / w) first drops (4 -> 3) at 11
    waves, one register set."""
    assert plan(68, F, NB, 1024) == (4, 272, 17, 8, SKEW, 1, 0, 78624 + 33280 + 2064) and 78624 + 33280 + 2064 == 113968
    assert plan(68, F, NB, 510) == (2, 224, 9, 8, PREFETCH, 1, 1, 8 * 225 * 36 + 33280 + 2064)
    assert plan(68, F, NB, 510, train=True) == plan(68, F, NB, 510)
    assert plan(68, F, NB, 768)[:7] == (3, 224, 13, 8, PREFETCH, 1, 1)
    assert plan(99, F, NB, 510)[:7] == (2, 224, 13, 8, PREFETCH, 1, 1)
    for N in (1, 37):
        assert plan(68, F, NB, N)[:7] == (1, 224, 5, 8, PREFETCH, 1, 1)
    assert plan(249, F, NB, 9)[:7] == (1, 256, 16, 8, PREFETCH, 1, 0)
    assert plan(500, F, NB, 3) == (1, 512, 32, 11, ONE_SET, 0, 0, 147744)
    # the staging steps of N = 510 one by one
    assert P.group(68, 4, 510) == (2, 160) and P.group(68, 4 * 42, 510) == (2, 160) and P.group(68, 4 * 43, 510) == (2, 160)
    assert P.group(68, 4 * 45, 510) == (2, 160) and P.group(68, 4 * 46, 510) == (2, 176) and P.group(68, F, 510) == (2, 224)


def test_hand_computed_skew_conditions():
    """The skew schedule needs T >= 16 whatever the switch says, fewer than 2048 (block, tile) tasks, at least 12 tiles of which the
    last round leaves three wave slots empty, and not 13."""
    for T, N in ((8, 70), (5, 3)):
        for env in (None, {"SMH_TCN_SKEW": "2"}, {"SMH_TCN_SKEW": "0"}):
            assert plan(T, F, NB, N, env=env).mode == PREFETCH
    assert plan(16, F, NB, 33, env={"SMH_TCN_SKEW": "2"}).mode == SKEW and plan(16, F, NB, 33).mode == PREFETCH
    p = plan(68, F, 80, 1030)
    assert (p.G, p.units, p.mode) == (4, 17, SKEW) and 80 * 17 == 1360
    p = plan(68, F, 160, 1030)
    assert (p.G, p.units, p.mode, p.split_last) == (4, 17, PREFETCH, 1) and 160 * 17 == 2720 >= 2048
    assert plan(68, F, 160, 1030, env={"SMH_TCN_SKEW": "2"}).mode == PREFETCH
    assert plan(68, F, 120, 1030).mode == SKEW and plan(68, F, 121, 1030).mode == PREFETCH  # 2040 < 2048 <= 2057
    # 9 .. 16 tiles at 16 frames a tile (W = 16, G = tiles): below 12 too few, 13 excluded, 14 .. 16 leave fewer than three slots
    modes = {u: plan(16, F, NB, 256 * u).mode for u in range(9, 17)}
    assert [u for u, m in modes.items() if m == SKEW] == [12] and all(plan(16, F, NB, 256 * u).units == u for u in modes)
    assert plan(16, F, NB, 256 * 13, env={"SMH_TCN_SKEW": "2"}).mode == SKEW
    assert [plan(68, F, NB, N).units for N in (256, 257, 513, 769)] == [5, 9, 13, 17]


def test_hand_computed_switches():
    """SMH_TCN_SKEW=0 / 2, SMH_TCN_SPLIT=0, SMH_TCN_G inside [1, gmax] only, SMH_TCN_WAVES clamped to 4..12 (a forced wave count
    survives the skew schedule up to 8), SMH_TCN_PREFETCH=0, and the lab form: inference only, lab builds only, its own LDS size."""
    assert plan(68, F, NB, 1024, env={"SMH_TCN_SKEW": "0"})[:7] == (4, 272, 17, 8, PREFETCH, 1, 1)
    assert plan(68, F, NB, 1024, env={"SMH_TCN_SKEW": "0", "SMH_TCN_SPLIT": "0"})[:7] == (4, 272, 17, 8, PREFETCH, 1, 0)
    assert plan(68, F, NB, 1024, env={"SMH_TCN_SKEW": "1"}).mode == SKEW and plan(68, F, NB, 510, env={"SMH_TCN_SKEW": "1"}).mode == PREFETCH
    assert plan(68, F, NB, 510, env={"SMH_TCN_SKEW": "2"})[:7] == (2, 224, 9, 8, SKEW, 1, 0)
    assert plan(68, F, NB, 1, env={"SMH_TCN_G": "4"})[:3] == (4, 272, 5) and plan(68, F, NB, 1024, env={"SMH_TCN_G": "5"}).G == 4
    assert plan(68, F, NB, 1024, env={"SMH_TCN_G": "1"})[:3] == (1, 224, 5) and plan(68, F, NB, 1024, env={"SMH_TCN_G": "0"}).G == 4
    assert plan(68, F, NB, 510, env={"SMH_TCN_WAVES": "9"})[3:7] == (9, ONE_SET, 1, 0)
    assert plan(68, F, NB, 510, env={"SMH_TCN_WAVES": "99"}).nwaves == 12 and plan(68, F, NB, 510, env={"SMH_TCN_WAVES": "1"})[3:7] == (4, PREFETCH, 1, 0)
    assert plan(68, F, NB, 1024, env={"SMH_TCN_WAVES": "6"})[3:5] == (6, SKEW) and plan(68, F, NB, 1024, env={"SMH_TCN_WAVES": "12"})[3:5] == (8, SKEW)
    assert plan(68, F, NB, 510, env={"SMH_TCN_PREFETCH": "0"})[3:7] == (8, ONE_SET, 1, 0)
    ring = 4 * (2 * 273 * 36 + 4 * 4160 + 128)
    lab = {"SMH_TCN_SKEW": "2", "SMH_TCN_SKEW16": "1"}
    assert plan(68, F, NB, 1024, env=lab, lab=True) == (4, 272, 17, 16, SKEW16, 1, 0, ring) and ring == 145696
    assert plan(68, F, NB, 1024, env=lab) == plan(68, F, NB, 1024) and plan(68, F, NB, 1024, True, lab, lab=True).mode == SKEW
    assert plan(68, F, NB, 1024, env={"SMH_TCN_SKEW": "0", "SMH_TCN_SKEW16": "1"}, lab=True).mode == PREFETCH


# ---- boundaries --------------------------------------------------------------------------------------------------------------------
def test_weight_slots_end_where_the_rows_pass_416():
    """x and y take 8 (GRP + 1) 36 bytes, the slots and the exchange area 35 344: they fit up to GRP + 1 <= (159 744 - 35 344) / 288
    = 431.9, and GRP is a multiple of 16: 416 rows keep them, 432 lose them.  One patch per workgroup from 137 frames on (272 // T),
    so that is patches of 417 frames and more; or, at any T, the layer-0 staging of ceil(F / 4) x 128 floats: 117 x 128 = 14 976
    = 416 x 36 still fits 416 rows (n_feat 468), 118 x 128 does not (n_feat 469: 420 -> 432 rows)."""
    assert 8 * 417 * 36 + 35344 <= P.NET_LDS_LIMIT < 8 * 433 * 36 + 35344
    assert plan(416, F, NB, 5)[:7] == (1, 416, 26, 8, SKEW, 1, 0)   # 26 tiles: 8 x 4 - 26 = 6 empty slots
    assert plan(417, F, NB, 5) == (1, 432, 27, 9, ONE_SET, 0, 0, 8 * 433 * 36)
    assert all(plan(T, F, NB, 1000).wlds == 1 for T in range(1, 417)) and not any(plan(T, F, NB, 1000).wlds for T in range(417, 513))
    assert plan(68, 468, NB, 3)[:7] == (1, 416, 5, 8, PREFETCH, 1, 1)
    assert plan(68, 469, NB, 3)[:7] == (1, 432, 5, 8, ONE_SET, 0, 0)
    assert plan(68, 480, NB, 1024)[:7] == (4, 432, 17, 9, ONE_SET, 0, 0)   # 17 tiles: 9 waves, two each and one with one
    assert plan(68, 480, NB, 1024, env={"SMH_TCN_SKEW": "2"}).mode == ONE_SET      # no slots, no skew schedule


def test_refusal_starts_where_the_activations_alone_pass_the_budget():
    """8 (GRP + 1) 36 > 159 744 from GRP + 1 = 555 on: 544 rows run, 560 are refused.  patch_size <= 512 never gets there; the
    staging does from ceil(F / 4) x 128 > 544 x 36 = 19 584, i.e. 154 k-steps, n_feat 613."""
    assert 8 * 545 * 36 <= P.NET_LDS_LIMIT < 8 * 561 * 36
    assert plan(512, F, NB, 3)[:2] == (1, 512)
    assert plan(68, 612, NB, 3) == (1, 544, 5, 8, ONE_SET, 0, 0, 8 * 545 * 36)
    with pytest.raises(Refused, match="patch_size 68 too long for the LDS-resident TCN"):
        plan(68, 613, NB, 3)


# ---- the branches the GPU tests reach ----------------------------------------------------------------------------------------------
def _params(fn, names):
    """The argument tuples of fn's parametrize mark over `names`."""
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == names]
    return list(mark.args[1])


def _gpu_cases():
    """(test, T, F, n_blocks, N, train, env) of every f32 forward the GPU tests named in the module docstring launch."""
    from tests import test_model_shapes_gpu as shapes, test_parity_gpu as parity, test_training_gpu as training
    out = []
    for ncls, W, N in _params(parity.test_b3mtl_forward_vs_oracle, "ncls,W,N"):
        out.append(("forward_vs_oracle", W, F, NB, N, False, {}))
    for W, N in _params(parity.test_b3mtl_block_schedules_agree, "W,N"):
        for env in ({"SMH_TCN_SKEW": "2", "SMH_TCN_SKEW16": "0"}, {"SMH_TCN_SKEW": "0", "SMH_TCN_SKEW16": "0"},
                    {"SMH_TCN_SKEW": "2", "SMH_TCN_SKEW16": "1"}, {"SMH_TCN_SKEW": "0", "SMH_TCN_SPLIT": "0"}):
            out.append(("block_schedules_agree", W, F, NB, N, False, env))
    for Fd, nb, nd, expect in _params(shapes.test_deep_block_schedules_agree_bit_for_bit, "F,nb,nd,expect_skew"):
        for skew in ("2", "0"):
            out.append(("deep_block_schedules expect %d" % (expect if skew == "2" else 0), 68, Fd, nb * nd, 1030, False, {"SMH_TCN_SKEW": skew}))
    for Fd, nb, nd, W, N, ncls in shapes.FORWARD_SHAPES:
        out.append(("forward_and_trunk_vs_oracle", W, Fd, nb * nd, N, False, {}))
    schedules = {"default": {}, "dwh_valu": {}, "skew": {"SMH_TCN_SKEW": "2"}}   # ("bf16" runs the split-bf16 forward)
    for ncls, N, W in _params(training.test_gradients_and_losses_vs_oracle, "ncls,N,W"):
        for s in _params(training.test_gradients_and_losses_vs_oracle, "schedule"):
            if s in schedules:
                out.append(("gradients_vs_oracle", W, F, NB, N, True, schedules[s]))
    for ncls, N, s in _params(training.test_gradients_and_losses_at_the_config4_batch, "ncls,N,schedule"):
        if s in schedules:
            out.append(("config4_batch", 68, F, NB, N, True, schedules[s]))
    return out


def test_gpu_cases_reach_every_plan_branch():
    """Every branch of plan_forward is run by a GPU test that holds its outputs to the oracle or to another schedule's bits: each
    mode (the 16-wave form in a lab build), the split last tile and the whole one, with and without the weight slots, in
    inference; the training forward on the skew and the two-set barrier schedule, split and whole (it never loses the slots: the
    backward ends at 264 frames); and the 13-tile exclusion under the default switches."""
    cases = _gpu_cases()
    assert len(cases) > 60
    reached = {False: set(), True: set()}
    for name, T, Fd, nb, N, train, env in cases:
        p = plan(T, Fd, nb, N, train, env, lab=True)
        reached[train] |= {"mode " + P.MODE_NAMES[p.mode], "split_last %d" % p.split_last, "wlds %d" % p.wlds}
        if name.startswith("deep_block_schedules"):
            assert int(p.mode == SKEW) == int(name[-1]), (name, p)
        if "SMH_TCN_SKEW" not in env and p.units == 13 and plan(T, Fd, nb, N, train, {"SMH_TCN_SKEW": "2"}).mode == SKEW:
            assert p.mode == PREFETCH and p.split_last == 1
            reached[train].add("13-tile exclusion")
        if not env.get("SMH_TCN_SKEW16") == "1":   # a production build reaches the same branches but the lab form
            assert plan(T, Fd, nb, N, train, env) == p
    assert reached[False] == {"mode one-set", "mode prefetch", "mode skew", "mode skew16", "split_last 0", "split_last 1", "wlds 0",
                              "wlds 1", "13-tile exclusion"}, reached[False]
    assert reached[True] == {"mode prefetch", "mode skew", "split_last 0", "split_last 1", "wlds 1"}, reached[True]
    # what the large cases are there for
    by = {(n, T, N, tuple(sorted(e.items()))): plan(T, Fd, nb, N, tr, e) for n, T, Fd, nb, N, tr, e in cases}
    assert by[("forward_vs_oracle", 500, 2, ())][3:7] == (11, ONE_SET, 0, 0)
    assert by[("forward_vs_oracle", 68, 1030, ())][:5] == (4, 272, 17, 8, SKEW)
    assert by[("forward_vs_oracle", 99, 700, ())][:7] == (2, 224, 13, 8, PREFETCH, 1, 1)
    assert by[("config4_batch", 68, 510, ())][:7] == (2, 224, 9, 8, PREFETCH, 1, 1)
