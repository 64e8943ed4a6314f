"""No GPU: every case of tests/test_heads_plans_gpu.py (the table of tests/heads_cases.py) sits on the heads plan it is named for
(tests/heads_plans.py), and its draw has no trunk gate inside float32 rounding."""
import pytest

from tests import heads_plans as P
from tests import heads_cases as H
from tests.heads_cases import CASES, CROSS_PLAN_N, DETERMINISM_CASES, case_id


def test_hand_computed_thresholds():
    """The boundaries worked out by hand from the launch code's arithmetic.
    B3_MTL / fusion, 3 classes: rows of 3 + 48 = 51 and 7 floats (both odd already): 232 N <= 124 928 bytes  ->  N <= 538.
    5 classes: rows of 5 + 64 = 69 and 11 floats: 320 N <= 124 928  ->  N <= 390.  1024 threads from N = 513.
    Cascaded: S / M / 3C kernel 4 (33 N + N) = 136 N <= 122 880  ->  N <= 903;  R kernel 4 (17 N + 2 N) = 76 N  ->  N <= 1616."""
    assert P.mtl_lds_bytes(3, 1) == 232 and P.mtl_lds_bytes(5, 1) == 320
    assert P.cascade_lds_bytes(1) == (136, 76)
    assert P.mtl_plan(3, 512) == ("staged", 512) and P.mtl_plan(3, 513) == ("staged", 1024)
    assert P.mtl_plan(3, 538) == ("staged", 1024) and P.mtl_plan(3, 539) == ("global", 1024)
    assert P.mtl_plan(5, 390) == ("staged", 512) and P.mtl_plan(5, 391) == ("global", 512)
    assert P.mtl_plan(5, 512) == ("global", 512) and P.mtl_plan(5, 513) == ("global", 1024)
    assert P.mtl_plan(3, 1) == ("staged", 512) and P.mtl_plan(3, 512, heads_global=True) == ("global", 512)
    assert P.mtl_plan(3, 530, heads_global=True) == ("global", 1024)
    assert P.cascade_plan(903) == {"sm": "staged", "r": "staged"} and P.cascade_plan(904) == {"sm": "global", "r": "staged"}
    assert P.cascade_plan(1616) == {"sm": "global", "r": "staged"} and P.cascade_plan(1617) == {"sm": "global", "r": "global"}
    # five classes never take the staged 1024-thread form, and the switch exists for B3_MTL / fusion only
    assert all(P.mtl_plan(5, N)[0] == "global" for N in range(513, 2000))
    with pytest.raises(ValueError):
        P.plan("cascaded", 3, 10, heads_global=True)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_gpu_cases_reach_the_plan_they_are_named_for(c):
    assert P.plan_name(c["kind"], c["ncls"], c["N"], c["heads_global"]) == c["plan"]
    assert c["N"] >= 100  # the gradient bounds of the GPU file are the project's bounds for N >= 100
    if c["heads_global"]:  # a forced case is one that would be staged otherwise
        assert P.plan_name(c["kind"], c["ncls"], c["N"]).startswith("staged")


@pytest.mark.parametrize("kind,ncls,N,plan", DETERMINISM_CASES)
def test_determinism_cases_reach_their_plan(kind, ncls, N, plan):
    assert P.plan_name(kind, ncls, N) == plan


def test_every_reachable_plan_is_covered_for_every_model_kind():
    """Every row of the plan table, for every model kind that can reach it, and both global forms of the cascaded kernels, has a
    case that is compared with a float64 reference.  Reachable without the switch: staged 512, global 512 (5 classes), staged 1024
    (3 classes), global 1024; B3_MTL also holds global 512 at 3 classes through SMH_HEADS_GLOBAL."""
    have = {(c["kind"], c["plan"]) for c in CASES}
    for kind in ("B3_MTL", "fusion"):
        for plan in ("global512", "staged1024", "global1024"):
            assert (kind, plan) in have, (kind, plan)
    # staged 512 is the plan of the models' existing training tests (N <= 512, 3 classes); B3_MTL has its 5-class edge here too
    assert ("B3_MTL", "staged512") in have
    for plan in ("sm_staged+r_staged", "sm_global+r_staged", "sm_global+r_global"):
        assert ("cascaded", plan) in have, plan
    # a forced global 512 case, a full-size trunk on each 1024-thread form, a case without head dropout on a global plan per kind
    assert any(c["heads_global"] and c["plan"] == "global512" and c["ncls"] == 3 for c in CASES)
    for plan in ("staged1024", "global1024"):
        assert any(c["full"] and c["kind"] == "B3_MTL" and c["plan"] == plan for c in CASES), plan
    for kind in P.KINDS:
        assert any(c["kind"] == kind and not c["drop_heads"] and "global" in c["plan"] for c in CASES), kind
    assert any(c["kind"] == "cascaded" and c["lw"] and c["plan"].endswith("r_global") for c in CASES)


def test_boundary_pairs_are_adjacent_and_on_both_sides():
    """512 | 513, 538 | 539 (3 classes), 390 | 391 (5 classes), 903 | 904 and 1616 | 1617 (cascaded): the two batch sizes are
    neighbours, take different plans, and both are cases."""
    pairs = [("B3_MTL", 3, 512, 513), ("B3_MTL", 3, 538, 539), ("B3_MTL", 5, 390, 391), ("cascaded", 3, 903, 904),
             ("cascaded", 3, 1616, 1617)]
    sizes = {(c["kind"], c["N"]) for c in CASES}
    for kind, ncls, a, b in pairs:
        assert b == a + 1
        assert P.plan_name(kind, ncls, a) != P.plan_name(kind, ncls, b), (kind, a, b)
        assert (kind, a) in sizes and (kind, b) in sizes, (kind, a, b)
    # the fusion model walks the same thresholds
    assert {("fusion", 513), ("fusion", 538), ("fusion", 539), ("fusion", 391)} <= sizes


def test_cross_plan_batches_are_staged_by_default_on_both_thread_counts():
    assert [P.mtl_plan(3, N) for N in CROSS_PLAN_N] == [("staged", 512), ("staged", 1024)]
    assert [P.mtl_plan(3, N, heads_global=True) for N in CROSS_PLAN_N] == [("global", 512), ("global", 1024)]


@pytest.mark.parametrize("c", [c for c in CASES if not c["full"]], ids=case_id)
def test_shallow_draws_have_no_gate_inside_float32_rounding(c):
    """The shallow cases are held to a few float32 roundings (four times the float32 floor of the reference graph).  A relu input or
    a tie of the channel maximum inside float32 rounding lets a float32 forward take the other branch, and on a two-block trunk one
    such gate moves the trunk tensors in front of it by 3e-3 .. 2e-2 (tests/test_heads_plans_gpu.py).  Every case's draw is the first
    seed whose float64 forward keeps the two largest channels of every row at least GAP_MIN = 1e-6 apart (relative) and every relu input
    -- the blocks', the trunk output's and the heads' behind BatchNorm(16) -- at least GATE_MIN = 1e-7 of the largest of its tensor: a change of N, of the seed or of the weights that loses this fails here."""
    def screened(seed):
        w, x, y, drop_tcn, drop_heads, heads, s = H.problem(c["kind"], c["ncls"], c["N"], seed=seed)
        gap, gate, head_gate = H.gate_margins(c["kind"], w, x, drop_tcn, s)
        return gap >= H.GAP_MIN and gate >= H.GATE_MIN and head_gate >= H.GATE_MIN, (seed, gap, gate, head_gate)

    ok, margins = screened(c["seed"])
    assert ok, margins
    for seed in range(c["seed"]):   # ... and it is the FIRST such draw: no draw was passed over for another reason
        ok, margins = screened(seed)
        assert not ok, margins
