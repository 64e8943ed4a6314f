"""The Conv2D MTL GPU cases reach the launch plans they are named for: checked on the CPU against tests/cnn_plans.py,
the restatement of the planner code, which a few hand-computed plans pin in turn."""
import pytest

from tests import cnn_plans as P
from tests.test_cnn_gpu import BF16_CASES, CHUNK_CASES
from tests.test_cnn_train_plans_gpu import FORCED, FORCED_CASES, TRAIN_CASES


def test_hand_computed_plans():
    # Doukhan 64 x 80: flatten 11 x 1 x 256 = 2816; fc1 at N = 5 has 1 x 4 tiles -> 512 / 4 -> 16 slices
    fc1 = P.layer("Doukhan", 64, 80, "fc1")
    assert fc1["K"] == 2816
    assert P.forward_plan(fc1, 5) == dict(M=5, ksteps=176, ksplit=16, ksteps_per=11, empty=0)
    assert P.forward_plan(fc1, 5, bf16=True) == dict(M=5, ksteps=88, ksplit=16, ksteps_per=6, empty=1)
    # Doukhan 240 x 68 conv3: 114 x 28 pixels, K = 9 * 128; N = 3 -> 75 tiles -> 7 slices
    c3 = P.layer("Doukhan", 240, 68, "conv3")
    assert (c3["OH"], c3["OW"], c3["K"]) == (114, 28, 1152)
    assert P.forward_plan(c3, 3, bf16=True) == dict(M=9576, ksteps=36, ksplit=7, ksteps_per=6, empty=1)
    # Jang W = 1: 30 x 1 x 128 = 3840 features into fc1 (2048 columns, 16 tiles)
    assert P.forward_plan(P.layer("Jang", 514, 1, "fc1"), 3, bf16=True)["empty"] == 1
    # Doukhan 30 x 68 conv1 at N = 160: 276 480 rows of 64 channels, 16 rows per pass -> 1080 blocks of 256 > 1024
    assert P.col_reduce_plan(160 * 27 * 64, 64) == dict(vec=True, slabs=1, rows_per_pass=16, rows_per_block=272,
                                                        blocks=1017, reblocked=True)
    # Jang W = 12 conv1 at N = 190: 547 200 rows of 32 channels -> 544 rows per block
    assert P.col_reduce_plan(190 * 240 * 12, 32) == dict(vec=True, slabs=1, rows_per_pass=32, rows_per_block=544,
                                                         blocks=1006, reblocked=True)
    assert P.col_reduce_plan(6, 4096)["slabs"] == 4 and P.col_reduce_plan(6, 2048)["slabs"] == 2
    assert not P.col_reduce_plan(6, 100)["vec"] and not P.col_reduce_plan(6, 96)["vec"]
    # Doukhan 30 x 68 conv2 weight gradient at N = 40: 825 k-steps of 16 pixels, 5 x 1 tiles of a 576 x 128 output
    c2 = P.layer("Doukhan", 30, 68, "conv2")
    cap = P.trainer_partial_floats(P.graph("Doukhan", 30, 68), P.trainer_cap(40))
    assert cap == 48 << 20
    assert P.wgrad_plan(c2, 40, cap)["ksplit"] == 49                      # min(1024/5, 825/16) = 51 -> 17 steps each
    p = P.wgrad_plan(c2, 40, cap, env=100)
    assert (p["ksteps_per"], p["ksplit"], p["empty_cut"]) == (9, 92, 8)
    p = P.wgrad_plan(c2, 40, cap, env=100000)                             # 825 slices of 73 728 floats do not fit
    assert p["cap_cut"] and (p["ksteps_per"], p["ksplit"]) == (2, 413) and p["partial"] <= cap
    d = P.dgrad_plan(c2, 40, cap, env=16)
    assert (d["ksteps"], d["ksplit"], d["ksteps_per"], d["empty"]) == (72, 16, 5, 1)
    d = P.dgrad_plan(P.layer("Jang", 514, 12, "conv1"), 8, cap, env=16)  # 3 input channels padded to 4 columns
    assert (d["ldc"], d["ksteps"], d["ksplit"], d["empty"]) == (4, 18, 16, 7)


def test_scalar_col_reduce_is_already_reached():
    """The scalar column reduction is not new ground: Papakostas conv1 (96 channels) and conv2 (384) take it for their
    bias gradients in every Papakostas training test.  What the new cases add is the scalar form on BatchNorm
    statistics (fc 100) and re-blocked (conv1 at N = 72)."""
    plans = P.col_reduce_plans("Papakostas", 61, 68, 6, fc=64)
    assert not plans["conv1"]["vec"] and not plans["conv2"]["vec"] and plans["conv3"]["vec"]


def _ok_forward(kind, H, W, N, fc, branch):
    layers = P.graph(kind, H, W, fc=fc or 64)
    sizes = P.passes(N)
    if branch == "ragged-pass":
        return len(sizes) > 1 and sizes[-1] < P.K_CHUNK
    if branch == "split-k":
        return any(P.forward_plan(L, n, bf16=True)["ksplit"] > 1 for L in layers for n in sizes)
    tag, name = branch.split(":")
    assert tag == "empty-slice"
    L = next(L for L in layers if L["name"] == name)
    return any(P.forward_plan(L, n, bf16=True)["empty"] > 0 for n in sizes)


@pytest.mark.parametrize("case", BF16_CASES, ids=lambda c: "%s-%dx%d-N%d-%s" % (c[0], c[1], c[2], c[3], c[5]))
def test_bf16_cases_reach_their_branch(case):
    assert _ok_forward(*case)


def test_bf16_cases_cover_every_empty_slice_shape_of_the_issue():
    names = {(c[0], c[1], c[2], c[5]) for c in BF16_CASES}
    for want in [("Doukhan", 64, 80, "empty-slice:fc1"), ("Doukhan", 240, 68, "empty-slice:conv3"),
                 ("Papakostas", 402, 249, "empty-slice:conv3"), ("Jang", 514, 1, "empty-slice:fc1"),
                 ("Jang", 514, 4, "empty-slice:fc1")]:
        assert want in names
    # one ragged multi-pass batch per network
    assert {c[0] for c in BF16_CASES if c[5] == "ragged-pass" and c[3] > P.K_CHUNK} == {"Doukhan", "Papakostas", "Jang"}


def test_chunk_cases_cross_pass_boundaries():
    """N = 64: one full pass; 65: a one-image last pass; 130: two full passes and a ragged one.  At these widths the
    split counts do not change with the pass (Jang conv3: 4 slices, Papakostas conv3: 16), but the split GEMMs of the
    ragged pass run on a different row-tile grid and lay their partials out over fewer rows."""
    assert P.passes(64) == [64] and P.passes(65) == [64, 1] and P.passes(130) == [64, 64, 2]
    for kind, H, W, name, s in (("Jang", 514, 12, "conv3", 4), ("Papakostas", 66, 40, "conv3", 16)):
        L = P.layer(kind, H, W, name, fc=64)
        full, last = P.forward_plan(L, 64), P.forward_plan(L, 1)
        assert full["ksplit"] == last["ksplit"] == s and -(-full["M"] // P.BM) > -(-last["M"] // P.BM)
    for kind in ("Papakostas", "Jang"):
        got = {(N, nc) for k, H, W, fc, N, nc in CHUNK_CASES if k == kind}
        assert got == {(N, nc) for N in (64, 65, 130) for nc in (3, 5)}


@pytest.mark.parametrize("case", TRAIN_CASES, ids=lambda c: "%s-N%d-%dcls-%s" % (c[0], c[3], c[4], c[6]))
def test_train_cases_reach_their_branch(case):
    kind, H, W, N, n_classes, fc, branches = case
    plans = P.col_reduce_plans(kind, H, W, N, fc=fc or 4096)
    for item in branches.split(","):
        if item == "5-class":
            assert n_classes == 5
            continue
        tag, name = item.split(":")
        p = plans[name]
        assert {"colred-reblocked": p["vec"] and p["reblocked"],
                "colred-slabs4": p["vec"] and p["slabs"] == 4,
                "colred-scalar": not p["vec"],
                "colred-scalar-reblocked": not p["vec"] and p["reblocked"]}[tag], (item, p)
    # the BatchNorm layers of the 3-class big cases: conv1 is the only one re-blocked
    if branches == "colred-reblocked:conv1":
        assert [n for n, p in plans.items() if p["reblocked"]] == ["conv1"]


def test_every_network_has_a_five_class_training_case():
    assert {c[0] for c in TRAIN_CASES if c[4] == 5} == {"Doukhan", "Papakostas", "Jang"}


@pytest.mark.parametrize("case", FORCED_CASES, ids=lambda c: "%s-N%d" % (c[0], c[3]))
def test_forced_plans_reach_their_branch(case):
    kind, H, W, N = case
    layers = P.graph(kind, H, W)
    cap = P.trainer_partial_floats(layers, P.trainer_cap(N))
    for var, val, branch in FORCED:
        if branch.startswith("wsplit"):
            plans = [P.wgrad_plan(L, N, cap, env=val) for L in layers if L["K"] > P.K_SMALL_K]
            default = [P.wgrad_plan(L, N, cap) for L in layers if L["K"] > P.K_SMALL_K]
            assert all(p["partial"] <= cap for p in plans)
            if branch == "wsplit-1":
                assert all(p["ksplit"] == 1 for p in plans) and any(p["ksplit"] > 1 for p in default)
            elif branch == "wsplit-empty-cut":
                assert any(p["empty_cut"] > 0 for p in plans)
            else:
                assert any(p["ksplit"] > d["ksplit"] for p, d in zip(plans, default))
                # Doukhan conv2 asks for 825 slices at N = 40: only the cap on the partial buffer keeps them in it
                assert any(p["cap_cut"] for p in plans) == (kind == "Doukhan")
        elif branch.startswith("dsplit"):
            plans = [P.dgrad_plan(L, N, cap, env=val) for L in layers if L["index"] > 0]
            default = [P.dgrad_plan(L, N, cap) for L in layers if L["index"] > 0]
            assert all(p["partial"] <= cap for p in plans)
            if branch == "dsplit-1":
                assert all(p["ksplit"] == 1 for p in plans) and any(p["ksplit"] > 1 for p in default)
            else:
                assert any(p["empty"] > 0 for p in plans) and not any(p["empty"] > 0 for p in default)
        elif branch == "wgrad-mfma":  # the first layer leaves the VALU small-K kernel for a split MODE-1 GEMM
            p = P.wgrad_plan(layers[0], N, cap, mfma=True)
            assert P.wgrad_plan(layers[0], N, cap)["kind"] == "smallk" and p["ksplit"] > 1 and p["partial"] <= cap
        else:
            assert branch == "pool-gather" and var == "SMH_CNN_POOL_GATHER"


def test_hand_computed_single_task_plans():
    # Jang single-task 257 x 12: one mel layer of 64 rows, then 64 x 12 -> 32 x 6 -> 16 x 3 -> 8 x 1 through valid pools; no Dense
    layers = P.graph("Jang", 257, 12, single=True)
    assert [(L["name"], L["index"], L["OH"], L["OW"], L["K"]) for L in layers] == \
        [("conv1", 1, 64, 12, 27), ("conv2", 3, 32, 6, 288), ("conv3", 5, 16, 3, 576)]
    assert P.graph("Doukhan", 21, 68, single=True) == P.graph("Doukhan", 21, 68)
    # Doukhan 64 x 80 conv4: 11 x 15 pixels, K = 9 * 128, 2 column tiles.  One image alone: 2 x 2 tiles -> 72 / 8 = 9 slices;
    # planned as a full pass of 64 images: 83 x 2 tiles -> 512 / 166 -> 4 slices, on the rows of the one image
    c4 = P.layer("Doukhan", 64, 80, "conv4")
    assert (c4["OH"], c4["OW"], c4["K"]) == (11, 15, 1152) and P.plan_images(1, single=True) == 64
    assert P.forward_plan(c4, 1) == dict(M=165, ksteps=72, ksplit=9, ksteps_per=8, empty=0)
    assert P.forward_plan(c4, 1, single=True) == dict(M=165, ksteps=72, ksplit=4, ksteps_per=18, empty=0)
    assert P.forward_plan(c4, 64, single=True) == P.forward_plan(c4, 64)
    assert P.tiles(165, 256) == (128, 2, 2) and P.tiles(129, 64) == (64, 2, 1)
    # Doukhan 30 x 68 fc1 at N = 8: 3 x 1 x 256 = 768 features, 48 k-steps -> 6 slices of 8 x 512 floats; a buffer of 10 000 holds 2
    fc1 = P.layer("Doukhan", 30, 68, "fc1")
    assert P.train_forward_plan(fc1, 8, 48 << 20) == dict(M=8, ksteps=48, ksplit=6, ksteps_per=8, partial=24576)
    assert P.train_forward_plan(fc1, 8, 10000) == dict(M=8, ksteps=48, ksplit=2, ksteps_per=24, partial=8192)
    # the workspace of that model at N = 5: activations of conv1 (27 x 64 x 64 floats per image); the largest partials are conv3's
    # (9 x 28 pixels x 5 = 1260 rows in 10 tiles, 72 k-steps -> 9 slices of 1260 x 128), ahead of conv2's 4 x 1650 x 128
    layers = P.graph("Doukhan", 30, 68)
    assert P.forward_partial_floats(layers, 5) == 9 * 1260 * 128
    assert P.workspace_bytes(layers, 30, 68, 5) == 2 * 4 * 27 * 64 * 64 * 5 + 4 * 9 * 1260 * 128
