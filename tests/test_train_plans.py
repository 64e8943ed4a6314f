"""No GPU: the boundaries of the training step's launch plan (tests/train_plans.py), worked out by hand from the kernels' LDS
layouts, and the three scalar-backward cases of tests/test_training_gpu.py: each on the route it names, and its draw a tenth
inside the GPU test's bound in a float32 evaluation of the reference graph."""
import numpy as np
import pytest

from tests import train_plans as P

VALU = {"SMH_TRAIN_VALU": "1"}


def _bwd(T, dtype=0, env=None, kind="B3_MTL", N=4):
    return P.backward(kind, T, 24, 3, N, dtype, env)


def test_f32_routes_by_patch_length():
    """MFMA short: 4 (4 RPm 36 + 4 32 36 + 80 + 32 + 112) bytes with RPm = T rounded up to 16 -- 93 056 at T = 128, far below the
    156 KB of the network kernels, so the 128 frames of its register prefetch are the limit.  Long (no kernel copies): 148 352
    at T = 256, its own limit.  Scalar: 4 (4 T 33 + 2 4096 + 32 + 3 T + 80) = 540 T + 33 216 <= 159 744 -> T <= 234 with the
    transposed kernel copies, 540 T + 16 832 without -> T <= 264; refused beyond."""
    assert P.NET_LDS_LIMIT == 159744
    assert _bwd(128)["lds"] == 93056 and _bwd(256)["lds"] == 148352
    assert [_bwd(T)["route"] for T in (1, 68, 128, 129, 249, 256, 257, 264)] == \
        ["mfma_short"] * 3 + ["mfma_long"] * 3 + ["scalar"] * 2
    assert _bwd(257)["use_wt"] == 0 and _bwd(264)["use_wt"] == 0 and _bwd(264)["lds"] == 540 * 264 + 16832
    with pytest.raises(P.Refused, match="at most 264 frames"):
        _bwd(265)
    assert [(_bwd(T)["RPm"], _bwd(T)["grid"], _bwd(T)["threads"]) for T in (68, 129)] == [(80, 4, 512), (144, 4, 512)]


def test_scalar_route_under_the_switch():
    assert P.scalar(234) == (540 * 234 + 33216, 1) and P.scalar(235) == (540 * 235 + 16832, 0)
    for T in (1, 68, 128, 234):
        p = _bwd(T, env=VALU)
        assert (p["route"], p["use_wt"], p["threads"], p["grid"]) == ("scalar", 1, 1024, 4), T
    for T in (235, 249, 264):
        assert (_bwd(T, env=VALU)["route"], _bwd(T, env=VALU)["use_wt"]) == ("scalar", 0), T
    with pytest.raises(P.Refused):
        _bwd(265, env=VALU)
    # the scalar kernel computes the Dense-on-trunk gradient itself: no dtrunk, no dwh, no d_gt; the switch overrides dtype 1 too
    p = _bwd(68, dtype=1, env=VALU)
    assert (p["route"], p["dwh"], p["dtrunk_x"], p["gt_patch_floats"], p["acts_last_only"]) == ("scalar", 0, 0, 0, 0)


def test_bf16_route_geometry():
    """Bytes per patch: xT 2 x 32 rows of 64 K32 + 48, three transposed pairs of 2 x 32 rows of 64 K32 + 16, du 2 (T + 1) 80:
    16 384 K32 + 6 304 + 160 T.  Two patches and the 21 KB operand slot fit 160 KB up to T = 96 (2 x 70 816 + 21 504 = 163 136);
    at T = 97 K32 becomes 4 (87 360 per patch) and one patch fits."""
    assert P.bf16_geo(96) == (2, 3, 70816) and P.bf16_geo(97) == (1, 4, 87360) and P.bf16_geo(68) == (2, 3, 66336)
    assert [P.bf16_geo(T)[1] for T in (1, 32, 33, 64, 65, 96, 97, 128)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [P.bf16_geo(T)[0] for T in (1, 32, 33, 64, 65, 96, 97, 128)] == [2] * 6 + [1] * 2
    assert P.bf16_geo(129) is None and P.bf16_geo(0) is None
    p = _bwd(68, dtype=1, N=5)
    assert (p["route"], p["grid"], p["threads"], p["lds"], p["acts_last_only"]) == ("bf16", 3, 1024, 2 * 66336 + 21504, 1)
    assert p["pack_bytes"] == 24 * 21504 + 5 * 68 * 32 * 4 and p["gt_patch_floats"] == 0
    p = _bwd(128, dtype=1, N=5)
    assert (p["route"], p["grid"], p["threads"], p["G"], p["K32"]) == ("bf16", 5, 512, 1, 4)
    # beyond 128 frames, and under SMH_BWD_BF16=0, dtype 1 keeps the f32 backward behind the bf16 forward -- which then saves every slot
    for T, env in ((129, None), (249, None), (68, {"SMH_BWD_BF16": "0"})):
        p = _bwd(T, dtype=1, env=env)
        assert p["route"].startswith("mfma") and p["acts_last_only"] == 0 and p["gt_patch_floats"] == T * 32, T
    assert _bwd(260, dtype=1)["route"] == "scalar"


def test_small_kernels_around_the_trunk_backward():
    p = P.backward("B3_MTL", 68, 24, 3, 510)
    assert (p["dtrunk_x"], p["dtrunk_y"], p["dwh"], p["dwh_x"], p["dwh_y"], p["dwh_z"]) == (136, 2, "mfma", 34, 4, 8)
    p = P.backward("B3_MTL", 68, 24, 5, 510, env={"SMH_DWH_VALU": "1"})
    assert (p["dwh"], p["dwh_x"], p["dwh_y"], p["dwh_z"]) == ("valu", 136, 32, 5)
    # dtrunk's grid.y: one per 16 tiles of 16 patches, at least 1, at most 8 -- 31 tiles at N = 496, 32 at 497, 127 at 2032, 128 at 2033
    assert [P.backward("single", 68, 1, 3, N)["dtrunk_y"] for N in (1, 496, 497, 2032, 2033, 5000)] == [1, 1, 2, 7, 8, 8]
    assert P.backward("single", 68, 1, 3, 8)["dwh_y"] == 1 and P.backward("cascaded", 68, 1, 5, 8)["dwh_y"] == 4


def test_the_fusion_trunks_take_the_mfma_route_whatever_the_switches():
    for env in (None, VALU, {"SMH_DWH_VALU": "1"}):
        p = P.plan("fusion", 68, 24, 3, 6, env=env)
        assert (p["forward"], p["route"], p["dwh"], p["dtrunk_x"], p["gt_patch_floats"]) == ("trunk_pair", "mfma_short", "none", 0, 0)
    assert P.plan("fusion", 256, 1, 3, 2)["route"] == "mfma_long"
    with pytest.raises(P.Refused, match="at most 256 frames"):
        P.plan("fusion", 257, 1, 3, 2)
    for kind in ("cascaded", "fusion", "single"):
        with pytest.raises(P.Refused, match="B3_MTL heads only"):
            P.plan(kind, 68, 1, 3, 2, dtype=1)


def test_heads_part_is_the_heads_restatements():
    """512 | 513, 538 | 539, 390 | 391, 903 | 904, 1616 | 1617 are pinned in tests/test_heads_plans.py; here: the step plan carries them."""
    assert P.heads("B3_MTL", 3, 538) == ("mtl", (1, 1024, 4, 232 * 538), (0, 0, 0, 0))
    assert P.heads("fusion", 3, 539) == ("mtl", (0, 1024, 4, 0), (0, 0, 0, 0))
    assert P.heads("B3_MTL", 5, 390) == ("mtl", (1, 512, 5, 320 * 390), (0, 0, 0, 0))
    assert P.heads("B3_MTL", 3, 512, {"SMH_HEADS_GLOBAL": "1"})[1] == (0, 512, 4, 0)
    assert P.heads("cascaded", 5, 903) == ("cascaded", (1, 512, 3, 136 * 903), (1, 512, 1, 76 * 903))
    assert P.heads("cascaded", 3, 1617) == ("cascaded", (0, 512, 3, 0), (0, 512, 1, 0))
    assert P.heads("single", 3, 513) == ("single", (0, 512, 1, 0), (0, 0, 0, 0))
    assert len(P.ints(P.plan("B3_MTL", 68, 24, 3, 6))) == len(P.FIELDS) == 27


# ---- the scalar-backward cases of tests/test_training_gpu.py ------------------------------------------------------------------------
SCALAR_CASES = [  # (ncls, N, W, env, use_wt): the table of the issue
    (3, 3, 68, VALU, 1),
    (3, 2, 249, VALU, 0),
    (3, 2, 260, None, 0),
]


@pytest.mark.parametrize("ncls,N,W,env,use_wt", SCALAR_CASES)
def test_scalar_cases_are_on_the_route_they_name(ncls, N, W, env, use_wt):
    p = P.plan("B3_MTL", W, 24, ncls, N, env=env)
    assert (p["route"], p["use_wt"], p["dwh"]) == ("scalar", use_wt, "none")


@pytest.mark.parametrize("ncls,N,W,env,use_wt", SCALAR_CASES)
def test_scalar_cases_are_well_conditioned(ncls, N, W, env, use_wt):
    """The reference graph evaluated in float32 on these draws gives every gradient tensor within a TENTH of the GPU test's bound
    (2e-3 max|ref|, + 2e-5 for a Dense(16) bias, + 1e-6 elsewhere): no relu gate or channel-maximum tie of the draw sits inside float32
    rounding, where the device's float32 forward could take the other branch (tests/test_single_task_ref.py does the same).  The order
    of a float32 sum, and with it the figure, follows torch's thread count: the evaluation runs on one thread."""
    import torch
    from oracle import b3_mtl, b3_mtl_train as tr
    from tests import heads_cases as HC
    from tests.test_training_gpu import SCALAR_LW, SCALAR_SEED, _problem
    w, x, y, drop_tcn, drop_heads = _problem(ncls, N, W=W, seed=SCALAR_SEED)
    heads = [n for n, _, _ in b3_mtl.head_spec(ncls)]
    args = ("B3_MTL", x, y, w, ncls, drop_tcn, drop_heads, heads, SCALAR_LW, dict(nb=3, nd=8))
    r64 = HC.reference(*args)                    # oracle.b3_mtl_train.forward_backward
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r32 = HC.reference(*args, dtype=np.float32)  # the same graph in torch at float32 (tests/test_cascaded_ref.py pins it to the oracle)
    finally:
        torch.set_num_threads(threads)
    for name, gref in r64["grads"].items():
        if name.endswith(tr.TRAINABLE_SKIP):
            continue
        err, scale = np.abs(r32["grads"][name] - gref).max(), max(np.abs(gref).max(), 1e-6)
        atol = 2e-5 if name.endswith("/dense/bias") else 1e-6
        assert err <= 0.1 * (2e-3 * scale + atol), (name, err, scale)
