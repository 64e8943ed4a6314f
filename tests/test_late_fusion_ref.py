"""CPU: the late-fusion reference of tests/late_fusion_ref.py -- its blend against the literal expression of
Late_Fusion_Results.py:422-423, its models against the references they are composed from, and the seeds of the GPU parity cases:
the reference alone leaves at most 1 % of a case's patches inside the 2e-4 margin that excludes a patch from the label comparison."""
import numpy as np
import pytest

from oracle import b3_mtl
from tests import cascaded_ref, late_fusion_ref as lref


@pytest.mark.parametrize("alpha", [0.5, 0.3, 0.0, 1.0])
def test_blend_is_the_drivers_expression(alpha):
    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64):
        pred_H, pred_P = (rng.random((50, 3)).astype(dt) for _ in range(2))
        PARAMS = {"late_fusion_alpha": alpha}
        pred = np.add(PARAMS['late_fusion_alpha']*pred_H, (1-PARAMS['late_fusion_alpha'])*pred_P)
        pred_lab = np.argmax(pred, axis=1)
        got = lref.blend(pred_H, pred_P, alpha)
        assert got.dtype == dt and np.array_equal(got, pred) and np.array_equal(np.argmax(got, axis=1), pred_lab)
    # on float32 arrays the expression is two rounded products and one rounded sum with float32 factors a, b
    a, b = np.float32(alpha), np.float32(1.0 - alpha)
    pH, pP = (rng.random((64, 5)).astype(np.float32) for _ in range(2))
    by_hand = ((a * pH).astype(np.float32) + (b * pP).astype(np.float32)).astype(np.float32)
    assert np.array_equal(lref.blend(pH, pP, alpha), by_hand)


def test_argmax_takes_the_first_maximum():
    pred = np.array([[0.25, 0.5, 0.5], [0.5, 0.5, 0.0], [0.1, 0.2, 0.7]], np.float32)
    assert list(np.argmax(lref.blend(pred, pred, 0.5), axis=1)) == [1, 0, 2]


@pytest.mark.parametrize("kind", ["mtl", "cascaded"])
def test_models_are_the_single_model_references(kind):
    W, F, ncls, N = 25, 16, 3, 4
    wH, wP = lref.init_weights(kind, 9, F, W, ncls)
    assert any(not np.array_equal(wH[k], wP[k]) for k in wH)  # two different models
    xH, xP = lref.inputs(N, W, F, 9)
    ref = lref.forward(kind, xH, xP, wH, wP, 0.3, ncls)
    single = b3_mtl.forward if kind == "mtl" else cascaded_ref.forward
    assert np.array_equal(ref["heads_H"], np.concatenate(single(xH, wH, ncls), axis=1))
    assert np.array_equal(ref["heads_P"], np.concatenate(single(xP, wP, ncls), axis=1))
    want = 0.3 * ref["heads_H"][:, -ncls:] + (1 - 0.3) * ref["heads_P"][:, -ncls:]
    assert np.array_equal(ref["pred"], want) and np.allclose(ref["pred"].sum(1), 1.0)
    # alpha = 1 / 0: one model alone
    assert np.array_equal(lref.forward(kind, xH, xP, wH, wP, 1.0, ncls)["pred"], ref["heads_H"][:, -ncls:])
    assert np.array_equal(lref.forward(kind, xH, xP, wH, wP, 0.0, ncls)["pred"], ref["heads_P"][:, -ncls:])


@pytest.mark.parametrize("case", lref.PARITY_CASES, ids=lambda c: "%s-W%d-c%d-F%d-N%d-a%g" % c[:6])
def test_parity_case_seeds_keep_the_label_comparison(case):
    ref = lref.case_reference(case)[4]
    left_out = int((ref["margin"] <= lref.MARGIN).sum())
    print("case %s: %d of %d patches inside the %.0e margin, smallest margin %.3g" % (case, left_out, case[4], lref.MARGIN, ref["margin"].min()))
    assert np.isfinite(ref["pred"]).all()
    assert left_out <= lref.MAX_LEFT_OUT * case[4]
