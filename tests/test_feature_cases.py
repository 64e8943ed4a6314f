"""No GPU: the case table of tests/feature_cases.py holds what it claims, at every length tests/test_feature_edges_gpu.py uses it at, and
its oracle (`reference_from_parts`) is `oracle.frontend.featuregram_from_S` behind the medians, bit for bit."""
import numpy as np
import pytest

from oracle import frontend as ofe
from tests import feature_cases as FC

K = 201
# (n_mels, rows per half) of the GPU test's contexts
BANKS = ((120, 120), (0, 201), (40, 40))


def _all_lengths(rows):
    return sorted(set(FC.lengths(rows, False)) | set(FC.lengths(rows, True)))


def test_budget_restated():
    """smh_feat.h's budget for the contexts of the GPU test: 240 rows end at 165 frames (133 with the layer-0 weights), 402 rows at 97."""
    assert FC.t_last(120, False) == 165 and FC.t_last(120, True) == 133
    assert FC.t_last(201, False) == 97 and FC.t_last(201, True) is None
    assert FC.t_last(40, False) == 501 and FC.t_last(40, True) == 469
    for rows in (120, 201, 40):
        Ts = FC.lengths(rows, False)
        assert {1, 2, 15, 16, 17, 33, 34} <= set(Ts) and Ts[-1] % 2 == 1 and Ts[-2] == Ts[-1] - 1


def test_blocked_round_trips():
    rng = np.random.default_rng(0)
    for T in (1, 2, 15, 16, 17, 33, 98):
        harm = rng.random((3, 24, T)).astype(np.float32) + 1.0
        hb = FC.blocked(harm)
        assert hb.shape == (3, (T + 15) // 16, 24, 16) and hb[0].size == FC.harm_buffer_floats(24, T)
        assert np.array_equal(FC.unblocked(hb, T), harm)
        for t in (0, T // 2, T - 1):
            assert np.array_equal(hb[:, t // 16, :, t % 16], harm[:, :, t])
        assert hb.sum(dtype=np.float64) == harm.sum(dtype=np.float64)  # the padding is zero


@pytest.mark.parametrize("feat", ofe.HPSS_FEATS)
def test_reference_from_parts_is_the_oracle_behind_the_medians(feat):
    rng = np.random.default_rng(1)
    S = np.abs(rng.standard_normal((K, 57))).astype(np.float32)
    S[20:30] = 0.0
    S[:, 40:] *= np.float32(1e-6)
    fv, parts = ofe.featuregram_from_S(S, feat, n_mels=120, return_parts=True)
    got = FC.reference_from_parts(S, parts["harm"], parts["perc"], 120 if "Mel" in feat else 0, feat.startswith("Log"))
    assert got.dtype == fv.dtype and np.array_equal(got, fv)
    assert FC.feat_name(120 if "Mel" in feat else 0, feat.startswith("Log")) == feat


@pytest.mark.parametrize("n_mels,rows", BANKS)
def test_mixed_reaches_every_mask_branch(n_mels, rows):
    """Every clip of `mixed`, every length: at least one live bin of each kind of fallback (exact zeros, denormal medians, the
    normalised form with a real ratio), own^2 underflowing under a normal den, exact 0.5 / 0.5 and 0 / 1 masks; from two frames on a
    wave that holds fallback and normal lanes at one bin, and pairs split either way; from 15 frames on more than 30 % of each dB
    half on the top-dB floor.  The reference is finite."""
    for T in _all_lengths(rows):
        S, harm, perc = FC.build("mixed", K, T)
        for b in range(S.shape[0]):
            pr = FC.premise("mixed", S[b], harm[b], perc[b], n_mels)
            tag = (n_mels, T, b, pr)
            assert pr["finite"], tag
            for kind in ("split_zeros", "tiny_z", "normalised", "own_underflow", "denormal", "equal", "one_zero"):
                assert pr[kind] >= 1, (kind, tag)
            assert pr["fallback"] >= pr["split_zeros"] + pr["tiny_z"] + pr["normalised"], tag
            if T >= 2:
                assert pr["mixed_waves"] >= 1 and pr["pairs_x_in_y_out"] >= 1 and pr["pairs_y_in_x_out"] >= 1, tag
            if T >= 15:
                assert min(pr["floor_fraction"]) > 0.3, tag


@pytest.mark.parametrize("n_mels,rows", BANKS)
def test_other_cases_hold_their_premises(n_mels, rows):
    for T in _all_lengths(rows):
        # max_last: the maximum of each half where it is claimed, every other frame >= 100 dB down and on the floor
        S, harm, perc = FC.build("max_last", K, T)
        for b, where in ((0, lambda a: a[1] == T - 1), (1, lambda a: a == (rows - 1, 0))):
            pr = FC.premise("max_last", S[b], harm[b], perc[b], n_mels)
            tag = (n_mels, T, b, pr)
            assert pr["finite"] and pr["fallback"] == 0, tag
            assert all(where(a) for a in pr["argmax"]), tag
            assert max(pr["rest_over_max"]) <= 1e-5 and min(pr["rest_on_floor"]) == 1.0, tag
        # all_zero / flat: every row constant
        for name in ("all_zero", "flat"):
            S, harm, perc = FC.build(name, K, T)
            for b in range(S.shape[0]):
                pr = FC.premise(name, S[b], harm[b], perc[b], n_mels)
                assert pr["finite"] and pr["constant_rows"] == pr["rows"] == 2 * rows, (name, n_mels, T, b, pr)
                assert (pr["equal"] == K * T) == (name == "flat"), (name, pr)
        # near_constant: both masks exactly 0.5 everywhere; from three frames on every row constant but for one frame
        S, harm, perc = FC.build("near_constant", K, T)
        for b in range(S.shape[0]):
            pr = FC.premise("near_constant", S[b], harm[b], perc[b], n_mels)
            assert pr["finite"] and pr["equal"] == K * T, (n_mels, T, b, pr)
            if T >= 3:
                # (mel row 0 of the 120-filter bank has no taps: constant 0 in both halves)
                assert pr["constant_rows"] == (2 if n_mels == 120 else 0), (n_mels, T, b, pr)
                assert pr["near_constant_rows"] + pr["constant_rows"] == pr["rows"] == 2 * rows, (n_mels, T, b, pr)
        # int16_scale: music-like only (no fallback bin), magnitudes up to 32768 x 1e5
        S, harm, perc = FC.build("int16_scale", K, T)
        pr = FC.premise("int16_scale", S[0], harm[0], perc[0], n_mels)
        assert pr["finite"] and pr["fallback"] == 0 and 1e8 < S.max() < 4e9, (n_mels, T, pr)


def test_near_constant_rows_need_the_low_part_of_the_mean():
    """At T = 98 the majority frames of a near-constant row sit 1.3 .. 2.7 ulp from the row mean (2^-16 / 98 of the value), and the mean's distance from the nearest
    f32 is a good part of an ulp on many rows: without the lo term the standardised values move by more than 1e-4 (the patch bound)."""
    S, harm, perc = FC.build("near_constant", K, 98)
    fv = FC.reference_from_parts(S[1], harm[1], perc[1], 0, False)[:K].astype(np.float64)
    mean = fv.mean(axis=1)
    hi = mean.astype(np.float32).astype(np.float64)
    scale = fv.std(axis=1)
    major = fv[:, 0]
    ulps = np.abs(major - mean) / np.spacing(major.astype(np.float32)).astype(np.float64)
    assert 1.3 < ulps.min() and ulps.max() < 2.7, float(np.median(ulps))
    moved = np.abs((major - mean) / scale - (major - hi) / scale)
    assert np.mean(moved > 1e-3) > 0.5, float(np.mean(moved > 1e-3))
