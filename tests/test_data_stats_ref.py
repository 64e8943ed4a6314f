"""CPU: the arithmetic of frame-level scaling and its host logic (no GPU).

* the one-pass identity sum((x - mu)^2) = M2 + T (m - mu)^2 on float64 per-file moments against the literal two-pass form of
  lib/preprocessing.py:461-586 in np.longdouble;
* the same statistics against the reference's arithmetic as numpy really runs it (float32 class sums), inside a DERIVED bound;
* lib.preprocessing.get_data_stats with the moments injected from numpy: order of the files, frame counts, the +1e-10, the 2- and
  3-class averages, the non-finite error; generators.data_stats_for_fold's pickle round trip; scale_data;
* the per-file-callable path of generator / test_file_wise_generator with frame_level_scaling on, bit for bit against the same
  generators with it off and a featuregram_fn that scales in float64 itself.
"""
import copy
import os
import pickle

import numpy as np
import pytest

from sm_hpss_mtl_amd import generators as gen
from sm_hpss_mtl_amd.lib import preprocessing as pp
from tests import data_stats_ref as ref
from tests.test_generators import F, W, _files, _fv, _params, _patches

CLASSES3 = ("music", "speech", "speech_music")


def _ulps(a, b):
    """Distance of two float32 arrays in units in the last place (same sign, finite)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _class_files(seed, classes, rows=13, n_files=6, max_frames=300, budget=2000):
    """Random dB-like featuregrams: T_i in 1 .. max_frames, at most `budget` frames per class; row means and spreads differ."""
    rng = np.random.default_rng(seed)
    out = {}
    for c in classes:
        Ts = rng.integers(1, max_frames + 1, size=n_files)
        Ts[0] = 1  # a single-frame file: M2 = 0, all of its share comes from T (m - mu)^2
        assert Ts.sum() <= budget
        base = rng.normal(-40.0, 10.0, size=(rows, 1))
        out[c] = [(base + rng.normal(0.0, 15.0, size=(rows, int(T))) * rng.uniform(0.2, 1.0, size=(rows, 1))).astype(np.float32) for T in Ts]
    return out


@pytest.mark.parametrize("classes", [CLASSES3[:2], CLASSES3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_pass_identity_against_the_two_pass_form(classes, seed):
    """The float64 moments carry an error of a few 2^-53 relative; half a float32 ulp is 2^-25: after astype(float32) the two forms
    differ only where the exact value sits at a rounding boundary, by one ulp."""
    cf = _class_files(seed, classes)
    one, two = ref.one_pass_stats(cf, classes), ref.two_pass_stats(cf, classes)
    assert one["frames"] == two["frames"]
    for k in ("mean", "stdev"):
        assert _ulps(one[k].astype(np.float32), two[k].astype(np.float32)).max() <= 1, k
        assert np.max(np.abs(one[k] - two[k]) / np.abs(two[k])) < 1e-12, k


@pytest.mark.parametrize("classes", [CLASSES3[:2], CLASSES3])
def test_class_means_against_the_reference_float32_arithmetic(classes):
    """The reference's np.float128 accumulators are overwritten by the first np.sum of a float32 array, so it sums each class in
    float32.  Any order of N_c - 1 float32 additions of N_c values errs by at most (N_c - 1) u sum|x| / (1 - (N_c - 1) u), u = 2^-24,
    which is below N_c u sum|x| while N_c^2 u <= 1 (N_c <= 4096; here <= 2000); divided by N_c: |dmean[f]| <= N_c 2^-24 mean|x[f]|."""
    cf = _class_files(7, classes)
    ours = ref.one_pass_stats(cf, classes)
    theirs = ref.float32_class_means(cf, classes)
    for c in classes:
        N = ours["frames"][c]
        assert N <= 2000
        mean_abs = np.concatenate(cf[c], axis=1).astype(np.float64).__abs__().mean(axis=1)
        d = np.abs(theirs[c].astype(np.longdouble) - ours["class_means"][c]).astype(np.float64)
        bound = N * 2.0 ** -24 * mean_abs
        print(c, "N =", N, "max |dmean| / bound =", float(np.max(d / bound)))
        assert np.all(d <= bound), c


def _stats_setup(tmp_path, classes):
    P = _params(tmp_path)
    P["classes"] = {i: c for i, c in enumerate(classes)}
    P["folder"] = str(tmp_path / "data")
    folder, files = _files(tmp_path)
    return P, files


def _numpy_moments(PARAMS, seen=None):
    def moments(specs):
        out = []
        for classname, sp, mu, db in specs:
            if seen is not None:
                seen.append((classname, sp, mu, db))
            fv = _fv(PARAMS, classname, PARAMS["feature_opDir"], sp, mu, db, 0, 0, "")
            out.append(ref.file_moments(fv))
        return out
    return moments


def _class_files_of(PARAMS, files, classes):
    folder = PARAMS["folder"]
    cf = {"music": [_fv(PARAMS, "music", "", "", folder + "/music/" + n, None, 0, 0, "") for n in files["music"]],
          "speech": [_fv(PARAMS, "speech", "", folder + "/speech/" + n, "", None, 0, 0, "") for n in files["speech"]]}
    if "speech_music" in classes:
        cf["speech_music"] = [_fv(PARAMS, "speech_music", "", folder + "/speech/" + m["speech"], folder + "/music/" + m["music"], m["SMR"],
                                  0, 0, "") for m in files["speech+music"]]
    return cf


@pytest.mark.parametrize("classes", [CLASSES3[:2], CLASSES3, ("speech", "speech_music", "music")])
def test_get_data_stats_with_injected_moments(tmp_path, classes):
    P, files = _stats_setup(tmp_path, classes)
    seen = []
    mean, stdev, nMu, nSp, nSpMu = pp.get_data_stats(P, files, moments_fn=_numpy_moments(P, seen), batch_files=5)
    # the reference's order: the classes in PARAMS['classes'] order, each list as given, mixtures from files['speech+music']
    want_order = []
    for c in classes:
        if c == "speech_music":
            want_order += [(c, P["folder"] + "/speech/" + m["speech"], P["folder"] + "/music/" + m["music"], m["SMR"]) for m in files["speech+music"]]
        elif c == "music":
            want_order += [(c, "", P["folder"] + "/music/" + n, None) for n in files["music"]]
        else:
            want_order += [(c, P["folder"] + "/speech/" + n, "", None) for n in files["speech"]]
    assert seen == want_order
    cf = _class_files_of(P, files, classes)
    two = ref.two_pass_stats(cf, classes)
    assert (nMu, nSp, nSpMu) == (two["frames"]["music"], two["frames"]["speech"], two["frames"].get("speech_music", 0))
    assert nMu == sum(a.shape[1] for a in cf["music"]) and (nSpMu > 0) == ("speech_music" in classes)
    assert mean.dtype == np.float32 and stdev.dtype == np.float32 and mean.shape == stdev.shape == (F,)
    assert _ulps(mean, two["mean"].astype(np.float32)).max() <= 1 and _ulps(stdev, two["stdev"].astype(np.float32)).max() <= 1
    # the same moments through the restatement: the same bits
    one = ref.one_pass_stats(cf, classes)
    assert np.array_equal(mean, one["mean"].astype(np.float32)) and np.array_equal(stdev, one["stdev"].astype(np.float32))
    # the average is over the CLASS means (unweighted), not over the frames
    pooled = np.concatenate([a for c in classes for a in cf[c]], axis=1).astype(np.float64).mean(axis=1)
    assert np.max(np.abs(mean - pooled)) > 1e-3


def test_class_mean_denominator_carries_the_1e_10():
    """One file of one frame per class: N_c + 1e-10 = 1.0000000001 moves the mean by 1e-10 relative -- visible in longdouble, and the
    restatement and get_data_stats agree on it bit for bit (checked above); here the figure itself."""
    cf = {"music": [np.full((2, 1), 3.0, np.float32)], "speech": [np.full((2, 1), 3.0, np.float32)]}
    one = ref.one_pass_stats(cf, CLASSES3[:2])
    rel = float((np.longdouble(3.0) - one["mean"][0]) / np.longdouble(3.0))
    assert 0.5e-10 < rel < 1.5e-10


def test_get_data_stats_names_the_file_with_a_non_finite_value(tmp_path):
    P, files = _stats_setup(tmp_path, CLASSES3)
    inner = _numpy_moments(P)
    bad_name = files["speech"][4]

    def moments(specs):
        out = inner(specs)
        for i, spec in enumerate(specs):
            if spec[1].endswith(bad_name) and spec[0] == "speech":
                s, m2, bad, T = out[i]
                bad = bad.copy()
                bad[2] = 1
                out[i] = (s, m2, bad, T)
        return out

    with pytest.raises(ValueError, match=bad_name):
        pp.get_data_stats(P, files, moments_fn=moments)
    with np.errstate(invalid="ignore"):
        s, m2, bad, T = ref.file_moments(np.array([[1.0, np.inf, 2.0], [1.0, 2.0, 3.0]], np.float32))
    assert bad.tolist() == [1, 0] and not np.isfinite(s[0])
    with pytest.raises(ValueError, match="NaN or inf"):  # also without the count: the moments themselves are not finite
        pp.get_data_stats(P, {"music": ["m.wav"], "speech": ["s.wav"], "speech+music": []},
                          moments_fn=lambda specs: [(s, m2, np.zeros(2, np.int32), T) for _ in specs])


def test_data_stats_for_fold_pickle_round_trip(tmp_path):
    P, files = _stats_setup(tmp_path, CLASSES3)
    P["fold"], P["train_files"] = 0, files
    calls = []

    def moments(specs):
        calls.append(len(specs))
        return _numpy_moments(P)(specs)

    nFrames = gen.data_stats_for_fold(P, moments_fn=moments)
    path = os.path.join(P["feature_opDir"], "data_stats_fold0_3class_train.pkl")  # Baseline_Results.py:609
    assert os.path.exists(path) and calls
    with open(path, "rb") as f:
        stats = pickle.load(f)
    assert sorted(stats) == ["mean", "nFrames", "stdev"] and stats["nFrames"] == nFrames and len(nFrames) == 3
    mean, stdev = P["mean_fold0"], P["stdev_fold0"]
    assert mean.dtype == np.float32 and np.array_equal(stats["mean"], mean) and np.array_equal(stats["stdev"], stdev)
    # a second call loads the pickle and computes nothing
    P2 = dict(P)
    del P2["mean_fold0"], P2["stdev_fold0"]
    n_before = len(calls)
    assert gen.data_stats_for_fold(P2, moments_fn=moments) == nFrames and len(calls) == n_before
    assert np.array_equal(P2["mean_fold0"], mean) and np.array_equal(P2["stdev_fold0"], stdev)


def test_scale_data_is_the_host_function_without_epsilon():
    rng = np.random.default_rng(3)
    FV = rng.normal(-40, 15, (F, 11)).astype(np.float32)
    mean, stdev = rng.normal(-40, 5, F).astype(np.float32), rng.uniform(1, 20, F).astype(np.float32)
    got = pp.scale_data(FV, mean, stdev)
    assert got.shape == FV.shape and np.array_equal(got, (FV - mean[:, None]) / stdev[:, None])
    assert np.array_equal(pp.scale_data(FV.astype(np.float64), mean.astype(np.float64), stdev.astype(np.float64)),
                          (FV.astype(np.float64) - mean[:, None].astype(np.float64)) / stdev[:, None].astype(np.float64))


# ---- the per-file-callable path of the generators ------------------------------------------------------------------------------
def _scaling_params(tmp_path):
    rng = np.random.default_rng(11)
    P = _params(tmp_path, noise=False)
    P["fold"] = 2
    P["mean_fold2"] = rng.normal(2000.0, 300.0, F).astype(np.float32)  # the stand-in featuregrams are ramps around their file key
    P["stdev_fold2"] = rng.uniform(50.0, 400.0, F).astype(np.float32)
    return P


def _fv_scaled_by_itself(P_on):
    mean, stdev = np.asarray(P_on["mean_fold2"], np.float64), np.asarray(P_on["stdev_fold2"], np.float64)

    def fv(PARAMS, classname, opdir, sp, mu, db, n_fft, n_mels, featName, save_feat=True):
        x = _fv(PARAMS, classname, opdir, sp, mu, db, n_fft, n_mels, featName, save_feat)
        return (x.astype(np.float64) - mean[:, None]) / (stdev[:, None] + 1e-10)
    return fv


def test_generator_scales_between_the_per_file_callables(tmp_path):
    P_on = _scaling_params(tmp_path)
    P_on["frame_level_scaling"] = True
    P_off = dict(P_on, frame_level_scaling=False)
    folder, files = _files(tmp_path)
    np.random.seed(123)
    ours = gen.generator(P_on, folder, copy.deepcopy(files), 7, featuregram_fn=_fv, patches_fn=_patches)
    got = [next(ours) for _ in range(9)]
    np.random.seed(123)
    yard = gen.generator(P_off, folder, copy.deepcopy(files), 7, featuregram_fn=_fv_scaled_by_itself(P_on), patches_fn=_patches)
    want = [next(yard) for _ in range(9)]
    for (xb, yb), (xr, yr) in zip(got, want):
        assert xb.shape == xr.shape == (21, W, F) and xb.dtype == np.float64
        assert np.array_equal(xb, xr)
        for k in yr:
            assert np.array_equal(yb[k], yr[k])
    # ... and it is a scaling: the unscaled batches differ
    np.random.seed(123)
    plain = next(gen.generator(P_off, folder, copy.deepcopy(files), 7, featuregram_fn=_fv, patches_fn=_patches))[0]
    assert not np.array_equal(plain, got[0][0])


def test_file_wise_generator_scales_between_the_per_file_callables(tmp_path):
    P_on = _scaling_params(tmp_path)
    P_on["frame_level_scaling"] = True
    P_off = dict(P_on, frame_level_scaling=False)

    def patches(PARAMS, FV, patch_size, patch_shift, featName):
        return _patches(PARAMS, FV, patch_size, 1, featName)

    for sp, mu, db in (("a/sp1.wav", "", None), ("", "a/mu1.wav", None), ("a/sp1.wav", "a/mu1.wav", 10)):
        x, y = gen.test_file_wise_generator(P_on, sp, mu, db, featuregram_fn=_fv, patches_fn=patches)
        xr, yr = gen.test_file_wise_generator(P_off, sp, mu, db, featuregram_fn=_fv_scaled_by_itself(P_on), patches_fn=patches)
        assert x.shape == xr.shape and x.shape[0] > 0 and x.shape[1:] == (W, F)
        assert np.array_equal(x, xr) and np.array_equal(y, yr)


@pytest.mark.parametrize("missing", ["fold", "mean_fold2", "stdev_fold2", "length"])
def test_generators_reject_missing_statistics(tmp_path, missing):
    P = _scaling_params(tmp_path)
    P["frame_level_scaling"] = True
    if missing == "length":
        P["mean_fold2"] = P["mean_fold2"][:-1]
        P["stdev_fold2"] = P["stdev_fold2"][:-1]
    else:
        del P[missing]
    folder, files = _files(tmp_path)
    with pytest.raises(ValueError):
        next(gen.generator(P, folder, copy.deepcopy(files), 4, featuregram_fn=_fv, patches_fn=_patches))
    with pytest.raises(ValueError):
        gen.test_file_wise_generator(P, "a/sp1.wav", "", None, featuregram_fn=_fv, patches_fn=_patches)
    full = dict(_scaling_params(tmp_path), frame_level_scaling=True, skewness_vector="mean")  # stays rejected, statistics or not
    with pytest.raises(ValueError, match="skewness_vector"):
        next(gen.generator(full, folder, copy.deepcopy(files), 4, featuregram_fn=_fv, patches_fn=_patches))
    with pytest.raises(ValueError, match="skewness_vector"):
        gen.test_file_wise_generator(full, "a/sp1.wav", "", None, featuregram_fn=_fv, patches_fn=_patches)
