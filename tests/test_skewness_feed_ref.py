"""CPU: the skewness-vector feed of the generators with the per-file callables injected (no GPU).

PARAMS['skewness_vector'] = 'Row' / 'Col' (Proposed_Work_Results.py:97-113, 475-481): every batch of patches goes through
tools.get_data_statistics(patches, 'skew', axis = 1 / 0), np.expand_dims(.., 2 / 1) and the Lemaire transpose, so that the network
sees (N, 1, F) / (N, W, 1).  Checked here against that composition written out with oracle.tools_stats on the batches the same call
yields WITHOUT the key (same numpy random state): values, shapes, labels and batch order.
"""
import copy
import os

import numpy as np
import pytest

from oracle import tools_stats
from sm_hpss_mtl_amd import generators as gen
from tests.test_generators import F, W, _files, _params, _patches

MODES = {"Row": (1, 2, (1, F)), "Col": (0, 1, (W, 1))}  # mode -> (get_data_statistics axis, expand_dims axis, yielded shape)


def _fv(PARAMS, classname, opdir, sp, mu, db, n_fft, n_mels, featName, save_feat=True):
    """Stand-in featuregram: (F, T) seeded by the file(s) it came from, T differs per file; row 2 is constant."""
    key = sum(map(ord, os.path.basename(sp) + os.path.basename(mu))) + (0 if db is None else 1000 + int(db))
    T = 5 + key % 9
    x = np.random.default_rng(key).gamma(2.0, 3.0, size=(F, T)).astype(np.float32)  # skewed on purpose
    x[2] = 1.5
    return x


def _oracle_vectors(batch_wf, mode):
    """batch (N, W, F) as the generator yields it without the key -> what the reference's composition makes of its (N, F, W) patches."""
    axis, expand, _ = MODES[mode]
    patches = np.transpose(batch_wf, (0, 2, 1))
    v = np.expand_dims(tools_stats.get_data_statistics(patches, "skew", axis), expand)
    return np.transpose(v, (0, 2, 1))


@pytest.mark.parametrize("mode", ["Row", "Col"])
def test_generator_yields_the_oracle_composition(tmp_path, mode):
    P_off = _params(tmp_path, noise=False)
    P_on = dict(P_off, skewness_vector=mode)
    folder, files = _files(tmp_path)
    np.random.seed(321)
    got = gen.generator(P_on, folder, copy.deepcopy(files), 7, featuregram_fn=_fv, patches_fn=_patches)
    got = [next(got) for _ in range(9)]
    np.random.seed(321)
    plain = gen.generator(P_off, folder, copy.deepcopy(files), 7, featuregram_fn=_fv, patches_fn=_patches)
    plain = [next(plain) for _ in range(9)]
    for (xb, yb), (xr, yr) in zip(got, plain):
        assert xr.shape == (21, W, F)
        assert xb.shape == (21,) + MODES[mode][2]
        want = _oracle_vectors(xr, mode)
        np.testing.assert_allclose(xb, want, rtol=1e-10, atol=1e-12)
        assert np.abs(want).max() > 0.1  # (not a comparison of zeros)
        assert set(yb) == set(yr) == {"R", "S", "M", "3C"}
        for k in yr:  # labels and batch order: untouched by the key
            np.testing.assert_array_equal(yb[k], yr[k])
    if mode == "Row":  # the constant row: skew 0, not NaN
        assert all(np.all(x[:, 0, 2] == 0.0) for x, _ in got)


@pytest.mark.parametrize("mode", ["Row", "Col"])
def test_generator_draws_the_same_noise_scale_with_the_key(tmp_path, mode):
    """Noise augmentation is untouched: the batch is the noiseless one plus a draw of its own shape."""
    P = dict(_params(tmp_path, noise=True), skewness_vector=mode)
    folder, files = _files(tmp_path)
    np.random.seed(5)
    x, _ = next(gen.generator(P, folder, copy.deepcopy(files), 7, featuregram_fn=_fv, patches_fn=_patches))
    assert x.shape == (21,) + MODES[mode][2] and np.all(np.isfinite(x))


@pytest.mark.parametrize("mode", ["Row", "Col"])
def test_file_wise_generator_yields_the_oracle_composition(tmp_path, mode):
    P_off = _params(tmp_path, noise=False)
    P_on = dict(P_off, skewness_vector=mode)

    def patches(PARAMS, FV, patch_size, patch_shift, featName):
        assert patch_shift == gen.HARDCODED_TEST_SHIFT
        return _patches(PARAMS, FV, patch_size, 1, featName)

    for sp, mu, db in (("a/sp1.wav", "", None), ("", "a/mu1.wav", None), ("a/sp1.wav", "a/mu1.wav", 10)):
        x, y = gen.test_file_wise_generator(P_on, sp, mu, db, featuregram_fn=_fv, patches_fn=patches)
        xr, yr = gen.test_file_wise_generator(P_off, sp, mu, db, featuregram_fn=_fv, patches_fn=patches)
        assert xr.shape[0] > 0 and xr.shape[1:] == (W, F)
        assert x.shape == (xr.shape[0],) + MODES[mode][2]
        np.testing.assert_allclose(x, _oracle_vectors(xr, mode), rtol=1e-10, atol=1e-12)
        np.testing.assert_array_equal(y, yr)


def test_scaling_comes_before_the_statistic(tmp_path):
    """With frame_level_scaling the fold's statistics are applied to the featuregram first (Baseline_Results.py:91-93), as without the key."""
    rng = np.random.default_rng(11)
    P_off = dict(_params(tmp_path, noise=False), frame_level_scaling=True, fold=2, mean_fold2=rng.normal(6.0, 1.0, F),
                 stdev_fold2=rng.uniform(1.0, 4.0, F))
    P_on = dict(P_off, skewness_vector="Col")
    folder, files = _files(tmp_path)
    np.random.seed(9)
    x, _ = next(gen.generator(P_on, folder, copy.deepcopy(files), 7, featuregram_fn=_fv, patches_fn=_patches))
    np.random.seed(9)
    xr, _ = next(gen.generator(P_off, folder, copy.deepcopy(files), 7, featuregram_fn=_fv, patches_fn=_patches))
    np.testing.assert_allclose(x, _oracle_vectors(xr, "Col"), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("value", ["RowCol", "row", True])
def test_other_values_stay_rejected(tmp_path, value):
    P = dict(_params(tmp_path), skewness_vector=value)
    folder, files = _files(tmp_path)
    with pytest.raises(ValueError, match="skewness_vector"):
        next(gen.generator(P, folder, copy.deepcopy(files), 4, featuregram_fn=_fv, patches_fn=_patches))
    with pytest.raises(ValueError, match="skewness_vector"):
        gen.test_file_wise_generator(P, "a/sp1.wav", "", None, featuregram_fn=_fv, patches_fn=_patches)


@pytest.mark.parametrize("mode", ["Row", "Col"])
def test_a_conv2d_model_is_rejected(tmp_path, mode):
    P = _params(tmp_path)
    m = "Doukhan_et_al_MTL"
    P.update(Model=m, n_fft={m: 400}, n_mels={m: 120}, featName={m: "LogMelHarmPercSpec"}, skewness_vector=mode)
    folder, files = _files(tmp_path)
    with pytest.raises(ValueError, match="skewness_vector"):
        next(gen.generator(P, folder, copy.deepcopy(files), 4, featuregram_fn=_fv, patches_fn=_patches))
    with pytest.raises(ValueError, match="skewness_vector"):
        gen.test_file_wise_generator(P, "a/sp1.wav", "", None, featuregram_fn=_fv, patches_fn=_patches)


def test_the_fusion_generator_keeps_rejecting_the_key(tmp_path):
    P = dict(_params(tmp_path), skewness_vector="Row")
    folder, files = _files(tmp_path)
    with pytest.raises(ValueError, match="skewness_vector"):
        next(gen.fusion_generator(P, folder, copy.deepcopy(files), 4, featuregram_fn=_fv, patches_fn=_patches))
