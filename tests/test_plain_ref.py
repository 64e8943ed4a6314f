"""Pins of tests/plain_ref.py, the restatement of get_featuregram's Spec / LogSpec / MelSpec / LogMelSpec branches
(lib/preprocessing.py:378-402) that tests/test_plain_gpu.py holds the device path to -- and the host-side configuration of that path
(`FrontendConfig.from_params`).  No GPU."""
import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import plain_ref as pr

FS, N_FFT, HOP = 16000, 400, 160


@pytest.fixture(scope="module")
def clip():
    from sm_hpss_mtl_amd.synth import synth_clips
    return synth_clips(1, seed=7, n_samples=8000)[0]


@pytest.fixture(scope="module")
def S(clip):
    return ofe.stft_mag(clip, N_FFT, N_FFT, HOP)


def test_the_16_kHz_basis_is_not_the_22050_Hz_one(S):
    """A path that took the '*HarmPerc*' context's basis (sr = 22 050) would miss by whole dB, not by a tolerance."""
    right = ofe.power_to_db(pr.mel_power(S, 120, FS) ** 2)
    wrong = ofe.power_to_db(pr.mel_power(S, 120, FS, sr=22050) ** 2)
    assert np.array_equal(right, pr.featuregram_from_S(S, "LogMelSpec", 120, FS))
    assert np.median(np.abs(right - wrong)) > 0.1 and np.max(np.abs(right - wrong)) > 3.0  # dB, against 1e-3
    b16, b22 = ofe.mel_basis(16000, N_FFT, 120), ofe.mel_basis(22050, N_FFT, 120)
    assert b16.shape == b22.shape == (120, 201) and np.max(np.abs(b16 - b22)) > 1e-3
    assert np.all(b16[:, -2:].sum(axis=0) > 0) or np.any(b16[-1] > 0)  # the 16 kHz basis reaches the top bins


def test_mel_projects_the_power_not_the_magnitude(S):
    right = pr.featuregram_from_S(S, "MelSpec", 120, FS)
    wrong = pr.mel_power(S, 120, FS, power=False)
    assert np.max(np.abs(right - wrong)) > 1e-2 * right.max()  # against 1e-5 of the maximum
    # the branch formulas, literally
    assert np.array_equal(pr.featuregram_from_S(S, "Spec"), S)
    assert np.array_equal(pr.featuregram_from_S(S, "LogSpec"), ofe.power_to_db(S ** 2))
    assert np.array_equal(pr.featuregram_from_S(S, "LogMelSpec", 120), ofe.power_to_db(right ** 2))
    assert (S ** 2).dtype == np.float32 and right.dtype == np.float32


def test_against_torch_stft_and_an_independent_filterbank(clip, S):
    """melspectrogram(y=..., sr=fs) rebuilt from torch.stft and, where importable, transformers' slaney filterbank and power_to_db."""
    win = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    Z = torch.stft(torch.from_numpy(clip).double(), N_FFT, hop_length=HOP, win_length=N_FFT, window=win, center=False,
                   return_complex=True)
    mag = Z.abs().numpy()
    assert mag.shape == S.shape
    assert np.max(np.abs(mag - S)) <= 1e-6 * S.max()
    au = pytest.importorskip("transformers.audio_utils")
    fb = au.mel_filter_bank(num_frequency_bins=201, num_mel_filters=120, min_frequency=0.0, max_frequency=FS / 2,
                            sampling_rate=FS, norm="slaney", mel_scale="slaney")  # (K, n_mels)
    mel = fb.T.astype(np.float64) @ (mag ** 2)
    ours = pr.featuregram_from_S(S, "MelSpec", 120, FS)
    assert np.max(np.abs(mel - ours)) <= 1e-5 * ours.max()
    db = au.power_to_db(mel ** 2, reference=1.0, min_value=1e-10, db_range=80.0)
    assert np.max(np.abs(db - pr.featuregram_from_S(S, "LogMelSpec", 120, FS))) <= 1e-3


def test_power_to_db_floor_and_clamp_by_hand():
    """Two-bin toys.  |S|**2 = [[1, 1e-6], [1e-12 -> amin 1e-10, 100]] -> dB [[0, -60], [-100, 20]]; the maximum 20 dB puts the
    floor at -60: the -100 rises to it.  Without a floor in reach the clamp alone acts: squares 1e-6, 1e-12, 1e-8, 1e-14 ->
    -60, -100 (clamped), -80, -100 (clamped); floor -140."""
    a = pr.featuregram_from_S(np.array([[1.0, 1e-3], [1e-6, 10.0]], np.float32), "LogSpec")
    np.testing.assert_allclose(a, [[0.0, -60.0], [-60.0, 20.0]], atol=1e-4)
    b = pr.featuregram_from_S(np.array([[1e-3, 1e-6], [1e-4, 1e-7]], np.float32), "LogSpec")
    np.testing.assert_allclose(b, [[-60.0, -100.0], [-80.0, -100.0]], atol=1e-4)
    # LogMelSpec squares the MEL POWER: the clamp sits at mel power 1e-5
    basis = ofe.mel_basis(FS, 2, 1)  # K = 2 bins, one filter
    S2 = np.array([[0.0, 0.0], [1.0, 1e-3]], np.float32)
    m = (basis.astype(np.float64) @ (S2 * S2).astype(np.float64)).astype(np.float32)
    want = 10.0 * np.log10(np.maximum(1e-10, m.astype(np.float64) ** 2))
    want = np.maximum(want, want.max() - 80.0)
    np.testing.assert_allclose(pr.featuregram_from_S(S2, "LogMelSpec", 1, FS), want, atol=1e-4)


def test_patches_tile_standardise_and_transpose():
    fv = np.random.default_rng(0).standard_normal((5, 30)).astype(np.float32)
    p = pr.feature_patches(fv, 68, 68)  # 30 frames tile three times: 30 < 68, then <= 68 -> 90
    assert p.shape == (1, 68, 5) and p.dtype == np.float32
    t = np.tile(fv, (1, 3))
    z = (t - t.mean(axis=1, keepdims=True)) / t.std(axis=1, keepdims=True)
    np.testing.assert_allclose(p[0], z[:, :68].T, atol=1e-5)
    # T = W: no tiling (the `<` of the rule), and tools.extract_patches' centre range(34, 68 - 34) is empty: no patch at all
    assert pr.feature_patches(t[:, :68], 68, 68).shape == (0, 68, 5)
    assert pr.feature_patches(t[:, :69], 68, 68).shape == (1, 68, 5)


PARAMS = {"Model": "Lemaire_et_al_MTL", "Tw": 25, "Ts": 10}  # no l_harm / l_perc


@pytest.mark.parametrize("name,n_mels,log", [("Spec", 0, False), ("LogSpec", 0, True), ("MelSpec", 120, False),
                                              ("LogMelSpec", 120, True)])
def test_from_params_maps_the_plain_names(name, n_mels, log):
    from sm_hpss_mtl_amd.frontend import FrontendConfig
    cfg = FrontendConfig.from_params(PARAMS, 400, 120, name)
    assert cfg.hpss is False and cfg.mel_sr == 16000.0 and cfg.n_mels == n_mels and cfg.log_db is log
    assert (cfg.n_fft, cfg.win_length, cfg.hop, cfg.stft_precision) == (400, 400, 160, "f32")
    assert FrontendConfig.from_params(dict(PARAMS, stft_precision="f64"), 512, 40, name, fs=8000).mel_sr == 8000.0


def test_from_params_keeps_the_hpss_default_and_still_refuses_unknown_names():
    from sm_hpss_mtl_amd.frontend import FrontendConfig
    assert FrontendConfig().hpss is True and FrontendConfig().mel_sr == 22050.0
    full = dict(PARAMS, l_harm={"Lemaire_et_al_MTL": 21}, l_perc={"Lemaire_et_al_MTL": 11})
    assert FrontendConfig.from_params(full, 400, 120, "LogMelHarmPercSpec").hpss is True
    with pytest.raises(KeyError):
        FrontendConfig.from_params(PARAMS, 400, 120, "LogMelHarmPercSpec")  # the HPSS names do need l_harm
    for bad in ("LogMelSpecH", "Mel", ""):
        with pytest.raises(ValueError):
            FrontendConfig.from_params(full, 400, 120, bad)
