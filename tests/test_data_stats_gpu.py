"""GPU: `Frontend.row_moments` (smh_row_moments_f64) and lib.preprocessing.get_data_stats on the device path.

row_moments, rows 1 / 31 / 32 / 33 / 240 (one wave's row, a partial and a full block of 16, more than one block) and T 1 / 2 / 63 / 64 /
65 / 129 / 1000 (below, at and beyond one lane stride): sum(x) within T 2^-52 sum|x| of math.fsum, M2 within 1e-10 relative of the
np.longdouble two-pass value (about 100 x T 2^-52 at T = 1000), a constant row exactly 0; the seven lengths as one ragged batch --
views of one buffer and separate tensors mixed -- bit for bit what each clip gives alone; a planted NaN and a planted inf counted at
their (clip, row).  get_data_stats: at most one float32 ulp from the two-pass restatement applied to get_featuregram's outputs."""
import math

import numpy as np
import pytest
import torch

from tests import data_stats_ref as ref

pytestmark = pytest.mark.gpu

TS = (1, 2, 63, 64, 65, 129, 1000)


@pytest.fixture(scope="module")
def fe():
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    return Frontend(FrontendConfig())


def _clip(rows, T, seed):
    """dB-like values (mean -40, spread 15); the last row is constant."""
    x = np.random.default_rng(seed).normal(-40.0, 15.0, size=(rows, T)).astype(np.float32)
    x[rows - 1] = np.float32(-37.3)
    return x


def _mixed_device(clips):
    """Even clips as views of ONE buffer (at float offsets that are not multiples of 4), odd ones as tensors of their own."""
    flat = torch.empty(sum(c.size + 1 for c in clips[::2]) + 1, dtype=torch.float32, device="cuda")
    out, o = [], 1
    for i, c in enumerate(clips):
        if i % 2 == 0:
            v = flat[o:o + c.size].view(c.shape)
            v.copy_(torch.from_numpy(c))
            o += c.size + 1
            out.append(v)
        else:
            out.append(torch.from_numpy(c).cuda())
    return out


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 240])
def test_row_moments_values_and_batch_invariance(fe, rows):
    clips = [_clip(rows, T, 100 * rows + T) for T in TS]
    if rows == 1:  # the only row is the constant one: add its dB-like twin
        clips = clips + [np.random.default_rng(5).normal(-40.0, 15.0, size=(1, 129)).astype(np.float32)]
    alone = [tuple(t[0].cpu().numpy() for t in fe.row_moments([torch.from_numpy(c).cuda()])) for c in clips]
    s, m2, bad = (t.cpu().numpy() for t in fe.row_moments(_mixed_device(clips)))
    assert s.shape == m2.shape == bad.shape == (len(clips), rows) and s.dtype == np.float64 and bad.dtype == np.int32
    assert not bad.any()
    for i, c in enumerate(clips):
        T = c.shape[1]
        for got, one in zip((s[i], m2[i], bad[i]), alone[i]):
            assert np.array_equal(got, one), (rows, T)  # a clip alone and in the ragged batch: the same bits
        x = c.astype(np.longdouble)
        want_s = np.array([math.fsum(map(float, row)) for row in c])
        bound_s = T * 2.0 ** -52 * np.abs(c.astype(np.float64)).sum(axis=1)
        assert np.all(np.abs(s[i] - want_s) <= bound_s), (rows, T, float(np.max(np.abs(s[i] - want_s) / bound_s)))
        mean = x.sum(axis=1) / np.longdouble(T)
        want_m2 = ((x - mean[:, None]) ** 2).sum(axis=1)
        err = np.abs(m2[i].astype(np.longdouble) - want_m2)
        assert np.all(err <= np.longdouble(1e-10) * want_m2), (rows, T, float(np.max(err / np.maximum(want_m2, 1e-300))))
        if np.all(c[rows - 1] == c[rows - 1, 0]):
            assert m2[i, rows - 1] == 0.0 and s[i, rows - 1] == float(c[rows - 1, 0]) * T
        if T == 1:
            assert not m2[i].any()


def test_row_moments_count_planted_non_finite_values(fe):
    rows = 33
    clips = [_clip(rows, T, 7 + T) for T in (65, 129, 64)]
    clean = [t.cpu().numpy() for t in fe.row_moments([torch.from_numpy(c).cuda() for c in clips])]
    clips[1][5, 70] = np.nan
    clips[2][32, 0] = np.inf
    s, m2, bad = (t.cpu().numpy() for t in fe.row_moments([torch.from_numpy(c).cuda() for c in clips]))
    want = np.zeros((3, rows), np.int32)
    want[1, 5] = want[2, 32] = 1
    assert np.array_equal(bad, want)
    assert np.isnan(s[1, 5]) and np.isinf(s[2, 32]) and not np.isfinite(m2[1, 5]) and not np.isfinite(m2[2, 32])
    ok = want == 0
    assert np.array_equal(s[ok], clean[0][ok]) and np.array_equal(m2[ok], clean[1][ok])  # every other (clip, row) as before


def test_row_moments_reject_bad_featuregrams(fe):
    a, b = torch.zeros((4, 9), device="cuda"), torch.zeros((5, 9), device="cuda")
    with pytest.raises(ValueError):
        fe.row_moments([a, b])
    with pytest.raises(ValueError):
        fe.row_moments([])
    with pytest.raises(TypeError):
        fe.row_moments([a.double()])
    with pytest.raises(TypeError):
        fe.row_moments([a.cpu()])


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("model,classes", [("Lemaire_et_al_MTL", 3), ("Lemaire_et_al", 2)])
def test_get_data_stats_on_the_device_matches_the_two_pass_restatement(tmp_path, model, classes):
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    folder, files = ref.dataset(tmp_path)
    P, Pr = ref.params(tmp_path, "feat_dev", model, classes), ref.params(tmp_path, "feat_ref", model, classes)
    feat, n_fft, n_mels, rows, _ = ref.MODELS[model]
    gen.fv_cache_clear()
    got = pp.get_data_stats(P, files, batch_files=4)  # ten files in three ragged batches (seven in two with 2 classes)
    cf = {"music": [pp.get_featuregram(Pr, "music", Pr["feature_opDir"], "", folder + "/music/" + n, None, n_fft, n_mels, feat) for n in files["music"]],
          "speech": [pp.get_featuregram(Pr, "speech", Pr["feature_opDir"], folder + "/speech/" + n, "", None, n_fft, n_mels, feat) for n in files["speech"]]}
    names = ("music", "speech")
    if classes == 3:
        names += ("speech_music",)
        cf["speech_music"] = [pp.get_featuregram(Pr, "speech_music", Pr["feature_opDir"], folder + "/speech/" + m["speech"],
                                                 folder + "/music/" + m["music"], m["SMR"], n_fft, n_mels, feat) for m in files["speech+music"]]
    assert all(a.shape[0] == rows and a.dtype == np.float32 for v in cf.values() for a in v)
    two = ref.two_pass_stats(cf, names)
    mean, stdev, nMu, nSp, nSpMu = got
    assert (nMu, nSp, nSpMu) == (two["frames"]["music"], two["frames"]["speech"], two["frames"].get("speech_music", 0))
    assert mean.dtype == stdev.dtype == np.float32 and mean.shape == stdev.shape == (rows,)
    print("ulps: mean", int(_ulps(mean, two["mean"].astype(np.float32)).max()), "stdev", int(_ulps(stdev, two["stdev"].astype(np.float32)).max()))
    assert _ulps(mean, two["mean"].astype(np.float32)).max() <= 1 and _ulps(stdev, two["stdev"].astype(np.float32)).max() <= 1
    # the reference's .npy cache was written, and the featuregrams stayed on the device: a second pass -- from the device cache,
    # then from the .npy files alone -- gives the same bits
    for cls in names:
        assert len(list((tmp_path / "feat_dev" / cls).glob("*.npy"))) == len(cf[cls])
    for clear in (False, True):
        if clear:
            gen.fv_cache_clear()
        again = pp.get_data_stats(P, files)
        assert np.array_equal(again[0], mean) and np.array_equal(again[1], stdev) and again[2:] == got[2:]
    gen.fv_cache_clear()
