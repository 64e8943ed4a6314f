"""CPU: the float64 restatement of HPSS audio separation (tests/hpss_audio_ref.py) is pinned here so that it can serve as the
yardstick of the device tests (tests/test_hpss_audio_gpu.py, tests/test_hpss_audio_frontend_gpu.py).

Bounds, each from reasoning and not from what the code gives:
  * ISTFT against scipy.signal.istft: both are float64 overlap-adds of the same float64 inverse transforms; the worst sample is
    sample 1 of the first frame, where the numerator w[1] * irfft[1] carries the transform's rounding noise (eps * log2(n_fft) of
    the frame's peak, 2.2e-16 * 9) times w[1] and is divided by wss[1] = w[1]^2: 2e-15 / w[1] = 2e-15 / 6.2e-5 = 3.2e-11 for a
    unit-peak signal.  Asserted: 1e-10.  (Measured: 4.6e-12.)
  * y_h + y_p = x on covered samples, in the wss-weighted distance d: a forward and an inverse float64 transform,
    2 * 9 stages * eps = 4e-15.  Asserted: 1e-14.  (Measured: 4e-16.)
  * Sine plus clicks: 1e-3 and 5e-2 are conditions the restatement meets with at least 4x room (5.1e-5, 1.2e-2)."""
import warnings

import numpy as np
import pytest
import scipy.signal

from tests import hpss_audio_ref as ref

CONFIGS = [(400, 400, 160), (512, 400, 160)]


def test_istft_matches_scipy():
    n_fft, wl, hop, N = 400, 400, 160, 4000
    x = ref.noise_tone(N, seed=1)
    K, T = 1 + n_fft // 2, 1 + (N - n_fft) // hop
    ones = np.ones((K, T), np.float32)  # harm == perc: both masks are 1/2
    out = ref.resynth(x, ones, ones, n_fft, wl, hop)
    w = ref.window(n_fft, wl)
    D = ref.stft(x, n_fft, wl, hop)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scipy warns that NOLA fails (sample 0 has wss = 0): expected
        _, y = scipy.signal.istft(0.5 * D / w.sum(), window=w, nperseg=n_fft, noverlap=n_fft - hop, boundary=False)
    cov = n_fft + hop * (T - 1)
    assert cov == 3920 and y.shape == (cov,)
    for c in ("harmonic", "percussive"):
        err = np.abs(out[c][:cov] - y).max()
        print("istft vs scipy, %s: %.3g" % (c, err))
        assert err <= 1e-10
        assert not out[c][cov:].any()


@pytest.mark.parametrize("n_fft,wl,hop,n_unc", [(400, 400, 160, 1), (512, 400, 160, 113)])
def test_components_sum_to_input(n_fft, wl, hop, n_unc):
    N = n_fft + 9 * hop + 77
    x = ref.noise_tone(N, seed=2)
    out = ref.separate(x, n_fft, wl, hop)
    cov = n_fft + hop * (ref.ofe.num_frames(N, n_fft, hop) - 1)
    unc = ref.uncovered(out["wss"][:cov])
    assert int(unc.sum()) == n_unc
    d = ref.distance((out["harmonic"] + out["percussive"])[:cov], x[:cov], out["wss"][:cov], 1.0)
    print("d(y_h + y_p, x) = %.3g" % d)
    assert d <= 1e-14
    for c in ("harmonic", "percussive"):
        assert not out[c][cov:].any()  # behind the last frame: exactly 0
        assert not out[c][:cov][unc].any()  # no window weight: the numerator, 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_softmask_branches(dtype):
    X = np.array([0.0, 1e-39, 0.0, 2.0, 3.0, 1.0], np.float32)
    R = np.array([0.0, 2e-39, 5.0, 0.0, 4.0, 1.0], np.float32)
    m = ref.softmask(X, R, dtype)
    assert m.dtype == dtype
    np.testing.assert_array_equal(m[:4], np.array([0.5, 0.5, 0.0, 1.0], dtype))  # both zero, both below tiny, one zero each way
    np.testing.assert_allclose(m[4:], [9.0 / 25.0, 0.5], rtol=4 * np.finfo(dtype).eps)
    np.testing.assert_allclose(m + ref.softmask(R, X, dtype), 1.0, rtol=4 * np.finfo(dtype).eps)
    # the float32 form is the oracle's softmask bit for bit
    np.testing.assert_array_equal(ref.softmask(X, R, np.float32), ref.ofe.softmask(X, R))


def test_sine_plus_clicks():
    x, sine, clicks = ref.sine_clicks()
    out = ref.separate(x, 400, 400, 160, 21, 11)
    eh, ep = ref.sine_clicks_errors(out["harmonic"], out["percussive"], sine, clicks)
    print("harmonic error energy %.3g of the sine's, percussive %.3g of the clicks'" % (eh, ep))
    assert eh <= 1e-3
    assert ep <= 5e-2


def test_f32_restatement_distance():
    """The float32 restatement's own distance from the float64 one: the unit the device bound is a multiple of."""
    for n_fft, wl, hop in CONFIGS:
        N = n_fft + 20 * hop + 77
        x = ref.noise_tone(N, seed=3)
        harm, perc = ref.random_medians(1 + n_fft // 2, 1 + (N - n_fft) // hop, seed=4)
        r64 = ref.resynth(x, harm, perc, n_fft, wl, hop, np.float64)
        r32 = ref.resynth(x, harm, perc, n_fft, wl, hop, np.float32)
        assert r32["harmonic"].dtype == np.float32
        for c in ("harmonic", "percussive"):
            d = ref.distance(r32[c], r64[c], r64["wss"], 1.0)
            print("(%d, %d, %d) %s: d_ref = %.3g" % (n_fft, wl, hop, c, d))
            assert 1e-8 < d < 1e-6  # float32 rounding of two ~9-stage transforms: a few eps = 6e-8
