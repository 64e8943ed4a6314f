"""CPU: the two host facts the f64 STFT mode (FrontendConfig(stft_precision="f64"), csrc/smh_stft_f64.hip) rests on.

1. numpy's |complex64| is not a correctly rounded hypot but  l = max(|re|, |im|), r = min(..) / l (f32 division),
   |z| = l * sqrtf(fmaf(r, r, 1)), 0 when l = 0.  stft_f64_kernel computes exactly this; a numpy whose complex64 abs differs
   is detected here.
2. The f64 transform's summation order does not survive the rounding to complex64: a host f64 DFT matrix product (another
   order than numpy's pocketfft rfft) followed by the formula reproduces oracle.frontend.stft_mag bit for bit.
"""
import numpy as np
import pytest

from oracle import frontend as ofe

F32 = np.float32
HALF_ULP_1 = 2.0 ** -24  # half an f32 ulp in [1, 2)


def _fmaf_rr1(r):
    """fmaf(r, r, 1) for f32 r in [0, 1], exactly: r*r is exact in f64, 1 + r*r is split into hi + lo (Fast2Sum), and an
    f32 rounding of hi that lands on a tie is redone from the sign of lo."""
    r2 = r.astype(np.float64) ** 2
    hi = 1.0 + r2
    lo = r2 - (hi - 1.0)
    y = hi.astype(F32)
    err = hi - y.astype(np.float64)
    up = (err == HALF_ULP_1) & (lo > 0)
    down = (err == -HALF_ULP_1) & (lo < 0)
    y = np.where(up, np.nextafter(y, F32(np.inf)), y)
    y = np.where(down, np.nextafter(y, F32(0)), y)
    return y.astype(F32)


def np_cabsf(re, im):
    """The magnitude formula of csrc/smh_stft_f64.hip (np_cabsf), in f32 on the host."""
    re, im = np.asarray(re, F32), np.asarray(im, F32)
    a, b = np.abs(re), np.abs(im)
    l, s = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (s / np.where(l == 0, F32(1), l)).astype(F32)
    out = (l * np.sqrt(_fmaf_rr1(r))).astype(F32)
    return np.where(l == 0, F32(0), out)


def test_fmaf_emulation_is_exact_on_ties():
    # 1 + 2^-24 is an f32 tie: exact value on it rounds to even (1), just above it rounds up
    r = np.array([2.0 ** -12, np.nextafter(F32(2.0 ** -12), F32(1)), 0.0, 1.0], F32)
    y = _fmaf_rr1(r)
    assert y[0] == F32(1) and y[1] == np.nextafter(F32(1), F32(2)) and y[2] == F32(1) and y[3] == F32(2)


def test_numpy_complex64_abs_is_the_pinned_formula():
    rng = np.random.default_rng(20261016)
    n = 200_000
    mag = 10.0 ** rng.uniform(-6, 3, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    re = (mag * np.cos(ang)).astype(F32)
    im = (mag * np.sin(ang)).astype(F32)
    # independent scales for the two parts too (ratios far from 1), zeros, one zero part, equal parts, signed zeros
    re2 = (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1, 1], n)).astype(F32)
    im2 = (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1, 1], n)).astype(F32)
    special_re = np.array([0, -0.0, 0, 1e-6, -3.5, 0, 7.25, 1e3, -1e3, 1e-6], F32)
    special_im = np.array([0, 0, -0.0, 0, 0, 2.0, 7.25, -1e3, 1e-6, -1e3], F32)
    zre = np.concatenate([re, re2, special_re, re[:1000], np.zeros(1000, F32)])
    zim = np.concatenate([im, im2, special_im, np.zeros(1000, F32), im[:1000]])
    z = (zre + 1j * zim).astype(np.complex64)
    ref = np.abs(z)
    got = np_cabsf(z.real, z.imag)
    assert ref.dtype == np.float32
    eq = got.view(np.uint32) == ref.view(np.uint32)
    assert eq.all(), "formula differs from np.abs(complex64) on %d of %d values (numpy %s), e.g. %r" % (
        int((~eq).sum()), eq.size, np.__version__, z[~eq][:4])


def _dft_stft_mag(y, n_fft, win_length, hop):
    """|STFT| through a host f64 DFT matrix product (angles 2 pi ((k n) mod N) / N, exactly reduced) and the pinned formula."""
    T = ofe.num_frames(len(y), n_fft, hop)
    w = ofe.hann_window(win_length, n_fft)
    idx = np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]
    x = w[:, None] * y[idx]
    K = 1 + n_fft // 2
    kn = (np.arange(K)[:, None] * np.arange(n_fft)[None, :]) % n_fft
    ang = 2 * np.pi * kn / n_fft
    re = (np.cos(ang) @ x).astype(F32)
    im = (-np.sin(ang) @ x).astype(F32)
    return np_cabsf(re, im)


@pytest.mark.parametrize("n_fft,win_length", [(400, 400), (512, 400)])
def test_f64_dft_and_formula_reproduce_the_oracle_bit_for_bit(clips4, n_fft, win_length):
    total = 0
    for y in clips4:
        ref = ofe.stft_mag(y, n_fft=n_fft, win_length=win_length, hop=160)
        got = _dft_stft_mag(y, n_fft, win_length, 160)
        assert got.shape == ref.shape
        eq = got.view(np.uint32) == ref.view(np.uint32)
        assert eq.all(), "%d of %d bins differ at n_fft=%d" % (int((~eq).sum()), eq.size, n_fft)
        total += eq.size
    assert total > 75_000


def test_frontend_config_validates_stft_precision():
    from sm_hpss_mtl_amd.frontend import FrontendConfig
    assert FrontendConfig().stft_precision == "f32"
    assert FrontendConfig(stft_precision="f64").stft_precision == "f64"
    for bad in ("f16", "F64", "", None, 64):
        with pytest.raises(ValueError):
            FrontendConfig(stft_precision=bad)


def test_from_params_reads_the_optional_stft_precision_key():
    from sm_hpss_mtl_amd.frontend import FrontendConfig
    P = {"Model": "Lemaire_et_al", "Tw": 25, "Ts": 10, "l_harm": {"Lemaire_et_al": 21}, "l_perc": {"Lemaire_et_al": 11}}
    assert FrontendConfig.from_params(P, 400, 120, "LogMelHarmPercSpec") == FrontendConfig()
    c = FrontendConfig.from_params(dict(P, stft_precision="f64"), 400, 120, "LogMelHarmPercSpec")
    assert c == FrontendConfig(stft_precision="f64") and c != FrontendConfig()
    with pytest.raises(ValueError):
        FrontendConfig.from_params(dict(P, stft_precision="f16"), 400, 120, "LogMelHarmPercSpec")
