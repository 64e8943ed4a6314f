"""numpy / scipy restatement of HPSS audio separation -- librosa.effects.hpss with this project's framing (center=False, periodic
Hann of win_length zero-padded centrally to n_fft) -- built from the oracle's primitives (TEST INFRASTRUCTURE, like oracle/frontend.py):

    D[:, t] = rfft(w * y[t*hop : t*hop + n_fft])                                     librosa.stft(center=False)
    mask_h  = softmask(harm, perc), mask_p = softmask(perc, harm)                     power 2, split_zeros, margin 1
    y_c     = istft(D * mask_c):  num[n] = sum_t w[n - t*hop] * irfft(D_c[:, t])[n - t*hop],  wss[n] = sum_t w^2[n - t*hop],
              y_c[n] = num[n] / wss[n] where wss[n] > FLT_MIN, else num[n]; 0 behind the last frame      librosa.istft(center=False, length=N)

Every function takes the dtype of ALL its arithmetic: np.float64 is the yardstick, np.float32 (scipy.fft keeps float32 transforms in
float32) measures what a float32 implementation of the same formulas loses, which is what the device's bound is a multiple of."""
import numpy as np
import scipy.fft

from oracle import frontend as ofe

FLT_MIN = float(np.finfo(np.float32).tiny)


def window(n_fft, win_length, dtype=np.float64):
    return ofe.hann_window(win_length, n_fft).astype(dtype)


def stft(y, n_fft, win_length, hop, dtype=np.float64):
    """(K, T) complex spectrogram in `dtype`'s precision."""
    y = np.asarray(y).astype(dtype)
    T = ofe.num_frames(len(y), n_fft, hop)
    idx = np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]
    frames = window(n_fft, win_length, dtype)[:, None] * y[idx]
    D = scipy.fft.rfft(frames, axis=0)
    assert D.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    return D


def softmask(X, X_ref, dtype=np.float64):
    """librosa.util.softmask(X, X_ref, power=2, split_zeros=True); the threshold is float32's tiny in either dtype."""
    X, X_ref = np.asarray(X).astype(dtype), np.asarray(X_ref).astype(dtype)
    Z = np.maximum(X, X_ref)
    bad = Z < FLT_MIN
    Z = np.where(bad, dtype(1), Z)
    m, r = (X / Z) ** 2, (X_ref / Z) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        out = m / (m + r)
    return np.where(bad, dtype(0.5), out).astype(dtype)


def window_sumsquare(N, T, n_fft, win_length, hop, dtype=np.float64):
    w2 = window(n_fft, win_length, dtype) ** 2
    wss = np.zeros(N, dtype)
    for t in range(T):
        wss[t * hop:t * hop + n_fft] += w2
    return wss


def istft(D, N, n_fft, win_length, hop, dtype=np.float64):
    """librosa.istft(D, hop_length=hop, win_length=win_length, center=False, length=N) -> (y, wss)."""
    T = D.shape[1]
    w = window(n_fft, win_length, dtype)
    frames = scipy.fft.irfft(D, n=n_fft, axis=0)
    assert frames.dtype == dtype
    frames = w[:, None] * frames
    num = np.zeros(N, dtype)
    for t in range(T):
        num[t * hop:t * hop + n_fft] += frames[:, t]
    wss = window_sumsquare(N, T, n_fft, win_length, hop, dtype)
    ok = wss > FLT_MIN
    y = num.copy()
    y[ok] = num[ok] / wss[ok]
    return y, wss


def resynth(y, harm, perc, n_fft, win_length, hop, dtype=np.float64):
    """The kernel's job: audio (N,) and the two medians (K, T) -> dict(harmonic, percussive, wss)."""
    D = stft(y, n_fft, win_length, hop, dtype)
    mh, mp = softmask(harm, perc, dtype), softmask(perc, harm, dtype)
    yh, wss = istft(D * mh, len(y), n_fft, win_length, hop, dtype)
    yp, _ = istft(D * mp, len(y), n_fft, win_length, hop, dtype)
    return {"harmonic": yh, "percussive": yp, "wss": wss}


def medians(y, n_fft, win_length, hop, l_harm, l_perc):
    """harm, perc (K, T) float32 as librosa.decompose.hpss forms them from |stft| (float64 rfft -> complex64 -> np.abs: float32)."""
    S = ofe.stft_mag(np.asarray(y, np.float32), n_fft, win_length, hop)
    return ofe.median_time(S, l_harm), ofe.median_freq(S, l_perc)


def separate(y, n_fft=400, win_length=400, hop=160, l_harm=21, l_perc=11, dtype=np.float64):
    """From the audio: librosa.effects.hpss(y, kernel_size=(l_harm, l_perc)) with this framing."""
    harm, perc = medians(y, n_fft, win_length, hop, l_harm, l_perc)
    return resynth(y, harm, perc, n_fft, win_length, hop, dtype)


def distance(a, b, wss, xmax):
    """d(a, b) = max_n |a[n] - b[n]| * wss[n] / max|x|: compares the overlap-add numerators (near a signal's ends wss is as small as
    3.8e-9 and the division amplifies any rounding of the numerator by 1 / wss)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) * np.asarray(wss, np.float64)) / xmax)


def uncovered(wss):
    return np.asarray(wss) <= FLT_MIN


def sine_clicks(N=16000, fs=16000):
    """(x, sine, clicks): a 440 Hz sine of amplitude 0.5 plus unit clicks every 2000 samples from sample 1000."""
    n = np.arange(N)
    sine = 0.5 * np.sin(2 * np.pi * 440.0 * n / fs)
    clicks = np.zeros(N)
    clicks[1000::2000] = 1.0
    return (sine + clicks).astype(np.float32), sine, clicks


def sine_clicks_errors(yh, yp, sine, clicks, lo=400, hi=15600):
    """(harmonic error energy / sine energy, percussive error energy / click energy) over samples lo .. hi - 1."""
    yh, yp = np.asarray(yh, np.float64)[lo:hi], np.asarray(yp, np.float64)[lo:hi]
    s, c = sine[lo:hi], clicks[lo:hi]
    return float(((yh - s) ** 2).sum() / (s ** 2).sum()), float(((yp - c) ** 2).sum() / (c ** 2).sum())


def noise_tone(N, seed, B=None):
    """Unit-peak white noise plus a tone: no bin is 100 dB below its frame's maximum."""
    rng = np.random.default_rng(seed)
    shape = (N,) if B is None else (B, N)
    x = rng.standard_normal(shape) + 0.7 * np.sin(2 * np.pi * 0.031 * np.arange(N) + rng.uniform(0, 6.28, shape[:-1] + (1,)))
    return (x / np.abs(x).max(axis=-1, keepdims=True)).astype(np.float32)


def random_medians(K, T, seed):
    """Positive (K, T) float32 pairs; about 5 % of the bins exact zeros in both, about 5 % zero in one only, a few below FLT_MIN
    (denormal) in both."""
    rng = np.random.default_rng(seed)
    harm = rng.gamma(2.0, 1.0, (K, T)).astype(np.float32)
    perc = rng.gamma(2.0, 1.0, (K, T)).astype(np.float32)
    u = rng.uniform(size=(K, T))
    harm[u < 0.05] = 0
    perc[u < 0.05] = 0
    harm[(u >= 0.05) & (u < 0.075)] = 0
    perc[(u >= 0.075) & (u < 0.10)] = 0
    tiny = (u >= 0.10) & (u < 0.11)
    harm[tiny] = np.float32(3e-39)
    perc[tiny] = np.float32(7e-40)
    return harm, perc
