"""numpy restatement of the four feature branches of the reference's get_featuregram WITHOUT harmonic-percussive separation
(lib/preprocessing.py:378-402), built from the oracle's primitives (TEST INFRASTRUCTURE, like oracle/frontend.py):

    Spec        np.abs(stft(y))                                                        (:381)
    LogSpec     power_to_db(np.abs(stft(y)) ** 2)                                      (:387-388)
    MelSpec     melspectrogram(y=y, sr=fs, n_fft, win_length, hop_length, n_mels)      (:394)
    LogMelSpec  power_to_db(melspectrogram(y=y, sr=fs, ...) ** 2)                      (:400-401)

[librosa] melspectrogram(y=...) forms S = np.abs(stft(y)) ** power with its default power = 2.0 and projects THAT with
filters.mel(sr=sr, n_fft, n_mels): the basis is built for sr = fs (16 kHz here, not the 22 050 Hz that the '*HarmPerc*' branches get
from melspectrogram(S=...) without sr), and what is projected is the power spectrogram, not the magnitude.  The squares are float32
products of float32 arrays, as numpy forms them.  Patches: get_feature_patches' plain branch (lib/preprocessing.py:137-142, 208-214):
tile-if-short, ONE StandardScaler over all rows, tools.extract_patches; the TCN generators transpose to (N, W, F)."""
import numpy as np

from oracle import frontend as ofe

PLAIN_FEATS = ("Spec", "LogSpec", "MelSpec", "LogMelSpec")


def mel_power(S, n_mels, fs=16000, sr=None, power=True):
    """mel_basis(sr = fs) @ |S|**2 with the float64-accumulate-then-round product the oracle states np.dot with.
    sr / power exist so that a test can form the two WRONG variants (the 22 050 Hz basis, the magnitude projection)."""
    S = np.asarray(S, dtype=np.float32)
    K = S.shape[0]
    basis = ofe.mel_basis(fs if sr is None else sr, 2 * (K - 1), n_mels)
    X = S * S if power else S  # float32 square
    return (basis.astype(np.float64) @ X.astype(np.float64)).astype(np.float32)


def featuregram_from_S(S, featName, n_mels=120, fs=16000):
    """Everything of the four branches behind np.abs(librosa.core.stft(...)), from a GIVEN magnitude spectrogram (K, T)."""
    S = np.asarray(S, dtype=np.float32)
    if featName == "Spec":
        return S.copy()
    if featName == "LogSpec":
        return ofe.power_to_db(S ** 2)
    if featName == "MelSpec":
        return mel_power(S, n_mels, fs)
    if featName == "LogMelSpec":
        return ofe.power_to_db(mel_power(S, n_mels, fs) ** 2)
    raise ValueError(featName)


def featuregram(y, featName, n_fft=400, n_mels=120, Tw=25, Ts=10, fs=16000):
    S = ofe.stft_mag(y, n_fft=n_fft, win_length=int(Tw * fs / 1000), hop=int(Ts * fs / 1000))
    return featuregram_from_S(S, featName, n_mels=n_mels, fs=fs)


def feature_patches(FV, patch_size, patch_shift):
    """(rows, T) -> float32 (nP, W, rows): tile, standardise every row over the frames, patch, transpose."""
    FV = ofe.tile_if_short(np.asarray(FV, dtype=np.float32), patch_size)
    return ofe.tcn_input(ofe.extract_patches(ofe.standardize_rows(FV), patch_size, patch_shift))
