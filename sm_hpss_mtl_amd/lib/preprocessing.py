"""Counterpart of lib/preprocessing.py for the hot path -- same function names, argument meaning and
return types as the reference, computed by the HIP library.

  get_featuregram      (preprocessing.py:355-457)  '*HarmPerc*' branches 404-444, Spec / LogSpec / MelSpec / LogMelSpec 378-402
  get_feature_patches  (preprocessing.py:137-292)
  normalize_signal     (preprocessing.py:114-132)
  mix_signals          (preprocessing.py:297-325)
  get_data_stats       (preprocessing.py:461-586)  one pass: the device's per-file row moments, combined on the host
  scale_data           (preprocessing.py:590-614)
plus the batched, device-resident fast path the reference does not have:
  featuregram_batch / feature_patches_batch.

Per-file functions are thin wrappers: one clip is a batch of one.  `load_and_preprocess_signal` (SURVEY 8f
rank 1) decodes .wav/.npy on the host and runs normalise -> rms -> removeSilence -> normalise on the device
(`smh_preprocess_signal_f32`); `preprocess_signal_batch` is the device-resident form for equal-length clips.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import frontend as _fe

_frontends = {}


def _frontend_for(cfg: _fe.FrontendConfig) -> _fe.Frontend:
    fe = _frontends.get(cfg)
    if fe is None:
        fe = _frontends[cfg] = _fe.Frontend(cfg)
    return fe


# ---- signal conditioning (host, numpy: a few vector ops per file) -------------------------------------
def normalize_signal(Xin):
    """preprocessing.py:130-131"""
    Xin = Xin - np.mean(Xin)
    Xin = Xin / np.max(np.abs(Xin))
    return Xin


def mix_signals(Xin_sp, Xin_mu, target_dB):
    """preprocessing.py:297-325 for one pair of signals: a batch of one through `smh_mix_signals_f32` (music looped / cut to
    the speech length, scaled to the target speech-to-music ratio, factors normalised to sum 1, then `normalize_signal`)."""
    sp = torch.from_numpy(np.ascontiguousarray(Xin_sp, dtype=np.float32)).cuda()[None]
    mu = torch.from_numpy(np.ascontiguousarray(Xin_mu, dtype=np.float32)).cuda()[None]
    return mix_signals_batch(sp, mu, [float(target_dB)])[0].cpu().numpy()


def removeSilence(Xin, fs, Tw, Ts, alpha=0.025, beta=0.075):
    """preprocessing.py:21-110, the pure-Python sibling of tools.removeSilence (not on the reference's own call
    path: load_and_preprocess_signal uses the Cython one).  Same frame / sample markers (computed on the device;
    the threshold is the Cython function's float32 one), but the output is really shortened: the samples before the
    first removed run and between runs -- like the reference, the piece after the LAST run is dropped -- and one run
    is enough to trigger it.  Returns (Xin_silrem, sample_silMarker float64, frame_silMarker int, totalSilDuration)."""
    from .. import silence as _sil
    Xin = np.asarray(Xin)
    frameSize, frameShift = int((Tw * fs) / 1000), int((Ts * fs) / 1000)
    d = torch.from_numpy(np.ascontiguousarray(Xin, dtype=np.float32)).cuda()
    energy = _sil.rms(d, frameSize, frameShift)
    _, _, sm, fm = _sil.remove_silence(d, energy, fs, Tw, Ts, alpha, beta, markers=True)
    sample_silMarker = sm[0].cpu().numpy().astype(np.float64)
    frame_silMarker = fm[0].cpu().numpy().astype(int)
    dd = np.diff(np.concatenate([[1.0], sample_silMarker, [1.0]]))
    starts, ends = np.where(dd == -1)[0], np.where(dd == 1)[0]
    totalSilDuration = float(sum((l - k) / fs for k, l in zip(starts, ends)))
    if len(starts) > 0:
        pieces = [Xin[:starts[0]]] + [Xin[ends[i - 1]:starts[i]] for i in range(1, len(starts))]
        Xin_silrem = np.concatenate(pieces) if len(pieces) > 1 else pieces[0]
    else:
        Xin_silrem = Xin
    return Xin_silrem, sample_silMarker, frame_silMarker, totalSilDuration


def mix_signals_batch(Xin_sp, Xin_mu, target_dB):
    """Device-resident form of `mix_signals` for float32 CUDA tensors (B, N), (B, N_mu) and B target SMRs."""
    from .. import silence as _sil
    return _sil.mix_signals(Xin_sp, Xin_mu, target_dB)


def _read_audio(fName, sr=16000):
    """Minimal loader for the 'next' row: .npy (float array already at 16 kHz) or PCM/float .wav."""
    if fName.endswith(".npy"):
        return np.load(fName).astype(np.float32), sr
    from scipy.io import wavfile
    fs, x = wavfile.read(fName)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)
    if fs != sr:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(fs), int(sr))
        x = resample_poly(x, sr // g, fs // g).astype(np.float32)
    return x, sr


def audio_num_samples(fName, sr=16000):
    """Samples `_read_audio` will return for this file (after resampling to sr), from the header alone where possible."""
    if fName.endswith(".npy"):
        return int(np.load(fName, mmap_mode="r").shape[0])
    import wave
    try:
        with wave.open(fName, "rb") as w:
            n, fs = w.getnframes(), w.getframerate()
    except (wave.Error, EOFError):  # float / extensible WAV: let scipy parse it
        x, _ = _read_audio(fName, sr)
        return int(len(x))
    if fs == sr:
        return int(n)
    from math import gcd
    g = gcd(int(fs), int(sr))
    up, down = sr // g, fs // g
    return int(-(-n * up // down))  # scipy.signal.resample_poly: ceil(n * up / down)


def feature_cache_path(feature_opDir, classname, fName_path_sp, fName_path_mu, target_dB):
    """<feature_opDir>/<classname>/<name>.npy as get_featuregram names it (preprocessing.py:357-363)."""
    if (fName_path_sp != '') and (fName_path_mu != ''):
        fName = (fName_path_sp.split('/')[-1].split('.')[0] + '_' + fName_path_mu.split('/')[-1].split('.')[0]
                 + '_' + str(target_dB) + 'dB')
    elif fName_path_sp != '':
        fName = fName_path_sp.split('/')[-1].split('.')[0]
    elif fName_path_mu != '':
        fName = fName_path_mu.split('/')[-1].split('.')[0]
    else:
        raise ValueError("get_featuregram: both file paths are empty")
    return feature_opDir + '/' + classname + '/' + fName + '.npy'


def preprocess_signal_batch(Xin, fs, Tw, Ts):
    """preprocessing.py:332-349 for a float32 CUDA tensor (B, N) of equal-length clips, device resident.
    Returns (Xin_silrem (B, N), n_keep (B,)): like the reference the output keeps the input length, retained
    samples first, then the normalised image of its tail of ones."""
    from .. import silence as _sil
    return _sil.preprocess_signal(Xin, fs, Tw, Ts)


def load_and_preprocess_signal(fName, Tw, Ts):
    """preprocessing.py:330-350 -> (Xin_silrem float32, fs)."""
    Xin, fs = _read_audio(fName)
    dx = torch.from_numpy(np.ascontiguousarray(Xin, dtype=np.float32)).cuda()
    out, _ = preprocess_signal_batch(dx[None], fs, Tw, Ts)
    Xin_silrem = out[0].cpu().numpy()
    if len(Xin_silrem) / fs < 0.1:  # :343-346; duplication keeps mean and max, so the order with :348-349 is free
        while len(Xin_silrem) / fs < 0.1:
            Xin_silrem = np.append(Xin_silrem, Xin_silrem)
    return Xin_silrem, fs


# ---- featuregram ------------------------------------------------------------------------------------------
def featuregram_batch(PARAMS, Xin, n_fft, n_mels, featName, W=None, shift=None, taps=False, fs=16000):
    """Device fast path: Xin float32 CUDA tensor (B, n_samples) of equal-length clips ->
    dict(fv=(B, 2*rows, T)[, patches=(B*nP, W, 2*rows) time-major, standardised]); for Spec / LogSpec / MelSpec / LogMelSpec
    fv=(B, rows, T) and patches=(B*nP, W, rows)."""
    cfg = _fe.FrontendConfig.from_params(PARAMS, n_fft, n_mels, featName, fs)
    return _frontend_for(cfg).run(Xin, W=W, shift=shift, taps=taps)


def featuregram_from_signal(PARAMS, Xin, n_fft, n_mels, featName, fs=16000):
    """One clip: the arithmetic of get_featuregram from `Xin` on (preprocessing.py:378-444)."""
    x = torch.from_numpy(np.ascontiguousarray(Xin, dtype=np.float32)).cuda()[None]
    return featuregram_batch(PARAMS, x, n_fft, n_mels, featName, fs=fs)["fv"][0].cpu().numpy()


def get_featuregram(PARAMS, classname, feature_opDir, fName_path_sp, fName_path_mu, target_dB, n_fft, n_mels,
                    featName, save_feat=True):
    """preprocessing.py:355-457: same naming, same .npy cache layout <feature_opDir>/<class>/<name>.npy."""
    cache = feature_cache_path(feature_opDir, classname, fName_path_sp, fName_path_mu, target_dB)
    if os.path.exists(cache):
        return np.load(cache, allow_pickle=False)
    if featName not in _fe.FEATS and featName not in _fe.HALF_FEATS and featName not in _fe.PLAIN_FEATS:
        raise ValueError("featName %r is not one of get_featuregram's feature names %s"
                         % (featName, sorted(_fe.FEATS) + sorted(_fe.HALF_FEATS) + sorted(_fe.PLAIN_FEATS)))
    if classname == 'speech_music':
        Xin_sp, fs = load_and_preprocess_signal(fName_path_sp, PARAMS['Tw'], PARAMS['Ts'])
        Xin_mu, fs = load_and_preprocess_signal(fName_path_mu, PARAMS['Tw'], PARAMS['Ts'])
        Xin = mix_signals(Xin_sp, Xin_mu, target_dB)
    elif classname in ('speech', 'muspeak'):
        Xin, fs = load_and_preprocess_signal(fName_path_sp, PARAMS['Tw'], PARAMS['Ts'])
    elif classname == 'music':
        Xin, fs = load_and_preprocess_signal(fName_path_mu, PARAMS['Tw'], PARAMS['Ts'])
    else:
        raise ValueError("unknown classname %r" % classname)
    fv = featuregram_from_signal(PARAMS, Xin, n_fft, n_mels, featName, fs)
    if save_feat:
        os.makedirs(feature_opDir + '/' + classname + '/', exist_ok=True)
        np.save(cache, fv)
    return fv


# ---- patches ------------------------------------------------------------------------------------------------
def get_feature_patches(PARAMS, FV, patch_size, patch_shift, featName):
    """preprocessing.py:137-292.  FV (nFeatures, nFrames) -> float64 (nP, F, W) (Lemaire models) or
    (nP, F, W, 1).  Tiling-if-short, the H/P split, StandardScaler and the patch gather run on the GPU."""
    FV = np.asarray(FV)
    if FV.ndim != 2:
        raise ValueError("FV should be of the shape (nFeatures, nFrames)")
    fe = _frontend_for(_fe.FrontendConfig())
    d = torch.from_numpy(np.ascontiguousarray(FV, dtype=np.float32)).cuda()
    F, T = d.shape
    scale = not PARAMS['frame_level_scaling']

    def run(rows):  # rows: (r, T) device tensor -> (nP, r, W) device tensor
        x = fe.standardize_rows(rows) if scale else rows
        return fe.extract_patches(x[None], patch_size, patch_shift, time_major=False)

    if featName in ('Spec', 'LogSpec', 'MelSpec', 'LogMelSpec'):
        patches = run(d)
    else:
        known = ('MelHarm', 'MelPerc', 'LogMelHarm', 'LogMelPerc', 'Harm', 'Perc', 'LogHarm', 'LogPerc')
        if not featName.startswith(known):
            raise ValueError("unknown featName %r" % featName)
        half = int(F / 2)
        base = featName.replace('LogMel', '').replace('Mel', '').replace('Log', '')  # HarmSpec/PercSpec/HarmPercSpec
        parts = []
        if base in ('HarmSpec', 'HarmPercSpec'):
            parts.append(run(d[:half]))
        if base in ('PercSpec', 'HarmPercSpec'):
            parts.append(run(d[half:]))
        if not parts:
            raise ValueError("unknown featName %r" % featName)
        patches = torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]
    patches = patches.cpu().numpy().astype(np.float64)
    if 'Lemaire_et_al' not in PARAMS['Model']:
        patches = np.expand_dims(patches, axis=3)
    return patches


# ---- frame-level scaling: the statistics of a training fold ------------------------------------------------------
def stats_file_specs(PARAMS, files):
    """The files get_data_stats visits, in its order (preprocessing.py:476-503): the classes in PARAMS['classes'] order,
    'speech_music' read from files['speech+music'] -> [(classname, sp_path, mu_path, target_dB)], paths under PARAMS['folder'] as
    the generators build them (the listed name as it is; the reference rewrites a speech / music name's extension to .wav, the same
    file in its .wav corpora)."""
    folder = PARAMS['folder']
    specs = []
    for clNum in PARAMS['classes'].keys():
        class_name = PARAMS['classes'][clNum]
        for fl in (files['speech+music'] if class_name == 'speech_music' else files[class_name]):
            if class_name == 'speech_music':
                specs.append(('speech_music', folder + '/speech/' + fl['speech'], folder + '/music/' + fl['music'], fl['SMR']))
            elif class_name == 'music':
                specs.append(('music', '', folder + '/music/' + fl, None))
            elif class_name == 'speech':
                specs.append(('speech', folder + '/speech/' + fl, '', None))
            else:
                raise ValueError("get_data_stats: unknown class %r" % (class_name,))
    return specs


def device_row_moments(PARAMS, specs):
    """[(sum (rows,) float64, m2 (rows,) float64, nonfinite (rows,) int, T)] of the files `specs`: ONE ragged front-end pass for the
    files the reference's .npy cache does not hold (written to it and kept on the device as the generators do) and ONE
    `Frontend.row_moments` launch for all of them."""
    from .. import generators as _gen
    model = PARAMS['Model']
    fe, fvs, _ = _gen._device_featuregrams_for(PARAMS, specs, PARAMS['featName'][model], PARAMS['n_fft'][model], PARAMS['n_mels'][model])
    if not fvs:
        return []
    s, m2, bad = (t.cpu().numpy() for t in fe.row_moments(fvs))
    return [(s[i], m2[i], bad[i], int(fv.shape[1])) for i, fv in enumerate(fvs)]


def get_data_stats(PARAMS, files, moments_fn=None, batch_files=256):
    """preprocessing.py:461-586 -> (overall_mean float32, stdev float32, nMuFrames, nSpFrames, nSpMuFrames): per feature row, the
    unweighted average of the class means and the standard deviation around it (divisor nFrames - 1) over every file of `files`.

    The reference walks its featuregram cache twice (the class sums, then the squared deviations from the overall mean).  Here each
    file is read ONCE, on the device: its row sums and M2 = sum((x - m)^2) around its own row mean m (`moments_fn(specs)`, default
    `device_row_moments`, `batch_files` files per ragged batch), and the host combines them in np.longdouble in file order -- around
    the overall mean mu, sum((x - mu)^2) = M2 + T (m - mu)^2 holds exactly.  A file with a NaN or an inf raises ValueError and is
    named: the reference drops such feature ROWS, which changes the row count and cannot feed a model."""
    ld = np.longdouble
    specs = stats_file_specs(PARAMS, files)
    moments_fn = moments_fn or (lambda chunk: device_row_moments(PARAMS, chunk))
    per_file = []  # (classname, sum, m2, T)
    for b0 in range(0, len(specs), int(batch_files)):
        chunk = specs[b0:b0 + int(batch_files)]
        got = moments_fn(chunk)
        if len(got) != len(chunk):
            raise RuntimeError("get_data_stats: %d files gave %d sets of moments" % (len(chunk), len(got)))
        for spec, (s, m2, bad, T) in zip(chunk, got):
            s, m2 = np.asarray(s, dtype=np.float64), np.asarray(m2, dtype=np.float64)
            if np.any(np.asarray(bad) != 0) or not (np.all(np.isfinite(s)) and np.all(np.isfinite(m2))):
                raise ValueError("get_data_stats: the featuregram of %s holds NaN or inf values"
                                 % " + ".join(repr(x) for x in spec[1:3] if x))
            per_file.append((spec[0], s.astype(ld), m2.astype(ld), int(T)))
    if not per_file:
        raise ValueError("get_data_stats: no files")
    rows = per_file[0][1].size
    sums = {c: np.zeros(rows, dtype=ld) for c in ('music', 'speech', 'speech_music')}
    frames = {'music': 0, 'speech': 0, 'speech_music': 0}
    for c, s, _, T in per_file:
        if s.size != rows:
            raise ValueError("get_data_stats: featuregrams of %d and of %d rows" % (rows, s.size))
        sums[c] = sums[c] + s
        frames[c] += T
    means = {c: sums[c] / (ld(frames[c]) + ld(1e-10)) for c in sums}  # :530-532
    n_classes = len(PARAMS['classes'])
    if n_classes == 2:
        overall_mean = (means['music'] + means['speech']) / ld(2)
    elif n_classes == 3:
        overall_mean = ((means['music'] + means['speech']) + means['speech_music']) / ld(3)
    else:
        raise ValueError("get_data_stats: 2 or 3 classes, got %d" % n_classes)
    var, nFrames = np.zeros(rows, dtype=ld), 0
    for _, s, m2, T in per_file:
        d = s / ld(T) - overall_mean
        var = var + (m2 + ld(T) * d * d)
        nFrames += T
    stdev = np.sqrt(var / ld(nFrames - 1))
    return (overall_mean.astype(np.float32), stdev.astype(np.float32), frames['music'], frames['speech'], frames['speech_music'])


def scale_data(FV, mean, stdev):
    """preprocessing.py:590-614: (FV - mean[:, None]) / stdev[:, None] on the host -- stdev itself, no epsilon (the generators
    use tools.scale_data, which adds 1e-10)."""
    FV = np.asarray(FV)
    M = np.repeat(np.array(mean, ndmin=2).T, np.shape(FV)[1], axis=1)
    S = np.repeat(np.array(stdev, ndmin=2).T, np.shape(FV)[1], axis=1)
    return np.divide(np.subtract(FV, M), S)
