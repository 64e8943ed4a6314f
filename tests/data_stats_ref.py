"""numpy restatements of frame-level scaling (no GPU, no libsmh): what lib.preprocessing.get_data_stats and the scaled patch feed
compute, written from the arithmetic alone.

  class_files: {'music': [...], 'speech': [...], 'speech_music': [...]} -- lists of (F, T_i) float32 featuregrams; `classes` is the
  tuple of class names in PARAMS['classes'] order (2 or 3 of them).

  two_pass_stats       the literal form of lib/preprocessing.py:461-586 in np.longdouble: class sums / (N_c + 1e-10), the unweighted
                       average of the class means, then sum((x - mu)^2) over every frame / (nFrames - 1), sqrt
  file_moments         what the device kernel hands the host per file: float64 sum(x) and M2 = sum((x - sum(x) / T)^2)
  one_pass_stats       the same statistics from those moments: sum((x - mu)^2) = M2 + T (m - mu)^2
  float32_class_means  the reference's arithmetic as it really runs: its float128 accumulators are replaced by the first np.sum of a
                       float32 array, so the class sums are float32
  scaled               tools.pyx:157-164 rounded once to float32
  patch_grid           extract_patches on the tiled-if-short featuregram, through the integer contracts given as plain functions
"""
import numpy as np

LD = np.longdouble
ORDER = ("music", "speech", "speech_music")  # the order the reference adds the class means in (:534-536)


def _overall(means, n_classes):
    if n_classes == 2:
        return (means["music"] + means["speech"]) / LD(2)
    return ((means["music"] + means["speech"]) + means["speech_music"]) / LD(3)


def _class_means(sums, frames, rows):
    return {c: sums.get(c, np.zeros(rows, LD)) / (LD(frames.get(c, 0)) + LD(1e-10)) for c in ORDER}


def two_pass_stats(class_files, classes):
    rows = next(iter(class_files[classes[0]])).shape[0]
    sums, frames = {}, {}
    for c in classes:
        sums[c], frames[c] = np.zeros(rows, LD), 0
        for fv in class_files[c]:
            sums[c] = sums[c] + np.sum(fv.astype(LD), axis=1)
            frames[c] += fv.shape[1]
    means = _class_means(sums, frames, rows)
    mu = _overall(means, len(classes))
    acc, n = np.zeros(rows, LD), 0
    for c in classes:
        for fv in class_files[c]:
            acc = acc + np.sum((fv.astype(LD) - mu[:, None]) ** 2, axis=1)
            n += fv.shape[1]
    return {"mean": mu, "stdev": np.sqrt(acc / LD(n - 1)), "class_means": means, "frames": frames}


def file_moments(fv):
    """(sum, M2, nonfinite, T) of one (F, T) float32 featuregram in float64."""
    x = np.asarray(fv, dtype=np.float32).astype(np.float64)
    s = x.sum(axis=1)
    m = s / x.shape[1]
    return s, ((x - m[:, None]) ** 2).sum(axis=1), (~np.isfinite(x)).sum(axis=1).astype(np.int32), x.shape[1]


def one_pass_stats(class_files, classes, moments=file_moments):
    rows = next(iter(class_files[classes[0]])).shape[0]
    per_file, sums, frames = [], {}, {}
    for c in classes:
        sums[c], frames[c] = np.zeros(rows, LD), 0
        for fv in class_files[c]:
            s, m2, _, T = moments(fv)
            per_file.append((s.astype(LD), m2.astype(LD), T))
            sums[c] = sums[c] + s.astype(LD)
            frames[c] += T
    means = _class_means(sums, frames, rows)
    mu = _overall(means, len(classes))
    acc, n = np.zeros(rows, LD), 0
    for s, m2, T in per_file:
        acc = acc + (m2 + LD(T) * (s / LD(T) - mu) ** 2)
        n += T
    return {"mean": mu, "stdev": np.sqrt(acc / LD(n - 1)), "class_means": means, "frames": frames}


def float32_class_means(class_files, classes):
    """The class means of preprocessing.py:483-532 with the dtypes numpy really gives them: np.sum of the float32 (T, F) array."""
    out = {}
    for c in classes:
        acc, n = None, 0
        for fv in class_files[c]:
            FV = np.asarray(fv, dtype=np.float32).T
            n += FV.shape[0]
            acc = np.sum(FV, axis=0) if acc is None else np.add(acc, np.sum(FV, axis=0))
        assert acc.dtype == np.float32
        acc /= n + 1e-10
        out[c] = acc
    return out


def scaled(fv, mean, stdev):
    mean, stdev = np.asarray(mean, np.float64), np.asarray(stdev, np.float64)
    return ((np.asarray(fv, np.float32).astype(np.float64) - mean[:, None]) / (stdev[:, None] + 1e-10)).astype(np.float32)


def patch_grid(x, W, shift, tiled_frames, num_patches, patch_start, time_major):
    """Patches of the (F, T) array x: tile-if-short, then patch p = frames start(p) .. start(p) + W - 1."""
    F, T = x.shape
    Tt = tiled_frames(T, W)
    xt = np.concatenate([x] * (Tt // T), axis=1)
    nP = num_patches(Tt, W, shift)
    out = np.stack([xt[:, patch_start(Tt, W, shift, p):patch_start(Tt, W, shift, p) + W] for p in range(nP)]) if nP else np.zeros((0, F, W), x.dtype)
    return np.ascontiguousarray(out.transpose(0, 2, 1)) if time_major else out


# ---- the end-to-end tests' corpus and configurations ---------------------------------------------------------------------------------
# Model -> (featName, n_fft, n_mels, featuregram rows, layout of the device batches)
MODELS = {"Lemaire_et_al_MTL": ("LogMelHarmPercSpec", 400, 120, 240, "time_major"),
          "Lemaire_et_al": ("LogMelSpec", 400, 21, 21, "time_major"),
          "Doukhan_et_al": ("MelSpec", 400, 21, 21, "image")}


def params(tmp, sub, model, classes=3, W=68, shift=34):
    feat, n_fft, n_mels, _, _ = MODELS[model]
    cl = {0: "music", 1: "speech", 2: "speech_music"} if classes == 3 else {0: "music", 1: "speech"}
    return {"Model": model, "classes": cl, "folder": str(tmp / "data"), "feature_opDir": str(tmp / sub), "W": W, "W_shift": shift,
            "n_fft": {model: n_fft}, "n_mels": {model: n_mels}, "featName": {model: feat}, "frame_level_scaling": False,
            "skewness_vector": None, "data_augmentation_with_noise": False, "Tw": 25, "Ts": 10, "l_harm": {model: 21}, "l_perc": {model: 11}}


def dataset(tmp):
    """Three short synthesised files per class (.npy audio at 16 kHz; 0.4 s is shorter than a patch of 68 frames: tiled) and four
    mixtures of them."""
    import os
    from sm_hpss_mtl_amd.synth import synth_clips
    folder = tmp / "data"
    names = {"speech": [], "music": []}
    lens = {"speech": (6400, 14000, 30000), "music": (9000, 20000, 12000)}
    for cls in names:
        os.makedirs(folder / cls, exist_ok=True)
        for i, n in enumerate(lens[cls]):
            name = "%s%02d.npy" % (cls[:2], i)
            np.save(folder / cls / name, synth_clips(1, seed=40 + 7 * i + (0 if cls == "speech" else 100), n_samples=n)[0])
            names[cls].append(name)
    mix = [{"speech": names["speech"][i % 3], "music": names["music"][(i + 1) % 3], "SMR": [-5, 0, 10, 20][i % 4]} for i in range(4)]
    return str(folder), {"speech": names["speech"], "music": names["music"], "speech+music": mix}
