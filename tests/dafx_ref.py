"""Numpy restatements of the segmentation driver's host logic, for the tests of sm_hpss_mtl_amd.dafx -- written from the line
numbers of DAFx12_Speech_Music_Detection_B3_MTL_v2.py they name, with MATERIALISED patches and host arrays only (the shape of
the reference's own code; the package keeps descriptors and a resident featuregram instead).

    extract_patches        lib/cython_impl/tools.pyx:24-34
    feature_patches        :260-294 (tile-if-short, then patches of the whole array: splitting H / P and re-joining is the identity)
    get_annotations        :145-224
    generator              :346-436 (noise off)
    patch_labels           :649-653
    numpy_gather           what smh_gather_windows_f32 computes, noise off"""
import csv
import os

import numpy as np


def extract_patches(FV, W, shift):
    """(F, T) -> (nP, F, W): one patch per centre W//2, W//2 + shift, ... below T - W//2; a patch that would run past the end is
    moved back to end there."""
    F, T = FV.shape
    half = int(W / 2)
    out = []
    for centre in range(half, T - half, shift):
        start = centre - half
        stop = min(start + W, T)
        if stop - start < W:
            start = stop - W
        out.append(FV[:, start:stop])
    if not out:
        return np.empty((0, F, W), FV.dtype)
    return np.stack(out)


def feature_patches(FV, W, shift, lemaire):
    """:260-294 without the model transpose: an array shorter than W is appended to itself until it is longer than W."""
    if FV.shape[1] < W:
        one = FV.copy()
        while FV.shape[1] <= W:
            FV = np.append(FV, one, axis=1)
    patches = extract_patches(FV, W, shift)
    if not lemaire:
        patches = np.expand_dims(patches, axis=3)
    return patches.astype(np.float32)


def _rows_of(path):
    rows, longest, count = {}, 0, 0
    with open(path, newline="\n") as fid:
        for row in csv.reader(fid, delimiter=",", quotechar="|"):
            if row == []:
                continue
            if count == 0:  # the header
                count = 1
                continue
            rows[count] = row
            count += 1
            longest = max(longest, float(row[0]) + float(row[1]))
    return rows, longest


def get_annotations(folder, fl, nFrames):
    """:145-216 without the cache -> (annotations_mu, annotations_sp, music_marker, speech_marker)."""
    mu, long_mu = _rows_of(os.path.join(folder, "labels", "music", fl + ".csv"))
    sp, long_sp = _rows_of(os.path.join(folder, "labels", "speech", fl + ".csv"))
    audio_length = np.max([long_mu, long_sp])
    markers = []
    for rows in (mu, sp):
        marker = np.zeros(nFrames)
        for k in rows:
            tmin, dur, label = float(rows[k][0]), float(rows[k][1]), int(rows[k][2])
            if dur == 0.0:
                continue
            a = np.max([0, int(np.floor((tmin / audio_length) * nFrames))])
            b = np.min([int(np.ceil(((tmin + dur) / audio_length) * nFrames)), nFrames - 1])
            if label == 1:
                marker[a:b] = 1
        markers.append(marker)
    return mu, sp, markers[0], markers[1]


def generator(FV, labels, W, W_shift, batchSize, signal_type, lemaire=True, log=None):
    """:346-436 with noise off, taken literally: two growing arrays of materialised patches.  FV (F, T) numpy; labels the track
    of the chosen signal type.  log: a list that receives (patches added to neg, patches added to pos) per refill."""
    neg_idx = np.squeeze(np.where(labels == 0))
    pos_idx = np.squeeze(np.where(labels == 1))
    n_neg, n_pos = np.shape(FV[:, neg_idx])[1], np.shape(FV[:, pos_idx])[1]
    part_size = W_shift * batchSize * 2
    if signal_type == "music":
        hop_neg, hop_pos = int(W_shift / 3), W_shift
    else:
        hop_neg, hop_pos = W_shift, int(W_shift / 3)
    i_neg = j_neg = i_pos = j_pos = 0
    q_neg = q_pos = None
    balance = [0, 0]
    while True:
        while np.min(balance) < batchSize:
            i_neg = j_neg
            if i_neg > n_neg:
                i_neg = np.random.randint(n_neg)
            j_neg = np.min([i_neg + part_size, n_neg])
            if (j_neg - i_neg) < part_size:
                i_neg = 0
            part_neg = FV[:, i_neg:j_neg]

            i_pos = j_pos
            if i_pos > n_pos:
                i_pos = np.random.randint(n_pos)
            j_pos = np.min([i_pos + part_size, n_pos])
            if (j_pos - i_pos) < part_size:
                i_pos = 0
            part_pos = FV[:, i_pos:j_pos]

            new_neg = feature_patches(part_neg, W, hop_neg, lemaire) if np.size(neg_idx) > W else np.empty([])
            new_pos = feature_patches(part_pos, W, hop_pos, lemaire) if np.size(pos_idx) > W else np.empty([])
            if np.size(new_neg) > 1:
                q_neg = new_neg if q_neg is None or np.size(q_neg) <= 1 else np.append(q_neg, new_neg, axis=0)
                balance[0] += new_neg.shape[0]
            if np.size(new_pos) > 1:
                q_pos = new_pos if q_pos is None or np.size(q_pos) <= 1 else np.append(q_pos, new_pos, axis=0)
                balance[1] += new_pos.shape[0]
            if log is not None:
                log.append((new_neg.shape[0] if np.size(new_neg) > 1 else 0, new_pos.shape[0] if np.size(new_pos) > 1 else 0))
        data = np.append(q_neg[:batchSize], q_pos[:batchSize], axis=0)
        label = np.array([0] * batchSize + [1] * batchSize)
        q_neg, q_pos = q_neg[batchSize:], q_pos[batchSize:]
        balance = (np.array(balance) - batchSize).tolist()
        if lemaire:
            data = np.transpose(data, axes=(0, 2, 1))
        yield data, label, (q_neg.shape[0], q_pos.shape[0])


def patch_labels(marker, W, shift):
    """:649-653: patches of the marker track as a one-row array (NOT tiled), mean over the patch > 0.5."""
    row = np.array(marker, ndmin=2)
    p = extract_patches(row, W, shift).astype(int)
    if p.shape[0] == 0:
        return np.zeros(0, int)
    return ((np.sum(np.squeeze(p, axis=1), axis=1) / p.shape[2]) > 0.5).astype(int)


def numpy_gather(FV, table, W, layout):
    """out[n][f][t] = FV[f][base + (first + t) % period]; layout 'time_major' transposes every patch."""
    t = np.arange(W)
    out = np.stack([FV[:, int(b) + (int(f) + t) % int(p)] for b, p, f in table]) if len(table) else np.empty((0, FV.shape[0], W), FV.dtype)
    return np.ascontiguousarray(out.transpose(0, 2, 1)) if layout == "time_major" else np.ascontiguousarray(out)
