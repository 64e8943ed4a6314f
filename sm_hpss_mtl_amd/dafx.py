"""The broadcast-segmentation workflow of DAFx12_Speech_Music_Detection_B3_MTL_v2.py under the driver's own names: what feeds the
fine-tuning of a cut-out head (persistence.HeadModel) and what scores its probability track.

    get_annotations(folder, fl, nFrames, opDir)            :145-224   host: CSV annotations -> frame markers, cached as .npz
    load_data(PARAMS, folder, file_list)                   :300-341   stored spectrograms -> ONE resident standardised featuregram
    generator(PARAMS, FV, labels_mu, labels_sp, batchSize) :346-436   the balanced fine-tuning batches, one launch per batch
    patch_labels(marker, W, shift)                         :649-653   host: the majority label of every test patch
    getPerformance(PtdLabels, GroundTruths, labels=None)   misc.py:95-103
    evaluate_file(PARAMS, fl, Train_Params)                :596-706   patch_probability_generator without the pickle cache

The reference's generator materialises every patch of a "part" of the featuregram on the host and queues the patches; once a
class's cursor has reached the end of its frames every refill is the whole range [0, n) again, and the queues only grow.  Here
the featuregram stays on the device ((240, 5.4 M) f32 = 5.2 GB for the driver's training set), a queue is a list of refills kept
as arithmetic progressions -- O(1) host memory per refill -- and a batch is one smh_gather_windows_f32 launch (csrc/smh_gather.hip)
over the descriptors it pops: gather, transpose and noise augmentation in one pass.  The batch sequence is the reference loop's,
taken literally (see FeedPlanner)."""
from __future__ import annotations

import collections
import csv
import ctypes as C
import math
import os
import time

import numpy as np

from . import _lib
from .batching import NOISE_SCALES

SIGNAL_TYPES = ("music", "speech")


# ---- :145-224 ------------------------------------------------------------------------------------------------------------------
def _annotation_rows(path):
    """One annotation file -> ({1: row, 2: row, ...}, the largest tmin + dur): the non-empty rows behind the header, as the
    strings the csv module gives, numbered from 1 (the shape the reference caches)."""
    with open(path, newline="") as f:
        body = [row for row in csv.reader(f, quotechar="|") if row][1:]
    ends = [float(row[0]) + float(row[1]) for row in body]
    return dict(enumerate(body, 1)), max(ends, default=0)


def _marker(rows, audio_length, nFrames):
    """The 0 / 1 frame track of one annotation file: a segment of label 1 and non-zero duration marks the frames from
    floor(tmin / audio_length * nFrames), not below 0, up to but not including ceil(tmax / audio_length * nFrames), at most
    nFrames - 1 -- so the last frame of a file is never marked."""
    marker = np.zeros(nFrames)
    for row in rows.values():
        tmin, dur, label = float(row[0]), float(row[1]), int(row[2])
        if dur == 0 or label != 1:
            continue
        first = max(0, math.floor(tmin / audio_length * nFrames))
        last = min(math.ceil((tmin + dur) / audio_length * nFrames), nFrames - 1)
        marker[first:last] = 1
    return marker


def get_annotations(folder, fl, nFrames, opDir):
    """DAFx12...:145-224 (the OFAI dafx annotations): folder/labels/music/<fl>.csv and folder/labels/speech/<fl>.csv, rows of
    (tmin, dur, label) in seconds -> (annotations_mu, annotations_sp, music_marker, speech_marker), the markers float64 arrays of
    nFrames entries.  audio_length is the larger of the two files' largest tmin + dur.  Cached in opDir/__annotations/<fl up to
    its first dot>.npz under the reference's four keys; a cached file is returned as np.load gives it (the annotation dicts as
    0-d object arrays), like the reference."""
    cache = os.path.join(opDir, "__annotations", fl.split(".")[0] + ".npz")
    if os.path.exists(cache):
        with np.load(cache, allow_pickle=True) as z:
            return z["annotations_mu"], z["annotations_sp"], z["music_marker"], z["speech_marker"]
    (mu, end_mu), (sp, end_sp) = (_annotation_rows(os.path.join(folder, "labels", kind, fl + ".csv")) for kind in ("music", "speech"))
    audio_length = max(end_mu, end_sp)
    music_marker, speech_marker = _marker(mu, audio_length, nFrames), _marker(sp, audio_length, nFrames)
    os.makedirs(os.path.dirname(cache), exist_ok=True)
    np.savez(cache, annotations_mu=mu, annotations_sp=sp, music_marker=music_marker, speech_marker=speech_marker)
    return mu, sp, music_marker, speech_marker


# ---- :230-255, :300-341 --------------------------------------------------------------------------------------------------------
def _frontend_for(PARAMS):
    """The context of the driver's featuregram: n_fft / n_mels / l_harm / l_perc of PARAMS['Model'], mel basis at librosa's default
    sr = 22050 (melspectrogram(S=...) is called without sr, :233, :239)."""
    from . import frontend as _fe
    from .lib.preprocessing import _frontend_for as cached
    model = PARAMS["Model"]
    n_fft = int(PARAMS["n_fft"][model])
    return cached(_fe.FrontendConfig(
        n_fft=n_fft, win_length=min(n_fft, int(PARAMS.get("Tw", 25) * 16)), hop=int(PARAMS.get("Ts", 10) * 16),
        n_mels=int(PARAMS["n_mels"][model]), l_harm=int(PARAMS.get("l_harm", {}).get(model, 21)),
        l_perc=int(PARAMS.get("l_perc", {}).get(model, 11))))


def _featuregram(PARAMS, fName, Spec):
    """get_featuregram (:230-255) of one stored magnitude spectrogram, on the device: (F, T) float32 CUDA tensor, not yet
    standardised.  LogMelHarmPercSpec: hpss_median -> features (soft masks, mel, power_to_db of the square).  LogMelSpec: the
    driver's own arithmetic, power_to_db(melspectrogram(S=Spec) ** 2) with the sr = 22050 basis (:233-234) -- mel and
    power_to_db_sq stage by stage; Frontend.plain_features is lib/preprocessing.py's LogMelSpec (mel of the POWER spectrogram at
    sr = fs), other numbers.  Cached in PARAMS['feature_opDir'] as the reference caches it."""
    import torch
    featName = PARAMS["featName"][PARAMS["Model"]]
    path = PARAMS["feature_opDir"] + "/" + fName + ".npy"
    if os.path.exists(path):
        return torch.from_numpy(np.ascontiguousarray(np.load(path, allow_pickle=True), dtype=np.float32)).cuda()
    fe = _frontend_for(PARAMS)
    S = torch.from_numpy(np.ascontiguousarray(Spec, dtype=np.float32)).cuda()[None]
    if S.dim() != 3 or S.shape[1] != fe.K:
        raise ValueError("%s: a (%d, T) magnitude spectrogram is expected for n_fft = %d, got %s"
                         % (fName, fe.K, fe.cfg.n_fft, tuple(S.shape[1:])))
    if featName == "LogMelSpec":
        fv = fe.power_to_db_sq(fe.mel(S))[0]
    elif featName == "LogMelHarmPercSpec":
        harm, perc = fe.hpss_median(S)
        fv = fe.features(S, harm, perc)["fv"][0]
    else:
        raise ValueError("featName %r: the segmentation driver computes LogMelSpec and LogMelHarmPercSpec featuregrams" % (featName,))
    os.makedirs(PARAMS["feature_opDir"], exist_ok=True)
    np.save(path, fv.cpu().numpy())
    return fv


def _standardised(PARAMS, fv):
    """:317-331 / :613-627: StandardScaler over the frames of the whole file, row by row -- so H and P are one call."""
    return _frontend_for(PARAMS).standardize_rows(fv)


def _npy_frames(path):
    """Frames of a stored (K, T) array from the .npy header alone (nothing of the data is read)."""
    with open(path, "rb") as f:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        return int(read(f)[0][1])


def load_data(PARAMS, folder, file_list):
    """DAFx12...:300-341 -> (FV, labels_mu, labels_sp).  FV is ONE resident float32 CUDA tensor (F, sum of T): every file's
    standardised featuregram is written into its column range on the device (no host round trip, no per-file list); the frame
    counts that size it come from the .npy headers, so every spectrogram is read once.  The labels are int32 numpy arrays of
    sum-of-T entries.  Files without folder/features/<f>.npy are skipped; annotations come from PARAMS['test_path'] and
    PARAMS['opDir'] as in the reference."""
    import torch
    paths = {f: os.path.join(folder, "features", f + ".npy") for f in file_list}
    present = [f for f in file_list if os.path.exists(paths[f])]
    if not present:
        raise ValueError("load_data: none of the %d files has a spectrogram under %s/features/" % (len(file_list), folder))
    total = sum(_npy_frames(paths[f]) for f in present)
    FV, col, mu, sp = None, 0, [], []
    for fName in present:
        fv = _featuregram(PARAMS, fName, np.load(paths[fName], allow_pickle=True))
        nFrames = int(fv.shape[1])
        if col + nFrames > total:
            raise ValueError("%s: its featuregram (cached in %s?) has more frames than its spectrogram" % (fName, PARAMS["feature_opDir"]))
        _, _, music_marker, speech_marker = get_annotations(PARAMS["test_path"], fName, nFrames, PARAMS["opDir"])
        if FV is None:
            FV = torch.empty((fv.shape[0], total), dtype=torch.float32, device=fv.device)
        FV[:, col:col + nFrames].copy_(_standardised(PARAMS, fv))
        col += nFrames
        mu.append(music_marker.astype(np.int32))
        sp.append(speech_marker.astype(np.int32))
    if col != total:
        raise ValueError("load_data: the featuregrams hold %d frames, the spectrograms %d (a stale cache in %s?)"
                         % (col, total, PARAMS["feature_opDir"]))
    return FV, np.concatenate(mu), np.concatenate(sp)


# ---- :346-436 ------------------------------------------------------------------------------------------------------------------
class _Refill:
    """The patches of one part: patch k is the window of W frames at smh_patch_start(tiled, W, hop, k) of the part
    [base, base + period) repeated to `tiled` frames (the tile-if-short rule).  Fixed size, however many patches.
    linear: the last patch starts at (count - 1) * hop.  The contract moves a start back only where the window would run past the
    end, and the windows' ends grow with k, so then every start is k * hop and a run of them is one arange."""
    __slots__ = ("base", "period", "tiled", "hop", "count", "consumed", "linear")

    def __init__(self, base, period, tiled, hop, count, linear):
        self.base, self.period, self.tiled, self.hop, self.count, self.consumed, self.linear = base, period, tiled, hop, count, 0, linear


class _ClassQueue:
    """One class of the reference loop: the part cursor (part_i, part_j), the length n of the class and its queue."""

    def __init__(self, name, n, hop):
        self.name, self.n, self.hop = name, int(n), int(hop)
        self.part_i = self.part_j = 0
        self.balance = 0
        self.queue = collections.deque()
        self.refills = self.retired = 0


class FeedPlanner:
    """The host half of `generator`: the reference loop (:346-420) on integers.  Its behaviours, kept as they are:
      - windows are cut from FV itself; the class's frames (FV_neg / FV_pos) only give the LENGTH n that bounds the parts (:377, :385);
      - part_j is not recomputed when part_i is reset to 0 (:375-376), so once the cursor has reached n every refill is [0, n);
      - every refill appends to BOTH classes, also the one that is already full: the faster queue grows without bound;
      - the np.random.randint branch (:372-373) cannot be reached, part_j <= n always; it is restated and consumes nothing;
      - music: negatives hop int(W_shift / 3), positives W_shift; speech: the reverse (:387-392);
      - a class is skipped while np.size(idx) <= W (:395, :398).
    One difference: a class that can never fill (no frames, or size(idx) <= W) makes the reference loop forever; `next_batch`
    raises ValueError instead, naming the class and its frame count.
    A queue is a deque of _Refill progressions: O(1) host memory per refill.  `next_batch` returns the (2 * batchSize, 3) int32
    table (base, period, first) of smh_gather_windows_f32, negatives first."""

    def __init__(self, labels, W, W_shift, batchSize, signal_type, n_feat=2):
        if signal_type not in SIGNAL_TYPES:
            raise ValueError("PARAMS['signal_type'] must be one of %s, got %r" % (SIGNAL_TYPES, signal_type))
        self.lib = _lib.load()
        self.W, self.W_shift, self.batchSize = int(W), int(W_shift), int(batchSize)
        if self.W < 1 or self.W_shift < 1 or self.batchSize < 1:
            raise ValueError("W, W_shift and batchSize must be positive, got %d, %d, %d" % (self.W, self.W_shift, self.batchSize))
        self.part_size = self.W_shift * self.batchSize * 2
        labels = np.asarray(labels)
        self.n_frames = int(labels.size)
        third = int(self.W_shift / 3)
        hops = (third, self.W_shift) if signal_type == "music" else (self.W_shift, third)
        self.classes = (_ClassQueue("negative (label 0)", np.count_nonzero(labels == 0), hops[0]),
                        _ClassQueue("positive (label 1)", np.count_nonzero(labels == 1), hops[1]))
        self.patch_floats = self.W * int(n_feat)  # for np.size(patches) > 1 of :400, :406

    def _refill(self, c):
        c.part_i = c.part_j
        if c.part_i > c.n:  # (:372-373: unreachable)
            c.part_i = np.random.randint(c.n)
        c.part_j = min(c.part_i + self.part_size, c.n)
        if (c.part_j - c.part_i) < self.part_size:
            c.part_i = 0
        if not c.n > self.W:
            return
        period = c.part_j - c.part_i
        tiled = self.lib.smh_tiled_frames(period, self.W)
        count = _lib.check(self.lib.smh_num_patches(tiled, self.W, c.hop), "smh_num_patches")
        if count * self.patch_floats > 1:
            linear = self.lib.smh_patch_start(tiled, self.W, c.hop, count - 1) == (count - 1) * c.hop
            c.queue.append(_Refill(c.part_i, period, tiled, c.hop, count, linear))
            c.refills += 1
            c.balance += count

    def _pop(self, c, table, row):
        need = self.batchSize
        while need:
            r = c.queue[0]
            take = min(need, r.count - r.consumed)
            rows = table[row:row + take]
            rows[:] = (r.base, r.period, 0)
            if r.linear:
                rows[:, 2] = np.arange(r.consumed * r.hop, (r.consumed + take) * r.hop, r.hop)
            else:
                rows[:, 2] = [self.lib.smh_patch_start(r.tiled, self.W, r.hop, k) for k in range(r.consumed, r.consumed + take)]
            r.consumed += take
            row += take
            need -= take
            if r.consumed == r.count:
                c.queue.popleft()
                c.retired += 1
        c.balance -= self.batchSize

    def next_batch(self):
        neg, pos = self.classes
        for c in self.classes:
            if not c.n > self.W or c.hop < 1:
                raise ValueError("generator: the %s class has %d frames of %d and a hop of %d: with np.size(idx) <= W = %d (or a "
                                 "hop of 0) it never yields a patch and the reference loops forever"
                                 % (c.name, c.n, self.n_frames, c.hop, self.W))
        while neg.balance < self.batchSize or pos.balance < self.batchSize:
            self._refill(neg)
            self._refill(pos)
        table = np.empty((2 * self.batchSize, 3), np.int32)
        self._pop(self.classes[0], table, 0)
        self._pop(self.classes[1], table, self.batchSize)
        return table


def gather_windows(FV, table, W, layout="time_major", noise_scale=0.0, seed=0, offset=0, out=None, ctx=None):
    """smh_gather_windows_f32 on a resident featuregram: FV (F, T) float32 CUDA tensor, table (N, 3) int32 host array of
    (base, period, first) -> (N, W, F) time-major or (N, F, W) image patches, plus N(0, noise_scale) from the (seed, offset) Philox
    stream (device_rng.add_normal_noise's draws over the finished batch).  One launch."""
    import torch
    from . import frontend as _fe
    if not (isinstance(FV, torch.Tensor) and FV.is_cuda and FV.dtype == torch.float32 and FV.dim() == 2 and FV.is_contiguous()):
        raise TypeError("gather_windows: FV must be a contiguous (F, T) float32 CUDA tensor")
    table = np.ascontiguousarray(table, dtype=np.int32)
    if table.ndim != 2 or table.shape[1] != 3:
        raise ValueError("gather_windows: the table must be (N, 3) int32 rows of (base, period, first), got %s" % (table.shape,))
    F, T = FV.shape
    N = table.shape[0]
    lay = _fe._layout(layout)
    shape = _fe._patch_shape(N, int(W), F, layout)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=FV.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError("gather_windows: out must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
    if N == 0:  # nothing to launch (an empty tensor has no address to hand to the entry)
        return out
    if ctx is None:
        from .inference import _frontend
        ctx = _frontend()
    _lib.check(ctx.lib.smh_gather_windows_f32(ctx._h, _fe._ptr(FV), F, T, table.ctypes.data_as(C.POINTER(C.c_int)), N, int(W), lay,
                                              float(noise_scale), int(seed), int(offset), _fe._ptr(out), _lib.current_stream()),
               "smh_gather_windows_f32")
    return out


def generator(PARAMS, FV, labels_mu, labels_sp, batchSize):
    """DAFx12...:346-436 on a resident featuregram: yields (batchData, batchLabel) for ever -- batchData a float32 CUDA tensor,
    (2 * batchSize, W, F) for the Lemaire models (the transposed TCN input of :422-424) and (2 * batchSize, F, W, 1) otherwise,
    batchSize negatives then batchSize positives of PARAMS['signal_type']; batchLabel [0] * batchSize + [1] * batchSize.  The same
    patches in the same order as the reference loop (FeedPlanner); each batch is one smh_gather_windows_f32 launch.  With
    PARAMS['data_augmentation_with_noise'] the scale is np.random.choice of the reference's four (the same numpy draw) and the
    noise itself comes from the device generator, seeded by device_rng.fresh_seed()."""
    from .device_rng import fresh_seed
    if PARAMS["signal_type"] not in SIGNAL_TYPES:
        raise ValueError("PARAMS['signal_type'] must be one of %s, got %r" % (SIGNAL_TYPES, PARAMS["signal_type"]))
    labels = labels_mu if PARAMS["signal_type"] == "music" else labels_sp
    if int(np.size(labels)) != int(FV.shape[1]):
        raise ValueError("generator: %d labels for a featuregram of %d frames" % (np.size(labels), FV.shape[1]))
    W = int(PARAMS["W"])
    planner = FeedPlanner(labels, W, PARAMS["W_shift"], batchSize, PARAMS["signal_type"], n_feat=int(FV.shape[0]))
    lemaire = "Lemaire_et_al" in PARAMS["Model"]
    batchLabel = np.array([0] * batchSize + [1] * batchSize)
    while 1:
        table = planner.next_batch()
        scale, seed = 0.0, 0
        if PARAMS["data_augmentation_with_noise"]:
            scale, seed = float(np.random.choice(NOISE_SCALES)), fresh_seed()
        batchData = gather_windows(FV, table, W, "time_major" if lemaire else "image", scale, seed, 0)
        if not lemaire:
            batchData = batchData[:, :, :, None]  # np.expand_dims(patches, axis=3) of :270
        yield batchData, batchLabel.copy()


# ---- :649-653 ------------------------------------------------------------------------------------------------------------------
def patch_labels(marker, W, shift):
    """DAFx12...:649-653: tools.extract_patches on the marker track (NOT tiled, as in the reference) and the majority of every
    patch -- label[p] = 1 where 2 * sum(marker[start_p : start_p + W]) > W.  Host integer code; int array of smh_num_patches
    entries."""
    lib = _lib.load()
    m = np.asarray(marker).astype(np.int64).reshape(-1)
    T, W, shift = int(m.size), int(W), int(shift)
    nP = _lib.check(lib.smh_num_patches(T, W, shift), "smh_num_patches")
    if nP == 0:
        return np.zeros(0, int)
    starts = np.fromiter((lib.smh_patch_start(T, W, shift, p) for p in range(nP)), np.int64, nP)
    cs = np.concatenate([[0], np.cumsum(m)])
    return (2 * (cs[starts + W] - cs[starts]) > W).astype(int)


# ---- misc.py:95-103 ------------------------------------------------------------------------------------------------------------
def getPerformance(PtdLabels, GroundTruths, labels=None):
    """lib/misc.py:95-103, the form the driver's summaries use (:679, :713) -> (ConfMat, precision, recall, fscore).  ConfMat is
    sklearn's confusion_matrix(y_true, y_pred) WITHOUT labels -- rows and columns are the sorted labels that occur in either --
    and precision / recall / fscore are precision_recall_fscore_support(beta=1, average=None, labels=labels) rounded to 4
    decimals, 0 where a denominator is 0 (sklearn's zero_division result; it warns, this does not).  labels=None: the labels that
    occur."""
    y_true = np.asarray(GroundTruths).reshape(-1)
    y_pred = np.asarray(PtdLabels).reshape(-1)
    if y_true.size != y_pred.size:
        raise ValueError("getPerformance: %d predictions for %d ground truths" % (y_pred.size, y_true.size))
    present = np.unique(np.concatenate([y_true, y_pred]))
    ConfMat = np.zeros((present.size, present.size), np.int64)
    np.add.at(ConfMat, (np.searchsorted(present, y_true), np.searchsorted(present, y_pred)), 1)
    labels = present if labels is None else np.asarray(labels)
    tp = np.array([np.count_nonzero((y_true == l) & (y_pred == l)) for l in labels], np.float64)
    n_pred = np.array([np.count_nonzero(y_pred == l) for l in labels], np.float64)
    n_true = np.array([np.count_nonzero(y_true == l) for l in labels], np.float64)

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros_like(a), where=b != 0)
    precision, recall = ratio(tp, n_pred), ratio(tp, n_true)
    fscore = ratio(2 * precision * recall, precision + recall)
    return ConfMat, np.round(precision, 4), np.round(recall, 4), np.round(fscore, 4)


# ---- :596-706 ------------------------------------------------------------------------------------------------------------------
def evaluate_file(PARAMS, fl, Train_Params):
    """patch_probability_generator (:596-706) without the pickle cache: featuregram and markers of PARAMS['test_path']/features/
    <fl>.npy, the dense pass of inference.patch_probabilities in 10 000-frame batches, the patch labels per batch (so the
    per-batch patch counts are the reference's), pred_lab = pred > 0.5 and the 2-class scores of PARAMS['signal_type'].  Returns
    the reference's result dict ({} for a missing file).  A last batch shorter than W gives the reference different counts of
    predictions (from the tiled batch) and labels (not tiled), and its getPerformance raises; here that is a ValueError naming
    the file, the batch and both counts."""
    from . import inference
    t0 = time.process_time()
    spec_path = os.path.join(PARAMS["test_path"], "features", fl + ".npy")
    if not os.path.exists(spec_path):
        return {}
    if PARAMS["signal_type"] not in SIGNAL_TYPES:
        raise ValueError("PARAMS['signal_type'] must be one of %s, got %r" % (SIGNAL_TYPES, PARAMS["signal_type"]))
    fv = _featuregram(PARAMS, fl, np.load(spec_path, allow_pickle=True))
    nFrames = int(fv.shape[1])
    _, _, music_marker, speech_marker = get_annotations(PARAMS["test_path"], fl, nFrames, PARAMS["opDir"])
    W, shift, chunk = int(PARAMS["W"]), int(PARAMS["W_shift_test"]), 10000
    fe = _frontend_for(PARAMS)
    labels_mu, labels_sp = [], []
    for lo in range(0, nFrames, chunk):
        hi = min(lo + chunk, nFrames)
        mu = patch_labels(music_marker[lo:hi], W, shift)
        n_pred = fe.num_patches(hi - lo, W, shift)  # get_feature_patches tiles a short batch, the markers are not
        if n_pred != len(mu):
            raise ValueError("evaluate_file: %s, batch (%d, %d): %d frames are fewer than W = %d, so the tiled batch gives %d "
                             "predictions and the markers %d labels" % (fl, lo, hi, hi - lo, W, n_pred, len(mu)))
        labels_mu.extend(mu)
        labels_sp.extend(patch_labels(speech_marker[lo:hi], W, shift))
    # patch_probabilities standardises the whole file (:613-627) and then every batch (:647) itself
    pred = inference.patch_probabilities(fv, Train_Params["model"], W, shift, batch_frames=chunk, dtype=PARAMS.get("model_dtype", "f32"))
    pred_lab = (pred > 0.5).astype(int)
    ConfMat, precision, recall, fscore = getPerformance(pred_lab, labels_mu if PARAMS["signal_type"] == "music" else labels_sp,
                                                        labels=[0, 1])
    return {"pred": pred, "pred_lab": pred_lab, "labels_sp": labels_sp, "labels_mu": labels_mu, "ConfMat": ConfMat,
            "precision": precision, "recall": recall, "fscore": fscore,
            "accuracy": np.round(np.trace(ConfMat) / np.sum(ConfMat), 4), "probability_genTime": time.process_time() - t0}
