"""CPU: the host half of sm_hpss_mtl_amd.dafx against the literal restatements of tests/dafx_ref.py -- the generator's descriptor
planner (its descriptors through a numpy gather, batch by batch, bit for bit), its refusals, get_annotations, patch_labels and
getPerformance (against sklearn).  The integer contracts come from libsmh.so, which loads without a GPU."""
import os

import numpy as np
import pytest

from tests import dafx_ref

from sm_hpss_mtl_amd import _lib, dafx

if not os.path.exists(_lib.LIB_PATH):
    pytest.skip("libsmh.so not built (run __graft_entry__.build())", allow_module_level=True)


def _labels(n=5000, seed=3):
    """n frames in runs of 50..400, about 40 % positives: 2 994 negatives and 2 006 positives at the defaults."""
    rng = np.random.RandomState(seed)
    lab = np.zeros(n, np.int32)
    t, v = 0, 0
    while t < n:
        run = int(rng.randint(50, 400))
        lab[t:t + run] = v
        t += run
        v = 1 - v if rng.rand() < 0.9 else v
    # trim to exactly 2 006 positives, so that the counts the cases below are worked out for hold whatever the runs were
    pos = np.flatnonzero(lab == 1)
    want = 2006 * n // 5000
    if pos.size > want:
        lab[pos[want:]] = 0
    elif pos.size < want:
        lab[np.flatnonzero(lab == 0)[-(want - pos.size):]] = 1
    return lab


@pytest.fixture(scope="module")
def fv5000():
    rng = np.random.RandomState(11)
    return rng.standard_normal((6, 5000)).astype(np.float32)


# (W, W_shift, batchSize, signal_type, batches, the (neg, pos) patches of every refill, the longer queue after the last batch)
# music, part_size 1 088: negatives hop 11, positives hop 34.  Refill 0: 90 / 30 patches.  Refill 1 (batch 1): the 2 006 positives
#   end inside the part, so it is [0, 2 006) = 57 patches, as every later one.  Refill 2 (batch 5): the 2 994 negatives end, [0, 2 994)
#   = 264 patches.  12 refills in 40 batches; the negative queue is 2 * 90 + 10 * 264 - 40 * 16 = 2 180 long.
# speech, part_size 36 < W = 68: every part is tiled to 72 frames, 1 / 2 patches per refill at hops 9 / 3, two refills per batch; the
#   56th part of the positives is [0, 2 006) = 646 patches: 55 * 2 + 5 * 646 - 30 * 2 = 3 280.
CASES = [
    pytest.param(99, 34, 16, "music", 40, [(90, 30), (90, 57)] + [(264, 57)] * 10, 2180, id="w99_music"),
    pytest.param(68, 9, 2, "speech", 30, [(1, 2)] * 55 + [(1, 646)] * 5, 3280, id="w68_speech_tiled"),
]


@pytest.mark.parametrize("W, W_shift, bs, signal_type, batches, refills, longest", CASES)
@pytest.mark.parametrize("lemaire", [True, False], ids=["time_major", "image"])
def test_planner_matches_literal_generator(fv5000, W, W_shift, bs, signal_type, batches, refills, longest, lemaire):
    lab = _labels()
    assert (int((lab == 0).sum()), int((lab == 1).sum())) == (2994, 2006)
    log = []
    ref = dafx_ref.generator(fv5000, lab, W, W_shift, bs, signal_type, lemaire=lemaire, log=log)
    planner = dafx.FeedPlanner(lab, W, W_shift, bs, signal_type, n_feat=fv5000.shape[0])
    layout = "time_major" if lemaire else "image"
    for b in range(batches):
        want, want_label, queued = next(ref)
        table = planner.next_batch()
        assert table.dtype == np.int32 and table.shape == (2 * bs, 3)
        got = dafx_ref.numpy_gather(fv5000, table, W, layout)
        if not lemaire:
            got = got[:, :, :, None]
        assert got.shape == want.shape, (b, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), "batch %d" % b
        assert tuple(c.balance for c in planner.classes) == queued, b
        assert np.array_equal(want_label, [0] * bs + [1] * bs)
    # the figures of the case: what every refill added, and how long the faster queue has grown
    assert log == refills, log
    assert max(queued) == longest, queued
    # host memory: one fixed-size progression per refill, however many patches it stands for
    for c, n_ref in zip(planner.classes, zip(*log)):
        assert c.refills == sum(1 for k in n_ref if k > 0)
        assert len(c.queue) + c.retired == c.refills
        assert all(type(r).__slots__ == ("base", "period", "tiled", "hop", "count", "consumed", "linear") and not hasattr(r, "__dict__")
                   for r in c.queue)
        assert sum(r.count - r.consumed for r in c.queue) == c.balance


def test_planner_refuses_a_class_that_cannot_fill():
    lab = np.zeros(400, np.int32)
    lab[:99] = 1  # size(pos_idx) == W
    with pytest.raises(ValueError, match=r"positive.* 99 frames"):
        dafx.FeedPlanner(lab, 99, 34, 4, "music").next_batch()
    lab[99] = 1  # one more: fills
    assert dafx.FeedPlanner(lab, 99, 34, 4, "music").next_batch().shape == (8, 3)
    with pytest.raises(ValueError, match=r"negative.* 0 frames"):
        dafx.FeedPlanner(np.ones(400, np.int32), 99, 34, 4, "speech").next_batch()
    with pytest.raises(ValueError, match="signal_type"):
        dafx.FeedPlanner(lab, 99, 34, 4, "noise")


MUSIC_CSV = """start,duration,label

0.0,2.5,1
2.5,0.0,1

2.5,1.5,0
4.0,6.0,1
"""
SPEECH_CSV = """start,duration,label
0.5,1.25,1
1.75,0.0,0
3.0,1.0,0

7.3,1.7,1
"""


def test_get_annotations(tmp_path):
    folder, opDir = str(tmp_path / "data"), str(tmp_path / "out")
    for kind, text in (("music", MUSIC_CSV), ("speech", SPEECH_CSV)):
        os.makedirs(os.path.join(folder, "labels", kind))
        with open(os.path.join(folder, "labels", kind, "rec-1.csv"), "w", newline="\n") as f:
            f.write(text)
    nFrames = 1003
    ref_mu, ref_sp, ref_mm, ref_sm = dafx_ref.get_annotations(folder, "rec-1", nFrames)
    mu, sp, mm, sm = dafx.get_annotations(folder, "rec-1", nFrames, opDir)
    assert mu == ref_mu and sp == ref_sp and len(mu) == 4 and len(sp) == 4  # header and empty rows dropped, dur == 0 rows kept here
    assert mm.dtype == np.float64 and np.array_equal(mm, ref_mm) and np.array_equal(sm, ref_sm)
    # audio_length is 10 s (music): the segment that ends there stops at nFrames - 1, the label-0 and dur == 0 rows mark nothing
    assert mm[-2] == 1 and mm[-1] == 0 and mm[:250].all() and not mm[251:401].any() and mm[402:-1].all()
    assert sm[51:175].all() and not sm[176:732].any() and sm[733:903].all() and not sm[904:].any()
    # the cache: the reference's four keys, and a second call reads them back
    path = os.path.join(opDir, "__annotations", "rec-1.npz")
    with np.load(path, allow_pickle=True) as z:
        assert sorted(z.files) == ["annotations_mu", "annotations_sp", "music_marker", "speech_marker"]
    os.remove(os.path.join(folder, "labels", "music", "rec-1.csv"))  # the second call must not need it
    mu2, sp2, mm2, sm2 = dafx.get_annotations(folder, "rec-1", nFrames, opDir)
    assert mu2.item() == mu and sp2.item() == sp and np.array_equal(mm2, mm) and np.array_equal(sm2, sm)


@pytest.mark.parametrize("T, W, shift", [(10000, 99, 1), (300, 68, 34), (99, 99, 1)])
def test_patch_labels(T, W, shift):
    rng = np.random.RandomState(T + W)
    marker = np.repeat(rng.randint(0, 2, T // 25 + 1), 25)[:T].astype(np.float64)
    got = dafx.patch_labels(marker, W, shift)
    want = dafx_ref.patch_labels(marker, W, shift)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert len(got) == len(range(W // 2, T - W // 2, shift)) > 0


def test_patch_labels_is_not_tiled():
    assert len(dafx.patch_labels(np.ones(50), 99, 1)) == 0 == len(dafx_ref.patch_labels(np.ones(50), 99, 1))


def test_get_performance_against_sklearn():
    import warnings

    from sklearn import metrics
    rng = np.random.RandomState(5)
    truth = rng.randint(0, 2, 4000)
    cases = [np.where(rng.rand(4000) < 0.8, truth, 1 - truth), np.zeros(4000, int), truth.copy()]
    for pred in cases:
        cm, p, r, f = dafx.getPerformance(pred, truth, labels=[0, 1])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rp, rr, rf, _ = metrics.precision_recall_fscore_support(y_true=truth, y_pred=pred, beta=1.0, average=None, labels=[0, 1])
        assert np.array_equal(cm, metrics.confusion_matrix(y_true=truth, y_pred=pred))
        assert np.array_equal(p, np.round(rp, 4)) and np.array_equal(r, np.round(rr, 4)) and np.array_equal(f, np.round(rf, 4))
    cm, p, r, f = dafx.getPerformance(np.zeros(4000, int), truth, labels=[0, 1])
    assert p[1] == 0 and r[1] == 0 and f[1] == 0 and r[0] == 1  # all-negative prediction: sklearn's zero-division result
    # labels=None: the labels that occur
    cm, p, r, f = dafx.getPerformance(np.zeros(10, int), np.zeros(10, int))
    assert cm.shape == (1, 1) and cm[0, 0] == 10 and list(p) == [1.0]
