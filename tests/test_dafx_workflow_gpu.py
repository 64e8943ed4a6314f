"""sm_hpss_mtl_amd.dafx end to end on two small synthetic recordings (n_mels = 20, F = 40): load_data against the stages done by
hand, the device generator against the literal host generator of tests/dafx_ref.py bit for bit, the fine-tuning of a cut-out
head fed by it, and evaluate_file against its parts."""
import os

import numpy as np
import pytest
import torch

from tests import dafx_ref

pytestmark = pytest.mark.gpu

FILES = {"rec-a": 400, "rec-b": 350}
# (tmin, dur, label) rows; both recordings are 4 s long by their annotations, so a frame is 10 ms (rec-a) or 11.4 ms (rec-b)
MUSIC = {"rec-a": [(0.0, 1.2, 1), (1.2, 0.9, 0), (2.1, 0.0, 1), (2.1, 1.9, 1)], "rec-b": [(0.0, 2.0, 0), (2.0, 2.0, 1)]}
SPEECH = {"rec-a": [(0.5, 2.0, 1), (2.5, 1.5, 0)], "rec-b": [(0.3, 1.0, 1), (1.3, 0.7, 0), (2.5, 1.4, 1)]}
W = 68


def _write_csv(path, rows):
    with open(path, "w", newline="\n") as f:
        f.write("start,duration,label\n\n")
        for r in rows:
            f.write("%r,%r,%d\n" % r)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    root = tmp_path_factory.mktemp("dafx")
    folder = str(root / "data")
    os.makedirs(os.path.join(folder, "features"))
    for kind, rows in (("music", MUSIC), ("speech", SPEECH)):
        os.makedirs(os.path.join(folder, "labels", kind))
        for fl in FILES:
            _write_csv(os.path.join(folder, "labels", kind, fl + ".csv"), rows[fl])
    specs = {}
    for i, (fl, T) in enumerate(FILES.items()):
        rng = np.random.RandomState(100 + i)
        # a magnitude spectrogram with some structure: a few steady partials, a few broadband onsets, a noise floor
        S = 0.05 * np.abs(rng.standard_normal((201, T)))
        S[rng.randint(5, 150, 6)] += 1.0 + 0.2 * rng.rand(6, 1)
        S[:, rng.randint(0, T, 8)] += 0.7
        specs[fl] = S.astype(np.float32)
        np.save(os.path.join(folder, "features", fl + ".npy"), specs[fl])
    model = "Lemaire_et_al_MTL"
    PARAMS = {
        "Model": model, "featName": {model: "LogMelHarmPercSpec"}, "n_fft": {model: 400}, "n_mels": {model: 20},
        "l_harm": {model: 21}, "l_perc": {model: 11}, "Tw": 25, "Ts": 10, "W": W, "W_shift": 34, "W_shift_test": 1,
        "signal_type": "music", "data_augmentation_with_noise": False, "test_path": folder,
        "feature_opDir": str(root / "feat") + "/", "opDir": str(root / "out") + "/",
    }
    return PARAMS, folder, specs


@pytest.fixture(scope="module")
def loaded(env):
    from sm_hpss_mtl_amd import dafx
    PARAMS, folder, _ = env
    FV, labels_mu, labels_sp = dafx.load_data(PARAMS, folder, ["rec-a", "missing", "rec-b"])
    return FV, labels_mu, labels_sp, FV.cpu().numpy()


def _other_model(PARAMS):
    """The same configuration under a model name without 'Lemaire_et_al': image patches (2 bs, F, W, 1)."""
    p = dict(PARAMS, Model="Doukhan_et_al_MTL")
    for k in ("featName", "n_fft", "n_mels", "l_harm", "l_perc"):
        p[k] = {"Doukhan_et_al_MTL": PARAMS[k]["Lemaire_et_al_MTL"]}
    return p


def test_load_data_is_the_stages_by_hand(env, loaded):
    from sm_hpss_mtl_amd import dafx
    PARAMS, folder, specs = env
    FV, labels_mu, labels_sp, _ = loaded
    fe = dafx._frontend_for(PARAMS)
    assert fe.rows == 20
    parts, mu, sp = [], [], []
    for fl, T in FILES.items():
        S = torch.from_numpy(specs[fl]).cuda()[None]
        harm, perc = fe.hpss_median(S)
        parts.append(fe.standardize_rows(fe.features(S, harm, perc)["fv"][0]))
        _, _, mm, sm = dafx.get_annotations(folder, fl, T, PARAMS["opDir"])
        ref = dafx_ref.get_annotations(folder, fl, T)
        assert np.array_equal(mm, ref[2]) and np.array_equal(sm, ref[3])
        mu.append(mm.astype(np.int32))
        sp.append(sm.astype(np.int32))
    assert FV.is_cuda and FV.dtype == torch.float32 and tuple(FV.shape) == (40, 750) and FV.is_contiguous()
    assert torch.equal(FV, torch.cat(parts, dim=1))
    assert labels_mu.dtype == np.int32 and np.array_equal(labels_mu, np.concatenate(mu))
    assert labels_sp.dtype == np.int32 and np.array_equal(labels_sp, np.concatenate(sp))
    assert min((labels_mu == 0).sum(), (labels_mu == 1).sum(), (labels_sp == 0).sum(), (labels_sp == 1).sum()) > W
    # the featuregram cache of the reference: the unstandardised featuregram per file, read back by a second call
    for fl, T in FILES.items():
        assert np.load(os.path.join(PARAMS["feature_opDir"], fl + ".npy")).shape == (40, T)
    FV2, mu2, sp2 = dafx.load_data(PARAMS, folder, ["rec-a", "rec-b"])
    assert torch.equal(FV2, FV) and np.array_equal(mu2, labels_mu) and np.array_equal(sp2, labels_sp)


@pytest.mark.parametrize("W_shift, bs", [(34, 2), (9, 2)], ids=["plain_parts", "tiled_parts"])
@pytest.mark.parametrize("signal_type", ["music", "speech"])
@pytest.mark.parametrize("lemaire", [True, False], ids=["time_major", "image"])
def test_generator_is_the_literal_generator(env, loaded, lemaire, signal_type, W_shift, bs):
    from sm_hpss_mtl_amd import dafx
    FV, labels_mu, labels_sp, host = loaded
    PARAMS = dict(env[0] if lemaire else _other_model(env[0]), signal_type=signal_type, W_shift=W_shift)
    labels = labels_mu if signal_type == "music" else labels_sp
    ref = dafx_ref.generator(host, labels, W, W_shift, bs, signal_type, lemaire=lemaire)
    gen = dafx.generator(PARAMS, FV, labels_mu, labels_sp, bs)
    for b in range(10):
        want, want_label, _ = next(ref)
        got, got_label = next(gen)
        assert got.is_cuda and tuple(got.shape) == ((2 * bs, W, 40) if lemaire else (2 * bs, 40, W, 1)) == want.shape
        assert np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), b
        assert np.array_equal(got_label, want_label) and np.array_equal(got_label, [0] * bs + [1] * bs)


def test_generator_noise_and_refusals(env, loaded):
    from sm_hpss_mtl_amd import batching, dafx
    FV, labels_mu, labels_sp, host = loaded
    PARAMS = dict(env[0], data_augmentation_with_noise=True)
    clean, _, _ = next(dafx_ref.generator(host, labels_mu, W, 34, 2, "music"))
    np.random.seed(4)
    scale = float(np.random.choice(batching.NOISE_SCALES))  # the numpy draw of the reference, :428
    np.random.seed(4)
    torch.manual_seed(9)
    x1, _ = next(dafx.generator(PARAMS, FV, labels_mu, labels_sp, 2))
    np.random.seed(4)
    torch.manual_seed(9)
    x2, _ = next(dafx.generator(PARAMS, FV, labels_mu, labels_sp, 2))
    assert torch.equal(x1, x2)  # np.random.seed + torch.manual_seed reproduce a batch
    z = (x1.cpu().numpy().astype(np.float64) - clean) / scale
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) + 1e-3 and abs(z.std() - 1) < 5 / np.sqrt(n) + 2e-3
    lab = np.zeros(750, np.int32)
    lab[:W] = 1
    with pytest.raises(ValueError, match=r"positive.* %d frames" % W):
        next(dafx.generator(dict(PARAMS), FV, lab, labels_sp, 2))
    with pytest.raises(ValueError, match="750 frames"):
        next(dafx.generator(dict(PARAMS), FV, lab[:-1], labels_sp, 2))


def _head_model(seed=5):
    from sm_hpss_mtl_amd import optimizers
    from sm_hpss_mtl_amd.model import B3MTL
    from sm_hpss_mtl_amd.persistence import Model
    trained = B3MTL(n_feat=40, patch_size=W, n_classes=3, seed=seed, nb_stacks=3, n_dilations=2)
    sub = Model(trained.input, trained.get_layer("M").output)
    sub.compile(loss="binary_crossentropy", optimizer=optimizers.Nadam(learning_rate=0.002), metrics="accuracy")
    return trained, sub


def test_fine_tuning_a_head_from_the_generator(env, loaded):
    """The driver's transfer_learn_model (:442-470) on the device generator: the fit call of the issue gives finite logs, and the
    first training loss EQUALS train_on_batch on the literal generator's first batch.  fit logs the mean over an epoch's steps, so
    the first step's loss is read from a fit of one step on a fresh model of the same seed (same weights, same dropout masks:
    that step is the first step of the two-step fit); with one step the logged mean is that step's loss itself.  The loss of a
    first step is a forward pass on equal bits through equal kernels, so it is compared with ==."""
    from sm_hpss_mtl_amd import dafx
    PARAMS = env[0]
    FV, labels_mu, labels_sp, host = loaded

    def feed():
        return dafx.generator(PARAMS, FV, labels_mu, labels_sp, 2)
    _, sub = _head_model()
    h = sub.fit(feed(), steps_per_epoch=2, validation_data=feed(), validation_steps=1, epochs=1, verbose=0)
    logs = {k: v[0] for k, v in h.history.items()}
    assert sorted(logs) == ["accuracy", "loss", "val_accuracy", "val_loss"] and all(np.isfinite(v) for v in logs.values()), logs
    _, one = _head_model()
    first = one.fit(feed(), steps_per_epoch=1, epochs=1, verbose=0).history
    _, twin = _head_model()
    x0, y0, _ = next(dafx_ref.generator(host, labels_mu, W, PARAMS["W_shift"], 2, "music"))
    want = twin.train_on_batch(x0, y0)
    print("first training loss: fit %.9g, train_on_batch on the literal batch %.9g" % (first["loss"][0], want[0]))
    assert first["loss"][0] == want[0] and first["accuracy"][0] == want[1]


def test_load_data_and_evaluate_file_log_mel_spec(env, tmp_path):
    """featName 'LogMelSpec' (:232-235): power_to_db(melspectrogram(S=Spec) ** 2) with the 22 050 Hz basis -- the mel and power_to_db_sq
    stages by hand, and their numpy restatement within the 1e-3 dB the project holds f32 dB features to."""
    from sm_hpss_mtl_amd import dafx, inference
    from sm_hpss_mtl_amd.model import B3MTL
    from sm_hpss_mtl_amd.persistence import Model
    base, folder, specs = env
    m = base["Model"]
    PARAMS = dict(base, featName={m: "LogMelSpec"}, feature_opDir=str(tmp_path / "feat") + "/", opDir=str(tmp_path / "out") + "/")
    fe = dafx._frontend_for(PARAMS)
    FV, labels_mu, labels_sp = dafx.load_data(PARAMS, folder, ["rec-a", "rec-b"])
    by_hand = {fl: fe.power_to_db_sq(fe.mel(torch.from_numpy(specs[fl]).cuda()[None]))[0] for fl in FILES}
    assert tuple(FV.shape) == (20, 750) and torch.equal(FV, torch.cat([fe.standardize_rows(by_hand[fl]) for fl in FILES], dim=1))
    assert len(labels_mu) == len(labels_sp) == 750
    for fl in FILES:
        sq = (fe.mel_basis().astype(np.float64) @ specs[fl].astype(np.float64)) ** 2
        db = 10.0 * np.log10(np.maximum(1e-10, sq))
        db = np.maximum(db, db.max() - 80.0)
        assert np.max(np.abs(by_hand[fl].cpu().numpy() - db)) < 1e-3
        assert np.array_equal(np.load(os.path.join(PARAMS["feature_opDir"], fl + ".npy")), by_hand[fl].cpu().numpy())
    trained = B3MTL(n_feat=20, patch_size=W, n_classes=3, seed=8, nb_stacks=3, n_dilations=2)
    sub = Model(trained.input, trained.get_layer("M").output)
    res = dafx.evaluate_file(PARAMS, "rec-a", {"model": sub})
    pred = inference.patch_probabilities(by_hand["rec-a"], sub, W, 1, batch_frames=10000)
    assert pred.shape == (400 - W,) and np.array_equal(res["pred"], pred)
    cm, p, r, f = dafx.getPerformance(res["pred_lab"], res["labels_mu"], labels=[0, 1])
    assert np.array_equal(res["ConfMat"], cm) and np.array_equal(res["fscore"], f)
    x, y = next(dafx.generator(PARAMS, FV, labels_mu, labels_sp, 2))
    assert tuple(x.shape) == (4, W, 20)


def test_evaluate_file_is_its_parts(env):
    from sm_hpss_mtl_amd import dafx, inference
    PARAMS, folder, specs = env
    trained, sub = _head_model(seed=8)
    res = dafx.evaluate_file(PARAMS, "rec-a", {"model": sub})
    assert sorted(res) == sorted(["pred", "pred_lab", "labels_sp", "labels_mu", "ConfMat", "precision", "recall", "fscore", "accuracy",
                                  "probability_genTime"])
    fe = dafx._frontend_for(PARAMS)
    S = torch.from_numpy(specs["rec-a"]).cuda()[None]
    harm, perc = fe.hpss_median(S)
    fv = fe.features(S, harm, perc)["fv"][0]
    pred = inference.patch_probabilities(fv, sub, W, 1, batch_frames=10000)
    assert pred.shape == (400 - W,) and np.array_equal(res["pred"], pred)
    assert np.array_equal(res["pred_lab"], (pred > 0.5).astype(int))
    _, _, mm, sm = dafx.get_annotations(folder, "rec-a", 400, PARAMS["opDir"])
    assert np.array_equal(res["labels_mu"], dafx.patch_labels(mm, W, 1)) and len(res["labels_mu"]) == 400 - W
    assert np.array_equal(res["labels_sp"], dafx.patch_labels(sm, W, 1))
    assert np.array_equal(res["labels_mu"], dafx_ref.patch_labels(mm, W, 1))
    cm, p, r, f = dafx.getPerformance(res["pred_lab"], res["labels_mu"], labels=[0, 1])
    assert np.array_equal(res["ConfMat"], cm) and np.array_equal(res["precision"], p) and np.array_equal(res["recall"], r)
    assert np.array_equal(res["fscore"], f) and res["accuracy"] == np.round(np.sum(np.diag(cm)) / np.sum(cm), 4)
    assert res["probability_genTime"] >= 0
    # the speech head is scored against the speech markers
    sp_res = dafx.evaluate_file(dict(PARAMS, signal_type="speech"), "rec-a",
                                {"model": type(sub)(trained, "S")})
    cm, p, r, f = dafx.getPerformance(sp_res["pred_lab"], sp_res["labels_sp"], labels=[0, 1])
    assert np.array_equal(sp_res["ConfMat"], cm) and np.array_equal(sp_res["fscore"], f)
    assert dafx.evaluate_file(PARAMS, "missing", {"model": sub}) == {}


def test_evaluate_file_refuses_a_last_batch_shorter_than_a_patch(env):
    """10 030 frames: the second 10 000-frame batch has 30 < W frames -- tiled, it gives predictions; its markers give no label."""
    from sm_hpss_mtl_amd import dafx
    PARAMS, folder, _ = env
    T = 10030
    rng = np.random.RandomState(3)
    np.save(os.path.join(folder, "features", "rec-long.npy"), np.abs(rng.standard_normal((201, T))).astype(np.float32))
    for kind in ("music", "speech"):
        _write_csv(os.path.join(folder, "labels", kind, "rec-long.csv"), [(0.0, 50.0, 1), (50.0, 50.3, 0)])
    _, sub = _head_model(seed=8)
    with pytest.raises(ValueError, match=r"rec-long, batch \(10000, 10030\).* 22 predictions .* 0 labels"):
        dafx.evaluate_file(PARAMS, "rec-long", {"model": sub})
