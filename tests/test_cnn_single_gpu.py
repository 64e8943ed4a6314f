"""The single-task Conv2D baselines (get_Doukhan_model / get_Papakostas_model / get_Jang_model, lib/baseline_architectures.py) on the
device against tests/cnn_single_ref.py: forward for two and three classes at the bounds tests/test_cnn_gpu.py::_check applies to the
MTL siblings (outputs 1e-4, features 2e-4 * max(1, |ref|), equal argmax, tensor names / order / shapes), one array from `predict`,
a row's bits independent of the batch, the bf16 forward, the refusals of smh_cnn_create, the builders and persistence."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cnn_single_ref as ref

pytestmark = pytest.mark.gpu

# (kind, H, W, N, fc, n_mels)
FORWARD_CASES = [("Doukhan", 21, 68, 3, 0, 0), ("Doukhan", 22, 80, 5, 0, 0), ("Doukhan", 21, 68, 70, 0, 0),
                 ("Papakostas", 61, 68, 3, 64, 0), ("Papakostas", 75, 41, 3, 128, 0), ("Papakostas", 201, 68, 2, 64, 0),
                 ("Jang", 257, 12, 3, 0, 64), ("Jang", 257, 20, 3, 0, 64), ("Jang", 257, 68, 3, 0, 64), ("Jang", 257, 20, 3, 0, 30)]


def _model(kind, H, W, n_classes, fc=0, n_mels=64):
    from sm_hpss_mtl_amd.cnn_models import CnnSingleTask
    return CnnSingleTask(kind, (H, W, 1), n_classes=n_classes, seed=0, fc_width=fc, n_mels=n_mels or 64)


@pytest.mark.parametrize("n_classes", [2, 3])
@pytest.mark.parametrize("kind,H,W,N,fc,n_mels", FORWARD_CASES, ids=["%s-%dx%d-N%d-fc%d-mel%d" % c for c in FORWARD_CASES])
def test_forward_matches_the_reference(kind, H, W, N, fc, n_mels, n_classes):
    w = ref.init_weights(kind, H, W, n_classes, seed=5, fc=fc or 64, n_mels=n_mels or 64, mel_signs=True)
    m = _model(kind, H, W, n_classes, fc, n_mels)
    assert m.weight_names() == list(w.keys())  # same tensors, same order, same Keras shapes
    assert [s for _, s, _ in m._spec] == [v.shape for v in w.values()]
    assert m.out_dim == n_classes and m.output_names == ["dense"] and m.metrics_names == ["loss", "accuracy"]
    m.set_weights_dict(w)
    x = np.random.default_rng(N + H).standard_normal((N, H, W, 1)).astype(np.float32)
    p_ref, f_ref = ref.forward(kind, x[..., 0], w, n_mels=n_mels or 64)
    feats = torch.empty((N, m.feat_dim), device="cuda")
    out = m.forward_device(torch.from_numpy(x).cuda(), features=feats).cpu().numpy()
    f = feats.cpu().numpy()
    assert f.shape == f_ref.shape and out.shape == (N, n_classes)
    ferr = float(np.max(np.abs(f - f_ref) / np.maximum(1.0, np.abs(f_ref))))
    oerr = float(np.abs(out - p_ref).max())
    print("%s %dx%d N=%d %d classes: features %.2e, outputs %.2e" % (kind, H, W, N, n_classes, ferr, oerr))
    assert ferr <= 2e-4 and oerr <= 1e-4
    assert np.allclose(out.sum(1), 1.0, atol=1e-5)
    top2 = np.sort(p_ref, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() > 2e-4  # the cases hold no near-tie (the smallest margin of any is 6.4e-4) ...
    assert np.array_equal(out.argmax(1), p_ref.argmax(1))  # ... so every row has one argmax, and it is the reference's
    got = m.predict(x)
    assert isinstance(got, np.ndarray) and got.shape == (N, n_classes) and np.array_equal(got, out)
    assert np.array_equal(m.predict(torch.from_numpy(x).cuda()), out)


@pytest.mark.parametrize("n_classes", [2, 3])
def test_a_row_has_the_same_bits_alone_and_in_a_batch_of_70(n_classes):
    """N = 70 is a full pass of 64 images and a ragged one of 6.  The single-task kinds plan the split-K of every pass as a full
    pass's (Doukhan's conv3 would otherwise split 9 ways at 3 images and 8 ways at 64), so the trunk gives a row the same bits in every
    batch; the tail's ordered four-wave sum does not depend on N either."""
    H, W = 21, 68
    m = _model("Doukhan", H, W, n_classes)
    m.set_weights_dict(ref.init_weights("Doukhan", H, W, n_classes, seed=5))
    x = np.random.default_rng(1).standard_normal((70, H, W)).astype(np.float32)
    big = m.predict(x)
    for rows in ([0, 1, 2], [62, 63, 64], [67, 68, 69]):
        assert np.array_equal(m.predict(x[rows]), big[rows]), rows


@pytest.mark.parametrize("kind,H,W,N,fc", [("Doukhan", 40, 68, 3, 0), ("Papakostas", 201, 68, 3, 128), ("Jang", 257, 20, 3, 0)])
def test_bf16_forward(kind, H, W, N, fc):
    """smh_cnn_forward_bf16 at the bound tests/test_cnn_gpu.py::test_bf16_operand_variant applies to the MTL sibling: features within
    3 % of their largest entry of the f32 path, outputs within 5e-2."""
    m = _model(kind, H, W, 3, fc)
    m.set_weights_dict(ref.init_weights(kind, H, W, 3, seed=5, fc=fc or 64))
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((N, H, W)).astype(np.float32)).cuda()
    f32f, bff = torch.empty((N, m.feat_dim), device="cuda"), torch.empty((N, m.feat_dim), device="cuda")
    o32 = m.forward_device(x, features=f32f).cpu().numpy()
    o16 = m.forward_device(x, features=bff, dtype="bf16").cpu().numpy()
    fe32, fe16 = f32f.cpu().numpy(), bff.cpu().numpy()
    ferr = np.abs(fe16 - fe32).max() / max(np.abs(fe32).max(), 1e-6)
    oerr = np.abs(o16 - o32).max()
    print("%s %dx%d: bf16 vs f32 features %.2e of max, outputs %.2e" % (kind, H, W, ferr, oerr))
    assert np.isfinite(o16).all() and 0 < ferr < 3e-2 and oerr < 5e-2


def test_create_refuses_other_class_counts():
    from sm_hpss_mtl_amd import _lib
    lib = _lib.require_gpu()
    for kind, H, n_classes, ok in ((3, 21, 5, False), (3, 21, 1, False), (4, 61, 5, False), (5, 257, 1, False), (0, 30, 2, False),
                                   (3, 21, 2, True), (5, 257, 3, True), (0, 30, 3, True)):
        h = C.c_void_p()
        cfg = _lib.CnnCfg(kind, H, 68, n_classes, 0, 0, 64, 0.0)
        rc = lib.smh_cnn_create(C.byref(cfg), C.byref(h))
        if ok:
            assert rc == 0 and lib.smh_cnn_out_dim(h) == (n_classes if kind >= 3 else 4 + n_classes)
            lib.smh_cnn_destroy(h)
        else:
            assert rc == _lib.SMH_E_INVALID and "n_classes" in _lib.last_error() and not h.value
    # the MTL Doukhan kind keeps its 24 x 68 floor, the single-task kind takes the reference's 21 rows; 257 rows are not 2 * 257
    h = C.c_void_p()
    assert lib.smh_cnn_create(C.byref(_lib.CnnCfg(0, 21, 68, 3, 0, 0, 0, 0.0)), C.byref(h)) == _lib.SMH_E_INVALID
    assert "at least 24 x 68" in _lib.last_error()
    assert lib.smh_cnn_create(C.byref(_lib.CnnCfg(5, 514, 68, 2, 0, 0, 0, 0.0)), C.byref(h)) == _lib.SMH_E_INVALID
    assert "n_fft/2 + 1" in _lib.last_error()
    assert lib.smh_cnn_create(C.byref(_lib.CnnCfg(3, 12, 68, 2, 0, 0, 0, 0.0)), C.byref(h)) == _lib.SMH_E_INVALID
    assert "too small" in _lib.last_error()
    from sm_hpss_mtl_amd.cnn_models import CnnSingleTask
    with pytest.raises(ValueError, match="n_classes"):
        CnnSingleTask("Doukhan", (21, 68, 1), n_classes=5)


# Baseline_Results.py's PARAMS entries of the three models
BASELINES = {"Doukhan_et_al": ("get_Doukhan_model", (21, 68, 1), 400, "Doukhan", 1e-4, "adam"),
             "Papakostas_et_al": ("get_Papakostas_model", (201, 68, 1), 400, "Papakostas", 1e-3, "sgd"),
             "Jang_et_al": ("get_Jang_model", (257, 68, 1), 512, "Jang", 1e-3, "adam")}


@pytest.mark.parametrize("name", sorted(BASELINES))
def test_builders_and_persistence(name, tmp_path):
    from sm_hpss_mtl_amd.cnn_models import CnnSingleTask
    from sm_hpss_mtl_amd.lib import baseline_architectures as ba
    from sm_hpss_mtl_amd.persistence import model_from_json
    fn, shape, n_fft, kind, lr, opt = BASELINES[name]
    P = {"Model": name, "input_shape": {name: shape}, "n_fft": {name: n_fft}}
    # (Papakostas at the reference's 4096-wide Dense layers holds 42 M weights: built once, for two classes)
    for n_classes in ((2,) if kind == "Papakostas" else (2, 3)):
        model, got_lr = getattr(ba, fn)(P, n_classes=n_classes)
        assert type(model) is CnnSingleTask and model.kind == kind and model.n_classes == n_classes
        assert model.input_shape == (None,) + shape and got_lr == pytest.approx(lr) and model.optimizer.kind == opt
        assert model.learning_rate(0) == pytest.approx(lr)
        assert model.loss_name == ("binary_crossentropy" if n_classes == 2 else "categorical_crossentropy")
        names = model.weight_names()
        assert names[-2:] == ["dense/kernel", "dense/bias"] and model.weights["dense/kernel"].shape[1] == n_classes
        if kind == "Papakostas":
            assert model.learning_rate(700) == pytest.approx(1e-4) and model.feat_dim == 4096
            assert np.all(model.weights["dense/bias"] == np.float32(0.1)) and 0.005 < model.weights["dense/kernel"].std() < 0.02
        elif kind == "Doukhan":
            assert model.feat_dim == 512 and np.all(model.weights["dense/bias"] == 0)
            lim = np.sqrt(6.0 / (512 + n_classes))
            assert np.abs(model.weights["dense/kernel"]).max() <= lim and model.weights["dense/kernel"].std() > 0.3 * lim
        else:
            assert model.feat_dim == 8192 and names[0] == "melCl0/kernel" and sum(n.startswith("melCl") for n in names) == 64
            k = model.weights["melCl5/kernel"]
            assert k.shape[1:] == (5, 1, 3) and k.min() >= 0 and k.max() > 0 and np.array_equal(k[:, 0, 0, 0], k[:, 4, 0, 2])
    with pytest.raises(ValueError, match="t_dim"):
        ba.get_Jang_model({"Model": "Jang_et_al", "input_shape": {"Jang_et_al": (257, 68, 1)}, "n_fft": {"Jang_et_al": 512}}, t_dim=3)
    # to_json -> model_from_json -> save_weights / load_weights (.h5 and .npz), on a small input
    small = {"Doukhan": (21, 68, 1), "Papakostas": (61, 68, 1), "Jang": (257, 12, 1)}[kind]
    a = CnnSingleTask(kind, small, n_classes=3, seed=1, fc_width=64)
    assert '"%s_SingleTask"' % kind in a.to_json()
    x = np.random.default_rng(0).standard_normal((3,) + small).astype(np.float32)
    for ext in (".h5", ".npz"):
        b = model_from_json(a.to_json(), seed=2)
        assert type(b) is CnnSingleTask and b.weight_names() == a.weight_names()
        path = str(tmp_path / ("w" + ext))
        a.save_weights(path)
        b.load_weights(path)
        wa, wb = a.get_weights_dict(), b.get_weights_dict()
        assert all(np.array_equal(wa[k], wb[k]) for k in wa)
        assert np.abs(a.predict(x) - b.predict(x)).max() <= 1e-6
