"""GPU: the intermediate-fusion MTL model (get_Lemaire_MTL_intermediate_fusion_model) -- the two-input forward and training step
(smh_fusion.hip and the trunk-only B3_MTL kernels) against the float64 reference of tests/fusion_ref.py, the model's surface, the
one-half feature names on the device front end, and the reference driver's sequence."""
import json
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import b3_mtl_train as tr
from tests import fusion_ref as fref

pytestmark = pytest.mark.gpu


def _model(W=68, F=120, ncls=3, seed=0):
    from sm_hpss_mtl_amd.lib.proposed_architectures import get_Lemaire_MTL_intermediate_fusion_model
    m, lr = get_Lemaire_MTL_intermediate_fusion_model(TR_STEPS=10, N_MELS=F, n_classes=ncls, patch_size=W, seed=seed)
    assert lr == 0.002 and m.out_dim == (7 if ncls == 3 else 11)
    return m


def _at_end(a):
    """A CUDA copy of `a` that ends exactly at the end of its allocation, with NaN in front of it."""
    a = np.ascontiguousarray(a, np.float32)
    pad = 1021
    buf = torch.full((pad + a.size,), float("nan"), device="cuda")
    buf[pad:] = torch.from_numpy(a.ravel()).cuda()
    return buf[pad:].view(a.shape)


@pytest.mark.parametrize("W,F,ncls,Ns", [(68, 120, 3, (1, 2, 3, 4, 5, 6, 510, 1030)), (99, 120, 5, (1, 7)), (249, 120, 3, (2, 5)),
                                         (68, 61, 5, (3, 17)), (99, 61, 3, (4,))])
def test_forward_matches_reference(W, F, ncls, Ns):
    m = _model(W, F, ncls)
    w = fref.init_weights(seed=W + F, n_feat=F, patch_size=W, n_classes=ncls, randomize_bn=True)
    m.set_weights_dict(w)
    for N in Ns:
        rng = np.random.default_rng(N + W)
        xH, xP = (rng.standard_normal((N, W, F)).astype(np.float32) for _ in range(2))
        got = m.predict([_at_end(xH), _at_end(xP)])
        ref = fref.forward(xH, xP, w, ncls)
        for g, r in zip(got, ref):
            assert g.shape == r.shape and np.abs(g - r).max() <= 1e-4 * max(1.0, np.abs(r).max()), (N, np.abs(g - r).max())
        assert np.array_equal(got[-1].argmax(1), ref[-1].argmax(1)), N
    m.check_status()


def test_dict_input_and_refusals():
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.model import FusionMTL
    from sm_hpss_mtl_amd.persistence import Model
    m = _model()
    m.set_weights_dict(fref.init_weights(seed=1))
    rng = np.random.default_rng(0)
    xH, xP = (rng.standard_normal((5, 68, 120)).astype(np.float32) for _ in range(2))
    a = m.predict([xH, xP])
    b = m.predict({"perc_input": xP, "harm_input": xH})
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    for bad in (xH, [xH], (xH, xP, xP), {"harm_input": xH}, {"harm_input": xH, "x": xP}):
        with pytest.raises((TypeError, ValueError)):
            m.predict(bad)
    with pytest.raises(ValueError):
        m.predict([xH, xP[:4]])
    with pytest.raises(ValueError):
        m.forward_device([xH, xP], dtype="bf16")
    with pytest.raises(ValueError):
        m.train_dtype = "bf16"
    with pytest.raises(ValueError):
        Model(m.input, m.get_layer("M").output)
    with pytest.raises(ValueError):
        FusionMTL(n_feat=120, patch_size=68, tcn_block="2.8")
    with pytest.raises(ValueError):
        m.forward_from_x0(torch.zeros((2, 2, 68, 32), device="cuda"))
    with pytest.raises(ValueError):
        m.forward_dense(torch.zeros((120, 200), device="cuda"))
    # the C ABI refuses every entry point that cannot serve the model, with a message
    lib, h = m.lib, m._h
    x = torch.zeros((2, 68, 240), device="cuda")
    out = torch.zeros((2, 16), device="cuda")
    p = lambda t: __import__("ctypes").c_void_p(t.data_ptr())  # noqa: E731
    st = _lib.current_stream()
    checks = [
        lib.smh_model_forward_f32(h, p(x), 2, p(out), None, st),
        lib.smh_model_forward_x0_f32(h, p(x), 2, p(out), None, st),
        lib.smh_model_forward_bf16(h, p(x), 2, p(out), st),
        lib.smh_model_forward_bf16_ex(h, p(x), 2, p(out), 1, st),
        lib.smh_model_forward_x0_bf16(h, p(x), 2, p(out), 1, st),
        lib.smh_model_forward_dense_f32(h, p(x), 200, 1, p(x), x.numel() * 4, p(out), st),
        lib.smh_model_check_train_dtype(h, 1),
    ]
    for rc in checks:
        assert rc == _lib.SMH_E_INVALID
    assert lib.smh_model_w0_ptr(h) is None
    tr_ = m._get_trainer(4)
    assert lib.smh_trainer_set_dtype(tr_, 1) == _lib.SMH_E_INVALID and "f32" in _lib.last_error()
    assert lib.smh_train_step_f32(tr_, p(x), p(x), 2, None, None, None, p(out), st) == _lib.SMH_E_INVALID
    assert "smh_fusion_train_step_f32" in _lib.last_error()
    cfg = _lib.ModelCfg(120, 68, 3, 32, 3, 3, 8, 1)
    hh = __import__("ctypes").c_void_p()
    assert lib.smh_model_create_heads(__import__("ctypes").byref(cfg), 2, __import__("ctypes").byref(hh)) == _lib.SMH_E_INVALID
    assert "block_variant" in _lib.last_error()


def _train_problem(N, W=68, F=120, ncls=3, seed=0):
    rng = np.random.default_rng(seed)
    xH, xP = (rng.standard_normal((N, W, F)).astype(np.float32) for _ in range(2))
    y = {"S": (rng.random((N, 1)) > 0.5).astype(np.float32), "M": (rng.random((N, 1)) > 0.5).astype(np.float32),
         "R": rng.random((N, 2 if ncls == 3 else 3)).astype(np.float32), "3C": np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, N)]}
    if ncls == 5:
        y["N"] = (rng.random((N, 1)) > 0.5).astype(np.float32)
    nh = 3 if ncls == 3 else 4
    drop_tcn = ((rng.random((2, N, 24, 32)) > 0.2) / 0.8).astype(np.float32)
    drop_heads = ((rng.random((N, nh, 16)) > 0.4) / 0.6).astype(np.float32)
    return xH, xP, y, drop_tcn, drop_heads


def _flat_to_dict(model, flat):
    out, o = {}, 0
    for name, shape, _, _ in model._spec:
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    return out


@pytest.mark.parametrize("N,ncls,W,lw", [(1, 3, 68, None), (2, 3, 68, None), (3, 5, 68, None), (4, 3, 68, {"S": 0.7, "R": 1.3}),
                                         (5, 3, 68, None), (6, 5, 68, {"M": 1.5, "3C": 0.5}), (48, 3, 99, None), (510, 3, 68, None)])
def test_train_step_gradients_and_bn_statistics_vs_reference(N, ncls, W, lw):
    m = _model(W, 120, ncls)
    if lw:
        m.compile(loss_weights=lw)
    w = fref.init_weights(seed=5, n_feat=120, patch_size=W, n_classes=ncls)
    m.set_weights_dict(w)
    xH, xP, y, dt, dh = _train_problem(N, W, ncls=ncls, seed=N)
    names = [n for n in m.output_names[:-1]]
    got = m.train_on_batch([_at_end(xH), _at_end(xP)], y, drop_tcn=torch.from_numpy(dt).cuda(), drop_heads=torch.from_numpy(dh).cuda(),
                           apply=False)
    ref = fref.torch_forward_backward(xH, xP, y, w, ncls, dt, {h: dh[:, i] for i, h in enumerate(names)}, lw)
    assert abs(got[0] - ref["loss"]) < 2e-4 * max(1.0, abs(ref["loss"]))
    for i, name in enumerate(names + ["3C"]):
        assert abs(got[1 + i] - ref["losses"][name]) < 2e-4 * max(1.0, abs(ref["losses"][name])), name
    assert abs(got[-1] - ref["acc"]) < 1e-6
    torch.cuda.synchronize()
    bucket = m._bucket_tensor().cpu().numpy()
    n, D = m.count_params(), 2 * W * 32
    assert bucket.size == n + 4 * 32 + 2 * D
    g = _flat_to_dict(m, bucket[:n])
    trunk_err, trunk_ref = {"tcn_H/": [], "tcn_P/": []}, {"tcn_H/": [], "tcn_P/": []}
    for name, gref in ref["grads"].items():
        if name.endswith(tr.TRAINABLE_SKIP):
            continue
        gg = g[name].astype(np.float64)
        if name.endswith("/dense/kernel"):
            gg = gg + 2 * tr.L2 * w[name]
        scale = max(np.abs(gref).max(), 1e-6)
        atol = 2e-5 if name.endswith("/dense/bias") else 1e-6
        if name.startswith("tcn_"):
            # The trunks' gradients pass 24 blocks of channel-max normalisation in f32, where a maximum tied within float32
            # rounding can take the other branch than in float64 (tests/test_model_shapes_gpu.py states the same for B3_MTL).
            # Finding: at N = 48, W = 99 trunk P's tensors sit up to 7.7e-3 relative L2 from the reference (s2_d2 conv kernel), the
            # same bits run to run; test_trunk_P_is_trunk_H_with_the_halves_swapped shows the P path computes what the H path does.
            # Held per tensor at 1e-2 relative L2 and over each whole trunk at 2e-3 below.
            assert np.linalg.norm(gg - gref) <= 1e-2 * max(np.linalg.norm(gref), 1e-6), (name, np.linalg.norm(gg - gref), np.linalg.norm(gref))
            for t in ("tcn_H/", "tcn_P/"):
                if name.startswith(t):
                    trunk_err[t].append(gg - gref), trunk_ref[t].append(gref)
        else:
            assert np.abs(gg - gref).max() <= 2e-3 * scale + atol, (name, np.abs(gg - gref).max(), scale)
    for t in trunk_err:
        e, r = np.concatenate([v.ravel() for v in trunk_err[t]]), np.concatenate([v.ravel() for v in trunk_ref[t]])
        assert np.linalg.norm(e) <= 2e-3 * np.linalg.norm(r), (t, np.linalg.norm(e) / np.linalg.norm(r))
    st = bucket[n:]
    for h, name in enumerate(names):
        mean, var = ref["bn_batch"][name]
        assert np.abs(st[h * 32:h * 32 + 16] - mean).max() <= 1e-4 * max(1.0, np.abs(mean).max())
        assert np.abs(st[h * 32 + 16:h * 32 + 32] - var).max() <= 1e-4 * max(1.0, np.abs(var).max())
    mean, var = ref["bn_batch"]["fusion_bn"]
    assert np.abs(st[128:128 + D] - mean).max() <= 1e-4 * max(1.0, np.abs(mean).max())
    assert np.abs(st[128 + D:] - var).max() <= 1e-4 * max(1.0, np.abs(var).max())


def test_trunk_P_is_trunk_H_with_the_halves_swapped():
    """Exchange the two trunks' weights and inputs and the two halves of the fused BatchNorm and of every Dense kernel: the model
    computes the same function, with trunk P doing what trunk H did.  Its gradients must then be trunk H's (the fused sums run in a
    different order: f32 rounding only) -- whatever the reference's float64 channel maxima do."""
    N, W = 48, 99
    m = _model(W, 120, 3)
    w = fref.init_weights(seed=5, n_feat=120, patch_size=W, n_classes=3)
    half = W * 32
    sw = OrderedDict()
    for k, v in w.items():
        if k.startswith("tcn_H/"):
            sw[k] = w["tcn_P/" + k[6:]]
        elif k.startswith("tcn_P/"):
            sw[k] = w["tcn_H/" + k[6:]]
        elif k.startswith("fusion_bn/") or k == "3C/kernel" or k.endswith("/dense/kernel"):
            sw[k] = np.concatenate([v[half:], v[:half]], axis=0)
        else:
            sw[k] = v
    xH, xP, y, dt, dh = _train_problem(N, W, seed=N)
    grads = []
    for ww, x, d in ((w, [xH, xP], dt), (sw, [xP, xH], dt[::-1].copy())):
        m.set_weights_dict(ww)
        m.train_on_batch(x, y, drop_tcn=torch.from_numpy(d).cuda(), drop_heads=torch.from_numpy(dh).cuda(), apply=False)
        torch.cuda.synchronize()
        grads.append(_flat_to_dict(m, m._bucket_tensor().cpu().numpy()[:m.count_params()].copy()))
    for k in grads[0]:
        if k.startswith("tcn_H/"):
            a, b = grads[0][k], grads[1]["tcn_P/" + k[6:]]
            assert np.linalg.norm(a - b) <= 1e-4 * max(np.linalg.norm(a), 1e-6), (k, np.linalg.norm(a - b) / np.linalg.norm(a))
            a, b = grads[0]["tcn_P/" + k[6:]], grads[1][k]
            assert np.linalg.norm(a - b) <= 1e-4 * max(np.linalg.norm(a), 1e-6), ("P", k, np.linalg.norm(a - b) / np.linalg.norm(a))
    for k in ("fusion_bn/gamma", "fusion_bn/beta"):
        a, b = grads[0][k], np.concatenate([grads[1][k][half:], grads[1][k][:half]])
        assert np.abs(a - b).max() <= 1e-4 * np.abs(a).max(), k


def test_moving_statistics_and_sgd_step_follow_the_reference():
    m = _model()
    w = fref.init_weights(seed=6)
    m.set_weights_dict(w)
    xH, xP, y, dt, dh = _train_problem(12, seed=2)
    m.train_on_batch([xH, xP], y, drop_tcn=torch.from_numpy(dt).cuda(), drop_heads=torch.from_numpy(dh).cuda())
    ref = fref.torch_forward_backward(xH, xP, y, w, 3, dt, {h: dh[:, i] for i, h in enumerate(("S", "M", "R"))})
    got = m.get_weights_dict()
    for key, pre in (("fusion_bn", "fusion_bn/"), ("S", "S/bn/"), ("R", "R/bn/")):
        mean, var = ref["bn_batch"][key]
        assert np.allclose(got[pre + "moving_mean"], 0.99 * w[pre + "moving_mean"] + 0.01 * mean, rtol=0, atol=1e-5), key
        assert np.allclose(got[pre + "moving_variance"], 0.99 * w[pre + "moving_variance"] + 0.01 * var, rtol=1e-5, atol=1e-5), key
    # one SGD step with momentum 0.9 from zero velocity: w - lr * clip(g) per tensor (clipnorm 1)
    lr = m.learning_rate(0)
    for name in ("fusion_bn/gamma", "tcn_P/s1_d4/conv/kernel", "tcn_H/initial_conv/kernel", "3C/kernel"):
        gref = ref["grads"][name]
        nrm = np.sqrt(np.sum(gref ** 2))
        want = w[name] - lr * gref * (min(1.0, 1.0 / nrm) if nrm > 0 else 1.0)
        assert np.abs(got[name] - want).max() <= 2e-3 * lr * max(np.abs(gref).max() * min(1.0, 1.0 / max(nrm, 1e-30)), 1e-6) + 1e-7, name


@pytest.mark.parametrize("opt", ["sgd", "adam", "nadam"])
def test_optimisers_and_deterministic_mode(opt):
    from sm_hpss_mtl_amd import optimizers
    runs = []
    for _ in range(2):
        m = _model(seed=1)
        m.deterministic_gradients = True
        if opt != "sgd":
            m.compile(optimizer=(optimizers.Adam if opt == "adam" else optimizers.Nadam)(learning_rate=1e-3))
        xH, xP, y, dt, dh = _train_problem(40, seed=7)
        w0 = m.get_weights()
        losses = [m.train_on_batch([xH, xP], y, drop_tcn=torch.from_numpy(dt).cuda(), drop_heads=torch.from_numpy(dh).cuda())
                  for _ in range(3)]
        grad = m._bucket_tensor().cpu().numpy().copy()
        w1 = m.get_weights()
        assert all(np.all(np.isfinite(l)) for l in losses)
        changed = [n for (n, _, _, _), a, b in zip(m._spec, w0, w1) if not np.array_equal(a, b)]
        assert any(n.startswith("tcn_H/") for n in changed) and any(n.startswith("tcn_P/") for n in changed)
        assert "fusion_bn/gamma" in changed and "fusion_bn/moving_mean" in changed
        runs.append((grad, w1))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_persistence_round_trip(tmp_path):
    from sm_hpss_mtl_amd.model import FusionMTL
    from sm_hpss_mtl_amd.persistence import model_from_json
    m = _model(99, 61, 5)
    m.set_weights_dict(fref.init_weights(seed=8, n_feat=61, patch_size=99, n_classes=5))
    js = m.to_json()
    assert json.loads(js)["class_name"] == "B3_MTL_Intermediate_Fusion"
    m2 = model_from_json(js)
    assert isinstance(m2, FusionMTL) and m2.to_json() == js and m2.count_params() == m.count_params()
    path = m.save_weights(str(tmp_path / "w.h5"))
    m2.load_weights(path)
    rng = np.random.default_rng(1)
    x = [rng.standard_normal((9, 99, 61)).astype(np.float32) for _ in range(2)]
    for a, b in zip(m.predict(x), m2.predict(x)):
        assert np.array_equal(a, b)


def test_half_feature_names_give_the_harm_perc_featuregram_and_its_halves():
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    from sm_hpss_mtl_amd.synth import synth_clips
    mdl = "Lemaire_et_al_MTL"
    P = {"Model": mdl, "Tw": 25, "Ts": 10, "l_harm": {mdl: 21}, "l_perc": {mdl: 11}, "frame_level_scaling": False}
    clip = synth_clips(1, seed=3)[0]
    for sib, (hn, pn) in (("LogMelHarmPercSpec", ("LogMelHarmSpec", "LogMelPercSpec")), ("MelHarmPercSpec", ("MelHarmSpec", "MelPercSpec"))):
        fv = pp.featuregram_from_signal(P, clip, 400, 120, sib)
        for name in (hn, pn):
            assert np.array_equal(pp.featuregram_from_signal(P, clip, 400, 120, name), fv), name
        both = pp.get_feature_patches(P, fv, 68, 34, sib)
        assert np.array_equal(pp.get_feature_patches(P, fv, 68, 34, hn), both[:, :120])
        assert np.array_equal(pp.get_feature_patches(P, fv, 68, 34, pn), both[:, 120:])


def _synthetic_gen(rng, n=48, W=68, F=120):
    while True:
        cls = rng.integers(0, 3, n)
        base = (cls[:, None, None] - 1.0) * 0.8
        xH = (rng.standard_normal((n, W, F)) * 0.3 + base).astype(np.float32)
        xP = (rng.standard_normal((n, W, F)) * 0.3 - base).astype(np.float32)
        y = {"S": (cls == 1).astype(np.float32)[:, None], "M": (cls == 0).astype(np.float32)[:, None],
             "R": np.stack([(cls != 1), (cls != 0)], 1).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[cls]}
        yield {"harm_input": torch.from_numpy(xH).cuda(), "perc_input": torch.from_numpy(xP).cuda()}, y


def test_fit_with_callbacks_and_the_two_input_generator(tmp_path):
    """fit on the batches fusion_generator yields (the device front end on synthetic clips), with EarlyStopping / ModelCheckpoint /
    CSVLogger; then a fit on synthetic separable batches lowers the loss."""
    from scipy.io import wavfile
    from sm_hpss_mtl_amd.callbacks import CSVLogger, EarlyStopping, ModelCheckpoint
    from sm_hpss_mtl_amd.generators import fusion_generator
    from sm_hpss_mtl_amd.synth import synth_clips
    folder = tmp_path / "data"
    names = {"speech": [], "music": []}
    clips = synth_clips(6, seed=4)
    for i, c in enumerate(clips):
        cls = "speech" if i % 2 else "music"
        (folder / cls).mkdir(parents=True, exist_ok=True)
        wavfile.write(str(folder / cls / ("f%d.wav" % i)), 16000, np.asarray(c, np.float32))
        names[cls].append("f%d.wav" % i)
    files = {"speech": names["speech"], "music": names["music"],
             "speech+music": [{"speech": names["speech"][0], "music": names["music"][0], "SMR": 5}]}
    mdl = "Lemaire_et_al_MTL"
    P = {"Model": mdl, "classes": {0: "music", 1: "speech", 2: "speech_music"}, "feature_opDir": str(tmp_path / "feat"), "W": 68,
         "W_shift": 34, "n_fft": {mdl: 400}, "n_mels": {mdl: 120}, "featName": {mdl: "LogMelHarmSpec"}, "frame_level_scaling": False,
         "skewness_vector": None, "data_augmentation_with_noise": True, "Tw": 25, "Ts": 10, "l_harm": {mdl: 21}, "l_perc": {mdl: 11}}
    m = _model(seed=2)
    np.random.seed(0)
    g = fusion_generator(P, str(folder), files, 4)
    bx, by = next(g)
    assert set(bx) == {"harm_input", "perc_input"} and tuple(bx["harm_input"].shape) == (12, 68, 120)
    wf = str(tmp_path / "best.h5")
    cbs = [CSVLogger(str(tmp_path / "log.csv")), EarlyStopping(monitor="val_loss", min_delta=0.01, patience=5, restore_best_weights=True),
           ModelCheckpoint(wf, monitor="val_loss", save_best_only=True, save_weights_only=True)]
    hist = m.fit(g, steps_per_epoch=2, epochs=2, validation_data=fusion_generator(P, str(folder), files, 4), validation_steps=1,
                 callbacks=cbs, verbose=0)
    assert len(hist.history["loss"]) == 2 and (tmp_path / "log.csv").exists()
    m2 = _model(seed=3)
    rng = np.random.default_rng(0)
    vgen = _synthetic_gen(np.random.default_rng(9))
    before = m2.evaluate(vgen, steps=2)
    m2.fit(_synthetic_gen(rng), steps_per_epoch=4, epochs=4, verbose=0)
    after = m2.evaluate(_synthetic_gen(np.random.default_rng(9)), steps=2)
    assert after[0] < before[0], (before, after)


def test_reference_driver_sequence(tmp_path):
    """Intermediate_Fusion_Results.py: build, fit (arrays), save weights and architecture, model_from_json + load_weights, compile,
    predict on test patches -- bit-identical to the trained model."""
    from sm_hpss_mtl_amd.lib.proposed_architectures import get_Lemaire_MTL_intermediate_fusion_model, model_from_json
    model, lr = get_Lemaire_MTL_intermediate_fusion_model(TR_STEPS=4, N_MELS=120, n_classes=3, patch_size=68, seed=5)
    gen = _synthetic_gen(np.random.default_rng(1), n=30)
    bx, by = next(gen)
    x = [bx["harm_input"].cpu().numpy(), bx["perc_input"].cpu().numpy()]
    model.fit(x, by, batch_size=10, epochs=2, verbose=0, validation_data=(x, by))
    model.save_weights(str(tmp_path / "w.h5"))
    with open(tmp_path / "arch.json", "w") as f:
        f.write(model.to_json())
    m2 = model_from_json(open(tmp_path / "arch.json").read())
    m2.load_weights(str(tmp_path / "w.h5"))
    m2.compile(loss={"S": "binary_crossentropy", "M": "binary_crossentropy", "R": "mean_squared_error",
                     "3C": "categorical_crossentropy"}, metrics={"3C": "accuracy"})
    tx, _ = next(gen)
    for a, b in zip(model.predict(tx), m2.predict(tx)):
        assert np.array_equal(a, b)
    res = m2.evaluate(x, by)
    assert len(res) == 6 and all(np.isfinite(res))


def test_b3mtl_alongside_still_matches_its_golden(golden_model):
    from oracle import b3_mtl
    from sm_hpss_mtl_amd.model import B3MTL
    fus = _model()
    fus.set_weights_dict(fref.init_weights(seed=3))
    b3 = B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=0)
    b3.set_weights_dict(b3_mtl.init_weights(seed=7, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True))
    x = np.random.default_rng(11).standard_normal((6, 68, 240)).astype(np.float32)
    fus.predict([x[:, :, :120], x[:, :, 120:]])
    got = np.concatenate(b3.predict(x), axis=1)
    assert np.abs(got - golden_model["out_c3_W68"]).max() <= 1e-4
