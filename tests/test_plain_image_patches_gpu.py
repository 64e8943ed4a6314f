"""The image patch layout of the plain front end (Spec / LogSpec / MelSpec / LogMelSpec): `layout="image"` on `Frontend.run`,
`plain_features` and `run_ragged` gives (nP, rows, W), what get_feature_patches returns and the single-task Conv2D baselines read.

The yardstick is the time-major output of the same call, pinned against tests/plain_ref.py by tests/test_plain_gpu.py: the image
patches are its permute(0, 2, 1) BIT FOR BIT (the finishing kernel forms one f32 value and only its address depends on the layout)
and the featuregram is the same bits.  One case is anchored on plain_ref directly.

Rows: 21 (MelSpec as Doukhan's baseline reads it: one partial block of the finishing kernel's 32 rows), 120, 201 (Spec, n_fft 400)
and 257 (LogSpec, n_fft 512: eight blocks and one row).  (W, shift) = (68, 34) overlapping, (68, 68) disjoint, and (249, 24) on a
one-second clip of 98 frames, which is tiled to more than W frames first so that a frame lands in several columns of a patch."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import plain_ref as pr

pytestmark = pytest.mark.gpu

# name -> (n_fft, n_mels, rows)
CONFIGS = {"Spec": (400, 0, 201), "LogSpec": (512, 0, 257), "MelSpec": (400, 21, 21), "LogMelSpec": (400, 120, 120)}
GEOMETRIES = ((68, 34), (68, 68), (249, 24))
_FE = {}


def _fe(name):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    if name not in _FE:
        n_fft, n_mels, rows = CONFIGS[name]
        _FE[name] = Frontend(FrontendConfig.from_params({"Model": "m", "Tw": 25, "Ts": 10}, n_fft, n_mels, name))
        assert _FE[name].rows == rows and not _FE[name].cfg.hpss
    return _FE[name]


def _noise(n, seed, scale=1.0):
    return (scale * 0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _same(img, tm, rows, W, what):
    assert tuple(img.shape) == (tm.shape[0], rows, W) and tuple(tm.shape[1:]) == (W, rows), (what, img.shape, tm.shape)
    assert img.is_contiguous() and torch.equal(img, tm.permute(0, 2, 1)), what


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_run_and_plain_features_image_is_time_major_transposed(name):
    fe = _fe(name)
    rows = CONFIGS[name][2]
    # 98 and 230 frames (several 64-frame chunks, the last one partial); three clips of different loudness
    for n, B in ((16000, 3), (37200, 2)):
        audio = torch.from_numpy(np.stack([_noise(n, 10 * b + n % 97, (1.0, 1e-3, 30.0)[b]) for b in range(B)])).cuda()
        S = fe.stft_mag(audio)
        for W, shift in GEOMETRIES:
            tm = fe.run(audio, W=W, shift=shift)
            img = fe.run(audio, W=W, shift=shift, layout="image")
            assert img["n_patches"] == tm["n_patches"] > 0 and torch.equal(img["fv"], tm["fv"])
            _same(img["patches"], tm["patches"], rows, W, (name, n, W, shift, "run"))
            ftm = fe.plain_features(S, W=W, shift=shift)
            fimg = fe.plain_features(S, W=W, shift=shift, layout="image")
            assert fimg["n_patches"] == tm["n_patches"] and torch.equal(fimg["fv"], ftm["fv"]) and torch.equal(fimg["fv"], tm["fv"])
            _same(fimg["patches"], ftm["patches"], rows, W, (name, n, W, shift, "plain_features"))
            assert torch.equal(fimg["patches"], img["patches"])
    # preallocated outputs are written in place, and a stale shape is refused
    out = {"fv": torch.empty_like(fimg["fv"]), "patches": torch.full_like(fimg["patches"], -7.0)}
    again = fe.plain_features(S, W=W, shift=shift, out=out, layout="image")
    assert again["patches"] is out["patches"] and torch.equal(out["patches"], fimg["patches"])
    with pytest.raises(ValueError, match="shape"):
        fe.plain_features(S, W=W, shift=shift, out={"patches": torch.empty_like(ftm["patches"])}, layout="image")


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_ragged_image_is_time_major_transposed(name):
    fe = _fe(name)
    n_fft, _, rows = CONFIGS[name]
    lens = (399, 4000, 16000, 37123)
    clips = [_noise(n, 50 + i, (1.0, 1e-3, 30.0)[i % 3]) for i, n in enumerate(lens)]
    for layout in ("time_major", "image"):  # 399 samples give no frame: refused in either layout
        with pytest.raises(ValueError):
            fe.run_ragged(clips, W=68, shift=34, layout=layout)
    # ... and a first clip of exactly W = 68 frames gives frames but no patch (the tiling rule is `<=`); 4000 samples are tiled
    clips[0] = _noise(n_fft + 67 * 160, 50)
    for W, shift in GEOMETRIES:
        tm = fe.run_ragged(clips, W=W, shift=shift)
        img = fe.run_ragged(clips, W=W, shift=shift, layout="image")
        assert img["T"] == tm["T"] and img["n_patches"] == tm["n_patches"] and img["T"][0] == 68
        if W == 68:
            assert img["n_patches"][0] == 0 and tuple(img["patches"][0].shape) == (0, rows, W)
        assert min(img["n_patches"][1:]) > 0
        for b, c in enumerate(clips):
            assert torch.equal(img["fv"][b], tm["fv"][b]), (name, W, shift, b)
            _same(img["patches"][b], tm["patches"][b], rows, W, (name, W, shift, b, "ragged"))
        # a clip gets in a ragged call what it gets alone (the odd-length clip too: it starts on a 16-byte boundary here)
        one = fe.run(torch.from_numpy(clips[3][None]).cuda(), W=W, shift=shift, layout="image")
        assert torch.equal(one["patches"], img["patches"][3])


def test_ragged_image_from_a_clip_off_the_8_byte_boundary():
    """Device clips are laid out by run_ragged itself, so the route for a clip that starts off an 8-byte boundary (processed alone,
    through smh_plain_frontend_layout_f32) is reached through the C entry: the second clip starts at an odd sample."""
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import _ptr, _stream
    fe = _fe("MelSpec")
    rows, W, shift, B = 21, 68, 34, 2
    lens = [16001, 20000]
    offs = [0, 16001]
    host = np.concatenate([_noise(lens[0], 1), _noise(lens[1], 2)])
    audio = torch.from_numpy(host).cuda()
    h_off, h_len = (C.c_longlong * B)(*offs), (C.c_int * B)(*lens)
    fv_off, p_off = (C.c_longlong * (B + 1))(), (C.c_longlong * (B + 1))()
    hT, hnP, work = (C.c_int * B)(), (C.c_int * B)(), C.c_size_t()
    lib = fe.lib
    _lib.check(lib.smh_plain_frontend_ragged_sizes(fe._h, h_off, h_len, B, W, shift, fv_off, p_off, hT, hnP, C.byref(work)))
    wk = torch.empty(work.value, dtype=torch.uint8, device="cuda")
    got = {}
    for lay in (0, 1):
        fv = torch.empty(int(fv_off[B]), dtype=torch.float32, device="cuda")
        pt = torch.full((int(p_off[B]),) + ((rows, W) if lay == 0 else (W, rows)), -7.0, dtype=torch.float32, device="cuda")
        _lib.check(lib.smh_plain_frontend_ragged_layout_f32(fe._h, _ptr(audio), h_off, h_len, B, W, shift, lay, _ptr(fv), _ptr(pt),
                                                            _ptr(wk), wk.numel(), _stream()))
        got[lay] = (fv, pt)
    assert int(hnP[0]) > 0 and int(hnP[1]) > 0
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1].permute(0, 2, 1))
    assert not bool((got[0][1] == -7.0).any())


def test_image_patches_against_the_reference():
    """MelSpec with 21 mels, the configuration of Doukhan's baseline: the image patches against plain_ref on the device's own S, at
    the bound tests/test_plain_gpu.py applies to the time-major patches (abs 1e-4)."""
    fe = _fe("MelSpec")
    W, shift = 68, 34
    audio = np.stack([_noise(24000, 70 + b, (1.0, 1e-3, 30.0)[b]) for b in range(3)])
    res = fe.run(torch.from_numpy(audio).cuda(), W=W, shift=shift, taps=True, layout="image")
    nP = res["n_patches"]
    patches, S = res["patches"].cpu().numpy(), res["S"].cpu().numpy()
    assert patches.shape == (3 * nP, 21, W) and nP > 1
    for b in range(3):
        ref = pr.feature_patches(pr.featuregram_from_S(S[b], "MelSpec", 21, 16000), W, shift)  # time-major (nP, W, 21)
        assert ref.shape == (nP, W, 21)
        err = float(np.max(np.abs(patches[b * nP:(b + 1) * nP] - ref.transpose(0, 2, 1))))
        assert err <= 1e-4, (b, err)


def test_no_patches_and_bad_layouts():
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import _ptr, _stream
    fe = _fe("LogMelSpec")
    rows = 120
    clips = np.stack([_noise(16000, 3), _noise(16000, 4)])
    audio = torch.from_numpy(clips).cuda()
    ref = fe.run(audio)
    res = fe.run(audio, layout="image")  # no W: no patches
    assert res["n_patches"] == 0 and "patches" not in res and torch.equal(res["fv"], ref["fv"])
    rag = fe.run_ragged([clips[0], clips[1][:9000]], layout="image")
    assert rag["n_patches"] == [0, 0] and "patches" not in rag and torch.equal(rag["fv"][0], ref["fv"][0])
    S = fe.stft_mag(audio)
    assert fe.plain_features(S, layout="image")["patches"] is None
    for call in (lambda: fe.run(audio, W=68, shift=34, layout="nhwc"), lambda: fe.run_ragged([clips[0]], W=68, shift=34, layout=0),
                 lambda: fe.plain_features(S, W=68, shift=34, layout="images")):
        with pytest.raises(ValueError, match="layout"):
            call()
    with pytest.raises(TypeError, match="unexpected keyword"):
        fe.plain_features(S, W=68, shift=34, patch_layout="image")
    # the C entries: SMH_E_INVALID with a text, and nothing launched -- the outputs keep their fill
    lib, h = fe.lib, fe._h
    B, N, T, W = 2, 16000, 98, 68
    nP = fe.num_patches(T, W, 34)
    fv = torch.full((B, rows, T), -7.0, device="cuda")
    pt = torch.full((B * nP, rows, W), -7.0, device="cuda")
    wk = torch.empty(max(lib.smh_plain_frontend_workspace_bytes(h, B, N), 1 << 20), dtype=torch.uint8, device="cuda")
    keys = torch.zeros(B, dtype=torch.int32, device="cuda")
    h_off, h_len = (C.c_longlong * B)(0, N), (C.c_int * B)(N, N)
    for bad in (2, -1):
        rcs = [lib.smh_plain_frontend_layout_f32(h, _ptr(audio), B, N, W, 34, bad, _ptr(fv), _ptr(pt), _ptr(wk), wk.numel(), None, _stream()),
               lib.smh_plain_features_layout_f32(h, _ptr(S), B, T, W, 34, bad, _ptr(fv), _ptr(pt), _ptr(keys), _stream()),
               lib.smh_plain_frontend_ragged_layout_f32(h, _ptr(audio), h_off, h_len, B, W, 34, bad, _ptr(fv), _ptr(pt), _ptr(wk),
                                                        wk.numel(), _stream())]
        for rc in rcs:
            assert rc == _lib.SMH_E_INVALID
            assert "patch_layout" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((fv == -7.0).all()) and bool((pt == -7.0).all())


# ---- the device generator with the single-task Conv2D baselines' configurations (Baseline_Results.py) --------------------------------
W = 68
# Model -> (featName, n_fft, n_mels, rows of the image)
MODELS = {"Doukhan_et_al": ("MelSpec", 400, 21, 21), "Papakostas_et_al": ("Spec", 400, 120, 201), "Jang_et_al": ("LogSpec", 512, 120, 257)}


def _params(tmp, sub, model, like, classes=3):
    feat, n_fft, n_mels, _ = MODELS[like]
    cl = {0: "music", 1: "speech", 2: "speech_music"} if classes == 3 else {0: "music", 1: "speech"}
    return {"Model": model, "classes": cl, "feature_opDir": str(tmp / sub), "W": W, "W_shift": 34, "n_fft": {model: n_fft},
            "n_mels": {model: n_mels}, "featName": {model: feat}, "frame_level_scaling": False, "skewness_vector": None,
            "data_augmentation_with_noise": False, "Tw": 25, "Ts": 10}


def _dataset(tmp):
    from sm_hpss_mtl_amd.synth import synth_clips
    folder = tmp / "data"
    names = {"speech": [], "music": []}
    lens = {"speech": (6400, 14000, 30000), "music": (9000, 20000, 12000)}  # 0.4 s: shorter than a patch, tiled
    for cls in names:
        os.makedirs(folder / cls, exist_ok=True)
        for i, n in enumerate(lens[cls]):
            name = "%s%02d.npy" % (cls[:2], i)
            np.save(folder / cls / name, synth_clips(1, seed=40 + 7 * i + (0 if cls == "speech" else 100), n_samples=n)[0])
            names[cls].append(name)
    mix = [{"speech": names["speech"][i % 3], "music": names["music"][(i + 1) % 3], "SMR": [-5, 0, 10, 20][i % 4]} for i in range(4)]
    return str(folder), {"speech": names["speech"], "music": names["music"], "speech+music": mix}


def _first(P, folder, files, seed=7):
    from sm_hpss_mtl_amd import generators as gen
    np.random.seed(seed)
    return next(gen.generator(P, folder, copy.deepcopy(files), 2))


@pytest.mark.parametrize("classes", [3, 2])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_generator_serves_the_single_task_baselines_from_the_device(tmp_path, model, classes):
    """(N, rows, W, 1) device batches and the one-hot lab['3C'], as for 'Lemaire_et_al'.  Yardstick: the same PARAMS under the name
    'Lemaire_et_al' (the time-major plain device path, tests/test_plain_gpu.py) with the same numpy seed in front of both; a second
    pass is served from the featuregram cache (standardize_rows + extract_patches, which divide where the fused kernel multiplies by
    1 / scale: within the 2e-4 tests/test_ragged_gpu.py allows between those routes)."""
    folder, files = _dataset(tmp_path)
    rows = MODELS[model][3]
    Pc, Pl = _params(tmp_path, "feat_cnn", model, model, classes), _params(tmp_path, "feat_tcn", "Lemaire_et_al", model, classes)
    xc, yc = _first(Pc, folder, files)
    xl, yl = _first(Pl, folder, files)
    N = classes * 2
    assert isinstance(xc, torch.Tensor) and xc.is_cuda and xc.dtype == torch.float32 and tuple(xc.shape) == (N, rows, W, 1)
    assert tuple(xl.shape) == (N, W, rows) and torch.equal(xc[..., 0], xl.permute(0, 2, 1))
    yc = np.asarray(yc)
    assert yc.shape == (N, classes) and np.array_equal(yc, np.asarray(yl))
    assert np.array_equal(yc.argmax(1), np.repeat(np.arange(classes), 2)) and yc.sum() == N
    assert len(list((tmp_path / "feat_cnn").rglob("*.npy"))) > 0
    xc2, yc2 = _first(Pc, folder, files)
    xl2, _ = _first(Pl, folder, files)
    assert tuple(xc2.shape) == (N, rows, W, 1) and torch.equal(xc2[..., 0], xl2.permute(0, 2, 1))
    assert float((xc2 - xc).abs().max()) <= 2e-4 and np.array_equal(np.asarray(yc2), yc)


@pytest.mark.parametrize("classes", [3, 2])
def test_doukhan_model_takes_the_generator_batches(tmp_path, classes):
    """PARAMS['Model'] = 'Doukhan_et_al', MelSpec with 21 mels: the model get_Doukhan_model builds from the SAME PARAMS takes the
    generator's device batch (N, 21, 68, 1) and its lab['3C'] -- for two classes the music / speech rows alone -- in `predict`,
    `train_on_batch` and `fit`."""
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.lib.baseline_architectures import get_Doukhan_model
    folder, files = _dataset(tmp_path)
    model = "Doukhan_et_al"
    P = _params(tmp_path, "feat_fit", model, model, classes)
    P["input_shape"] = {model: (21, W, 1)}
    net, lr = get_Doukhan_model(P, n_classes=classes, seed=0)
    assert lr == pytest.approx(1e-4) and net.n_classes == classes
    x, y = _first(P, folder, files)
    N = 2 * classes
    assert x.is_cuda and tuple(x.shape) == (N, 21, W, 1) and np.asarray(y).shape == (N, classes)
    dev = net.predict(x)
    assert isinstance(dev, np.ndarray) and dev.shape == (N, classes) and np.isfinite(dev).all() and np.allclose(dev.sum(1), 1.0, atol=1e-5)
    assert np.array_equal(dev, net.predict(x.cpu().numpy()))
    before = net.get_weights_dict()["dense/kernel"].copy()
    loss, acc = net.train_on_batch(x, y)
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and net.iterations == 1
    assert np.abs(net.get_weights_dict()["dense/kernel"] - before).max() > 0
    after = net.predict(x)
    assert after.shape == (N, classes) and np.isfinite(after).all() and not np.array_equal(after, dev)
    ev = net.evaluate(x, y)
    assert len(ev) == 2 and np.isfinite(ev).all()
    np.random.seed(7)
    h = net.fit(gen.generator(P, folder, copy.deepcopy(files), 2), steps_per_epoch=2, epochs=1, verbose=0)
    assert np.isfinite(h.history["loss"]).all() and net.iterations == 3
    torch.cuda.synchronize()
    # the front end's rows must match the model's input height: a mismatch is the model's shape error, not a fault
    P201 = _params(tmp_path, "feat_201", model, "Papakostas_et_al", classes)
    x201, _ = _first(P201, folder, files)
    with pytest.raises(ValueError, match="expected input"):
        net.predict(x201)


def test_file_wise_generator_rows_equal_get_feature_patches(tmp_path):
    """PARAMS['Model'] = 'Doukhan_et_al', MelSpec with 21 mels: every patch of a file at the hard-coded shift 68, (nP, 21, 68, 1),
    equal to what the ragged call gives the conditioned signal and -- within 2e-4, the cached-featuregram route's bound -- to
    lib.preprocessing.get_feature_patches of the file's featuregram."""
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.frontend import FrontendConfig
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    folder, files = _dataset(tmp_path)
    model = "Doukhan_et_al"
    P = _params(tmp_path, "feat", model, model)
    sp, mu = folder + "/speech/" + files["speech"][2], folder + "/music/" + files["music"][1]
    fe = pp._frontend_for(FrontendConfig.from_params(P, 400, 21, "MelSpec"))
    for args, lab in (((sp, "", None), 1), (("", mu, None), 0), ((sp, mu, 10), 2)):
        x, y = gen.test_file_wise_generator(P, *args)
        if lab == 2:
            audio = pp.mix_signals(pp.load_and_preprocess_signal(sp, 25, 10)[0], pp.load_and_preprocess_signal(mu, 25, 10)[0], 10)
        else:
            audio = pp.load_and_preprocess_signal(sp if lab == 1 else mu, 25, 10)[0]
        res = fe.run_ragged([np.ascontiguousarray(audio, dtype=np.float32)], W=W, shift=68, layout="image")
        want = res["patches"][0]
        assert x.is_cuda and x.shape[0] > 0 and tuple(x.shape) == (want.shape[0], 21, W, 1) and torch.equal(x[..., 0], want)
        assert y.shape == (x.shape[0], 3) and np.all(y[:, lab] == 1) and y.sum() == x.shape[0]
        host = pp.get_feature_patches(P, res["fv"][0].cpu().numpy(), W, 68, "MelSpec")
        assert host.shape == tuple(x.shape) and float(np.max(np.abs(host - x.cpu().numpy()))) <= 2e-4
    assert not os.path.exists(tmp_path / "feat" / "speech")  # save_feat=False
