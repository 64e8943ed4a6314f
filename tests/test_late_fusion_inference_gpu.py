"""GPU: the late-fusion ensemble's inference without materialised input halves -- from the feature kernel's per-half layer-0 partials
(smh_late_fusion_forward_x0_f32: Frontend.features_l0 -> LateFusion.forward_from_x0_halves, pipeline.HotPath), dense file-level
inference on a whole H||P featuregram (smh_late_fusion_forward_dense_f32: LateFusion.forward_dense, inference.patch_probabilities)
and the driver's file-wise test loop (late_fusion.predict_file / test_model).

Bounds: against the float64 reference of tests/late_fusion_ref.py and between two device paths whose layer 0 sums in different
orders, |diff| <= 1e-4 * max(1, |ref|) -- the bound of tests/test_late_fusion_gpu.py; labels where the top-two margin exceeds 2e-4."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import late_fusion_ref as lref
from tests.test_late_fusion_gpu import make_pair, np_blend

pytestmark = pytest.mark.gpu


def at_end_of_buffer(x, pad=64):
    """x as a contiguous device tensor whose last element is the last element of its data, with NaN in the `pad` floats that follow
    (the helper of tests/test_model_shapes_gpu.py): a kernel that reads past its input turns outputs into NaN, without a fault."""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.full((x.size + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:x.size] = torch.from_numpy(x.ravel()).cuda()
    return buf[:x.size].view(x.shape)


def _clips(B, seed):
    """B one-second clips: the synthetic speech / music / noise clips with white noise of a random level on top."""
    from sm_hpss_mtl_amd.synth import synth_clips
    rng = np.random.default_rng(seed)
    y = synth_clips(B, seed=seed)
    return (y + rng.standard_normal(y.shape) * rng.uniform(0.0, 0.1, (B, 1))).astype(np.float32)


def _close(a, b, what):
    a, b = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (a, b))
    err, bound = np.abs(a - b), 1e-4 * np.maximum(1.0, np.abs(b))
    print("%s: max |diff| = %.3g" % (what, err.max() if err.size else 0.0))
    assert a.shape == b.shape and np.isfinite(a).all() and (err <= bound).all(), (what, err.max())


# ---------------------------------------------------------------------------------------------------
# 3. layer-0 partials
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W,ncls,n_mels", [("mtl", 68, 3, 120), ("cascaded", 99, 5, 120), ("cascaded", 68, 3, 40), ("mtl", 99, 5, 40)])
def test_x0_halves_match_reference_on_the_patches(kind, W, ncls, n_mels):
    """features_l0(model=ensemble) on the device's own S / harm / perc -> forward_from_x0_halves, against the float64 reference on the
    halves of the patches the same call returned.  One patch per clip (hop = W), so B * nP = B."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    fe = Frontend(FrontendConfig(n_mels=n_mels))
    ens, mH, mP, wH, wP = make_pair(kind, W, ncls, n_mels, seed=W + n_mels)
    ens.alpha = 0.3
    for B in (1, 3, 16, 17, 257):
        audio = torch.from_numpy(_clips(B, seed=B + W)).cuda()
        taps = fe.run(audio, taps=True)
        res = fe.features_l0(taps["S"], taps["harm"], taps["perc"], 0, W, W, ens, patches=True)
        assert res["n_patches"] == 1 and tuple(res["x0p"].shape) == (B, 2, W, 32)
        labels = torch.empty((B,), dtype=torch.int32, device="cuda")
        got = ens.forward_from_x0_halves(res["x0p"], labels=labels)
        ens.check_status()
        p = res["patches"].cpu().numpy()
        assert p.shape == (B, W, 2 * n_mels) and np.isfinite(p).all()
        ref = lref.forward(kind, p[:, :, :n_mels], p[:, :, n_mels:], wH, wP, 0.3, ncls)
        # (front-end patches are not drawn for their margins: the cap on left-out patches is the reference's own business here)
        keep = ref["margin"] > lref.MARGIN
        _close(got, ref["pred"], "x0 halves %s W=%d ncls=%d n_mels=%d B=%d" % (kind, W, ncls, n_mels, B))
        assert np.array_equal(labels.cpu().numpy()[keep], ref["labels"][keep]) and keep.mean() >= 0.99
        # and the device's own patch path on the same halves
        dev = ens.forward_device([res["patches"][:, :, :n_mels], res["patches"][:, :, n_mels:]])
        _close(got, dev, "x0 halves against forward_device B=%d" % B)


def _read_w0(ens):
    """The (2 * n_feat, 32) array behind w0_ptr(), read back with a device-to-device copy."""
    ptr = ens.w0_ptr()
    assert ptr
    dst = torch.empty((2 * ens.n_feat, 32), device="cuda")
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(ptr), dst.numel() * 4, 3) == 0  # hipMemcpyDeviceToDevice
    return dst.cpu().numpy()


def _w0_of(*ws):
    return np.concatenate([np.asarray(w["tcn/initial_conv/kernel"], np.float32).reshape(-1, 32) for w in ws])


def test_w0_ptr_holds_both_kernels_and_follows_either_model():
    ens, mH, mP, wH, wP = make_pair("mtl", 68, 3, 120, seed=1)
    assert np.array_equal(_read_w0(ens), _w0_of(wH, wP)) and not np.array_equal(_w0_of(wH), _w0_of(wP))
    x0p = torch.randn((5, 2, 68, 32), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    before = ens.forward_from_x0_halves(x0p).clone()
    wH2, wP2 = lref.init_weights("mtl", 31, 120, 68, 3)
    mP.set_weights_dict(wP2)
    assert np.array_equal(_read_w0(ens), _w0_of(wH, wP2))
    mH.set_weights_dict(wH2)
    assert np.array_equal(_read_w0(ens), _w0_of(wH2, wP2))
    assert not torch.equal(before, ens.forward_from_x0_halves(x0p))
    # a training step of one model moves its kernel on the device: the array follows
    rng = np.random.default_rng(0)
    N = 12
    x = rng.standard_normal((N, 68, 120)).astype(np.float32)
    cls = rng.integers(0, 3, N)
    y = {"S": (cls == 1).astype(np.float32)[:, None], "M": (cls == 0).astype(np.float32)[:, None],
         "R": rng.random((N, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[cls]}
    mH.compile()
    mH.train_on_batch(x, y, drop_tcn=None, drop_heads=None, apply=True)
    after = mH.get_weights_dict()
    assert not np.array_equal(_w0_of(after), _w0_of(wH2))
    assert np.array_equal(_read_w0(ens), _w0_of(after, wP2))
    ens.check_status()


# ---------------------------------------------------------------------------------------------------
# 4. dense
# ---------------------------------------------------------------------------------------------------
# (68, 1, 2300): 2233 patches and (25, 7, 15000): 2140 -- past one 2048-patch chunk; (68, 68, 5000): hop = W; (68, 1, 69): one patch
@pytest.mark.parametrize("kind,W,shift,Tc", [("mtl", 68, 1, 69), ("mtl", 68, 1, 2300), ("cascaded", 68, 7, 700), ("cascaded", 25, 7, 15000),
                                             ("mtl", 68, 68, 5000), ("cascaded", 99, 99, 1000), ("mtl", 99, 1, 1000)])
def test_dense_matches_forward_device_on_built_patches(kind, W, shift, Tc, monkeypatch):
    F, ncls, alpha = 120, 3, 0.3
    ens, mH, mP, wH, wP = make_pair(kind, W, ncls, F, seed=W + shift)
    ens.alpha = alpha
    rng = np.random.default_rng(W + shift + Tc)
    fv = rng.standard_normal((2 * F, Tc)).astype(np.float32)
    starts = ofe.patch_starts(Tc, W, shift)
    nP = ens.lib.smh_num_patches(Tc, W, shift)
    assert nP == len(starts) and nP > 0
    labels = torch.full((nP,), -1, dtype=torch.int32, device="cuda")
    heads = torch.full((2, nP, mH.out_dim), float("nan"), device="cuda")
    got = ens.forward_dense(at_end_of_buffer(fv), shift, labels=labels, heads=heads)
    ens.check_status()
    assert tuple(got.shape) == (nP, ncls)
    dfv = torch.from_numpy(fv).cuda()
    x = torch.stack([dfv[:, s:s + W].T for s in starts])  # (nP, W, 2F): the built patches
    dlab = torch.empty((nP,), dtype=torch.int32, device="cuda")
    dheads = torch.empty((2, nP, mH.out_dim), device="cuda")
    dev = ens.forward_device([x[:, :, :F].contiguous(), x[:, :, F:].contiguous()], labels=dlab, heads=dheads)
    _close(got, dev, "dense %s W=%d shift=%d Tc=%d" % (kind, W, shift, Tc))
    _close(heads, dheads, "dense heads")
    # pred and labels are the blend of the heads the same call returned, bit for bit
    h = heads.cpu().numpy()
    want = np_blend(h[0], h[1], alpha, ncls)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(labels.cpu().numpy(), np.argmax(want, axis=1))
    # the float64 reference on a subset: both ends and both sides of every chunk boundary
    edges = [np.arange(c - 3, c + 3) for c in range(2048, nP, 2048)]
    sel = np.unique(np.concatenate([np.arange(0, nP, max(1, nP // 40)), np.arange(min(nP, 5)), np.arange(max(nP - 5, 0), nP)] + edges))
    xs = x[torch.from_numpy(sel).cuda()].cpu().numpy()
    ref = lref.forward(kind, xs[:, :, :F], xs[:, :, F:], wH, wP, alpha, ncls)
    _close(got.cpu().numpy()[sel], ref["pred"], "dense against the float64 reference")
    keep = ref["margin"] > lref.MARGIN
    assert np.array_equal(labels.cpu().numpy()[sel][keep], ref["labels"][keep])
    # the paired launch and two launches agree bit for bit, without the optional outputs too
    monkeypatch.setenv("SMH_LATE_FUSION_TWO_LAUNCH", "1")
    two = ens.forward_dense(at_end_of_buffer(fv), shift)
    monkeypatch.delenv("SMH_LATE_FUSION_TWO_LAUNCH")
    assert torch.equal(got, two)


def test_dense_edges():
    ens, _, _, _, _ = make_pair("mtl", 68, 3, 120, seed=2)
    e = ens.forward_dense(torch.zeros((240, 68), device="cuda"))  # Tc = W, even W: no patch
    assert tuple(e.shape) == (0, 3)
    with pytest.raises(ValueError):
        ens.forward_dense(torch.zeros((120, 200), device="cuda"))
    with pytest.raises(ValueError):
        ens.forward_dense(torch.zeros((240, 67), device="cuda"))
    with pytest.raises(ValueError):
        ens.forward_dense(torch.zeros((240, 200), device="cuda"), shift=0)
    with pytest.raises((TypeError, ValueError)):
        ens.forward_dense(torch.zeros((240, 200)))
    with pytest.raises(ValueError):
        ens.forward_from_x0_halves(torch.zeros((2, 2, 99, 32), device="cuda"))
    e = ens.forward_from_x0_halves(torch.empty((0, 2, 68, 32), device="cuda"))
    assert tuple(e.shape) == (0, 3)
    fv = at_end_of_buffer(np.random.default_rng(1).standard_normal((240, 333)))
    a, b = ens.forward_dense(fv, 5).clone(), ens.forward_dense(fv, 5).clone()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    ens.check_status()


def test_patch_probabilities_dense_and_patch_tracks_agree(monkeypatch):
    from sm_hpss_mtl_amd import inference as inf
    ens, _, _, wH, wP = make_pair("mtl", 68, 3, 120, seed=4)
    rng = np.random.default_rng(8)
    fv = (rng.standard_normal((240, 3000)) * rng.uniform(0.5, 2.0, (240, 1)) + rng.normal(0, 1, (240, 1))).astype(np.float32)
    monkeypatch.delenv("SMH_DENSE_PATCHES", raising=False)
    dense = inf.patch_probabilities(fv, ens, 68, 1, output="3C", batch_frames=1100)
    monkeypatch.setenv("SMH_DENSE_PATCHES", "1")
    built = inf.patch_probabilities(fv, ens, 68, 1, output="3C", batch_frames=1100)
    monkeypatch.delenv("SMH_DENSE_PATCHES")
    n = 2 * len(ofe.patch_starts(1100, 68, 1)) + len(ofe.patch_starts(800, 68, 1))
    assert dense.shape == built.shape == (n, 3) and dense.dtype == np.float32
    _close(dense, built, "patch_probabilities: dense against patch track")
    assert np.allclose(dense.sum(1), 1.0, atol=1e-5)
    # the first batch against the float64 reference: get_feature_patches standardises each half over the batch
    whole = (fv.astype(np.float64) - fv.mean(1, keepdims=True)) / fv.std(1, keepdims=True)
    chunk = whole[:, :1100]
    chunk = ((chunk - chunk.mean(1, keepdims=True)) / chunk.std(1, keepdims=True)).astype(np.float32)
    sel = range(0, 1032, 40)
    x = np.stack([chunk[:, s:s + 68].T for s in sel])
    ref = lref.forward("mtl", x[:, :, :120], x[:, :, 120:], wH, wP, 0.5, 3)
    _close(dense[0:1032:40], ref["pred"], "patch_probabilities against the float64 reference")
    with pytest.raises(ValueError):
        inf.patch_probabilities(fv, ens, 68, 1, output="S")
    with pytest.raises(ValueError):  # a W the ensemble was not built for takes the patch path, which refuses it
        inf.patch_probabilities(fv, ens, 99, 1, output="3C")


# ---------------------------------------------------------------------------------------------------
# 5. pipeline
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 48])
def test_hotpath_with_an_ensemble(B):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.pipeline import HotPath
    from sm_hpss_mtl_amd.synth import synth_clips
    fe = Frontend(FrontendConfig())
    ens, mH, mP, wH, wP = make_pair("mtl", 68, 3, 120, seed=6)
    audio = torch.from_numpy(synth_clips(B, seed=4)).cuda()
    fused = HotPath(fe, ens, batch=B, n_samples=16000, keep_patches=True)
    plain = HotPath(fe, ens, batch=B, n_samples=16000, keep_patches=True, fuse_l0=False)
    assert fused.fuse_l0 and not plain.fuse_l0
    a, b = fused.step(audio).clone(), plain.step(audio).clone()
    ens.check_status()
    assert tuple(a.shape) == tuple(b.shape) == (B * fused.nP, 3) and torch.isfinite(a).all()
    assert torch.equal(fused.patches, plain.patches)
    # the HotPath-free paths: features_l0 -> forward_from_x0_halves, and forward_device on the halves of the patches
    # (on the spectrogram and medians the step left behind, in the layout its median launch wrote: the feature kernel's route and
    # with it the last bits of the patches follow the layout)
    res = fe.features_l0(fused.S, fused.harm, fused.perc, fused.layout, 68, 68, ens, patches=True)
    assert torch.equal(res["patches"], fused.patches)
    assert torch.equal(a, ens.forward_from_x0_halves(res["x0p"]))
    assert torch.equal(b, ens.forward_device([plain.patches[:, :, :120], plain.patches[:, :, 120:]]))
    _close(a, b, "HotPath fuse_l0 True / False")
    p = plain.patches.cpu().numpy()
    ref = lref.forward("mtl", p[:, :, :120], p[:, :, 120:], wH, wP, 0.5, 3)
    _close(a, ref["pred"], "HotPath fused B=%d against the float64 reference" % B)
    with pytest.raises(ValueError, match="trunk"):
        HotPath(fe, ens, batch=B, n_samples=16000, keep_trunk=True)
    with pytest.raises(ValueError, match="f32"):
        HotPath(fe, ens, batch=B, n_samples=16000, model_dtype="bf16")
    with pytest.raises(ValueError):
        HotPath(fe, ens, batch=B, n_samples=16000, patch=99)
    with pytest.raises(ValueError):
        HotPath(Frontend(FrontendConfig(n_mels=40)), ens, batch=B, n_samples=16000)


# ---------------------------------------------------------------------------------------------------
# 7. predict_file / test_model
# ---------------------------------------------------------------------------------------------------
M = "Lemaire_et_al_MTL"


def _write_wavs(tmp):
    """Two speech-like and two music-like three-second WAVs (16 kHz, int16) under <tmp>/data/<class>/."""
    from scipy.io import wavfile

    from sm_hpss_mtl_amd.synth import synth_clips
    clips = synth_clips(12, seed=21)
    rng = np.random.default_rng(3)
    names = {"speech": ["sp0.wav", "sp1.wav"], "music": ["mu0.wav", "mu1.wav"]}
    k = 0
    for cls, ns in names.items():
        os.makedirs(tmp / "data" / cls, exist_ok=True)
        for n in ns:
            y = np.concatenate([clips[k], clips[k + 1], clips[k + 2]]) + 0.01 * rng.standard_normal(48000)
            k += 3
            wavfile.write(str(tmp / "data" / cls / n), 16000, np.int16(np.clip(y / np.abs(y).max(), -1, 1) * 30000))
    return str(tmp / "data"), names


def _params(tmp, folder, names):
    return {"Model": M, "classes": {0: "music", 1: "speech", 2: "speech_music"}, "folder": folder, "W": 68, "W_shift": 68,
            "feature_opDir_H": str(tmp / "feat_H"), "feature_opDir_P": str(tmp / "feat_P"), "n_fft": {M: 400}, "n_mels": {M: 120},
            "l_harm": {M: 21}, "l_perc": {M: 11}, "featName": {M: ["LogMelHarmSpec", "LogMelPercSpec"]}, "Tw": 25, "Ts": 10,
            "frame_level_scaling": False, "skewness_vector": None, "late_fusion_alpha": 0.3,
            "test_files": {"speech": names["speech"], "music": names["music"],
                           "speech+music": [{"speech": "sp0.wav", "music": "mu1.wav", "SMR": 0},
                                            {"speech": "sp1.wav", "music": "mu0.wav", "SMR": 10}]}}


def _two_call_form(PARAMS, tmp, mH, mP, sp, mu, dB):
    """The driver's own steps (:393-399, 412-423): test_file_wise_generator per model on its half feature, predict, numpy blend."""
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    preds = []
    for i, (model, side) in enumerate(((mH, "H"), (mP, "P"))):
        P = copy.deepcopy(PARAMS)
        P["featName"][M] = PARAMS["featName"][M][i]
        P["feature_opDir"] = str(tmp / ("two_call_" + side))
        x, _ = gen.test_file_wise_generator(P, sp, mu, dB, featuregram_fn=pp.get_featuregram, patches_fn=pp.get_feature_patches)
        preds.append(model.predict(x)[-1])
    a = PARAMS["late_fusion_alpha"]
    pred = np.add(a * preds[0], (1 - a) * preds[1])
    return pred, np.argmax(pred, axis=1)


def test_predict_file_and_test_model(tmp_path, monkeypatch):
    from sm_hpss_mtl_amd import late_fusion as lf
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    folder, names = _write_wavs(tmp_path)
    PARAMS = _params(tmp_path, folder, names)
    ens, mH, mP, _, _ = make_pair("mtl", 68, 3, 120, seed=8)
    calls = []
    real = pp.featuregram_from_signal

    def counting(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    sp0, mu0 = folder + "/speech/sp0.wav", folder + "/music/mu0.wav"
    files = [(sp0, "", None), ("", mu0, None), (sp0, folder + "/music/mu1.wav", 0), (folder + "/speech/sp1.wav", mu0, 10)]
    want = [_two_call_form(PARAMS, tmp_path, mH, mP, *f) for f in files]
    monkeypatch.setattr(pp, "featuregram_from_signal", counting)
    for f, (wp, wl) in zip(files, want):
        n0 = len(calls)
        pred, lab = lf.predict_file(PARAMS, ens, *f)
        assert len(calls) == n0 + 1, "one featuregram computation per file"
        assert ens.alpha == 0.5, "PARAMS' alpha holds for the call only"
        assert pred.dtype == np.float32 and pred.shape == wp.shape and pred.shape[0] >= 1
        assert np.array_equal(pred, wp) and np.array_equal(lab, wl), f
        pred2, _ = lf.predict_file(PARAMS, ens, *f)  # the H cache now holds it
        assert len(calls) == n0 + 1 and np.array_equal(pred2, pred)
    assert sorted(os.listdir(tmp_path / "feat_H")) == ["music", "speech", "speech_music"] and not os.path.exists(tmp_path / "feat_P")

    # test_model: music, speech, then the pairs at their annotated SMR
    PARAMS["feature_opDir_H"] = str(tmp_path / "feat_H2")
    n0 = len(calls)
    PtdLabels, Predictions, GroundTruth, ConfMat = lf.test_model(PARAMS, ens, None)
    assert len(calls) == n0 + 6
    order = ([("", folder + "/music/" + n, None, 0) for n in names["music"]] + [(folder + "/speech/" + n, "", None, 1) for n in names["speech"]]
             + [(folder + "/speech/" + i["speech"], folder + "/music/" + i["music"], i["SMR"], 2) for i in PARAMS["test_files"]["speech+music"]])
    exp = [_two_call_form(PARAMS, tmp_path, mH, mP, *o[:3]) for o in order]
    assert np.array_equal(Predictions, np.concatenate([e[0] for e in exp])) and np.array_equal(PtdLabels, np.concatenate([e[1] for e in exp]))
    truth = np.concatenate([np.full(len(e[1]), o[3]) for e, o in zip(exp, order)])
    assert np.array_equal(GroundTruth, truth)
    assert ConfMat.shape == (3, 3) and ConfMat.sum() == len(truth)
    for i in range(3):
        for j in range(3):
            assert ConfMat[i, j] == int(((truth == i) & (PtdLabels == j)).sum())
    # a target SMR: the pairs alone, mixed at that ratio
    PtdLabels5, Predictions5, GroundTruth5, _ = lf.test_model(PARAMS, ens, 5)
    exp5 = [_two_call_form(PARAMS, tmp_path, mH, mP, o[0], o[1], 5) for o in order[4:]]
    assert np.array_equal(Predictions5, np.concatenate([e[0] for e in exp5])) and np.all(GroundTruth5 == 2)
    assert len(PtdLabels5) == len(Predictions5)
    # refusals of the PARAMS surface
    bad = copy.deepcopy(PARAMS)
    bad["featName"][M] = "LogMelHarmPercSpec"
    with pytest.raises(ValueError):
        lf.predict_file(bad, ens, sp0, "", None)
    bad["featName"][M] = ["LogMelPercSpec", "LogMelHarmSpec"]
    with pytest.raises(ValueError):
        lf.predict_file(bad, ens, sp0, "", None)
    bad = copy.deepcopy(PARAMS)
    bad["late_fusion_alpha"] = 1.5
    with pytest.raises(ValueError):
        lf.predict_file(bad, ens, sp0, "", None)
