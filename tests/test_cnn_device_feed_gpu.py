"""The Conv2D MTL models fed from the device front end: `generators.generator` / `test_file_wise_generator` with
PARAMS['Model'] = Doukhan_et_al_MTL / Papakostas_et_al_MTL / Jang_et_al_MTL yield (N, 2F, W, 1) CUDA batches written in that layout
by the front end's kernels.

The yardstick is the same PARAMS under the name 'Lemaire_et_al_MTL' (the time-major device path, pinned against the reference's
sequential loop by tests/test_ragged_gpu.py): with the same numpy seed in front of both, the Conv2D batch is the Lemaire batch's
permute(0, 2, 1) bit for bit, and the labels are equal.  A second pass, served from the featuregram cache, takes other kernels
(standardize_rows + extract_patches, whose scaler divides where the fused kernels multiply by 1 / scale): it equals the cached
Lemaire pass bit for bit and the first pass within the 2e-4 tests/test_ragged_gpu.py allows between those two routes.

Files: .npy audio of different lengths under a temporary folder, one of them (0.4 s) shorter than a patch, one beyond the LDS image."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W = 68
# Model -> (featName, n_fft, n_mels, rows of the image)
MODELS = {"Doukhan_et_al_MTL": ("MelHarmPercSpec", 400, 120, 240),
          "Papakostas_et_al_MTL": ("HarmPercSpec", 400, 120, 402),
          "Jang_et_al_MTL": ("LogHarmPercSpec", 512, 120, 514)}


def _params(tmp, sub, model, like):
    """PARAMS of `model` with the feature configuration of the Conv2D model `like` (its own, or -- for the Lemaire twin -- borrowed)."""
    feat, n_fft, n_mels, _ = MODELS[like]
    return {"Model": model, "classes": {0: "music", 1: "speech", 2: "speech_music"}, "feature_opDir": str(tmp / sub), "W": W, "W_shift": 34,
            "n_fft": {model: n_fft}, "n_mels": {model: n_mels}, "featName": {model: feat}, "frame_level_scaling": False,
            "skewness_vector": None, "data_augmentation_with_noise": False, "Tw": 25, "Ts": 10, "l_harm": {model: 21}, "l_perc": {model: 11}}


def _dataset(tmp):
    from sm_hpss_mtl_amd.synth import synth_clips
    folder = tmp / "data"
    names = {"speech": [], "music": []}
    lens = {"speech": (6400, 14000, 30000), "music": (9000, 20000, 12000)}  # 0.4 s: shorter than a patch; 30000: beyond the LDS image
    for cls in names:
        os.makedirs(folder / cls, exist_ok=True)
        for i, n in enumerate(lens[cls]):
            name = "%s%02d.npy" % (cls[:2], i)
            np.save(folder / cls / name, synth_clips(1, seed=40 + 7 * i + (0 if cls == "speech" else 100), n_samples=n)[0])
            names[cls].append(name)
    mix = [{"speech": names["speech"][i % 3], "music": names["music"][(i + 1) % 3], "SMR": [-5, 0, 10, 20][i % 4]} for i in range(4)]
    return str(folder), {"speech": names["speech"], "music": names["music"], "speech+music": mix}


def _first(P, folder, files, seed=7, n=1, **kw):
    from sm_hpss_mtl_amd import generators as gen
    np.random.seed(seed)
    g = gen.generator(P, folder, copy.deepcopy(files), 2, **kw)
    return [next(g) for _ in range(n)]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_generator_serves_the_conv2d_models_from_the_device(tmp_path, model):
    folder, files = _dataset(tmp_path)
    rows = MODELS[model][3]
    Pc, Pl = _params(tmp_path, "feat_cnn", model, model), _params(tmp_path, "feat_tcn", "Lemaire_et_al_MTL", model)
    (xc, yc), = _first(Pc, folder, files)
    (xl, yl), = _first(Pl, folder, files)
    assert isinstance(xc, torch.Tensor) and xc.is_cuda and xc.dtype == torch.float32 and tuple(xc.shape) == (6, rows, W, 1)
    assert tuple(xl.shape) == (6, W, rows)
    assert torch.equal(xc[..., 0], xl.permute(0, 2, 1))
    assert sorted(yc) == sorted(yl) == ["3C", "M", "R", "S"]
    for k in yc:
        np.testing.assert_array_equal(np.asarray(yc[k]), np.asarray(yl[k]))
    # second pass: every file of the batch now has its featuregram in the cache (the .npy file and its device copy)
    assert len(list((tmp_path / "feat_cnn").rglob("*.npy"))) > 0
    (xc2, yc2), = _first(Pc, folder, files)
    (xl2, _), = _first(Pl, folder, files)
    assert tuple(xc2.shape) == (6, rows, W, 1) and torch.equal(xc2[..., 0], xl2.permute(0, 2, 1))
    assert float((xc2 - xc).abs().max()) <= 2e-4
    for k in yc:
        np.testing.assert_array_equal(np.asarray(yc[k]), np.asarray(yc2[k]))


def test_file_wise_generator_serves_images_at_the_hard_coded_shift(tmp_path):
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.frontend import FrontendConfig
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    folder, files = _dataset(tmp_path)
    model = "Doukhan_et_al_MTL"
    Pc, Pl = _params(tmp_path, "feat", model, model), _params(tmp_path, "feat", "Lemaire_et_al_MTL", model)
    sp, mu = folder + "/speech/" + files["speech"][2], folder + "/music/" + files["music"][1]
    fe = pp._frontend_for(FrontendConfig.from_params(Pc, 400, 120, "MelHarmPercSpec"))
    for args, lab in (((sp, "", None), 1), (("", mu, None), 0), ((sp, mu, 10), 2)):
        x, y = gen.test_file_wise_generator(Pc, *args)
        xl, yl = gen.test_file_wise_generator(Pl, *args)
        if lab == 2:
            audio = pp.mix_signals(pp.load_and_preprocess_signal(sp, 25, 10)[0], pp.load_and_preprocess_signal(mu, 25, 10)[0], 10)
        else:
            audio = pp.load_and_preprocess_signal(sp if lab == 1 else mu, 25, 10)[0]
        want = fe.run_ragged([np.ascontiguousarray(audio, dtype=np.float32)], W=W, shift=68, layout="image")["patches"][0]
        assert x.is_cuda and x.shape[0] > 0 and tuple(x.shape) == (want.shape[0], 240, W, 1)
        assert torch.equal(x[..., 0], want) and torch.equal(x[..., 0], xl.permute(0, 2, 1))
        assert np.array_equal(y, yl) and y.shape == (x.shape[0], 3) and np.all(y[:, lab] == 1) and y.sum() == x.shape[0]
    assert not os.path.exists(tmp_path / "feat" / "speech")  # save_feat=False (Proposed_Work_Results.py:465-469)


def test_data_parallel_ranks_hold_the_rows_of_the_single_process_batch(tmp_path):
    from sm_hpss_mtl_amd.sharding import class_block_rows
    folder, files = _dataset(tmp_path)
    model = "Doukhan_et_al_MTL"
    (x, y), = _first(_params(tmp_path, "feat_1", model, model), folder, files)
    seen = []
    for r in range(2):
        (xr, yr), = _first(_params(tmp_path, "feat_r%d" % r, model, model), folder, files, rank=r, world=2)
        mine = class_block_rows(3, 2, r, 2)
        assert tuple(xr.shape) == (3, 240, W, 1) and torch.equal(xr, x[torch.from_numpy(mine).cuda()])
        for k in y:
            np.testing.assert_array_equal(np.asarray(yr[k]), np.asarray(y[k])[mine])
        seen.extend(mine.tolist())
    assert sorted(seen) == list(range(6))


def test_doukhan_model_fed_from_the_device_path(tmp_path):
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.lib.proposed_architectures import get_Doukhan_MTL_model
    folder, files = _dataset(tmp_path)
    model = "Doukhan_et_al_MTL"
    P = _params(tmp_path, "feat_fit", model, model)
    P["input_shape"] = {model: (240, W, 1)}
    net, _ = get_Doukhan_MTL_model(P, n_classes=3, seed=0)
    (x, _), = _first(P, folder, files)
    dev = net.predict(x)
    host = net.predict(x.cpu().numpy())
    assert len(dev) == len(host) and all(np.array_equal(a, b) for a, b in zip(dev, host))
    np.random.seed(7)
    h = net.fit(gen.generator(P, folder, copy.deepcopy(files), 2), steps_per_epoch=2, epochs=1, verbose=0)
    assert np.isfinite(h.history["loss"]).all()
    net._check_device_status()  # a model with a device error word raises here if a kernel set it ...
    torch.cuda.synchronize()    # ... and any fault of the step's kernels surfaces here
    # the front end's rows must match the model's input height: a mismatch is the model's shape error, not a fault
    P402 = _params(tmp_path, "feat_402", model, "Papakostas_et_al_MTL")
    (x402, _), = _first(P402, folder, files)
    with pytest.raises(ValueError, match="expected input"):
        net.predict(x402)
