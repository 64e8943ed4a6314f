"""CPU: the cascaded-MTL reference (tests/cascaded_ref.py) pinned against the oracle, and the host side of the cascaded model --
canonical weight order, parameter count, the Keras-layout weight loader."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest

from oracle import b3_mtl, b3_mtl_train as tr
from tests import cascaded_ref as cref


def _problem(N, W=68, ncls=3, seed=0, n_heads=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, W, 240)).astype(np.float32)
    y = {"S": (rng.random((N, 1)) > 0.5).astype(np.float32), "M": (rng.random((N, 1)) > 0.5).astype(np.float32),
         "R": rng.random((N, 2)).astype(np.float32), "3C": np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, N)]}
    drop_tcn = ((rng.random((N, 24, 32)) > 0.2) / 0.8).astype(np.float32)
    drop_heads = ((rng.random((N, n_heads, 16)) > 0.4) / 0.6).astype(np.float32)
    return x, y, drop_tcn, drop_heads


def test_torch_build_with_standard_heads_reproduces_the_training_oracle():
    """heads='mtl': the torch graph of the reference is the oracle's training step -- trunk, SpatialDropout1D, batch-statistics
    BN, Dropout, Keras losses, l2 -- so the cascaded graph built on the same code inherits those conventions."""
    N = 5
    x, y, dt, dh = _problem(N, seed=1)
    w = b3_mtl.init_weights(seed=3, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True)
    lw = {"S": 0.7, "R": 1.3}
    masks = {h: dh[:, i] for i, h in enumerate(("S", "M", "R"))}
    ref = tr.forward_backward(x, y, w, 3, dt, masks, lw)
    got = cref.torch_forward_backward(x, y, w, 3, dt, masks, lw, heads="mtl")
    assert abs(got["loss"] - ref["loss"]) < 1e-10 * max(1.0, abs(ref["loss"]))
    for k, v in ref["losses"].items():
        assert abs(got["losses"][k] - v) < 1e-10, k
    assert got["acc"] == ref["acc"]
    for k, g in ref["grads"].items():
        if k.endswith(tr.TRAINABLE_SKIP):
            continue
        assert np.abs(got["grads"][k] - g).max() <= 1e-9 * max(np.abs(g).max(), 1e-6), k
    for h in ("S", "M", "R"):
        m, v = got["bn_batch"][h + "/bn"]
        assert np.allclose(m, ref["bn_batch"][h][0], rtol=0, atol=1e-12) and np.allclose(v, ref["bn_batch"][h][1], rtol=0, atol=1e-12)


def test_inference_reference_shares_trunk_R_and_3C_with_the_oracle():
    """The cascaded model's R and '3C' are B3_MTL's (same layers on the same trunk): the numpy forward of the reference must give the
    oracle's R and 3C; S and M see R through the concatenation BatchNorm."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((4, 68, 240)).astype(np.float32)
    w = cref.init_weights(seed=5)
    ow = b3_mtl.init_weights(seed=5, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True)
    S, M, R, C3 = cref.forward(x, w)
    oS, oM, oR, oC3 = b3_mtl.forward(x, ow)
    assert np.abs(R - oR).max() < 1e-5 and np.abs(C3 - oC3).max() < 1e-6
    assert S.shape == (4, 1) and M.shape == (4, 1) and np.all((S > 0) & (S < 1))
    # S depends on R: change R's output bias, S moves; B3_MTL's S would not
    w2 = OrderedDict(w)
    w2["R/out/bias"] = w["R/out/bias"] + 1.0
    S2 = cref.forward(x, w2)[0]
    assert np.abs(S2 - S).max() > 1e-4


def test_cascade_gradient_reaches_R_through_the_concatenation():
    """Training: d loss_S / d r flows into R's head.  Against central differences of the reference's own loss on R's out kernel."""
    import torch  # noqa: F401 (the reference needs it)
    N = 4
    x, y, dt, dh = _problem(N, seed=3)
    w = cref.init_weights(seed=6)
    masks = {h: dh[:, i] for i, h in enumerate(("S", "M", "R"))}
    got = cref.torch_forward_backward(x, y, w, 3, dt, masks)
    eps = 1e-4
    for (i, c) in ((0, 0), (5, 1)):  # R's out kernel (its bias is not a test: BN18 removes the batch mean of r)
        wp, wm = OrderedDict(w), OrderedDict(w)
        wp["R/out/kernel"] = w["R/out/kernel"].astype(np.float64).copy()
        wm["R/out/kernel"] = w["R/out/kernel"].astype(np.float64).copy()
        wp["R/out/kernel"][i, c] += eps
        wm["R/out/kernel"][i, c] -= eps
        lp = cref.torch_forward_backward(x, y, wp, 3, dt, masks)["loss"]
        lm = cref.torch_forward_backward(x, y, wm, 3, dt, masks)["loss"]
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - got["grads"]["R/out/kernel"][i, c]) < 1e-6 * max(1.0, abs(fd))
    # ... and it is not R's MSE alone: cut the path (S and M ignore r) and R's gradient changes
    wc = OrderedDict(w)
    for h in ("S", "M"):
        wc[h + "/out/kernel"] = w[h + "/out/kernel"].copy()
        wc[h + "/out/kernel"][16:] = 0.0
    cut = cref.torch_forward_backward(x, y, wc, 3, dt, masks)
    assert np.abs(got["grads"]["R/out/kernel"] - cut["grads"]["R/out/kernel"]).max() > 1e-5
    assert np.abs(got["grads"]["R/dense/kernel"] - cut["grads"]["R/dense/kernel"]).max() > 1e-7


@pytest.mark.parametrize("ncls", [3, 5])
def test_weight_spec_and_count(ncls):
    from sm_hpss_mtl_amd.model import HEADS_CASCADED, head_spec, initial_weights, weight_spec
    spec = weight_spec(240, 68, ncls, heads=HEADS_CASCADED)
    names = [n for n, _, _, _ in spec]
    assert [h for h, _, _ in head_spec(ncls, HEADS_CASCADED)] == ["S", "M", "R"]
    assert names == list(cref.init_weights(seed=0, n_classes=ncls))
    shapes = {n: s for n, s, _, _ in spec}
    assert shapes["S/out/kernel"] == (18, 1) and shapes["M/cat_bn/moving_variance"] == (18,) and shapes["R/out/kernel"] == (16, 2)
    assert shapes["3C/kernel"] == (68 * 32, ncls) and "N/dense/kernel" not in shapes
    mtl = weight_spec(240, 68, 3)
    n_casc = sum(int(np.prod(s)) for _, s, _, _ in spec)
    n_mtl = sum(int(np.prod(s)) for _, s, _, _ in mtl)
    assert n_casc == n_mtl + 2 * (4 * 18 + 2) + 68 * 32 * (ncls - 3) + (ncls - 3)
    _, w = initial_weights(240, 68, ncls, seed=1, heads=HEADS_CASCADED)
    assert list(w) == names
    assert np.all(w["S/cat_bn/gamma"] == 1) and np.all(w["S/cat_bn/moving_mean"] == 0) and np.all(w["M/cat_bn/moving_variance"] == 1)


def test_public_entry_point_exists():
    from sm_hpss_mtl_amd.lib import proposed_architectures as pa
    assert callable(pa.get_Lemaire_Cascaded_MTL_model)
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL
    assert issubclass(CascadedMTL, B3MTL) and CascadedMTL.CLASS_NAME != B3MTL.CLASS_NAME


def keras_style_cascaded(w, ncls, T, F, shuffle=True):
    """(layers, arch) as tf.keras would save get_Lemaire_Cascaded_MTL_model: auto-named hidden layers, the graph of
    cascade_MTL_modifications (:195-234) in the architecture JSON.  shuffle=False lists the head layers in creation order."""
    layers, cfg = OrderedDict(), []

    def add(cls, name, inbound, weights=None, **conf):
        layers[name] = OrderedDict((name + "/" + k + ":0", v) for k, v in (weights or {}).items())
        cfg.append({"class_name": cls, "name": name, "config": dict(name=name, **conf),
                    "inbound_nodes": [[[i, 0, 0, {}] for i in inbound]] if inbound else []})

    add("InputLayer", "input_1", [], batch_input_shape=[None, T, F])
    add("Conv1D", "tcn_initial_conv", ["input_1"], {"kernel": w["tcn/initial_conv/kernel"], "bias": w["tcn/initial_conv/bias"]})
    prev, n = "tcn_initial_conv", 0
    for s in range(3):
        for i in range(8):
            d, p = 2 ** i, "tcn/s%d_d%d" % (s, 2 ** i)
            dc = "tcn_dilated_conv_%d_tanh_s%d" % (d, s)
            add("Conv1D", dc, [prev], {"kernel": w[p + "/conv/kernel"], "bias": w[p + "/conv/bias"]}, dilation_rate=[d])
            add("SpatialDropout1D", "sdrop_%d" % (n + 1), [dc], rate=0.25)
            c1 = "conv1d_%d" % (n + 1)
            add("Conv1D", c1, ["sdrop_%d" % (n + 1)], {"kernel": w[p + "/conv1x1/kernel"], "bias": w[p + "/conv1x1/bias"]})
            add("Add", "add_%d" % (n + 1), [prev, c1])
            prev, n = "add_%d" % (n + 1), n + 1
    add("Flatten", "flatten_1", [prev])
    num = {"R": 1, "S": 2, "M": 3}  # creation order of cascade_MTL_modifications
    order = ["M", "S", "R"] if shuffle else ["R", "S", "M"]
    for h in order:
        add("Dense", "dense_%d" % num[h], ["flatten_1"], {"kernel": w[h + "/dense/kernel"], "bias": w[h + "/dense/bias"]}, units=16)
    for h in order:
        add("BatchNormalization", "batch_normalization_%d" % (2 * num[h]), ["dense_%d" % num[h]],
            {k: w[h + "/bn/" + k] for k in ("gamma", "beta", "moving_mean", "moving_variance")})
        add("Activation", "activation_%d" % num[h], ["batch_normalization_%d" % (2 * num[h])])
        add("Dropout", "dropout_%d" % num[h], ["activation_%d" % num[h]], rate=0.4)
        if h == "R":
            add("Dense", "R", ["dropout_1"], {"kernel": w["R/out/kernel"], "bias": w["R/out/bias"]}, units=2)
    for h in order:
        if h == "R":
            continue
        add("Concatenate", "concatenate_%d" % num[h], ["dropout_%d" % num[h], "R"])
        add("BatchNormalization", "batch_normalization_%d" % (2 * num[h] + 1), ["concatenate_%d" % num[h]],
            {k: w[h + "/cat_bn/" + k] for k in ("gamma", "beta", "moving_mean", "moving_variance")})
        add("Dense", h, ["batch_normalization_%d" % (2 * num[h] + 1)], {"kernel": w[h + "/out/kernel"], "bias": w[h + "/out/bias"]}, units=1)
    add("Dense", "3C", ["flatten_1"], {"kernel": w["3C/kernel"], "bias": w["3C/bias"]}, units=ncls)
    arch = {"class_name": "Functional", "config": {"name": "model_1", "layers": cfg, "input_layers": [["input_1", 0, 0]],
                                                     "output_layers": [[h, 0, 0] for h in ("S", "M", "R", "3C")]}}
    return layers, arch


@pytest.mark.parametrize("ncls", [3, 5])
def test_keras_written_cascaded_weight_file_is_traced_through_the_architecture_json(tmp_path, ncls):
    from sm_hpss_mtl_amd import h5io, persistence
    if not h5io.available():
        pytest.skip("libhdf5 not found on this machine")
    w = OrderedDict((k, np.asarray(v, np.float32)) for k, v in cref.init_weights(seed=4, n_classes=ncls).items())
    layers, arch = keras_style_cascaded(w, ncls, 68, 240)
    wf, af = str(tmp_path / "fold0_model.h5"), str(tmp_path / "fold0_model.json")
    h5io.write_layers(wf, layers)
    json.dump(arch, open(af, "w"))
    got = persistence.load_weights_file(wf)
    assert list(got) == list(w)
    for k in w:
        assert np.array_equal(got[k], w[k]), k
    # without the JSON a scrambled file cannot be mapped right; one in creation order can
    os.remove(af)
    blind = persistence.load_weights_file(wf)
    assert not np.array_equal(blind["R/dense/kernel"], w["R/dense/kernel"])
    layers2, _ = keras_style_cascaded(w, ncls, 68, 240, shuffle=False)
    h5io.write_layers(str(tmp_path / "b.h5"), layers2)
    plain = persistence.load_weights_file(str(tmp_path / "b.h5"))
    assert list(plain) == list(w) and all(np.array_equal(plain[k], w[k]) for k in w)
