"""GPU: the cascaded-MTL model (get_Lemaire_Cascaded_MTL_model) -- the cascaded tail of the forward kernels on every f32 entry
point, the cascaded heads-training kernels (smh_train_cascade.hip) against the float64 torch reference, and the model's surface."""
import json
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import b3_mtl, b3_mtl_train as tr
from tests import cascaded_ref as cref

pytestmark = pytest.mark.gpu


def _weights(m, seed, W, ncls, block="2.3"):
    """Cascaded weights in the model's canonical order (the 2.8 block takes its trunk from oracle.b3_mtl.init_weights_v2)."""
    w = cref.init_weights(seed=seed, patch_size=W, n_classes=ncls)
    if block == "2.8":
        v2 = b3_mtl.init_weights_v2(seed=seed, n_feat=m.n_feat, patch_size=W, n_classes=3, randomize_bn=True)
        w = OrderedDict([(k, v) for k, v in v2.items() if k.startswith("tcn/")] + [(k, v) for k, v in w.items() if not k.startswith("tcn/")])
    elif m.n_feat != 240:
        base = b3_mtl.init_weights(seed=seed, n_feat=m.n_feat, patch_size=W, n_classes=3, randomize_bn=True)
        w = OrderedDict((k, base[k] if k.startswith("tcn/") else v) for k, v in w.items())
    return w


def _model(W=68, F=240, ncls=3, block="2.3", seed=0):
    from sm_hpss_mtl_amd.lib.proposed_architectures import get_Lemaire_Cascaded_MTL_model
    m, lr = get_Lemaire_Cascaded_MTL_model(TR_STEPS=10, N_MELS=F, n_classes=ncls, patch_size=W, seed=seed, tcn_block=block)
    assert lr == 0.002 and m.out_dim == 4 + ncls and m.output_names == ["S", "M", "R", "3C"]
    return m


@pytest.mark.parametrize("W,F,ncls,block,N", [(68, 240, 3, "2.3", 1030), (68, 120, 5, "2.3", 7), (99, 240, 3, "2.3", 33),
                                              (249, 240, 5, "2.3", 3), (68, 240, 3, "2.8", 17), (99, 120, 5, "2.8", 5),
                                              (249, 120, 3, "2.8", 2), (68, 240, 5, "2.3", 1)])
def test_forward_matches_reference(W, F, ncls, block, N):
    m = _model(W, F, ncls, block)
    w = _weights(m, 3, W, ncls, block)
    m.set_weights_dict(w)
    x = np.random.default_rng(W + N).standard_normal((N, W, F)).astype(np.float32)
    got = m.predict(x)
    ref = cref.forward(x, w, ncls)
    for g, r in zip(got, ref):
        # 1e-4 of the output's scale: the 2.8 block has no channel normalisation, its R outputs reach a few hundred (f32 rounding
        # there is ~1e-4 absolute); the 2.3 block's outputs are O(1), where this is 1e-4 absolute
        assert g.shape == r.shape and np.abs(g - r).max() <= 1e-4 * max(1.0, np.abs(r).max()), np.abs(g - r).max()
    assert np.array_equal(got[-1].argmax(1), ref[-1].argmax(1))


@pytest.mark.parametrize("W,ncls", [(68, 3), (99, 5)])
def test_x0_and_dense_entry_points_equal_the_plain_forward(W, ncls):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    m = _model(W, 240, ncls)
    w = _weights(m, 4, W, ncls)
    m.set_weights_dict(w)
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((37, W, 240)).astype(np.float32)).cuda()
    ref = m.forward_device(x)
    k0 = torch.from_numpy(w["tcn/initial_conv/kernel"][0]).cuda()  # (240, 32)
    x0p = torch.stack([x[:, :, :120] @ k0[:120], x[:, :, 120:] @ k0[120:]], dim=1).contiguous()  # per-half layer-0 partials
    got = m.forward_from_x0(x0p)
    torch.cuda.synchronize()
    assert float((got - ref).abs().max()) <= 2e-5
    fv = torch.from_numpy(rng.standard_normal((240, 3 * W + 11)).astype(np.float32)).cuda()
    dense = m.forward_dense(fv, 7)
    patches = Frontend(FrontendConfig()).extract_patches(fv[None], W, 7, time_major=True)
    plain = m.forward_device(patches.contiguous())
    torch.cuda.synchronize()
    assert dense.shape == plain.shape and float((dense - plain).abs().max()) <= 2e-5
    m.check_status()


def _train_problem(N, W=68, ncls=3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, W, 240)).astype(np.float32)
    y = {"S": (rng.random((N, 1)) > 0.5).astype(np.float32), "M": (rng.random((N, 1)) > 0.5).astype(np.float32),
         "R": rng.random((N, 2)).astype(np.float32), "3C": np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, N)]}
    drop_tcn = ((rng.random((N, 24, 32)) > 0.2) / 0.8).astype(np.float32)
    drop_heads = ((rng.random((N, 3, 16)) > 0.4) / 0.6).astype(np.float32)
    return x, y, drop_tcn, drop_heads


def _flat_to_dict(model, flat):
    out, o = {}, 0
    for name, shape, _, _ in model._spec:
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    return out


@pytest.mark.parametrize("N,ncls,lw", [(1, 3, None), (2, 3, None), (3, 5, None), (4, 3, {"S": 0.7, "R": 1.3}), (5, 3, None),
                                       (6, 5, {"M": 1.5, "3C": 0.5}), (510, 3, None)])
def test_train_step_gradients_and_bn_statistics_vs_reference(N, ncls, lw):
    m = _model(68, 240, ncls)
    if lw:
        m.compile(loss_weights=lw)
    w = _weights(m, 5, 68, ncls)
    m.set_weights_dict(w)
    x, y, dt, dh = _train_problem(N, ncls=ncls, seed=N)
    got = m.train_on_batch(x, y, drop_tcn=torch.from_numpy(dt).cuda(), drop_heads=torch.from_numpy(dh).cuda(), apply=False)
    ref = cref.torch_forward_backward(x, y, w, ncls, dt, {h: dh[:, i] for i, h in enumerate(("S", "M", "R"))}, lw)
    # losses: [total, S, M, R, 3C, 3C accuracy] (the total includes the l2 term like Keras)
    assert abs(got[0] - ref["loss"]) < 2e-4 * max(1.0, abs(ref["loss"]))
    for i, name in enumerate(["S", "M", "R", "3C"]):
        assert abs(got[1 + i] - ref["losses"][name]) < 2e-4 * max(1.0, abs(ref["losses"][name])), name
    assert abs(got[-1] - ref["acc"]) < 1e-6
    torch.cuda.synchronize()
    bucket = m._bucket_tensor().cpu().numpy()
    n = m.count_params()
    assert bucket.size == n + 4 * 32 + 2 * 36
    g = _flat_to_dict(m, bucket[:n])
    for name, gref in ref["grads"].items():
        if name.endswith(tr.TRAINABLE_SKIP):
            continue
        gg = g[name].astype(np.float64)
        if name.endswith("/dense/kernel"):
            gg = gg + 2 * tr.L2 * w[name]  # the l2 term is added at apply time on the device
        scale = max(np.abs(gref).max(), 1e-6)
        atol = 2e-5 if name.endswith("/dense/bias") else 1e-6  # analytically zero in front of a BatchNorm (test_training_gpu.py)
        assert np.abs(gg - gref).max() <= 2e-3 * scale + atol, (name, np.abs(gg - gref).max(), scale)
    st = bucket[n:]
    for h, name in enumerate(("S", "M", "R")):
        mean, var = ref["bn_batch"][name + "/bn"]
        assert np.abs(st[h * 32:h * 32 + 16] - mean).max() <= 1e-4 * max(1.0, np.abs(mean).max())
        assert np.abs(st[h * 32 + 16:h * 32 + 32] - var).max() <= 1e-4 * max(1.0, np.abs(var).max())
    for h, name in enumerate(("S", "M")):
        mean, var = ref["bn_batch"][name + "/cat_bn"]
        c = 128 + h * 36
        assert np.abs(st[c:c + 18] - mean).max() <= 1e-4 * max(1.0, np.abs(mean).max())
        assert np.abs(st[c + 18:c + 36] - var).max() <= 1e-4 * max(1.0, np.abs(var).max())


def test_moving_statistics_follow_the_batch_after_a_step():
    m = _model()
    w = _weights(m, 6, 68, 3)
    m.set_weights_dict(w)
    x, y, dt, dh = _train_problem(12, seed=2)
    m.train_on_batch(x, y, drop_tcn=torch.from_numpy(dt).cuda(), drop_heads=torch.from_numpy(dh).cuda())
    ref = cref.torch_forward_backward(x, y, w, 3, dt, {h: dh[:, i] for i, h in enumerate(("S", "M", "R"))})
    got = m.get_weights_dict()
    for key in ("S/bn", "M/cat_bn", "S/cat_bn", "R/bn"):
        mean, var = ref["bn_batch"][key]
        assert np.allclose(got[key + "/moving_mean"], 0.99 * w[key + "/moving_mean"] + 0.01 * mean, rtol=0, atol=1e-5), key
        assert np.allclose(got[key + "/moving_variance"], 0.99 * w[key + "/moving_variance"] + 0.01 * var, rtol=1e-5, atol=1e-5), key


@pytest.mark.parametrize("opt", ["sgd", "adam", "nadam"])
def test_optimisers_and_deterministic_mode(opt):
    from sm_hpss_mtl_amd import optimizers
    runs = []
    for _ in range(2):
        m = _model(seed=1)
        m.deterministic_gradients = True
        if opt != "sgd":
            m.compile(optimizer=(optimizers.Adam if opt == "adam" else optimizers.Nadam)(learning_rate=1e-3))
        x, y, dt, dh = _train_problem(40, seed=7)
        w0 = m.get_weights()
        losses = [m.train_on_batch(x, y, drop_tcn=torch.from_numpy(dt).cuda(), drop_heads=torch.from_numpy(dh).cuda())
                  for _ in range(3)]
        grad = m._bucket_tensor().cpu().numpy().copy()
        w1 = m.get_weights()
        assert all(np.all(np.isfinite(l)) for l in losses)
        assert any(not np.array_equal(a, b) for a, b in zip(w0, w1))
        runs.append((grad, w1))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


@pytest.mark.parametrize("N", [904, 1617])
def test_global_memory_heads_are_bit_reproducible(N):
    """The cascaded heads kernels add their batch sums per wave and then in wave order (smh_train_cascade.hip: "reproducible
    whatever smh_trainer_set_deterministic says"), in the global-memory forms too: N = 904 (the S / M / 3C kernel reads global
    memory) and N = 1617 (the R kernel as well; tests/heads_plans.py).  With deterministic_gradients the trunk's weight gradients are
    order-independent as well: three runs, `torch.equal` on the whole bucket (gradient and batch statistics)."""
    m = _model()
    m.set_weights_dict(_weights(m, 5, 68, 3))
    m.deterministic_gradients = True
    x, y, dt, dh = _train_problem(N, seed=N)
    xd, dtd, dhd = torch.from_numpy(x).cuda(), torch.from_numpy(dt).cuda(), torch.from_numpy(dh).cuda()
    runs = []
    for _ in range(3):
        m.train_on_batch(xd, y, drop_tcn=dtd, drop_heads=dhd, apply=False)
        torch.cuda.synchronize()
        runs.append(m._bucket_tensor().clone())
    assert torch.isfinite(runs[0]).all() and float(runs[0][:m.count_params()].abs().max()) > 0
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_fit_loss_falls(tmp_path):
    rng = np.random.default_rng(0)
    m = _model(seed=1)

    def batch(n=48):
        cls = rng.integers(0, 3, n)
        x = rng.standard_normal((n, 68, 240)).astype(np.float32) * 0.3 + (cls[:, None, None] - 1.0) * 0.8
        y = {"S": (cls == 1).astype(np.float32)[:, None], "M": (cls == 0).astype(np.float32)[:, None],
             "R": np.stack([(cls != 1), (cls != 0)], 1).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[cls]}
        return x, y

    def gen():
        while True:
            yield batch()
    vx, vy = batch(96)
    before = m.evaluate(vx, vy)
    hist = m.fit(gen(), steps_per_epoch=4, epochs=5, validation_data=(vx, vy), verbose=0, csv_log=str(tmp_path / "log.csv"))
    after = m.evaluate(vx, vy)
    assert len(before) == len(m.metrics_names) == 6 and len(hist.history["loss"]) == 5
    assert after[0] < before[0], (before, after)


def test_persistence_round_trip(tmp_path):
    from sm_hpss_mtl_amd.model import CascadedMTL
    from sm_hpss_mtl_amd.persistence import model_from_json
    m = _model(99, 120, 5)
    w = _weights(m, 8, 99, 5)
    m.set_weights_dict(w)
    js = m.to_json()
    assert json.loads(js)["class_name"] == "B3_MTL_Cascaded"
    m2 = model_from_json(js)
    assert isinstance(m2, CascadedMTL) and m2.to_json() == js and m2.count_params() == m.count_params()
    path = m.save_weights(str(tmp_path / "w.h5"))
    m2.load_weights(path)
    x = np.random.default_rng(1).standard_normal((9, 99, 120)).astype(np.float32)
    for a, b in zip(m.predict(x), m2.predict(x)):
        assert np.array_equal(a, b)


def test_bf16_and_head_model_are_refused():
    from sm_hpss_mtl_amd.persistence import Model
    m = _model()
    x = torch.zeros((2, 68, 240), device="cuda")
    with pytest.raises(Exception, match="cascaded"):
        m.forward_device(x, dtype="bf16")
    with pytest.raises(ValueError):
        m.train_dtype = "bf16"
    assert m.train_dtype == "f32"
    with pytest.raises(ValueError):
        Model(m.input, m.get_layer("M").output)


def test_b3mtl_alongside_still_matches_its_golden(golden_model):
    from sm_hpss_mtl_amd.model import B3MTL
    casc = _model()
    casc.set_weights_dict(_weights(casc, 3, 68, 3))
    b3 = B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=0)
    b3.set_weights_dict(b3_mtl.init_weights(seed=7, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True))
    x = np.random.default_rng(11).standard_normal((6, 68, 240)).astype(np.float32)
    casc.predict(x)
    got = np.concatenate(b3.predict(x), axis=1)
    assert np.abs(got - golden_model["out_c3_W68"]).max() <= 1e-4
