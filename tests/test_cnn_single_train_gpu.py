"""Training of the single-task Conv2D baselines on the device against tests/cnn_single_ref.py (torch autograd, float64):
`train_on_batch(apply=False)` at the bounds of tests/test_cnn_train_gpu.py -- loss rel 2e-4 / abs 2e-5, loss == data loss + penalty
at rel 2e-4, accuracy 1e-6, gradients per tensor err / max |g| < 1e-3 (Jang 2e-3) + 4 x the float32-torch floor, analytic zeros as
noise --, one optimiser step per kind against the reference's Adam / SGD fed with the device gradients (3e-7 + 1e-6 max |w|, Jang
2e-6; moving statistics 2e-4 max(1, |v|)), fit / evaluate, the batch of one, and the trainer that grows.

The cases, seeds and the float32 floor are those tests/test_cnn_single_ref.py checks on the CPU.

The kind-1 (`l2()`) optimiser segments of the MTL Jang model share opt_kernel with the new l1_l2 kind:
`test_jang_mtl_step_has_the_bits_of_the_parent_build` compares one Adam step of the MTL Jang model on a fixed input with
tests/golden/jang_mtl_adam_step.npz, written on an MI355X by a build of the commit before the l1_l2 kind (every tensor's SHA-256, the
small tensors in full); `test_jang_mtl_l2_step_is_unchanged` checks the same step's arithmetic against
oracle.cnn_mtl_train.adam_step."""
import hashlib
import os

import numpy as np
import pytest

from tests import cnn_single_ref as ref
from tests.test_cnn_single_ref import GRAD_RTOL, TRAIN_CASES, analytic_zeros, batch, masks, noise_bound, train_case

pytestmark = pytest.mark.gpu


def _model(kind, H, W, n_classes, fc=0, w=None):
    from sm_hpss_mtl_amd.cnn_models import CnnSingleTask
    m = CnnSingleTask(kind, (H, W, 1), n_classes=n_classes, seed=0, fc_width=fc or 64)
    if w is not None:
        m.set_weights_dict(w)
    return m


@pytest.mark.parametrize("n_classes", [2, 3])
@pytest.mark.parametrize("kind,H,W,N,fc,dropout", TRAIN_CASES)
def test_train_step_matches_autograd(kind, H, W, N, fc, dropout, n_classes):
    w, x, y, drop = train_case(kind, H, W, N, fc, dropout, n_classes)
    m = _model(kind, H, W, n_classes, fc, w)
    if dropout:
        spec = m.dropout_spec(N)
        assert [d for d, _ in spec] == [mk.shape[1] for mk in drop]
    r64 = ref.forward_backward(kind, x, y, w, n_classes, drop=drop)
    r32 = ref.forward_backward(kind, x, y, w, n_classes, drop=drop, dtype=np.float32)
    raw = m.train_on_batch(x, y, drop=drop, apply=False, sync=False).cpu().numpy()
    loss, acc = m.losses_to_list(raw)
    print("%s %dx%d N=%d %d classes: raw losses %s, reference loss %.6f penalty %.6f acc %.4f" % (kind, H, W, N, n_classes, raw, r64["loss"], r64["penalty"], r64["acc"]))
    assert raw.shape == (4,) and raw[0] == pytest.approx(r64["loss"], rel=2e-4, abs=2e-5) and raw[1] == raw[0]
    assert raw[3] == pytest.approx(r64["penalty"], rel=2e-4, abs=2e-5)
    assert loss == pytest.approx(r64["loss"] + r64["penalty"], rel=2e-4) and acc == pytest.approx(r64["acc"], abs=1e-6)
    got = m.gradients()
    zeros = analytic_zeros(kind, r64["grads"])
    bad = []
    for name, g in r64["grads"].items():
        err = np.abs(got[name].astype(np.float64) - g).max()
        if name in zeros:
            if err > noise_bound(name, r64["grads"]):
                bad.append("%s: noise %.3e" % (name, err))
            continue
        scale = np.abs(g).max()
        floor = np.abs(r32["grads"][name].astype(np.float64) - g).max()
        print("%-22s err/max %.2e   f32-torch floor %.2e" % (name, err / scale, floor / scale))
        if not err / scale < GRAD_RTOL[kind] + 4 * floor / scale:
            bad.append("%s: max err %.3e (f32 floor %.3e) vs max |g| %.3e" % (name, err, floor, scale))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind,H,W,N,fc", [("Doukhan", 21, 68, 6, 0), ("Papakostas", 61, 68, 6, 64), ("Jang", 257, 12, 4, 0)])
def test_one_optimiser_step(kind, H, W, N, fc):
    """The update arithmetic against the reference's optimiser fed with the DEVICE gradients (Adam's first step is sign descent, so
    gradient noise must not enter).  Jang: the mel kernels hold both signs and exact zeros, so sign(w) and sign(0) = 0 count."""
    n_classes = 2
    w, x, y, _ = train_case(kind, H, W, N, fc, False, n_classes)
    if kind == "Jang":
        k = w["melCl3/kernel"]
        assert (k > 0).any() and (k < 0).any() and (k == 0).any()
    m = _model(kind, H, W, n_classes, fc, w)
    r64 = ref.forward_backward(kind, x, y, w, n_classes)
    m.train_on_batch(x, y, drop=None, apply=False)
    g = {k: v.astype(np.float64) for k, v in m.gradients().items()}
    m.apply_gradients()
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    if kind == "Papakostas":
        assert m.optimizer.kind == "sgd"
        nw = ref.sgd_step(kind, w64, g, r64["bn_batch"], 1e-3)
    else:
        assert m.optimizer.kind == "adam"
        nw, _, _ = ref.adam_step(kind, w64, g, {}, {}, r64["bn_batch"], 1, {"Doukhan": 1e-4, "Jang": 1e-3}[kind])
    got = m.get_weights_dict()
    rel = 2e-6 if kind == "Jang" else 1e-6
    for name, v in nw.items():
        tol = 2e-4 * max(1.0, np.abs(v).max()) if name.endswith(("moving_mean", "moving_variance")) else 3e-7 + rel * np.abs(v).max()
        assert np.abs(got[name].astype(np.float64) - v).max() <= tol, name
    assert m.iterations == 1


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jang_mtl_adam_step.npz")


def jang_mtl_adam_step():
    """The fixed case of the golden file: the MTL Jang model at (514, 4), generic seeded weights, four images, one Adam step without
    dropout -> the weights after the step."""
    from oracle import cnn_mtl
    from sm_hpss_mtl_amd.cnn_models import CnnMTL
    W, N = 4, 4
    m = CnnMTL("Jang", (514, W, 1), seed=0)
    m.set_weights_dict(cnn_mtl.init_jang(seed=4, W=W, mel_init=False))
    rng = np.random.default_rng(2)
    x = rng.normal(size=(N, 514, W)).astype(np.float32)
    c = np.arange(N) % 3
    y = {"S": (c == 1).astype(np.float32)[:, None], "M": (c == 0).astype(np.float32)[:, None],
         "R": rng.uniform(0, 1, size=(N, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[c]}
    m.train_on_batch(x, y, drop=None, drop_heads=None)
    return m.get_weights_dict()


def golden_arrays(w):
    """What the golden file holds: the SHA-256 of every tensor's bytes (the Dense kernels hold millions of weights), and every tensor
    of at most 4096 weights in full."""
    out = {"sha256": np.array([k + " " + hashlib.sha256(np.ascontiguousarray(v, np.float32).tobytes()).hexdigest() for k, v in w.items()])}
    out.update({"w:" + k.replace("/", "__"): np.asarray(v, np.float32) for k, v in w.items() if v.size <= 4096 and "melCl" not in k})
    return out


def test_jang_mtl_step_has_the_bits_of_the_parent_build():
    want = np.load(GOLDEN)
    got = golden_arrays(jang_mtl_adam_step())
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        if k != "sha256":
            assert np.array_equal(got[k], want[k]), k
    diff = [a.split()[0] for a, b in zip(got["sha256"], want["sha256"]) if a != b]
    assert len(got["sha256"]) == len(want["sha256"]) and not diff, diff


def test_jang_mtl_l2_step_is_unchanged():
    """The MTL Jang model's kind-1 segments (l2() on every kernel) through the opt_kernel that now also holds the l1_l2 kind: one
    Adam step against oracle.cnn_mtl_train.adam_step at tests/test_cnn_train_gpu.py's bound."""
    from oracle import cnn_mtl, cnn_mtl_train
    from sm_hpss_mtl_amd.cnn_models import CnnMTL
    W, N = 12, 4
    w = cnn_mtl.init_jang(seed=4, W=W, mel_init=False)
    m = CnnMTL("Jang", (514, W, 1), seed=0)
    m.set_weights_dict(w)
    rng = np.random.default_rng(2)
    x = rng.normal(size=(N, 514, W)).astype(np.float32)
    c = np.arange(N) % 3
    y = {"S": (c == 1).astype(np.float32)[:, None], "M": (c == 0).astype(np.float32)[:, None],
         "R": rng.uniform(0, 1, size=(N, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[c]}
    r = cnn_mtl_train.forward_backward(x, y, w, kind="Jang")
    res = dict(zip(m.metrics_names, m.train_on_batch(x, y, drop=None, drop_heads=None, apply=False)))
    assert res["loss"] == pytest.approx(r["loss"] + r["l2"], rel=2e-4)
    g = {k: v.astype(np.float64) for k, v in m.gradients().items()}
    m.apply_gradients()
    nw, _, _ = cnn_mtl_train.adam_step({k: v.astype(np.float64) for k, v in w.items()}, g, {}, {}, r["bn_batch"], 1, lr=1e-3, kind="Jang")
    got = m.get_weights_dict()
    for name, v in nw.items():
        tol = 2e-4 * max(1.0, np.abs(v).max()) if name.endswith(("moving_mean", "moving_variance")) else 3e-7 + 2e-6 * np.abs(v).max()
        assert np.abs(got[name].astype(np.float64) - v).max() <= tol, name


@pytest.mark.parametrize("kind,H,W,n_classes", [("Doukhan", 21, 68, 2), ("Jang", 257, 12, 3)])
def test_fit_and_evaluate(kind, H, W, n_classes):
    w = ref.init_weights(kind, H, W, n_classes, seed=3, mel_signs=True)
    m = _model(kind, H, W, n_classes, 0, w)
    x, y = batch(kind, H, W, 12, n_classes, 5)
    # evaluate == the reference's inference-mode loss (+ penalty) and accuracy
    ev = m.evaluate(x, y)
    want = ref.inference_losses(kind, x, y, w, n_classes)
    assert len(ev) == 2 and ev[0] == pytest.approx(want[0], rel=2e-4, abs=2e-5) and ev[1] == pytest.approx(want[1], abs=1e-6)
    with pytest.raises(ValueError):
        m.train_on_batch(x[:1], y[:1])
    h = m.fit(x, y, batch_size=12, epochs=6, verbose=0)
    losses = h.history["loss"]
    assert np.isfinite(losses).all() and losses[-1] < losses[0] and set(h.history) >= {"loss", "accuracy"}


@pytest.mark.parametrize("kind,H,W", [("Doukhan", 21, 68), ("Jang", 257, 12)])
def test_the_trainer_grows_and_keeps_the_adam_moments(kind, H, W):
    """Two steps at 24 images, then one at 60: the trainer grows from its first capacity (48) to 60.  A model whose trainer had 60
    rows from the start must hold the same weights bit for bit (ordered sums that follow the batch, not the capacity): the Adam
    moments and the step count travelled."""
    w = ref.init_weights(kind, H, W, 2, seed=3, mel_signs=True)
    x, y = batch(kind, H, W, 60, 2, 6)
    res = []
    for presize in (False, True):
        m = _model(kind, H, W, 2, 0, w)
        if presize:
            m._get_trainer(60)
        for _ in range(2):
            m.train_on_batch(x[:24], y[:24], drop=None)
        assert m._trainer_cap == (60 if presize else 48)
        m.train_on_batch(x, y, drop=None)
        assert m._trainer_cap == 60 and m.iterations == 3
        res.append(m.get_weights_dict())
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k
    assert np.abs(res[0]["dense/kernel"] - w["dense/kernel"]).max() > 0
