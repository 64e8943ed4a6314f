"""CPU: tests/cnn_single_ref.py, the torch restatement of the single-task Conv2D baselines, against itself -- output shapes at the
reference's inputs, softmax rows, the two-class loss rule, the l1_l2 penalty and its gradient, and the rule of
tests/test_single_task_ref.py for the GPU training cases: evaluated in float32, every gradient stays within a TENTH of the bound the
GPU test applies (1e-3 of max |g|; Jang 2e-3) of its float64 evaluation, so that bound measures the device and not the cases."""
import numpy as np
import pytest

from tests import cnn_single_ref as ref

# (kind, H, W, N, fc, dropout): the training cases of tests/test_cnn_single_train_gpu.py
TRAIN_CASES = [("Doukhan", 21, 68, 6, 0, False), ("Doukhan", 21, 68, 7, 0, True), ("Papakostas", 61, 68, 6, 64, False),
               ("Jang", 257, 12, 4, 0, False), ("Jang", 257, 20, 3, 0, True)]
GRAD_RTOL = {"Doukhan": 1e-3, "Papakostas": 1e-3, "Jang": 2e-3}
RATES = {"Doukhan": (0.2, 0.3, 0.4, 0.5), "Papakostas": (0.5, 0.5), "Jang": (0.4, 0.4, 0.4)}


def bn_biases(kind):
    """The biases in front of a BatchNorm: their gradient is zero analytically, so it is checked as noise."""
    n_conv, n_fc = {"Doukhan": (4, 4), "Papakostas": (0, 2), "Jang": (3, 0)}[kind]
    return {"conv%d/bias" % (i + 1) for i in range(n_conv)} | {"fc%d/bias" % (i + 1) for i in range(n_fc)}


def analytic_zeros(kind, grads64):
    """Tensors whose gradient is zero analytically, so that `relative to max |g|` has no meaning and both sides hold rounding noise:
    the biases in front of a BatchNorm, and any tensor whose float64 gradient is below 1e-9 of the model's largest -- Doukhan's
    bn4/beta at the reference's 21 x 68 input, where the last pooling leaves ONE pixel per channel: while every pooled maximum is
    positive, beta shifts a feature by the same amount in every sample, and fc1's BatchNorm removes a per-batch shift."""
    top = max(np.abs(g).max() for g in grads64.values())
    return bn_biases(kind) | {k for k, g in grads64.items() if np.abs(g).max() <= 1e-9 * top}


def noise_bound(name, grads64):
    """What an analytic zero may hold: 1e-5 of the gradient it sits next to (a bias: its kernel's; a beta: its gamma's), at least 1e-5
    -- the rule tests/test_cnn_train_gpu.py applies to the biases in front of a BatchNorm."""
    sib = name.replace("/bias", "/kernel").replace("/beta", "/gamma")
    return 1e-5 * max(1.0, float(np.abs(grads64[sib]).max()))


def batch(kind, H, W, N, n_classes, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, H, W)).astype(np.float32)
    return x, np.eye(n_classes, dtype=np.float32)[np.arange(N) % n_classes]


def drop_dims(kind, H, W, fc, n_mels=64):
    """Width of every Dropout layer's input, in graph order."""
    if kind == "Doukhan":
        return [512] * 4
    if kind == "Papakostas":
        return [fc] * 2
    dims, h, w_ = [], n_mels, W
    for c in (32, 64, 128):
        dims.append(h * w_ * c)
        h, w_ = h // 2, w_ // 2
    return dims


def masks(kind, H, W, N, fc, seed, on):
    if not on:
        return None
    rng = np.random.default_rng(seed)
    return [((rng.uniform(size=(N, d)) < 1 - r) / (1 - r)).astype(np.float32) for d, r in zip(drop_dims(kind, H, W, fc), RATES[kind])]


def train_case(kind, H, W, N, fc, dropout, n_classes):
    w = ref.init_weights(kind, H, W, n_classes, seed=3, fc=fc or 64, mel_signs=True)
    # batch seed 2: among seeds 1 .. 6 the one at which NO case has a ReLU gate or a pooling maximum that float32 rounding flips (seed 1
    # flips one in Doukhan N = 7 and in Papakostas with two classes: 1e-2 and 2e-1 of max |g|); worst here 3e-5
    x, y = batch(kind, H, W, N, n_classes, 2)
    return w, x, y, masks(kind, H, W, N, fc, 7, dropout)


@pytest.mark.parametrize("n_classes", [2, 3])
def test_shapes_at_the_reference_inputs(n_classes):
    # Doukhan (21, 68): 18x64 -> 9x32 -> 7x30 -> 5x28 -> 3x14 -> 1x12 -> 1x1x256 in front of the Dense blocks
    from oracle import cnn_mtl as oc
    assert oc.doukhan_shapes(21, 68) == (1, 1, 256)
    w = ref.init_weights("Doukhan", 21, 68, n_classes)
    assert w["fc1/kernel"].shape == (256, 512) and w["dense/kernel"].shape == (512, n_classes)
    x = np.random.default_rng(0).normal(size=(2, 21, 68)).astype(np.float32)
    p, f = ref.forward("Doukhan", x, w)
    assert p.shape == (2, n_classes) and f.shape == (2, 512) and np.allclose(p.sum(1), 1.0, atol=1e-12)
    # Papakostas (201, 68): Flatten -> 4096 -> 4096 -> n (the tensors alone: a 4096-wide forward is not a CPU test)
    D = oc.papakostas_shapes(201, 68)[2]
    assert ref.feat_dim("Papakostas", 201, 68) == 4096 and D == 6 * 2 * 512  # 99x32 -> 50x16 -> 24x7 -> 12x4 -> 6x2
    w = ref.init_weights("Papakostas", 61, 68, n_classes, fc=64)
    p, f = ref.forward("Papakostas", np.random.default_rng(1).normal(size=(2, 61, 68)).astype(np.float32), w)
    assert p.shape == (2, n_classes) and f.shape == (2, 64) and np.allclose(p.sum(1), 1.0, atol=1e-12)
    # Jang (257, 68): 64x68x3 -> 32x34x32 -> 16x17x64 -> 8x8x128 -> 8192
    assert ref.jang_shapes(68) == (8, 8, 8192) and ref.jang_shapes(20, 30) == (3, 2, 3 * 2 * 128)
    w = ref.init_weights("Jang", 257, 12, n_classes)
    assert list(w)[:2] == ["melCl0/kernel", "melCl1/kernel"] and list(w)[-2:] == ["dense/kernel", "dense/bias"]
    assert not any(k.startswith(("fc", "harm_", "perc_")) for k in w) and sum(k.startswith("melCl") for k in w) == 64
    p, f = ref.forward("Jang", np.random.default_rng(2).normal(size=(2, 257, 12)).astype(np.float32), w)
    assert p.shape == (2, n_classes) and f.shape == (2, ref.jang_shapes(12)[2]) and np.allclose(p.sum(1), 1.0, atol=1e-12)


def test_two_class_rule_and_penalty():
    import torch
    p = torch.tensor([[0.9, 0.1], [0.4, 0.6], [0.5, 0.5]], dtype=torch.float64)
    t = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    loss, acc = ref.loss_and_accuracy(p, t, 2)
    e = 1e-7
    want = np.mean([-np.log(0.9 + e), -np.log(1 - 0.1 + e), -np.log(0.4 + e), -np.log(1 - 0.6 + e), -np.log(1 - 0.5 + e), -np.log(0.5 + e)])
    assert float(loss) == pytest.approx(want, rel=1e-12)
    assert acc == pytest.approx((2 + 0 + 1) / 6)  # binary accuracy over the N x 2 outputs: 0.5 > 0.5 is False
    w = {"melCl0/kernel": np.array([1.0, -2.0, 0.0]), "conv1/kernel": np.array([5.0])}
    assert ref.penalty("Jang", w) == pytest.approx(0.01 * 5.0 + 0.01 * 3.0) and ref.penalty("Doukhan", w) == 0.0
    assert np.array_equal(ref._reg_grad("Jang", "melCl0/kernel", w["melCl0/kernel"]), [0.02 + 0.01, -0.04 - 0.01, 0.0])
    assert ref._reg_grad("Jang", "conv1/kernel", w["conv1/kernel"]) == 0.0


@pytest.mark.parametrize("n_classes", [2, 3])
@pytest.mark.parametrize("kind,H,W,N,fc,dropout", TRAIN_CASES)
def test_float32_evaluation_stays_within_a_tenth_of_the_gpu_bound(kind, H, W, N, fc, dropout, n_classes):
    w, x, y, drop = train_case(kind, H, W, N, fc, dropout, n_classes)
    r64 = ref.forward_backward(kind, x, y, w, n_classes, drop=drop)
    r32 = ref.forward_backward(kind, x, y, w, n_classes, drop=drop, dtype=np.float32)
    assert r32["loss"] == pytest.approx(r64["loss"], rel=2e-5, abs=2e-6) and r32["acc"] == r64["acc"]
    assert r64["probs"].min() > 1e-6  # no clip is active: the cases test the arithmetic, not the clamp
    zeros = analytic_zeros(kind, r64["grads"])
    assert bn_biases(kind) <= zeros
    for name, g in r64["grads"].items():
        err, scale = np.abs(r32["grads"][name] - g).max(), np.abs(g).max()
        if name in zeros:  # torch's float32 backward leaves rounding noise there, the device an exact zero: nothing to compare
            assert np.isfinite(r32["grads"][name]).all() and np.abs(g).max() <= noise_bound(name, r64["grads"])
        else:
            assert err <= 0.1 * GRAD_RTOL[kind] * scale + 1e-9, (name, err, scale)


def test_full_params_without_a_gpu_fail_in_require_gpu():
    """Argument handling needs no GPU; with full PARAMS and no GPU a builder fails where the library is asked for a device (with
    one it builds: tests/test_cnn_single_gpu.py)."""
    import torch
    from sm_hpss_mtl_amd.lib import baseline_architectures as ba
    cases = () if torch.cuda.is_available() else ((ba.get_Doukhan_model, "Doukhan_et_al", (21, 68, 1)), (ba.get_Papakostas_model, "Papakostas_et_al", (201, 68, 1)),
                                                  (ba.get_Jang_model, "Jang_et_al", (257, 68, 1)))
    for fn, model, shape in cases:
        P = {"Model": model, "input_shape": {model: shape}, "n_fft": {model: 512}}
        with pytest.raises(RuntimeError, match="no HIP device"):
            fn(P)
    with pytest.raises(ValueError, match="t_dim"):
        ba.get_Jang_model({"Model": "Jang_et_al", "input_shape": {"Jang_et_al": (257, 68, 1)}, "n_fft": {"Jang_et_al": 512}}, t_dim=3)
    with pytest.raises(ValueError, match="n_classes"):
        ba.get_Doukhan_model({"Model": "m", "input_shape": {"m": (21, 68, 1)}}, n_classes=5)
