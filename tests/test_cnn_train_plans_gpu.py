"""Training step of the Conv2D MTL baselines where the reduction and split-K plans of smh_cnn_train.hip change: the
re-blocked BatchNorm column reduction (more than kMaxRed row blocks), the 4-slab and the scalar forms of it, 5-class
heads, and every plan switch the trainer reads (SMH_CNN_WSPLIT / DSPLIT / WGRAD_MFMA / POOL_GATHER).  Against
oracle/cnn_mtl_train.py (torch autograd, f64) with the rules of tests/test_cnn_train_gpu.py; the BatchNorm batch
statistics (column sums, untouched by the arg-max flips those rules allow for) within 1e-5 relative plus the f32 floor.
tests/test_cnn_plans.py confirms on the CPU that each case reaches the branch its id names."""
import numpy as np
import pytest

from oracle import b3_mtl

pytestmark = pytest.mark.gpu

RTOL = {"Doukhan": 1e-3, "Papakostas": 1e-3, "Jang": 2e-3}  # as tests/test_cnn_train_gpu.py states them per network
BN_RTOL = 1e-5

# (kind, H, W, N, n_classes, fc, branches): "<branch>:<layer>" items checked by tests/test_cnn_plans.py
TRAIN_CASES = [
    ("Doukhan", 30, 68, 160, 3, 0, "colred-reblocked:conv1"),
    ("Jang", 514, 12, 190, 3, 0, "colred-reblocked:conv1"),
    ("Papakostas", 61, 68, 6, 3, 4096, "colred-slabs4:fc1,colred-slabs4:fc2"),
    # fc 100 is accepted (a multiple of 4); conv1's bias gradient (96 columns) takes the scalar form re-blocked at N = 72
    ("Papakostas", 61, 68, 72, 3, 100, "colred-scalar:fc1,colred-scalar-reblocked:conv1"),
    ("Doukhan", 30, 68, 8, 5, 0, "5-class"),
    ("Papakostas", 61, 68, 6, 5, 64, "5-class"),
    ("Jang", 514, 12, 4, 5, 0, "5-class"),
]
ADAM_CASE = 0  # the largest batch: one Adam step after it

# one case per network with BatchNorm, each plan switch in turn (branch ids checked by tests/test_cnn_plans.py)
FORCED_CASES = [("Doukhan", 30, 68, 40), ("Jang", 514, 12, 8)]
FORCED = [("SMH_CNN_WSPLIT", "1", "wsplit-1"), ("SMH_CNN_WSPLIT", "100", "wsplit-empty-cut"),
          ("SMH_CNN_WSPLIT", "100000", "wsplit-large"), ("SMH_CNN_DSPLIT", "1", "dsplit-1"),
          ("SMH_CNN_DSPLIT", "16", "dsplit-empty"), ("SMH_CNN_WGRAD_MFMA", "1", "wgrad-mfma"),
          ("SMH_CNN_POOL_GATHER", "1", "pool-gather")]


def labels(N, n_classes, seed):
    """Targets in the layout of head_spec(n_classes): S, M (and N) one-hot flags of the class, R uniform, 3C one-hot."""
    rng = np.random.default_rng(seed)
    c = np.arange(N) % n_classes
    flag = {"S": 1, "M": 0, "N": 2}
    y = {}
    for name, odim, act in b3_mtl.head_spec(n_classes):
        y[name] = (c == flag[name]).astype(np.float32)[:, None] if act == "sigmoid" else \
            rng.uniform(0, 1, size=(N, odim)).astype(np.float32)
    y["3C"] = np.eye(n_classes, dtype=np.float32)[c]
    return y


def _setup(kind, H, W, n_classes, fc):
    from oracle import cnn_mtl
    from sm_hpss_mtl_amd.cnn_models import CnnMTL
    if kind == "Doukhan":
        w = cnn_mtl.init_doukhan(seed=3, H=H, W=W, n_classes=n_classes)
    elif kind == "Papakostas":
        w = cnn_mtl.init_papakostas(seed=4, H=H, W=W, n_classes=n_classes, fc=fc)
    else:
        w = cnn_mtl.init_jang(seed=2, W=W, n_classes=n_classes, mel_init=False)
    m = CnnMTL(kind, (H, W, 1), n_classes=n_classes, seed=0, fc_width=fc)
    m.set_weights_dict(w)
    return m, w


def _before_bn(kind, name):
    """Biases in front of a BatchNorm: analytically zero gradients (both sides hold rounding noise only)."""
    if not name.endswith("/bias") or name.endswith("out/bias") or name == "3C/bias":
        return False
    return kind != "Papakostas" or not name.startswith("conv")


def _check_grads(kind, got, ref, ref32):
    """The rule of tests/test_cnn_train_gpu.py for small images: per tensor, max error / max |g| below rtol plus four
    times the distance of the same graph evaluated in float32 by torch."""
    bad, worst = [], ("", 0.0)
    for name, g in ref.items():
        err = np.abs(got[name].astype(np.float64) - g).max()
        if _before_bn(kind, name):
            if kind == "Doukhan" and err > 1e-5 * max(1.0, np.abs(ref[name.replace("/bias", "/kernel")]).max()):
                bad.append("%s: noise %.3e" % (name, err))
            continue
        scale = max(np.abs(g).max(), 1e-12)
        floor = np.abs(ref32[name].astype(np.float64) - g).max()
        if err / scale > worst[1]:
            worst = (name, err / scale)
        if not err / scale < RTOL[kind] + 4 * floor / scale:
            bad.append("%s: max err %.3e (f32 floor %.3e) vs max |g| %.3e" % (name, err, floor, scale))
    assert not bad, "\n".join(bad[:20])
    return worst


def device_bn_batch(m, kind, H, W, n_classes, fc):
    """{BatchNorm name: (batch mean, variance for the moving update)} from the trainer's bucket [gradient | statistics]:
    2 * OC floats per Conv2D / Dense layer in graph order (BatchNorm or not), then 32 per head."""
    from tests import cnn_plans
    st = m._bucket_tensor().cpu().numpy()[m.count_params():]
    out, off = {}, 0
    for L in cnn_plans.graph(kind, H, W, fc=fc or 4096):
        oc, name = L["OC"], L["name"]
        if L["bn"]:
            out["bn" + name[4:] if name.startswith("conv") else name + "_bn"] = (st[off:off + oc], st[off + oc:off + 2 * oc])
        off += 2 * oc
    for h, (name, _, _) in enumerate(b3_mtl.head_spec(n_classes)):
        o = off + 32 * h
        out[name + "/bn"] = (st[o:o + 16], st[o + 16:o + 32])
    return out


def _check_bn(got, ref, ref32):
    """Batch mean relative to the column scale, variance relative to the largest variance: within BN_RTOL plus four
    times the f32 floor (the heads' variances over a handful of rows of a 4096-wide Dense sit at 1.0e-5)."""
    assert sorted(got) == sorted(ref)
    worst = 0.0
    for k, (mr, vr) in ref.items():
        ms, vs = max(np.abs(mr).max(), np.sqrt(vr.max())), vr.max()
        mg, vg = (a.astype(np.float64) for a in got[k])
        em, ev = np.abs(mg - mr).max() / ms, np.abs(vg - vr).max() / vs
        fm, fv = np.abs(ref32[k][0] - mr).max() / ms, np.abs(ref32[k][1] - vr).max() / vs
        worst = max(worst, em, ev)
        assert em <= BN_RTOL + 4 * fm and ev <= BN_RTOL + 4 * fv, \
            "%s: mean %.3e (floor %.3e), variance %.3e (floor %.3e) relative" % (k, em, fm, ev, fv)
    return worst


def _step(m, kind, x, y, ref, n_classes):
    res = dict(zip(m.metrics_names, m.train_on_batch(x, y, drop=None, drop_heads=None, apply=False)))
    for name, _, _ in b3_mtl.head_spec(n_classes):
        assert res[name + "_loss"] == pytest.approx(ref["losses"][name], rel=2e-4, abs=2e-5), name
    assert res["3C_loss"] == pytest.approx(ref["losses"]["3C"], rel=2e-4, abs=2e-5)
    assert res["loss"] == pytest.approx(ref["loss"] + ref["l2"], rel=2e-4)
    return m.gradients()


@pytest.mark.parametrize("kind,H,W,N,n_classes,fc,branch", TRAIN_CASES,
                         ids=["%s-%dx%d-N%d-%dcls-%s" % (c[0], c[1], c[2], c[3], c[4], c[6]) for c in TRAIN_CASES])
def test_train_step_plans_match_autograd(kind, H, W, N, n_classes, fc, branch):
    from oracle import cnn_mtl_train
    m, w = _setup(kind, H, W, n_classes, fc)
    if n_classes == 5:
        assert m.output_names == ["S", "M", "N", "R", "3C"] and m.out_dim == 11
    x = np.random.default_rng(N + W).normal(size=(N, H, W)).astype(np.float32)
    y = labels(N, n_classes, N)
    ref = cnn_mtl_train.forward_backward(x, y, w, n_classes=n_classes, kind=kind)
    ref32 = cnn_mtl_train.forward_backward(x, y, w, n_classes=n_classes, kind=kind, dtype=np.float32)
    got = _step(m, kind, x, y, ref, n_classes)
    worst = _check_grads(kind, got, ref["grads"], ref32["grads"])
    bn = _check_bn(device_bn_batch(m, kind, H, W, n_classes, fc), ref["bn_batch"], ref32["bn_batch"])
    print("%s: worst gradient %s %.2e, worst batch statistic %.2e relative" % (branch, worst[0], worst[1], bn))
    if (kind, H, W, N, n_classes, fc, branch) != TRAIN_CASES[ADAM_CASE]:
        return
    # one Adam step, checked against the oracle's Adam fed with the device gradients (as test_jang_train_step does)
    from oracle import cnn_mtl_train as ot
    g64 = {k: v.astype(np.float64) for k, v in got.items()}
    m.apply_gradients()
    nw, _, _ = ot.adam_step({k: v.astype(np.float64) for k, v in w.items()}, g64, {}, {}, ref["bn_batch"], 1,
                            lr=m.initial_learning_rate, n_classes=n_classes, kind=kind)
    new = m.get_weights_dict()
    for k, v in nw.items():
        tol = 2e-4 * max(1.0, np.abs(v).max()) if k.endswith(("moving_mean", "moving_variance")) else 3e-7 + 2e-6 * np.abs(v).max()
        assert np.abs(new[k].astype(np.float64) - v).max() <= tol, k


@pytest.mark.parametrize("kind,H,W,N", FORCED_CASES, ids=["%s-%dx%d-N%d" % c for c in FORCED_CASES])
def test_forced_plans_match_autograd_and_the_default_plan(kind, H, W, N, monkeypatch):
    """Each switch changes only the order of the sums: every forced run against the oracle with the same rules, and
    within 1e-5 relative of the default plan's gradients.  The gather form of the pooling backward routes each window
    to the same (first) maximum as the tile form and adds nothing but that one value: bit-identical gradients, ties
    included (both forms pick the first maximum in the same scan order)."""
    from oracle import cnn_mtl_train
    for var, _, _ in FORCED:
        monkeypatch.delenv(var, raising=False)
    m, w = _setup(kind, H, W, 3, 0)
    x = np.random.default_rng(N + W).normal(size=(N, H, W)).astype(np.float32)
    y = labels(N, 3, N)
    ref = cnn_mtl_train.forward_backward(x, y, w, kind=kind)
    ref32 = cnn_mtl_train.forward_backward(x, y, w, kind=kind, dtype=np.float32)
    base = _step(m, kind, x, y, ref, 3)
    _check_grads(kind, base, ref["grads"], ref32["grads"])
    for var, val, branch in FORCED:
        monkeypatch.setenv(var, val)
        got = _step(m, kind, x, y, ref, 3)
        monkeypatch.delenv(var)
        worst = _check_grads(kind, got, ref["grads"], ref32["grads"])
        _check_bn(device_bn_batch(m, kind, H, W, 3, 0), ref["bn_batch"], ref32["bn_batch"])
        if branch == "pool-gather":
            for k in base:
                assert np.array_equal(got[k], base[k]), (branch, k)
            continue
        drift = 0.0
        for k, g in base.items():
            if _before_bn(kind, k):
                continue
            d = np.abs(got[k].astype(np.float64) - g).max() / max(np.abs(g).max(), 1e-30)
            drift = max(drift, d)
            assert d <= 1e-5, "%s: %s moved %.3e relative from the default plan" % (branch, k, d)
        print("%s=%s (%s): worst vs oracle %s %.2e, vs default plan %.2e" % (var, val, branch, worst[0], worst[1], drift))
