"""GPU: the late-fusion ensemble (late_fusion.LateFusion over smh_late_fusion_*) on patches.

1. Bit-identity: `heads` equals the two models' own forward_device outputs, `pred` equals numpy's float32 blend of those, `labels`
   equals np.argmax of that, and the paired launch equals SMH_LATE_FUSION_TWO_LAUNCH=1 -- under the default schedule choice and
   under SMH_TCN_SKEW=0 / 2 and SMH_TCN_SPLIT=0.
2. Parity with the float64 reference of tests/late_fusion_ref.py: |pred - ref| <= 1e-4 * max(1, |ref|) -- the bound each model's own
   forward is held to (tests/test_parity_gpu.py); a convex combination cannot exceed it -- and the same labels wherever the
   reference's top-two margin exceeds 2e-4 (at most 1 % of the patches left out; tests/test_late_fusion_ref.py holds the seeds to it).
3. Refusals through Python and the raw C ABI; N = 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import late_fusion_ref as lref

pytestmark = pytest.mark.gpu

NS = (1, 3, 16, 17, 48, 257, 1024)
ALPHAS = (0.5, 0.3, 0.0, 1.0)
SCHEDULES = ({}, {"SMH_TCN_SKEW": "0"}, {"SMH_TCN_SKEW": "2"}, {"SMH_TCN_SPLIT": "0"})


def make_pair(kind, W, ncls, F=120, seed=0):
    """(ensemble, model H, model P, weights H, weights P)."""
    from sm_hpss_mtl_amd.late_fusion import LateFusion
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL
    cls = B3MTL if kind == "mtl" else CascadedMTL
    ws = lref.init_weights(kind, seed, F, W, ncls)
    ms = []
    for w in ws:
        m = cls(n_feat=F, patch_size=W, n_classes=ncls, seed=0)
        m.set_weights_dict(w)
        ms.append(m)
    return LateFusion(ms[0], ms[1]), ms[0], ms[1], ws[0], ws[1]


def np_blend(hH, hP, alpha, ncls):
    """numpy's blend of the two models' float32 '3C' outputs, exactly the driver's expression."""
    pred_H, pred_P = hH[:, -ncls:], hP[:, -ncls:]
    assert pred_H.dtype == pred_P.dtype == np.float32
    return np.add(alpha * pred_H, (1 - alpha) * pred_P)


def _set_env(monkeypatch, env):
    for k in ("SMH_TCN_SKEW", "SMH_TCN_SPLIT", "SMH_LATE_FUSION_TWO_LAUNCH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------------
# 1. bit-identity to the two-call form
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mtl", "cascaded"])
@pytest.mark.parametrize("W,ncls", [(68, 3), (68, 5), (99, 3), (99, 5), (249, 3), (249, 5)])
def test_bit_identical_to_two_forward_calls(kind, W, ncls, monkeypatch):
    F = 120
    ens, mH, mP, _, _ = make_pair(kind, W, ncls, F, seed=W + ncls)
    g = torch.Generator(device="cuda").manual_seed(W * 10 + ncls)
    for N in NS:
        xH, xP = (torch.randn((N, W, F), device="cuda", generator=g) for _ in range(2))
        for env in SCHEDULES:
            what = "%s W=%d ncls=%d N=%d %s" % (kind, W, ncls, N, env)
            _set_env(monkeypatch, env)
            own = [mH.forward_device(xH).cpu().numpy(), mP.forward_device(xP).cpu().numpy()]
            assert np.isfinite(own[0]).all() and np.isfinite(own[1]).all(), what
            for alpha in ALPHAS:
                ens.alpha = alpha
                res = {}
                for two in ("0", "1"):
                    monkeypatch.setenv("SMH_LATE_FUSION_TWO_LAUNCH", two)
                    heads = torch.full((2, N, mH.out_dim), float("nan"), device="cuda")
                    labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
                    pred = ens.forward_device([xH, xP], labels=labels, heads=heads)
                    res[two] = (pred.cpu().numpy(), labels.cpu().numpy(), heads.cpu().numpy())
                monkeypatch.delenv("SMH_LATE_FUSION_TWO_LAUNCH")
                pred, labels, heads = res["0"]
                assert np.array_equal(heads[0], own[0]) and np.array_equal(heads[1], own[1]), what
                want = np_blend(own[0], own[1], alpha, ncls)
                assert pred.dtype == np.float32 and pred.shape == (N, ncls)
                assert np.array_equal(pred, want), (what, alpha)
                assert np.array_equal(labels, np.argmax(want, axis=1)), (what, alpha)
                for a, b in zip(res["0"], res["1"]):
                    assert np.array_equal(a, b), (what, alpha, "paired != two launches")
            if N in (3, 48):  # without the optional outputs: the workspace holds the heads
                assert np.array_equal(ens.forward_device({"harm_input": xH, "perc_input": xP}).cpu().numpy(), pred)
    ens.check_status()


def test_blend_ties_and_predict_surface():
    """Two models with the same weights on the same input give pred_H == pred_P: the blend at alpha = 0.5 returns them unchanged;
    predict / predict_classes / predict_heads return the reference's objects."""
    ens, mH, mP, wH, _ = make_pair("mtl", 68, 3, 120, seed=3)
    mP.set_weights_dict(wH)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((20, 68, 120)).astype(np.float32)
    own = mH.predict(x)
    pred = ens.predict([x, x])
    assert isinstance(pred, np.ndarray) and pred.dtype == np.float32 and np.array_equal(pred, own[-1])
    lab = ens.predict_classes([x, x])
    assert lab.dtype == np.int64 and np.array_equal(lab, np.argmax(own[-1], axis=1))
    hs = ens.predict_heads([x, x])
    assert len(hs) == 2 and all(len(h) == len(own) for h in hs)
    for h in hs:
        assert all(np.array_equal(a, b) for a, b in zip(h, own))
    # the ensemble follows set_weights of either model
    _, wP2 = lref.init_weights("mtl", 50, 120, 68, 3)
    mP.set_weights_dict(wP2)
    ens.alpha = 0.3
    want = np_blend(own[-1], mP.predict(x)[-1], 0.3, 3)
    assert np.array_equal(ens.predict([x, x]), want) and not np.array_equal(want, own[-1])


# ---------------------------------------------------------------------------------------------------
# 2. parity with the float64 reference
# ---------------------------------------------------------------------------------------------------
def check_against_reference(pred, labels, ref, what):
    """pred (N, n_classes) / labels (N) numpy from the device against late_fusion_ref.forward's dict."""
    err = np.abs(pred - ref["pred"])
    bound = 1e-4 * np.maximum(1.0, np.abs(ref["pred"]))
    keep = ref["margin"] > lref.MARGIN
    print("%s: max |pred - ref| = %.3g (bound 1e-4), %d of %d patches outside the label comparison"
          % (what, err.max(), int((~keep).sum()), len(keep)))
    assert np.isfinite(pred).all() and (err <= bound).all(), (what, err.max())
    assert (~keep).sum() <= lref.MAX_LEFT_OUT * len(keep), what
    assert np.array_equal(labels[keep], ref["labels"][keep]), what


@pytest.mark.parametrize("case", lref.PARITY_CASES, ids=lambda c: "%s-W%d-c%d-F%d-N%d-a%g" % c[:6])
def test_parity_with_float64_reference(case):
    from sm_hpss_mtl_amd.late_fusion import LateFusion
    kind, W, ncls, F, N, alpha, seed = case
    xH, xP, wH, wP, ref = lref.case_reference(case)
    ens, mH, mP, _, _ = make_pair(kind, W, ncls, F, seed=seed)
    assert all(np.array_equal(mH.get_weights_dict()[k], wH[k]) for k in wH)
    ens = LateFusion(mH, mP, alpha=alpha)
    labels = torch.empty((N,), dtype=torch.int32, device="cuda")
    heads = torch.empty((2, N, mH.out_dim), device="cuda")
    pred = ens.forward_device([torch.from_numpy(xH).cuda(), torch.from_numpy(xP).cuda()], labels=labels, heads=heads)
    ens.check_status()
    check_against_reference(pred.cpu().numpy(), labels.cpu().numpy(), ref, "late fusion %s" % (case,))
    for i, k in enumerate(("heads_H", "heads_P")):
        assert np.abs(heads[i].cpu().numpy() - ref[k]).max() <= 1e-4 * max(1.0, np.abs(ref[k]).max())


# ---------------------------------------------------------------------------------------------------
# 3. refusals and N = 0
# ---------------------------------------------------------------------------------------------------
def test_python_refusals():
    from sm_hpss_mtl_amd.late_fusion import LateFusion
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL, FusionMTL
    a = B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=0)
    b = B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=1)
    for other in (B3MTL(n_feat=40, patch_size=68, n_classes=3, seed=0), B3MTL(n_feat=120, patch_size=99, n_classes=3, seed=0),
                  B3MTL(n_feat=120, patch_size=68, n_classes=5, seed=0), B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=0, nb_stacks=2),
                  B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=0, n_dilations=6)):
        with pytest.raises(ValueError, match="geometry"):
            LateFusion(a, other)
    with pytest.raises(ValueError, match="head kind"):
        LateFusion(a, CascadedMTL(n_feat=120, patch_size=68, n_classes=3, seed=0))
    with pytest.raises(ValueError, match="intermediate-fusion"):
        LateFusion(a, FusionMTL(n_feat=120, patch_size=68, n_classes=3, seed=0))
    with pytest.raises(ValueError, match="2.3"):
        LateFusion(a, B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=0, tcn_block="2.8"))
    with pytest.raises(ValueError, match="twice"):
        LateFusion(a, a)
    with pytest.raises(TypeError):
        LateFusion(a, object())
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            LateFusion(a, b, alpha=bad)
    ens = LateFusion(a, b)
    assert ens.alpha == 0.5 and ens.n_feat == 120 and ens.patch_size == 68 and ens.n_classes == ens.out_dim == 3
    assert ens.output_names == ["3C"]
    with pytest.raises(ValueError, match="alpha"):
        ens.alpha = 2
    ens.alpha = 1
    assert ens.alpha == 1.0
    x = torch.zeros((4, 68, 120), device="cuda")
    with pytest.raises(TypeError):
        ens.forward_device(x)
    with pytest.raises(ValueError):
        ens.forward_device({"harm_input": x})
    with pytest.raises(ValueError):
        ens.forward_device([x, torch.zeros((3, 68, 120), device="cuda")])
    with pytest.raises(ValueError):
        ens.forward_device([x, torch.zeros((4, 68, 40), device="cuda")])
    with pytest.raises(ValueError):
        ens.forward_device([x, x], out=torch.zeros((4, 7), device="cuda"))
    with pytest.raises(ValueError):
        ens.forward_device([x, x], labels=torch.zeros((4,), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ens.forward_device([x, x], heads=torch.zeros((2, 4, 3), device="cuda"))
    # N = 0: empty outputs, nothing launched
    e = ens.forward_device([torch.zeros((0, 68, 120), device="cuda")] * 2)
    assert tuple(e.shape) == (0, 3)
    ens.check_status()


def test_c_abi_refusals():
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL, FusionMTL
    lib, st = _lib.require_gpu(), _lib.current_stream()
    a = B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=0)
    b = B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=1)
    a._sync_weights(), b._sync_weights()

    def refused(rc):
        assert rc == _lib.SMH_E_INVALID and len(_lib.last_error()) > 0, (rc, _lib.last_error())
        return _lib.last_error()

    def create(x, y):
        h = C.c_void_p()
        return lib.smh_late_fusion_create(x._h if x is not None else None, y._h if y is not None else None, C.byref(h)), h

    assert "geometry" in refused(create(a, B3MTL(n_feat=40, patch_size=68, n_classes=3, seed=0))[0])
    assert "geometry" in refused(create(a, B3MTL(n_feat=120, patch_size=68, n_classes=5, seed=0))[0])
    assert "head kind" in refused(create(CascadedMTL(n_feat=120, patch_size=68, n_classes=3, seed=0), a)[0])
    assert "intermediate-fusion" in refused(create(FusionMTL(n_feat=120, patch_size=68, n_classes=3, seed=0), a)[0])
    assert "block_variant" in refused(create(a, B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=0, tcn_block="2.8"))[0])
    assert "twice" in refused(create(a, a)[0])
    assert "null" in refused(create(a, None)[0])
    rc, e = create(a, b)
    assert rc == 0 and e
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    N = 4
    x = torch.zeros((N, 68, 120), device="cuda")
    x0p = torch.zeros((N, 2, 68, 32), device="cuda")
    fv = torch.zeros((240 * 200 + 4,), device="cuda")
    pred = torch.zeros((200, 3), device="cuda")
    work = torch.zeros((1 << 16,), device="cuda")
    wb = work.numel() * 4
    need = lib.smh_late_fusion_workspace_bytes(e, N)
    assert need == 4 * 2 * N * a.out_dim and need % 16 == 0 and lib.smh_late_fusion_x0_workspace_bytes(e, N) == need
    assert lib.smh_late_fusion_workspace_bytes(e, 3) == 4 * 44  # 2 * 3 * 7 = 42 floats, in whole 16-byte units
    assert lib.smh_late_fusion_workspace_bytes(e, 0) == 0 and lib.smh_late_fusion_workspace_bytes(None, 4) == 0
    fwd = lib.smh_late_fusion_forward_f32
    for alpha in (-0.5, 1.5, float("nan")):
        assert "alpha" in refused(fwd(e, p(x), p(x), N, alpha, p(work), wb, p(pred), None, None, st))
    assert "null workspace" in refused(fwd(e, p(x), p(x), N, 0.5, None, wb, p(pred), None, None, st))
    assert "workspace of" in refused(fwd(e, p(x), p(x), N, 0.5, p(work), need - 4, p(pred), None, None, st))
    assert "16-byte" in refused(fwd(e, p(x), p(x), N, 0.5, p(work, 4), wb - 4, p(pred), None, None, st))
    assert "null" in refused(fwd(e, p(x), None, N, 0.5, p(work), wb, p(pred), None, None, st))
    assert "null" in refused(fwd(None, p(x), p(x), N, 0.5, p(work), wb, p(pred), None, None, st))
    assert "null" in refused(fwd(e, p(x), p(x), N, 0.5, p(work), wb, None, None, None, st))
    refused(fwd(e, p(x), p(x), -1, 0.5, p(work), wb, p(pred), None, None, st))
    assert fwd(e, p(x), p(x), 0, 0.5, None, 0, p(pred), None, None, st) == 0  # N = 0: a no-op, no workspace needed
    fx0 = lib.smh_late_fusion_forward_x0_f32
    assert "alpha" in refused(fx0(e, p(x0p), N, 1.5, p(work), wb, p(pred), None, None, st))
    assert "null workspace" in refused(fx0(e, p(x0p), N, 0.5, None, wb, p(pred), None, None, st))
    assert "workspace of" in refused(fx0(e, p(x0p), N, 0.5, p(work), need - 4, p(pred), None, None, st))
    assert "16-byte" in refused(fx0(e, p(x0p), N, 0.5, p(work, 4), wb - 4, p(pred), None, None, st))
    assert "16-byte" in refused(fx0(e, p(x0p, 4), N - 1, 0.5, p(work), wb, p(pred), None, None, st))
    assert fx0(e, p(x0p), 0, 0.5, None, 0, p(pred), None, None, st) == 0
    fd = lib.smh_late_fusion_forward_dense_f32
    from oracle import frontend as ofe
    nP = len(ofe.patch_starts(200, 68, 1))
    need = lib.smh_late_fusion_dense_workspace_bytes(e, 200, 1)
    assert need == 4 * (2 * 200 * 32 + (2 * nP * a.out_dim + 3) // 4 * 4)
    assert lib.smh_late_fusion_dense_workspace_bytes(e, 100000, 1) == 4 * (2 * 100000 * 32 + 2 * 2048 * a.out_dim)  # bounded by the chunk
    assert lib.smh_late_fusion_dense_workspace_bytes(e, 67, 1) == 0 and lib.smh_late_fusion_dense_workspace_bytes(e, 200, 0) == 0
    assert "alpha" in refused(fd(e, p(fv), 200, 1, -1.0, p(work), wb, p(pred), None, None, st))
    assert "patch_size" in refused(fd(e, p(fv), 67, 1, 0.5, p(work), wb, p(pred), None, None, st))
    assert "shift" in refused(fd(e, p(fv), 200, 0, 0.5, p(work), wb, p(pred), None, None, st))
    assert "null workspace" in refused(fd(e, p(fv), 200, 1, 0.5, None, wb, p(pred), None, None, st))
    assert "workspace of" in refused(fd(e, p(fv), 200, 1, 0.5, p(work), need - 4, p(pred), None, None, st))
    assert "16-byte" in refused(fd(e, p(fv), 200, 1, 0.5, p(work, 4), wb - 4, p(pred), None, None, st))
    assert "16-byte" in refused(fd(e, p(fv, 4), 200, 1, 0.5, p(work), wb, p(pred), None, None, st))
    assert lib.smh_late_fusion_w0_ptr(None, st) is None
    lib.smh_late_fusion_destroy(e)
    lib.smh_late_fusion_destroy(None)
    odd = [B3MTL(n_feat=62, patch_size=68, n_classes=3, seed=s) for s in (0, 1)]
    for m in odd:
        m._sync_weights()
    rc, e2 = create(*odd)
    assert rc == 0
    assert "multiple of 4" in refused(fd(e2, p(fv), 200, 1, 0.5, p(work), wb, p(pred), None, None, st))
    lib.smh_late_fusion_destroy(e2)
    # nothing above launched anything
    torch.cuda.synchronize()
    a.check_status(), b.check_status()
