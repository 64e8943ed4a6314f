"""GPU: the intermediate-fusion model's inference without materialised input halves -- from the feature kernel's per-half layer-0
partials (smh_fusion_forward_x0_f32: Frontend.features_l0 -> FusionMTL.forward_from_x0_halves, pipeline.HotPath) and dense file-level
inference on a whole H||P featuregram (smh_fusion_forward_dense_f32: FusionMTL.forward_dense, inference.patch_probabilities) --
against the float64 reference of tests/fusion_ref.py on the patches themselves, both trunks in one launch against two launches, the
layer-0 operand array (smh_fusion_w0_ptr) against the weights, and the refusals of the new entry points.

Bound on the logits: 1e-4 * max(1, |ref|) and the same '3C' argmax -- what tests/test_fusion_gpu.py holds forward_device to and
tests/test_bench_path_gpu.py the B3_MTL x0 path."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import fusion_ref as fref

pytestmark = pytest.mark.gpu


def _fusion(W=68, F=120, ncls=3, seed=0, wseed=None):
    from sm_hpss_mtl_amd.model import FusionMTL
    m = FusionMTL(n_feat=F, patch_size=W, n_classes=ncls, TR_STEPS=10, seed=seed)
    w = fref.init_weights(seed=W + F if wseed is None else wseed, n_feat=F, patch_size=W, n_classes=ncls, randomize_bn=True)
    m.set_weights_dict(w)
    return m, w


def at_end_of_buffer(x, pad=64):
    """x as a contiguous device tensor whose last element is the last element of its data, with NaN in the `pad` floats that follow
    (the helper of tests/test_model_shapes_gpu.py): a kernel that reads past its input turns outputs into NaN, without a fault."""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.full((x.size + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:x.size] = torch.from_numpy(x.ravel()).cuda()
    return buf[:x.size].view(x.shape)


def _check(got, ref, ncls, what):
    """got (N, out_dim) device tensor or array, ref: fusion_ref.forward's list."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = np.concatenate(ref, axis=1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = np.abs(got - ref).max(), 1e-4 * max(1.0, np.abs(ref).max())
    print("%s: max |diff| = %.3g (bound %.3g)" % (what, err, bound))
    assert np.isfinite(got).all() and err <= bound, (what, err)
    assert np.array_equal(got[:, -ncls:].argmax(1), ref[:, -ncls:].argmax(1)), what


def _clips(B, seed):
    """B one-second clips: the synthetic speech / music / noise clips with white noise of a random level on top."""
    from sm_hpss_mtl_amd.synth import synth_clips
    rng = np.random.default_rng(seed)
    y = synth_clips(B, seed=seed)
    return (y + rng.standard_normal(y.shape) * rng.uniform(0.0, 0.1, (B, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# 1. x0 halves == patches
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ncls,n_mels", [(68, 3, 120), (99, 5, 120), (68, 5, 40), (99, 3, 40)])
def test_x0_halves_match_reference_on_the_patches(W, ncls, n_mels):
    """features_l0(model=fusion) on the device's own S / harm / perc -> forward_from_x0_halves, against fusion_ref.forward on the
    halves of the patches the same call returned.  One patch per clip (hop = W), so B * nP = B: one workgroup, a partial 16-row tile
    of fusion_dense_kernel, a partial last trunk workgroup (257 patches: two per workgroup)."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    fe = Frontend(FrontendConfig(n_mels=n_mels))
    m, w = _fusion(W, n_mels, ncls)
    for B in (1, 3, 16, 17, 257):
        audio = torch.from_numpy(_clips(B, seed=B + W)).cuda()
        taps = fe.run(audio, taps=True)
        res = fe.features_l0(taps["S"], taps["harm"], taps["perc"], 0, W, W, m, patches=True)
        assert res["n_patches"] == 1 and tuple(res["x0p"].shape) == (B, 2, W, 32)
        got = m.forward_from_x0_halves(res["x0p"])
        m.check_status()
        p = res["patches"].cpu().numpy()
        assert p.shape == (B, W, 2 * n_mels) and np.isfinite(p).all()
        ref = fref.forward(p[:, :, :n_mels], p[:, :, n_mels:], w, ncls)
        _check(got, ref, ncls, "x0 halves W=%d ncls=%d n_mels=%d N=%d" % (W, ncls, n_mels, B))
        # and the device's own patch path on the same halves
        dev = m.forward_device([res["patches"][:, :, :n_mels], res["patches"][:, :, n_mels:]])
        assert float((got - dev).abs().max()) <= 1e-4


# ---------------------------------------------------------------------------------------------------
# 2. dense == patches
# ---------------------------------------------------------------------------------------------------
def _host_patches(fv, W, shift, sel=None):
    starts = ofe.patch_starts(fv.shape[1], W, shift)
    idx = range(len(starts)) if sel is None else sel
    x = np.stack([fv[:, starts[i]:starts[i] + W].T for i in idx]) if len(starts) else np.zeros((0, W, fv.shape[0]), np.float32)
    return starts, x


# (68, 1, 68): an even W at Tc = W has NO patch on tools.extract_patches' grid (centres range(34, 34)); (68, 1, 69) is the one-patch
# case.  (68, 3, 517): the last centre (481) is the last one whose window still fits, 2 frames short of the end.
# (68, 2, 4200): 2067 patches, past one 2048-patch chunk of the dense entry.
@pytest.mark.parametrize("W,shift,Tc", [(68, 1, 68), (68, 1, 69), (68, 1, 300), (68, 3, 517), (25, 7, 400), (99, 1, 1000),
                                        (68, 2, 4200)])
def test_dense_matches_reference_on_host_patches(W, shift, Tc):
    m, w = _fusion(W, 120, 3)
    rng = np.random.default_rng(W + shift + Tc)
    fv = rng.standard_normal((240, Tc)).astype(np.float32)
    starts, x = _host_patches(fv, W, shift)
    nP = m.lib.smh_num_patches(Tc, W, shift)
    assert nP == len(starts)
    got = m.forward_dense(at_end_of_buffer(fv), shift)
    m.check_status()
    assert tuple(got.shape) == (nP, m.out_dim)
    assert all(s == i * shift and s + W <= Tc for i, s in enumerate(starts))  # (on this grid no window needs the clamp to Tc - W)
    if nP == 0:
        return
    sel = np.arange(nP)
    if nP > 2048:  # the float64 reference on a strided subset plus both ends and both sides of the chunk boundary
        sel = np.unique(np.concatenate([np.arange(0, nP, 9), np.arange(20), np.arange(nP - 20, nP), np.arange(2038, 2058)]))
        assert sel.size >= 200 and 2047 in sel and 2048 in sel
    ref = fref.forward(x[sel][:, :, :120], x[sel][:, :, 120:], w, 3)
    _check(got[torch.from_numpy(sel).cuda()], ref, 3, "dense W=%d shift=%d Tc=%d" % (W, shift, Tc))


def test_dense_one_chunk_of_10000_frames():
    """One batch of the file walk: 10 000 frames at hop 1 (9 932 patches, five chunks of the dense entry) -- the float64 reference on
    a strided subset of >= 200 patches plus the first and last 20 and the patches around every chunk boundary; every other row
    against the device's own patch path."""
    W, Tc = 68, 10000
    m, w = _fusion(W, 120, 3)
    fv = np.random.default_rng(5).standard_normal((240, Tc)).astype(np.float32)
    got = m.forward_dense(at_end_of_buffer(fv), 1)
    m.check_status()
    starts = ofe.patch_starts(Tc, W, 1)
    nP = len(starts)
    assert nP == m.lib.smh_num_patches(Tc, W, 1) == 9932 and tuple(got.shape) == (nP, m.out_dim)
    edges = np.concatenate([np.arange(c - 3, c + 3) for c in range(2048, nP, 2048)])
    sel = np.unique(np.concatenate([np.arange(0, nP, 45), np.arange(20), np.arange(nP - 20, nP), edges]))
    assert sel.size >= 240
    x = np.stack([fv[:, starts[i]:starts[i] + W].T for i in sel])
    ref = fref.forward(x[:, :, :120], x[:, :, 120:], w, 3)
    _check(got[torch.from_numpy(sel).cuda()], ref, 3, "dense 10000 frames")
    dfv = torch.from_numpy(fv).cuda()
    for lo in range(0, nP, 2500):  # all rows: the windows of the frame-level layer 0 against materialised halves
        hi = min(lo + 2500, nP)
        xs = dfv.unfold(1, W, 1)[:, lo:hi].permute(1, 2, 0)  # (n, W, 240)
        dev = m.forward_device([xs[:, :, :120].contiguous(), xs[:, :, 120:].contiguous()])
        assert float((got[lo:hi] - dev).abs().max()) <= 1e-4, lo


# ---------------------------------------------------------------------------------------------------
# 3. one launch == two launches
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew", [None, "2"])
def test_one_launch_equals_two_launches(skew, monkeypatch):
    if skew is None:
        monkeypatch.delenv("SMH_TCN_SKEW", raising=False)
    else:
        monkeypatch.setenv("SMH_TCN_SKEW", skew)
    m, _ = _fusion(68, 120, 3)
    g = torch.Generator(device="cuda").manual_seed(3)
    runs = []
    for N in (1, 48, 300, 1030):
        x0p = torch.randn((N, 2, 68, 32), device="cuda", generator=g)
        runs.append(("x0 N=%d" % N, lambda x=x0p: m.forward_from_x0_halves(x)))
        xs = [torch.randn((N, 68, 120), device="cuda", generator=g) for _ in range(2)]
        runs.append(("patches N=%d" % N, lambda x=xs: m.forward_device(x)))
    for shift, Tc in ((1, 600), (3, 700), (1, 2300)):
        fv = torch.randn((240, Tc), device="cuda", generator=g)
        runs.append(("dense shift=%d Tc=%d" % (shift, Tc), lambda f=fv, s=shift: m.forward_dense(f, s)))
    for what, fn in runs:
        monkeypatch.delenv("SMH_FUSION_TWO_LAUNCH", raising=False)
        one = fn().clone()
        monkeypatch.setenv("SMH_FUSION_TWO_LAUNCH", "1")
        two = fn().clone()
        m.check_status()
        assert torch.isfinite(one).all() and torch.equal(one, two), what


# ---------------------------------------------------------------------------------------------------
# 4. determinism and edges
# ---------------------------------------------------------------------------------------------------
def test_determinism_and_edges():
    m, _ = _fusion(68, 120, 3)
    rng = np.random.default_rng(11)
    for N in (1, 5, 257):
        x0p = at_end_of_buffer(rng.standard_normal((N, 2, 68, 32)))
        a, b = m.forward_from_x0_halves(x0p).clone(), m.forward_from_x0_halves(x0p).clone()
        assert torch.isfinite(a).all() and torch.equal(a, b), N
    for shift, Tc in ((1, 69), (1, 500), (5, 333)):
        fv = at_end_of_buffer(rng.standard_normal((240, Tc)))
        a, b = m.forward_dense(fv, shift).clone(), m.forward_dense(fv, shift).clone()
        assert torch.isfinite(a).all() and torch.equal(a, b), (shift, Tc)
    # N = 0: an empty tensor, nothing launched (no workspace is even passed)
    e = m.forward_from_x0_halves(torch.empty((0, 2, 68, 32), device="cuda"))
    assert tuple(e.shape) == (0, m.out_dim)
    assert m.lib.smh_fusion_forward_x0_f32(m._h, C.c_void_p(16), 0, None, 0, C.c_void_p(16), None) == 0
    e = m.forward_dense(torch.zeros((240, 68), device="cuda"))  # Tc = W, even W: no patch
    assert tuple(e.shape) == (0, m.out_dim)
    out_of = torch.empty((3, m.out_dim), device="cuda")
    got = m.forward_from_x0_halves(at_end_of_buffer(rng.standard_normal((3, 2, 68, 32))), out=out_of)
    assert got is out_of
    m.check_status()


# ---------------------------------------------------------------------------------------------------
# 5. smh_fusion_w0_ptr follows the weights
# ---------------------------------------------------------------------------------------------------
def _read_w0(m):
    """The (2 * n_feat, 32) array behind smh_fusion_w0_ptr, read back with a device-to-device copy."""
    ptr = m.lib.smh_fusion_w0_ptr(m._h)
    assert ptr
    dst = torch.empty((2 * m.n_feat, 32), device="cuda")
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(ptr), dst.numel() * 4, 3) == 0  # hipMemcpyDeviceToDevice
    return dst.cpu().numpy()


def _w0_of(w):
    return np.concatenate([np.asarray(w["tcn_%s/initial_conv/kernel" % t], np.float32).reshape(-1, 32) for t in "HP"])


def test_w0_ptr_follows_the_weights():
    m, w = _fusion(68, 120, 3)
    m._sync_weights()
    assert np.array_equal(_read_w0(m), _w0_of(w))
    w2 = fref.init_weights(seed=77, n_feat=120, patch_size=68, n_classes=3, randomize_bn=True)
    m.set_weights_dict(w2)
    m._sync_weights()
    assert np.array_equal(_read_w0(m), _w0_of(w2)) and not np.array_equal(_w0_of(w), _w0_of(w2))
    rng = np.random.default_rng(0)
    N = 12
    x0p = torch.from_numpy(rng.standard_normal((N, 2, 68, 32)).astype(np.float32)).cuda()
    before = m.forward_from_x0_halves(x0p).clone()
    xs = [rng.standard_normal((N, 68, 120)).astype(np.float32) for _ in range(2)]
    cls = rng.integers(0, 3, N)
    y = {"S": (cls == 1).astype(np.float32)[:, None], "M": (cls == 0).astype(np.float32)[:, None],
         "R": rng.random((N, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[cls]}
    m.compile()
    m.train_on_batch(xs, y, drop_tcn=None, drop_heads=None, apply=True)
    after_w = m.get_weights_dict()
    assert not np.array_equal(_w0_of(after_w), _w0_of(w2))  # the step moved the layer-0 kernels
    assert np.array_equal(_read_w0(m), _w0_of(after_w))
    after = m.forward_from_x0_halves(x0p)
    assert not torch.equal(before, after)
    m.check_status()
    # a B3_MTL model has no such array
    from sm_hpss_mtl_amd.model import B3MTL
    b3 = B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=0)
    assert b3.lib.smh_fusion_w0_ptr(b3._h) is None


# ---------------------------------------------------------------------------------------------------
# 6. pipeline
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 48])
def test_hotpath_with_a_fusion_model(B):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.pipeline import HotPath
    from sm_hpss_mtl_amd.synth import synth_clips
    fe = Frontend(FrontendConfig())
    m, w = _fusion(68, 120, 3)
    audio = torch.from_numpy(synth_clips(B, seed=4)).cuda()
    fused = HotPath(fe, m, batch=B, n_samples=16000, keep_patches=True)
    plain = HotPath(fe, m, batch=B, n_samples=16000, keep_patches=True, fuse_l0=False)
    assert fused.fuse_l0 and not plain.fuse_l0
    a, b = fused.step(audio).clone(), plain.step(audio).clone()
    m.check_status()
    assert tuple(a.shape) == (B * fused.nP, m.out_dim) and torch.isfinite(a).all()
    bound = 1e-4 * max(1.0, float(a.abs().max()), float(b.abs().max()))
    err = float((a - b).abs().max())
    print("HotPath fuse_l0 True / False: max |diff| = %.3g (bound %.3g)" % (err, bound))
    assert err <= bound
    assert torch.equal(a[:, -3:].argmax(1), b[:, -3:].argmax(1))
    assert torch.equal(fused.patches, plain.patches)
    dev = m.forward_device([plain.patches[:, :, :120], plain.patches[:, :, 120:]])
    assert torch.equal(b, dev)
    p = plain.patches.cpu().numpy()
    _check(a, fref.forward(p[:, :, :120], p[:, :, 120:], w, 3), 3, "HotPath fused B=%d" % B)
    with pytest.raises(ValueError):
        HotPath(fe, m, batch=B, n_samples=16000, keep_trunk=True)
    with pytest.raises(ValueError):
        HotPath(fe, m, batch=B, n_samples=16000, model_dtype="bf16")


# ---------------------------------------------------------------------------------------------------
# 7. patch_probabilities
# ---------------------------------------------------------------------------------------------------
def test_patch_probabilities_dense_and_patch_tracks_agree(monkeypatch):
    from sm_hpss_mtl_amd import inference as inf
    m, w = _fusion(68, 120, 3)
    rng = np.random.default_rng(8)
    fv = (rng.standard_normal((240, 3000)) * rng.uniform(0.5, 2.0, (240, 1)) + rng.normal(0, 1, (240, 1))).astype(np.float32)
    names = m.output_names
    for output in ("S", "M", "3C"):
        monkeypatch.delenv("SMH_DENSE_PATCHES", raising=False)
        dense = inf.patch_probabilities(fv, m, 68, 1, output=output, batch_frames=1100)
        monkeypatch.setenv("SMH_DENSE_PATCHES", "1")
        built = inf.patch_probabilities(fv, m, 68, 1, output=output, batch_frames=1100)
        n = 2 * len(ofe.patch_starts(1100, 68, 1)) + len(ofe.patch_starts(800, 68, 1))
        assert dense.shape == built.shape == (n,) and dense.dtype == np.float32
        err = float(np.abs(dense - built).max())
        print("patch_probabilities %s: dense / patch tracks max |diff| = %.3g" % (output, err))
        assert np.isfinite(dense).all() and err <= 1e-4
        assert output in names
        sm = inf.medfilt(dense, 501)
        assert sm.shape == dense.shape and np.isfinite(sm).all()
    # the first batch against the float64 reference: get_feature_patches standardises each half over the batch
    monkeypatch.delenv("SMH_DENSE_PATCHES", raising=False)
    track = inf.patch_probabilities(fv, m, 68, 1, output="S", batch_frames=1100)
    whole = (fv.astype(np.float64) - fv.mean(1, keepdims=True)) / fv.std(1, keepdims=True)
    chunk = whole[:, :1100]
    chunk = ((chunk - chunk.mean(1, keepdims=True)) / chunk.std(1, keepdims=True)).astype(np.float32)
    _, x = _host_patches(chunk, 68, 1, sel=range(0, 1032, 40))
    ref = fref.forward(x[:, :, :120], x[:, :, 120:], w, 3)[0][:, 0]
    assert np.abs(track[0:1032:40] - ref).max() <= 1e-4
    # a W the model was not built for takes the patch path, which refuses it
    with pytest.raises(ValueError):
        inf.patch_probabilities(fv, m, 99, 1, output="S")


# ---------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals():
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.model import B3MTL
    from sm_hpss_mtl_amd.pipeline import HotPath
    m, _ = _fusion(68, 120, 3)
    m._sync_weights()
    b3 = B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=0)
    b3._sync_weights()
    lib, st = m.lib, _lib.current_stream()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    x0p = torch.zeros((2, 2, 68, 32), device="cuda")
    fv = torch.zeros((240 * 200 + 4,), device="cuda")
    out = torch.zeros((200, m.out_dim), device="cuda")
    work = torch.zeros((1 << 22,), device="cuda")
    wb = work.numel() * 4

    def refused(rc):
        assert rc == _lib.SMH_E_INVALID and len(_lib.last_error()) > 0, (rc, _lib.last_error())
        return _lib.last_error()

    # a B3_MTL handle on every smh_fusion_* symbol of this change
    assert lib.smh_fusion_w0_ptr(b3._h) is None
    assert lib.smh_fusion_x0_workspace_bytes(b3._h, 4) == 0 and lib.smh_fusion_dense_workspace_bytes(b3._h, 200, 1) == 0
    assert "fusion" in refused(lib.smh_fusion_forward_x0_f32(b3._h, p(x0p), 2, p(work), wb, p(out), st))
    assert "fusion" in refused(lib.smh_fusion_forward_dense_f32(b3._h, p(fv), 200, 1, p(work), wb, p(out), st))
    # the fusion model: short chunk, hop 0, misaligned inputs, short workspaces
    assert "patch_size" in refused(lib.smh_fusion_forward_dense_f32(m._h, p(fv), 67, 1, p(work), wb, p(out), st))
    assert "shift" in refused(lib.smh_fusion_forward_dense_f32(m._h, p(fv), 200, 0, p(work), wb, p(out), st))
    assert "16-byte" in refused(lib.smh_fusion_forward_dense_f32(m._h, p(fv, 4), 200, 1, p(work), wb, p(out), st))
    assert "16-byte" in refused(lib.smh_fusion_forward_dense_f32(m._h, p(fv), 200, 1, p(work, 4), wb - 4, p(out), st))
    need = lib.smh_fusion_dense_workspace_bytes(m._h, 200, 1)
    assert need == 4 * (2 * 200 * 32 + len(ofe.patch_starts(200, 68, 1)) * 2 * 68 * 32)
    assert lib.smh_fusion_dense_workspace_bytes(m._h, 10000, 1) == 4 * (2 * 10000 * 32 + 2048 * 2 * 68 * 32)  # bounded by the chunk
    assert "workspace" in refused(lib.smh_fusion_forward_dense_f32(m._h, p(fv), 200, 1, p(work), need - 4, p(out), st))
    assert lib.smh_fusion_dense_workspace_bytes(m._h, 67, 1) == 0 and lib.smh_fusion_dense_workspace_bytes(m._h, 200, 0) == 0
    need = lib.smh_fusion_x0_workspace_bytes(m._h, 2)
    assert need == 4 * 2 * 2 * 68 * 32
    assert "workspace" in refused(lib.smh_fusion_forward_x0_f32(m._h, p(x0p), 2, p(work), need - 4, p(out), st))
    assert "16-byte" in refused(lib.smh_fusion_forward_x0_f32(m._h, p(x0p, 4), 1, p(work), wb, p(out), st))
    refused(lib.smh_fusion_forward_x0_f32(m._h, p(x0p), -1, p(work), wb, p(out), st))
    # per-branch n_feat off the four-row steps of the frame-level layer 0
    from sm_hpss_mtl_amd.model import FusionMTL
    odd = FusionMTL(n_feat=61, patch_size=68, n_classes=3, seed=0)
    odd._sync_weights()
    assert "multiple of 4" in refused(lib.smh_fusion_forward_dense_f32(odd._h, p(fv), 200, 1, p(work), wb, p(out), st))
    # nothing above launched anything
    torch.cuda.synchronize()
    m.check_status()
    # Python surface
    with pytest.raises(ValueError):
        m.forward_dense(torch.zeros((120, 200), device="cuda"))
    with pytest.raises(ValueError):
        m.forward_dense(torch.zeros((240, 67), device="cuda"))
    with pytest.raises(ValueError):
        m.forward_dense(torch.zeros((240, 200), device="cuda"), shift=0)
    with pytest.raises((TypeError, ValueError)):
        m.forward_dense(torch.zeros((240, 200)))
    with pytest.raises((TypeError, ValueError)):
        m.forward_from_x0_halves(torch.zeros((2, 2, 68, 32)))
    with pytest.raises(ValueError):
        m.forward_from_x0_halves(torch.zeros((2, 2, 99, 32), device="cuda"))
    with pytest.raises(ValueError):
        m.forward_from_x0_halves(x0p, out=torch.zeros((3, m.out_dim), device="cuda"))
    with pytest.raises(ValueError) as ei:
        m.forward_from_x0(x0p)
    assert "forward_from_x0_halves" in str(ei.value)
    fe = Frontend(FrontendConfig())
    S = torch.zeros((1, fe.K, 98), device="cuda")
    with pytest.raises(ValueError):  # wrong W
        fe.features_l0(S, S, S, 0, 99, 99, m)
    fe40 = Frontend(FrontendConfig(n_mels=40))
    S40 = torch.zeros((1, fe40.K, 98), device="cuda")
    with pytest.raises(ValueError):  # 2 * n_feat != the featuregram's rows
        fe40.features_l0(S40, S40, S40, 0, 68, 68, m)
    with pytest.raises(ValueError):
        HotPath(fe, m, batch=2, n_samples=16000, patch=99)
    with pytest.raises(ValueError):
        HotPath(fe40, m, batch=2, n_samples=16000)
    with pytest.raises(ValueError):
        HotPath(fe, m, batch=2, n_samples=16000, keep_trunk=True)
    with pytest.raises(ValueError):
        HotPath(fe, m, batch=2, n_samples=16000, model_dtype="bf16")
