"""Dense file-level inference on split bf16 operands (smh_model_forward_dense_bf16; B3MTL.forward_dense(dtype="bf16");
inference.patch_probabilities(dtype="bf16")) and the driver's single-output sub-model in patch_probabilities.

The dense bf16 entry is the split-operand kernel of tests/test_bf16_gpu.py reading every patch as a window of the per-frame layer-0
partials (2, Tc, 32) that l0_frames_kernel leaves in d_work.  So it is held to two things:
  1. bit-identity with `forward_from_x0(dtype="bf16")` on the same windows gathered into (N, 2, W, 32) -- same N, hence the same launch
     plan, the same sums in the same order; no tolerance;
  2. the bounds tests/test_bf16_gpu.py already holds the split kernel to at these seeds: 1e-4 of the f32 kernel and of the oracle,
     '3C' argmax agreement >= 99.5 %.
Shapes: the smallest that reach every branch of the plan, G = min(ceil(N / 256), 272 // W) patches per workgroup."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import b3_mtl, frontend as ofe
from tests import tcn_plans

pytestmark = pytest.mark.gpu

TOL_SPLIT = 1e-4    # tests/test_bf16_gpu.py
MIN_AGREE = 0.995   # tests/test_bf16_gpu.py
SEEDS = {(3, 68): 7, (5, 68): 1, (3, 99): 2}  # the weights tests/test_bf16_gpu.py holds to 1e-4
F32, BF16 = "smh_model_forward_dense_f32", "smh_model_forward_dense_bf16"

# (W, shift, Tc, classes, patches N, patches per workgroup G)
ROWS = [
    (68, 1, 1001, 3, 933, 4),   # 17 column tiles on 9 waves; the last workgroup holds 1 of 4 patches
    (68, 1, 700, 5, 632, 3),    # 13 tiles; the last workgroup holds 2 of 3; 5-class heads
    (68, 3, 517, 3, 150, 1),    # a hop that is not 1; one patch per workgroup
    (99, 1, 400, 3, 302, 2),    # odd W; 13 tiles
    (99, 7, 169, 3, 11, 1),     # hop 7; few patches
    (68, 1, 69, 3, 1, 1),       # a single patch
    (68, 5, 68, 3, 0, 0),       # no patch: (0, out_dim), nothing launched
]
IDS = ["W%d-s%d-T%d-c%d" % r[:4] for r in ROWS]


@functools.lru_cache(maxsize=None)
def _model(ncls, W):
    from sm_hpss_mtl_amd.model import B3MTL
    w = b3_mtl.init_weights(seed=SEEDS[(ncls, W)], n_feat=240, patch_size=W, n_classes=ncls, randomize_bn=True)
    m = B3MTL(n_feat=240, patch_size=W, n_classes=ncls, seed=0)
    m.set_weights_dict(w)
    return m, w


@functools.lru_cache(maxsize=None)
def _fv(Tc):
    return np.random.default_rng(Tc).standard_normal((240, Tc)).astype(np.float32)


def _p(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset)


def _dense_c(m, entry, fv, shift, work, work_bytes, out, work_offset=0, Tc=None):
    from sm_hpss_mtl_amd import _lib
    m._sync_weights()
    return getattr(m.lib, entry)(m._h, _p(fv), fv.shape[1] if Tc is None else Tc, shift, _p(work, work_offset), work_bytes, _p(out),
                                 _lib.current_stream())


def test_table_matches_the_plan_and_stays_in_bounds():
    """The table's counts and plans from the shapes alone, and -- before anything reads a window on the device -- that the last frame
    of the last patch is a row of the (2, Tc, 32) array in both halves."""
    for W, shift, Tc, ncls, N, G in ROWS:
        starts = ofe.patch_starts(Tc, W, shift)
        assert len(starts) == N == len(range(W // 2, Tc - W // 2, shift))
        assert starts == [min(p * shift, Tc - W) for p in range(N)]
        if N:
            assert G == tcn_plans.group(W, 240, N)[0]
            last = starts[-1] + W - 1
            assert 0 <= starts[0] and last <= Tc - 1 and Tc + last <= 2 * Tc - 1


@pytest.mark.parametrize("W,shift,Tc,ncls,N,G", ROWS, ids=IDS)
def test_windows_bit_identical_to_gathered_partials(W, shift, Tc, ncls, N, G):
    """1. The window is read correctly: the C entry's output equals forward_from_x0(dtype="bf16") on the windows of d_work, bit for
    bit; and the f32 dense entry leaves the same d_work bits."""
    m, _ = _model(ncls, W)
    fv = torch.from_numpy(_fv(Tc)).cuda()
    nbytes = m.lib.smh_model_dense_workspace_bytes(m._h, Tc)
    assert nbytes == 4 * 2 * Tc * 32
    work = torch.full((2, Tc, 32), -7.0, device="cuda")
    work32 = torch.full((2, Tc, 32), -7.0, device="cuda")
    out = torch.full((max(N, 1), m.out_dim), -7.0, device="cuda")
    out32 = torch.full((max(N, 1), m.out_dim), -7.0, device="cuda")
    assert _dense_c(m, BF16, fv, shift, work, nbytes, out) == N
    assert _dense_c(m, F32, fv, shift, work32, nbytes, out32) == N
    torch.cuda.synchronize()
    if N == 0:  # nothing launched: neither the per-frame pass nor the forward
        assert bool((work == -7.0).all()) and bool((out == -7.0).all())
        assert tuple(m.forward_dense(fv, shift, dtype="bf16").shape) == (0, m.out_dim)
        return
    assert torch.equal(work, work32)
    starts = torch.tensor(ofe.patch_starts(Tc, W, shift), device="cuda")
    idx = starts[:, None] + torch.arange(W, device="cuda")[None]
    x0p = work[:, idx].permute(1, 0, 2, 3).contiguous()  # (N, 2, W, 32)
    ref = m.forward_from_x0(x0p, dtype="bf16")
    api = m.forward_dense(fv, shift, dtype="bf16")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref)
    assert torch.equal(api, out)


@pytest.mark.parametrize("W,shift,Tc,ncls,N,G", [r for r in ROWS if r[4]], ids=[i for i, r in zip(IDS, ROWS) if r[4]])
def test_dense_bf16_close_to_f32_and_oracle(W, shift, Tc, ncls, N, G):
    """2. Closeness, with the bounds of tests/test_bf16_gpu.py."""
    m, w = _model(ncls, W)
    fv = _fv(Tc)
    d = torch.from_numpy(fv).cuda()
    ref = m.forward_dense(d, shift)
    got = m.forward_dense(d, shift, dtype="bf16")
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (N, m.out_dim) and torch.isfinite(got).all()
    err = float((got - ref).abs().max())
    agree = float((got[:, -ncls:].argmax(1) == ref[:, -ncls:].argmax(1)).float().mean())
    n8 = min(8, N)
    patches = np.stack([fv[:, s:s + W].T for s in ofe.patch_starts(Tc, W, shift)[:n8]])
    small = np.concatenate(b3_mtl.forward(patches, w, ncls), axis=1)
    oerr = float(np.max(np.abs(got[:n8].cpu().numpy() - small)))
    print("dense bf16 W=%d shift=%d Tc=%d: vs dense f32 max abs %.3e, argmax agreement %.4f, vs oracle (first %d) %.3e"
          % (W, shift, Tc, err, agree, n8, oerr))
    assert err <= TOL_SPLIT and agree >= MIN_AGREE, (err, agree)
    assert oerr <= TOL_SPLIT


def _tracks(inf, fv, m, W, **kw):
    return {dt: inf.patch_probabilities(fv, m, W, 1, "M", dtype=dt, **kw) for dt in ("f32", "bf16")}


def test_patch_probabilities_bf16(monkeypatch):
    """3. Two full chunks of 1000 frames and one of 500, through the dense branch and (SMH_DENSE_PATCHES=1) through the built
    patches: each bf16 track against the dense f32 track (the built path computes layer 0 on split operands, the dense path in exact
    f32 -- they are not compared with each other)."""
    from sm_hpss_mtl_amd import inference as inf
    m, _ = _model(3, 68)
    fv = np.random.default_rng(2500).standard_normal((240, 2500)).astype(np.float32) * 10 - 40
    monkeypatch.delenv("SMH_DENSE_PATCHES", raising=False)
    t = _tracks(inf, fv, m, 68, batch_frames=1000)
    assert t["f32"].shape == t["bf16"].shape == (2 * 932 + 432,)
    err = float(np.max(np.abs(t["bf16"] - t["f32"])))
    monkeypatch.setenv("SMH_DENSE_PATCHES", "1")
    b = _tracks(inf, fv, m, 68, batch_frames=1000)
    errs = {dt: float(np.max(np.abs(b[dt] - t["f32"]))) for dt in b}
    print("patch_probabilities: dense bf16 vs dense f32 %.3e; built patches vs dense f32: f32 %.3e, bf16 %.3e" % (err, errs["f32"], errs["bf16"]))
    assert b["bf16"].shape == t["f32"].shape
    assert err <= TOL_SPLIT and errs["bf16"] <= TOL_SPLIT and errs["f32"] <= TOL_SPLIT


def test_patch_probabilities_bf16_short_last_chunk(monkeypatch):
    """3. (cont.) The 298-frame file of test_patch_probabilities_vs_oracle in batches of 120: the last chunk (58 frames) is shorter
    than W, is tiled and takes the built-patch branch with forward_device(dtype="bf16")."""
    from sm_hpss_mtl_amd import inference as inf
    from sm_hpss_mtl_amd.synth import synth_clips
    monkeypatch.delenv("SMH_DENSE_PATCHES", raising=False)
    fv = ofe.featuregram(synth_clips(1, seed=3, n_samples=48000)[0], "LogMelHarmPercSpec")
    assert fv.shape == (240, 298)
    m, _ = _model(3, 68)
    t = _tracks(inf, fv, m, 68, batch_frames=120)
    assert t["f32"].shape == t["bf16"].shape == (2 * (120 - 68) + len(ofe.patch_starts(116, 68, 1)),)
    err = float(np.max(np.abs(t["bf16"] - t["f32"])))
    print("patch_probabilities, 298 frames in batches of 120: bf16 vs f32 %.3e" % err)
    assert err <= TOL_SPLIT


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["M", "S"])
def test_sub_model_track_is_the_full_models_column(name, dtype, monkeypatch):
    """4. The driver's Model(model.input, model.get_layer(name).output) goes straight into the file-level call."""
    from sm_hpss_mtl_amd import inference as inf
    from sm_hpss_mtl_amd.persistence import HeadModel, Model
    monkeypatch.delenv("SMH_DENSE_PATCHES", raising=False)
    m, _ = _model(3, 68)
    fv = _fv(700) * 10 - 40
    sub = Model(m.input, m.get_layer(name).output)
    assert isinstance(sub, HeadModel)
    got = inf.patch_probabilities(fv, sub, 68, dtype=dtype)
    ref = inf.patch_probabilities(fv, m, 68, output=name, dtype=dtype)
    assert got.shape == ref.shape == (632,) and np.array_equal(got, ref)
    assert np.array_equal(inf.patch_probabilities(fv, sub, 68, output=name, dtype=dtype), ref)
    other = "S" if name == "M" else "M"
    assert not np.array_equal(inf.patch_probabilities(fv, m, 68, output=other, dtype=dtype), ref)
    with pytest.raises(ValueError):
        inf.patch_probabilities(fv, sub, 68, output=other, dtype=dtype)


def test_refusals_python():
    """5. An unknown dtype, and "bf16" on every model without a bf16 path, are ValueErrors before anything is launched."""
    from sm_hpss_mtl_amd import inference as inf
    from sm_hpss_mtl_amd.late_fusion import LateFusion
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL, FusionMTL, SingleTaskTCN
    m, _ = _model(3, 68)
    fv = torch.from_numpy(_fv(100)).cuda()
    out = torch.full((32, m.out_dim), -7.0, device="cuda")
    with pytest.raises(ValueError, match="dtype must be"):
        m.forward_dense(fv, 1, out, dtype="fp8")
    with pytest.raises(ValueError, match="dtype must be"):
        inf.patch_probabilities(fv, m, 68, dtype="fp8")
    others = [(CascadedMTL(n_feat=240, patch_size=68, n_classes=3, seed=0), 240),
              (FusionMTL(n_feat=120, patch_size=68, n_classes=3, seed=0), 240),
              (SingleTaskTCN(n_feat=80, patch_size=68, n_classes=3, seed=0), 80),
              (LateFusion(B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=0), B3MTL(n_feat=120, patch_size=68, n_classes=3, seed=1)), 240),
              (B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=0, tcn_block="2.8"), 240)]
    for model, rows in others:
        who = type(model).__name__
        x = fv[:rows].contiguous()
        o = torch.full((32, model.out_dim), -7.0, device="cuda")
        with pytest.raises(ValueError, match="B3_MTL"):
            model.forward_dense(x, 1, o, dtype="bf16")
        with pytest.raises(ValueError, match="dtype must be"):
            model.forward_dense(x, 1, o, dtype="fp8")
        with pytest.raises(ValueError, match="B3_MTL"):
            inf.patch_probabilities(x, model, 68, output=model.output_names[-1], dtype="bf16")
        torch.cuda.synchronize()
        assert bool((o == -7.0).all()), who
        if who != "B3MTL":  # (the 2.8 block has no dense path at all) the f32 call is what it was
            assert tuple(model.forward_dense(x, 1, dtype="f32").shape) == (32, model.out_dim), who
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


@pytest.mark.parametrize("case", ["Tc=W-1", "shift=0", "workspace one byte short", "d_work offset by 4 bytes"])
def test_refusals_c_entry(case):
    """5. (cont.) The C entry's own checks: a negative code, a message in smh_last_error(), d_out unwritten."""
    from sm_hpss_mtl_amd import _lib
    m, _ = _model(3, 68)
    Tc = 100
    fv = torch.from_numpy(_fv(Tc)).cuda()
    nbytes = m.lib.smh_model_dense_workspace_bytes(m._h, Tc)
    work = torch.full((2 * Tc * 32 + 4,), -7.0, device="cuda")
    out = torch.full((32, m.out_dim), -7.0, device="cuda")
    kw = {"Tc=W-1": dict(Tc=67), "shift=0": dict(shift=0), "workspace one byte short": dict(work_bytes=nbytes - 1),
          "d_work offset by 4 bytes": dict(work_offset=4)}[case]
    args = dict(shift=1, work_bytes=nbytes)
    args.update(kw)
    rc = _dense_c(m, BF16, fv, args.pop("shift"), work, args.pop("work_bytes"), out, **args)
    torch.cuda.synchronize()
    assert rc < 0 and BF16 in _lib.last_error(), (rc, _lib.last_error())
    assert bool((out == -7.0).all()) and bool((work == -7.0).all())
    # and the same call with nothing wrong runs
    assert _dense_c(m, BF16, fv, 1, work, nbytes, out) == 32


def test_operand_cache_follows_weight_updates():
    """6. The split operand cache is rebuilt by weight version on the dense entry too."""
    from sm_hpss_mtl_amd.model import B3MTL
    w = b3_mtl.init_weights(seed=3, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True)
    m = B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=0)
    m.set_weights_dict(w)
    fv = torch.from_numpy(_fv(100)).cuda()
    a = m.forward_dense(fv, 1, dtype="bf16").clone()
    m.set_weights_dict({k: (v * np.float32(0.5) if k.endswith("3C/kernel") else v) for k, v in w.items()})
    b = m.forward_dense(fv, 1, dtype="bf16")
    ref = m.forward_dense(fv, 1)
    torch.cuda.synchronize()
    assert not torch.equal(a, b) and float((b - ref).abs().max()) <= TOL_SPLIT
