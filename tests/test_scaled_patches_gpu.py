"""GPU: `Frontend.scaled_patches` (smh_scaled_patches_f32) and the generators' device path with PARAMS['frame_level_scaling'].

scaled_patches is bit for bit np.float32((np.float64(x) - mean) / (stdev + 1e-10)) gathered on the smh_patch_start grid: rows 21 / 32 /
33 / 240 (a partial block of 32, a full one, one row beyond, several) x (T, W, shift) with T below W (tiled), equal to it (no patch
at even W), one beyond, patches that overlap, that tile exactly, and T beyond one 256-frame segment x both layouts; the seven
lengths as one ragged batch -- views of one buffer and separate tensors mixed -- against each clip alone.  End to end: the device
batches of generator / test_file_wise_generator equal get_feature_patches (scaling on) of tools.scale_data per file."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import data_stats_ref as ref

pytestmark = pytest.mark.gpu

CASES = ((3, 8, 8), (8, 8, 8), (9, 8, 3), (64, 5, 2), (65, 68, 68), (137, 68, 68), (700, 99, 34))
ROWS = (21, 32, 33, 240)


@pytest.fixture(scope="module")
def fe():
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    return Frontend(FrontendConfig())


def _stats(rows):
    rng = np.random.default_rng(rows)
    return rng.normal(-40.0, 5.0, rows).astype(np.float32), rng.uniform(3.0, 20.0, rows).astype(np.float32)


def _clip(rows, T):
    return np.random.default_rng(1000 * rows + T).normal(-40.0, 15.0, size=(rows, T)).astype(np.float32)


def _want(fe, x, mean, stdev, W, shift, layout):
    lib = fe.lib
    return ref.patch_grid(ref.scaled(x, mean, stdev), W, shift, lib.smh_tiled_frames, lib.smh_num_patches, lib.smh_patch_start,
                          layout == "time_major")


@pytest.mark.parametrize("layout", ["time_major", "image"])
@pytest.mark.parametrize("rows", ROWS)
def test_scaled_patches_are_the_float64_arithmetic_on_the_patch_grid(fe, rows, layout):
    mean, stdev = _stats(rows)
    for T, W, shift in CASES:
        x = _clip(rows, T)
        got = fe.scaled_patches([torch.from_numpy(x).cuda()], mean, stdev, W, shift, layout=layout)
        want = _want(fe, x, mean, stdev, W, shift, layout)
        assert len(got) == 1 and tuple(got[0].shape) == want.shape and got[0].dtype == torch.float32, (T, W, shift)
        assert (want.shape[0] == 0) == ((T, W) == (8, 8))  # range(W / 2, T - W / 2, shift) is empty there
        assert np.array_equal(got[0].cpu().numpy(), want), (rows, T, W, shift)


@pytest.mark.parametrize("layout", ["time_major", "image"])
@pytest.mark.parametrize("rows", ROWS)
def test_ragged_batch_of_mixed_tensors_equals_each_clip_alone(fe, rows, layout):
    mean, stdev = _stats(rows)
    dm, ds = torch.from_numpy(mean).cuda(), torch.from_numpy(stdev.astype(np.float64)).cuda()  # tensors of either dtype do as well
    clips = [_clip(rows, T) for T, _, _ in CASES]
    # even clips: views of ONE buffer at float offsets that are not multiples of 4; odd ones: tensors of their own
    flat = torch.empty(sum(c.size + 1 for c in clips[::2]) + 1, dtype=torch.float32, device="cuda")
    dev, o = [], 1
    for i, c in enumerate(clips):
        if i % 2 == 0:
            v = flat[o:o + c.size].view(c.shape)
            v.copy_(torch.from_numpy(c))
            o += c.size + 1
            dev.append(v)
        else:
            dev.append(torch.from_numpy(c).cuda())
    for W, shift in sorted({(W, shift) for _, W, shift in CASES}):
        got = fe.scaled_patches(dev, dm, ds, W, shift, layout=layout)
        assert len(got) == len(clips)
        base = next(g.data_ptr() - 0 for g in got if g.shape[0])  # (the first clip, T = 3, always has patches)
        assert got[0].shape[0] > 0
        for i, c in enumerate(clips):
            alone = fe.scaled_patches([torch.from_numpy(c).cuda()], mean, stdev, W, shift, layout=layout)[0]
            assert got[i].shape == alone.shape and torch.equal(got[i], alone), (rows, c.shape[1], W, shift)
            assert np.array_equal(alone.cpu().numpy(), _want(fe, c, mean, stdev, W, shift, layout))
            if got[i].shape[0]:  # views of one buffer, in order
                assert got[i].data_ptr() == base + 4 * rows * W * sum(int(g.shape[0]) for g in got[:i])


@pytest.mark.parametrize("layout", [0, 1])
def test_entry_writes_its_patches_and_nothing_else(fe, layout):
    """The C entry on a buffer with a guard band on both sides: every patch element is written, no float beside them is."""
    from sm_hpss_mtl_amd import _lib
    rows, W, shift = 33, 8, 3
    mean, stdev = _stats(rows)
    clips = [torch.from_numpy(_clip(rows, T)).cuda() for T in (3, 9, 700, 65)]
    B = len(clips)
    h_T = (C.c_int * B)(*[int(c.shape[1]) for c in clips])
    off = (C.c_longlong * (B + 1))()
    total = fe.lib.smh_scaled_patches_count(h_T, B, W, shift, off)
    n, guard = int(total) * W * rows, 4096
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
    dm, ds = torch.from_numpy(mean.astype(np.float64)).cuda(), torch.from_numpy(stdev.astype(np.float64)).cuda()
    h_fv = (C.c_void_p * B)(*[c.data_ptr() for c in clips])
    rc = fe.lib.smh_scaled_patches_f32(fe._h, h_fv, h_T, B, rows, C.c_void_p(dm.data_ptr()), C.c_void_p(ds.data_ptr()), W, shift, layout,
                                       C.c_void_p(buf.data_ptr() + 4 * guard), _lib.current_stream())
    assert rc == 0, _lib.last_error()
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + n:]).all() and np.isfinite(host[guard:guard + n]).all()
    want = np.concatenate([_want(fe, c.cpu().numpy(), mean, stdev, W, shift, "time_major" if layout else "image").ravel() for c in clips])
    assert np.array_equal(host[guard:guard + n], want)


def test_more_clips_than_one_table_holds_are_split_on_the_host(fe):
    """A table of one launch holds 2048 clips; 2051 tiny clips take two launches of either kernel: the outputs of the second start
    where the first one's end (moments at clip 2048, patches behind the first 2048 clips' patches)."""
    rows, n, W, shift = 3, 2051, 4, 2
    mean, stdev = _stats(rows)
    rng = np.random.default_rng(9)
    Ts = [1 + i % 7 for i in range(n)]
    clips = [rng.normal(-40.0, 15.0, size=(rows, T)).astype(np.float32) for T in Ts]
    flat = torch.from_numpy(np.concatenate([c.ravel() for c in clips])).cuda()
    views, o = [], 0
    for c in clips:
        views.append(flat[o:o + c.size].view(c.shape))
        o += c.size
    s, m2, bad = (t.cpu().numpy() for t in fe.row_moments(views))
    assert s.shape == (n, rows) and not bad.any()
    want_s = np.stack([c.astype(np.float64).sum(axis=1) for c in clips])  # at most seven float32 values: every order is exact
    want_m2 = np.stack([((c.astype(np.float64) - c.astype(np.float64).mean(axis=1, keepdims=True)) ** 2).sum(axis=1) for c in clips])
    assert np.array_equal(s, want_s) and np.all(np.abs(m2 - want_m2) <= 1e-10 * want_m2)
    got = fe.scaled_patches(views, mean, stdev, W, shift)
    assert len(got) == n
    for i in (0, 1, 2046, 2047, 2048, 2049, 2050):
        assert np.array_equal(got[i].cpu().numpy(), _want(fe, clips[i], mean, stdev, W, shift, "time_major")), i
    whole = torch.cat(got).cpu().numpy()
    assert np.array_equal(whole, np.concatenate([_want(fe, c, mean, stdev, W, shift, "time_major") for c in clips]))


def test_scaled_patches_reject_bad_arguments(fe):
    a = torch.zeros((4, 9), device="cuda")
    ok = np.ones(4)
    with pytest.raises(ValueError):
        fe.scaled_patches([a], np.ones(5), ok, 8, 8)
    with pytest.raises(ValueError):
        fe.scaled_patches([a], ok, np.ones(3), 8, 8)
    with pytest.raises(ValueError):
        fe.scaled_patches([a, torch.zeros((5, 9), device="cuda")], ok, ok, 8, 8)
    with pytest.raises(ValueError):
        fe.scaled_patches([a], ok, ok, 8, 0)
    with pytest.raises(ValueError):
        fe.scaled_patches([a], ok, ok, 8, 8, layout="nhwc")


# ---- end to end: the generators' device path -----------------------------------------------------------------------------------------
def _host_yardstick(P_on):
    """The reference's per-file sequence with this package's host functions: get_featuregram, tools.scale_data (float64,
    (fv - mean) / (stdev + 1e-10)), get_feature_patches with frame_level_scaling on (no StandardScaler)."""
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    from sm_hpss_mtl_amd.lib.cython_impl import tools
    mean, stdev = P_on["mean_fold0"], P_on["stdev_fold0"]

    def fv(PARAMS, classname, opdir, sp, mu, db, n_fft, n_mels, featName, save_feat=True):
        return tools.scale_data(pp.get_featuregram(PARAMS, classname, opdir, sp, mu, db, n_fft, n_mels, featName, save_feat), mean, stdev)

    def patches(PARAMS, FV, patch_size, patch_shift, featName):
        return pp.get_feature_patches(P_on, FV, patch_size, patch_shift, featName)
    return fv, patches


@pytest.mark.parametrize("model", sorted(ref.MODELS))
def test_device_generators_with_frame_level_scaling(tmp_path, model):
    from sm_hpss_mtl_amd import generators as gen
    folder, files = ref.dataset(tmp_path)
    rows, layout = ref.MODELS[model][3:]
    gen.fv_cache_clear()
    # the fold's statistics, on the device, from a feature cache of their own (the generator below starts from the audio)
    Ps = ref.params(tmp_path, "feat_stats", model)
    Ps["fold"], Ps["train_files"] = 0, files
    nFrames = gen.data_stats_for_fold(Ps)
    assert len(nFrames) == 3 and all(n > 0 for n in nFrames) and Ps["mean_fold0"].shape == (rows,)
    gen.fv_cache_clear()
    P_on = ref.params(tmp_path, "feat_dev", model)
    P_on.update(frame_level_scaling=True, fold=0, mean_fold0=Ps["mean_fold0"], stdev_fold0=Ps["stdev_fold0"])
    P_off = ref.params(tmp_path, "feat_ref", model)
    fv_fn, patches_fn = _host_yardstick(P_on)
    bs, n_batches = 2, 3

    def device_batches():
        np.random.seed(7)
        g = gen.generator(P_on, folder, copy.deepcopy(files), bs)
        return [next(g) for _ in range(n_batches)]

    got = device_batches()
    np.random.seed(7)
    yard = gen.generator(P_off, folder, copy.deepcopy(files), bs, featuregram_fn=fv_fn, patches_fn=patches_fn)
    want = [next(yard) for _ in range(n_batches)]
    shape = (3 * bs, 68, rows) if layout == "time_major" else (3 * bs, rows, 68, 1)
    for (xb, yb), (xr, yr) in zip(got, want):
        assert isinstance(xb, torch.Tensor) and xb.is_cuda and xb.dtype == torch.float32 and tuple(xb.shape) == shape == xr.shape
        assert np.array_equal(xb.cpu().numpy().astype(np.float64), xr)
        if isinstance(yr, dict):
            for k in yr:
                assert np.array_equal(np.asarray(yb[k], np.float64), np.asarray(yr[k], np.float64))
        else:
            assert np.array_equal(np.asarray(yb), np.asarray(yr))
    # a second epoch is served from the device featuregram cache (and the .npy files the first one wrote): the same bits
    assert len(list((tmp_path / "feat_dev").rglob("*.npy"))) > 0 and len(gen._FV_CACHE) > 0
    for (xb, _), (xa, _) in zip(got, device_batches()):
        assert torch.equal(xb, xa)
    # every patch of one test file at the hard-coded shift 68
    sp, mu = folder + "/speech/" + files["speech"][2], folder + "/music/" + files["music"][0]
    for args in ((sp, "", None), ("", mu, None), (sp, mu, 10)):
        x, y = gen.test_file_wise_generator(P_on, *args)
        xr, yr = gen.test_file_wise_generator(P_off, *args, featuregram_fn=fv_fn, patches_fn=patches_fn)
        assert x.is_cuda and tuple(x.shape) == xr.shape and x.shape[0] >= 1
        assert np.array_equal(x.cpu().numpy().astype(np.float64), xr) and np.array_equal(y, yr)
    # statistics of another row count are refused
    P_bad = dict(P_on, mean_fold0=P_on["mean_fold0"][:-1], stdev_fold0=P_on["stdev_fold0"][:-1])
    with pytest.raises(ValueError):
        gen.test_file_wise_generator(P_bad, sp, "", None)
    gen.fv_cache_clear()
