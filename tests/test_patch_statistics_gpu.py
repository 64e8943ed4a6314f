"""Frontend.patch_statistics (smh_patch_statistics) against code that predates it.

The reference value is oracle.tools_stats.get_data_statistics(P.astype(float64), stat, axis), P the image-layout patches the existing
entries give for the same featuregram: Frontend.patches_from_featuregram (per-file StandardScaler), or Frontend.scaled_patches when
statistics are supplied.  The value under the statistic is therefore held bit for bit to the existing kernels, and what is left is the
order of the float64 sums (index order on the device, pairwise in numpy): rtol = 1e-10, atol = 1e-12 as tests/test_tools_gpu.py for the
same statistic and the same cause; the float32 output is that rounded once more, rtol = 2^-24 on top.

Every featuregram sits at the very end of its allocation with NaN in the floats behind it: an over-read shows as NaN, not as a fault.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tools_stats

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-10, 1e-12
GEOMETRIES = [(68, 68), (68, 34), (5, 2), (249, 24)]
T_SHORT = {68: 30, 249: 98, 5: 3, 300: 98}  # tiled-if-short
T_LONG = 2500                               # crosses the row segments of both kernels


def frame_counts(W):
    return [T_SHORT[W], W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, T_LONG]


@functools.lru_cache(maxsize=None)
def frontend():
    from sm_hpss_mtl_amd.frontend import Frontend
    return Frontend()


def at_end_of_buffer(x, pad=64):
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.full((x.size + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:x.size] = torch.from_numpy(x.ravel()).cuda()
    return buf[:x.size].view(x.shape)


def featuregram(rows, T, W, seed):
    """Seeded normal float32; with three rows or more, row 1 is constant over the file and row 2 over the window of patch 0 only."""
    x = (np.random.default_rng(seed).standard_normal((rows, T)) * 7.0 - 3.0).astype(np.float32)
    if rows >= 3:
        x[1] = 0.37
        if T > W:
            x[2, :W] = -11.25
    return x


@functools.lru_cache(maxsize=None)
def per_file_case(rows, W, shift):
    """[(device featuregram, its image patches (nP, rows, W) from patches_from_featuregram as float32 numpy)] -- computed once."""
    fe, out = frontend(), []
    for k, T in enumerate(frame_counts(W)):
        fv = at_end_of_buffer(featuregram(rows, T, W, seed=1000 * rows + 10 * W + k))
        P = fe.patches_from_featuregram(fv, W, shift, layout="image").cpu().numpy()
        assert P.shape == (fe.num_patches(T, W, shift), rows, W) and np.isfinite(P).all()
        P.setflags(write=False)
        out.append((fv, P))
    return out


def oracle(P, stat, axis):
    if P.shape[0] == 0:
        return np.zeros((0, P.shape[2] if axis == 0 else P.shape[1]))
    return tools_stats.get_data_statistics(P.astype(np.float64), stat, axis)


def check(got, P, stat, axis, W, rows, ref=None):
    ref = oracle(P, stat, axis) if ref is None else ref
    assert tuple(got.shape) == ref.shape == (P.shape[0], W if axis == 0 else rows)
    g = got.cpu().numpy()
    assert np.isfinite(g).all()
    if ref.size:
        print("  nP=%d max|d|=%.3e" % (P.shape[0], float(np.max(np.abs(g.astype(np.float64) - ref)))))
    if got.dtype == torch.float64:
        np.testing.assert_allclose(g, ref, rtol=RTOL, atol=ATOL)
    else:
        assert got.dtype == torch.float32
        np.testing.assert_allclose(g.astype(np.float64), ref, rtol=RTOL + 2.0 ** -24, atol=ATOL)
    return g


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("W,shift", GEOMETRIES)
@pytest.mark.parametrize("rows", [1, 21, 240])
def test_skew_ragged_batch_and_alone(rows, W, shift, axis):
    fe, case = frontend(), per_file_case(rows, W, shift)
    fvs = [fv for fv, _ in case]
    counts = [P.shape[0] for _, P in case]
    assert 0 in counts or W % 2 == 1  # T = W: no patch for an even W (an odd W leaves exactly one)
    assert counts[2] == 1 and counts[0] >= 1 and counts[-1] > 2
    batch64 = fe.patch_statistics(fvs, W, shift, axis, "skew", dtype=torch.float64)
    batch32 = fe.patch_statistics(fvs, W, shift, axis)  # the default: skew, float32
    for (fv, P), g64, g32 in zip(case, batch64, batch32):
        ref = oracle(P, "skew", axis)
        a = check(g64, P, "skew", axis, W, rows, ref)
        b = check(g32, P, "skew", axis, W, rows, ref)
        assert np.array_equal(a.astype(np.float32), b)  # one rounding of the float64 result
        alone = fe.patch_statistics([fv], W, shift, axis, "skew", dtype=torch.float64)
        assert len(alone) == 1 and np.array_equal(alone[0].cpu().numpy(), a)  # bit-identical alone and in the batch
    if rows >= 3 and axis == 1:  # the constant rows: exactly 0, not NaN
        for g64, T in zip(batch64, frame_counts(W)):
            if T > W:
                g = g64.cpu().numpy()
                assert np.all(g[:, 1] == 0.0) and g[0, 2] == 0.0


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("stat", ["mean", "variance", "skew", "kurtosis"])
def test_every_statistic(stat, axis):
    rows, (W, shift) = 21, GEOMETRIES[1]
    fe, case = frontend(), per_file_case(rows, W, shift)
    for dtype in (torch.float64, torch.float32):
        got = fe.patch_statistics([fv for fv, _ in case], W, shift, axis, stat, dtype=dtype)
        for (_, P), g, T in zip(case, got, frame_counts(W)):
            g = check(g, P, stat, axis, W, rows)
            if stat == "kurtosis" and axis == 1 and T > W:
                assert np.all(g[:, 1] == -3.0) and g[0, 2] == -3.0  # m2 == 0


@pytest.mark.parametrize("axis", [1, 0])
def test_a_long_patch_takes_the_wider_ring(axis):
    """W = 300: axis 1 doubles its LDS ring to 1024 frames and halves its rows per workgroup."""
    rows, W, shift = 21, 300, 7
    fe = frontend()
    for k, T in enumerate((98, 301, 1500)):
        fv = at_end_of_buffer(featuregram(rows, T, W, seed=77 + k))
        P = fe.patches_from_featuregram(fv, W, shift, layout="image").cpu().numpy()
        check(fe.patch_statistics([fv], W, shift, axis, "skew", dtype=torch.float64)[0], P, "skew", axis, W, rows)


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("W,shift", [(68, 34), (249, 24)])
def test_fold_statistics_mode(W, shift, axis):
    """With mean / stdev the value is scaled_patches': (float32)((x - mean[r]) / (stdev[r] + 1e-10)); one row has stdev == 0."""
    rows, fe = 21, frontend()
    rng = np.random.default_rng(4)
    mean, stdev = rng.normal(-3.0, 2.0, rows), rng.uniform(0.5, 9.0, rows)
    stdev[5] = 0.0
    fvs = [at_end_of_buffer(featuregram(rows, T, W, seed=300 + k)) for k, T in enumerate(frame_counts(W)[:-1] + [700])]
    Ps = [p.cpu().numpy() for p in fe.scaled_patches(fvs, mean, stdev, W, shift, layout="image")]
    assert all(np.isfinite(p).all() for p in Ps) and max(np.abs(p).max() for p in Ps if p.size) > 1e9
    for dtype in (torch.float64, torch.float32):
        got = fe.patch_statistics(fvs, W, shift, axis, "skew", mean=mean, stdev=torch.from_numpy(stdev), dtype=dtype)
        for fv, P, g in zip(fvs, Ps, got):
            a = check(g, P, "skew", axis, W, rows)
            alone = fe.patch_statistics([fv], W, shift, axis, "skew", mean=mean, stdev=stdev, dtype=dtype)[0]
            assert np.array_equal(alone.cpu().numpy(), a)


def test_no_patch_is_no_error():
    fe = frontend()
    fv = at_end_of_buffer(featuregram(21, 68, 68, seed=1))
    for axis, width in ((1, 21), (0, 68)):
        got = fe.patch_statistics([fv], 68, 68, axis)
        assert len(got) == 1 and tuple(got[0].shape) == (0, width)
    torch.cuda.synchronize()


def test_argument_errors():
    fe = frontend()
    fv = at_end_of_buffer(featuregram(21, 100, 68, seed=2))
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 68, 34, 2)
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 68, 34, 1, stat="median")
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 0, 34, 1)
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 68, 0, 1)
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 68, 34, 1, mean=np.zeros(20), stdev=np.ones(20))
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 68, 34, 0, mean=np.zeros(21))
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 68, 34, 0, dtype=torch.float16)
    with pytest.raises(ValueError):
        fe.patch_statistics([], 68, 34, 0)
    with pytest.raises(ValueError):
        fe.patch_statistics([fv], 8193, 34, 1)  # axis 1 holds a patch's frames in LDS
    torch.cuda.synchronize()
