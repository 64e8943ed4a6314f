"""GPU: the device path of the generators with PARAMS['skewness_vector'] = 'Row' / 'Col' against the same call with the per-file
callables (the reference's composition on the host: get_featuregram, [scale_data,] get_feature_patches, get_data_statistics,
expand_dims, transpose).  The callables are this package's own host functions, whose featuregrams and patches are the device path's
bit for bit (tests/test_scaled_patches_gpu.py, tests/test_ragged_gpu.py), so what separates the two sides is the order of the float64
sums -- rtol = 1e-10, atol = 1e-12 as tests/test_patch_statistics_gpu.py -- and the one rounding of the device feed to float32,
rtol = 2^-24 on top.  W = 68, W_shift = 34, both modes, with and without frame_level_scaling."""
import copy

import numpy as np
import pytest
import torch

from tests import data_stats_ref as ref

pytestmark = pytest.mark.gpu

MODEL = "Lemaire_et_al_MTL"
ROWS, W = 240, 68
RTOL, ATOL = 1e-10 + 2.0 ** -24, 1e-12


def _callables(P):
    from sm_hpss_mtl_amd.lib import preprocessing as pp

    def patches(PARAMS, FV, patch_size, patch_shift, featName):
        return pp.get_feature_patches(P, FV, patch_size, patch_shift, featName)
    return pp.get_featuregram, patches


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("mode", ["Row", "Col"])
def test_device_generators_with_skewness_vectors(tmp_path, mode, scaling):
    from sm_hpss_mtl_amd import generators as gen
    folder, files = ref.dataset(tmp_path)
    gen.fv_cache_clear()
    P_dev = ref.params(tmp_path, "feat_dev", MODEL)
    P_dev["skewness_vector"] = mode
    if scaling:
        Ps = ref.params(tmp_path, "feat_stats", MODEL)
        Ps["fold"], Ps["train_files"] = 0, files
        gen.data_stats_for_fold(Ps)
        gen.fv_cache_clear()
        P_dev.update(frame_level_scaling=True, fold=0, mean_fold0=Ps["mean_fold0"], stdev_fold0=Ps["stdev_fold0"])
    P_host = dict(P_dev, feature_opDir=str(tmp_path / "feat_ref"))
    P_plain = dict(P_dev, skewness_vector=None, feature_opDir=str(tmp_path / "feat_plain"))
    fv_fn, patches_fn = _callables(P_host)
    bs, n_batches = 2, 3
    shape = (3 * bs, 1, ROWS) if mode == "Row" else (3 * bs, W, 1)

    def device_batches(P):
        np.random.seed(7)
        g = gen.generator(P, folder, copy.deepcopy(files), bs)
        return [next(g) for _ in range(n_batches)]

    got = device_batches(P_dev)
    np.random.seed(7)
    yard = gen.generator(P_host, folder, copy.deepcopy(files), bs, featuregram_fn=fv_fn, patches_fn=patches_fn)
    want = [next(yard) for _ in range(n_batches)]
    gen.fv_cache_clear()
    plain = device_batches(P_plain)  # the same call without the key: same labels, same batch order, as many rows
    for (xb, yb), (xr, yr), (xp, yp) in zip(got, want, plain):
        assert isinstance(xb, torch.Tensor) and xb.is_cuda and xb.dtype == torch.float32 and tuple(xb.shape) == shape == xr.shape
        assert tuple(xp.shape) == (3 * bs, W, ROWS)
        g = xb.cpu().numpy().astype(np.float64)
        print(mode, scaling, "max |d| =", float(np.abs(g - xr).max()), "max |ref| =", float(np.abs(xr).max()))
        assert np.abs(xr).max() > 0.05
        np.testing.assert_allclose(g, xr, rtol=RTOL, atol=ATOL)
        for k in yr:
            assert np.array_equal(np.asarray(yb[k], np.float64), np.asarray(yr[k], np.float64))
            assert np.array_equal(np.asarray(yb[k], np.float64), np.asarray(yp[k], np.float64))
    # a second epoch is served from the device featuregram cache: the same bits
    gen.fv_cache_clear()
    first = device_batches(P_dev)
    assert len(gen._FV_CACHE) > 0
    for (xa, _), (xb, _), (xc, _) in zip(got, first, device_batches(P_dev)):
        assert torch.equal(xa, xb) and torch.equal(xb, xc)
    # every vector of one test file at the hard-coded shift 68
    sp, mu = folder + "/speech/" + files["speech"][2], folder + "/music/" + files["music"][0]
    for args in ((sp, "", None), ("", mu, None), (sp, mu, 10)):
        x, y = gen.test_file_wise_generator(P_dev, *args)
        xr, yr = gen.test_file_wise_generator(P_host, *args, featuregram_fn=fv_fn, patches_fn=patches_fn)
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == xr.shape == (xr.shape[0],) + shape[1:] and x.shape[0] >= 1
        np.testing.assert_allclose(x.cpu().numpy().astype(np.float64), xr, rtol=RTOL, atol=ATOL)
        assert np.array_equal(y, yr)
    gen.fv_cache_clear()
