"""GPU: B3_MTL at the two input shapes of the skewness-vector feed, against the numpy oracle.

PARAMS['skewness_vector'] = 'Row' builds get_Lemaire_MTL_model(N_MELS = 2F, patch_size = 1) for (N, 1, 2F) batches and 'Col'
(N_MELS = 1, patch_size = W) for (N, W, 1) (Proposed_Work_Results.py:861-866).  smh_model_create_heads accepts both (n_feat >= 1,
patch_size >= 1) and no other test runs them: a one-frame patch makes every dilated tap but the centre one read the causal padding, and
n_feat = 1 leaves the generic layer-0 branch a single feature.  Tolerances: the forward's 1e-4 with equal argmax of SURVEY 8(d') and
tests/test_parity_gpu.py; the training step's of tests/test_model_shapes_gpu.py.  Inputs sit at the end of their buffer with NaN
behind them."""
import copy

import numpy as np
import pytest
import torch

from oracle import b3_mtl, b3_mtl_train as tr
from tests import data_stats_ref as ref
from tests.test_model_shapes_gpu import at_end_of_buffer, flat_to_dict, host, model, oracle_forward, problem, rows_to_check, weights

pytestmark = pytest.mark.gpu

SHAPES = [(240, 1), (1, 68), (1, 249)]  # (n_feat, patch_size)
NCLS, NB, ND = 3, 3, 8


@pytest.mark.parametrize("N", [1, 3, 48])
@pytest.mark.parametrize("F,W", SHAPES)
def test_forward_vs_oracle(F, W, N):
    w = weights(F, W, NCLS, NB, ND)
    m = model(F, W, NCLS, NB, ND, w)
    x = np.random.default_rng(F * 7 + W + N).standard_normal((N, W, F)).astype(np.float32)
    out = host(m.forward_device(at_end_of_buffer(x)))
    m.check_status()
    assert out.shape == (N, m.out_dim) and np.isfinite(out).all()
    sel = rows_to_check(N)
    want, _ = oracle_forward(x[sel], w, NCLS, NB, ND)
    print("F=%d W=%d N=%d max |d| = %.3e" % (F, W, N, float(np.abs(out[sel] - want).max())))
    np.testing.assert_allclose(out[sel], want, atol=1e-4, rtol=0)
    assert np.array_equal(out[sel][:, -NCLS:].argmax(1), want[:, -NCLS:].argmax(1))


@pytest.mark.parametrize("F,W", SHAPES[:2])
def test_f32_training_step_vs_oracle(F, W):
    """train_on_batch(apply=False) with fixed dropout masks against oracle.b3_mtl_train.forward_backward: losses, accuracy and every
    gradient tensor, with the bounds tests/test_model_shapes_gpu.py holds a batch below 100 patches to."""
    N = 48
    w, x, y, drop_tcn, drop_heads = problem(F, W, NCLS, NB, ND, N, seed=F + N)
    lw = {"S": 0.7, "R": 1.3}
    m = model(F, W, NCLS, NB, ND, w, loss_weights=lw)
    heads = [n for n, _, _ in b3_mtl.head_spec(NCLS)]
    got = m.train_on_batch(at_end_of_buffer(x), y, drop_tcn=torch.from_numpy(drop_tcn).cuda(),
                           drop_heads=torch.from_numpy(drop_heads).cuda(), apply=False)
    want = tr.forward_backward(x, y, w, NCLS, drop_tcn, {h: drop_heads[:, i] for i, h in enumerate(heads)}, lw, nb_stacks=NB, n_dil=ND)
    assert abs(got[0] - want["loss"]) < 2e-4 * max(1.0, abs(want["loss"]))
    for i, name in enumerate(heads + ["3C"]):
        assert abs(got[1 + i] - want["losses"][name]) < 2e-4 * max(1.0, abs(want["losses"][name])), name
    assert abs(got[-1] - want["acc"]) < 1e-6
    g = flat_to_dict(m, host(m._grad_tensor()))
    for name, gref in want["grads"].items():
        if name.endswith(tr.TRAINABLE_SKIP):
            continue
        gg = g[name].astype(np.float64)
        if name.endswith("/dense/kernel"):
            gg = gg + 2 * tr.L2 * w[name]  # the l2 term is added at apply time on the device
        scale = max(np.abs(gref).max(), 1e-6)
        atol = 2e-5 if name.endswith("/dense/bias") else 1e-6
        err = np.abs(gg - gref).max()
        assert np.isfinite(gg).all() and err <= 2e-3 * scale + atol, (name, err, scale)


@pytest.mark.parametrize("mode", ["Row", "Col"])
def test_a_generator_batch_trains_and_predicts(tmp_path, mode):
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.model import B3MTL
    folder, files = ref.dataset(tmp_path)
    gen.fv_cache_clear()
    P = ref.params(tmp_path, "feat", "Lemaire_et_al_MTL")
    P["skewness_vector"] = mode
    np.random.seed(3)
    x, y = next(gen.generator(P, folder, copy.deepcopy(files), 2))
    F, W = (240, 1) if mode == "Row" else (1, 68)
    N = 6
    assert tuple(x.shape) == (N, W, F) and bool(torch.isfinite(x).all())
    m = B3MTL(n_feat=F, patch_size=W, n_classes=3, seed=1)
    losses = m.train_on_batch(x, y)
    assert len(losses) >= 5 and np.all(np.isfinite(np.asarray(losses, np.float64)))
    outs = m.predict(x=x)
    assert [tuple(o.shape) for o in outs] == [(N, 1), (N, 1), (N, 2), (N, 3)]
    assert all(np.isfinite(np.asarray(o)).all() for o in outs)
    gen.fv_cache_clear()
