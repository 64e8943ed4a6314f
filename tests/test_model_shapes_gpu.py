"""GPU: the B3_MTL network away from n_feat = 240 and the default 3 stacks x 8 dilations, against the numpy oracle.

The library accepts any n_feat >= 1, patch_size <= 512, nb_stacks >= 1 and 1 <= n_dilations <= 16; the reference sweeps
n_mels over 20..120 (n_feat = 2 n_mels) and W over 25..100 (Hyperparameter_Selection.py:542-545), and tunes 3..8 dilations and
3..10 stacks (B3_architecture_tuning.py:254-255).  Every other GPU test runs n_feat = 240 with 24 blocks, where the paths below
never run.  Why each shape is here:

- n_feat != 240 takes the generic layer-0 branch of b3mtl_forward_kernel (the vectorised one needs FQ = n_feat / 4 = 60); 61 and
  75 (n_feat % 4 != 0) and 402 (the non-mel HarmPerc width at n_fft = 400; FQ * 4 = 404) zero-pad each lane's last k steps.
  Every input is placed at the very end of its buffer with NaN just behind it, so a layer-0 load past the last row would
  reach the outputs.
- Depths (1, 1), (3, 3), (3, 6), (3, 8), (10, 8), (10, 16): the dilation wraps at n_dilations (1 << (blk % n_dil)), the saved
  activation slots and SpatialDropout masks are sized by n_blocks, and the skewed block schedule runs only while
  n_blocks x column tiles < 2048: (10, 8) at W = 68 with four patches per workgroup (17 tiles) stays on its side, (10, 16)
  crosses to the barrier schedule.
- W in {25, 50, 75, 100} (the sweep) and 68; N = 1 (one workgroup), 3 and 307 (a prime: several workgroups, a partial last one).
- The split-bf16 forward tiles layer 0 in ceil(n_feat / 32) steps: 20, 61, 100 and 200 end in a partial step, 61 on its
  unaligned scalar path; 402 is refused.
- Dense inference refuses n_feat % 8 != 0 (20, 60, 100 of the sweep); 40, 80, 160 and 200 run.
- The training step: the layer-0 weight gradient in 16-wide feature tiles with a masked tail (20, 61, 120, 402), the backward
  loop over n_blocks, the weight-offset tables of the optimiser step at another n_feat / n_blocks.
- The front end at n_mels = 20 / 40 / 80: the mel CSR and the feature-kernel segment plans, and the fused layer-0 partials
  (2 n_mels wide), for a 1 s clip and a 10 s clip (the streaming kernels; the fused layer-0 path takes 998 frames at
  n_mels = 20 and refuses them at 40 and 80, where a featuregram half no longer fits its LDS tile).

Tolerances are those of the same quantity at n_feat = 240 (tests/test_parity_gpu.py, test_training_gpu.py, test_bf16_gpu.py,
test_inference_gpu.py); where a shape needs another bound the test says why."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import b3_mtl, b3_mtl_train as tr, frontend as ofe
from tests import cascaded_ref as cref

pytestmark = pytest.mark.gpu

TOL_SPLIT = 1e-4   # tests/test_bf16_gpu.py: split-bf16 forward against the f32 forward and the oracle
MIN_AGREE = 0.995


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def at_end_of_buffer(x, pad=64):
    """x as a contiguous device tensor whose last element is the last element of its data, with NaN in the `pad` floats that
    follow: a kernel that reads past the last row of the batch turns outputs into NaN (in-bounds memory: no fault)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.full((x.size + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:x.size] = torch.from_numpy(x.ravel()).cuda()
    return buf[:x.size].view(x.shape)


def weights(F, W, ncls, nb, nd, seed=7):
    return b3_mtl.init_weights(seed=seed, n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dil=nd, randomize_bn=True)


def model(F, W, ncls, nb, nd, w=None, **kw):
    from sm_hpss_mtl_amd.model import B3MTL
    m = B3MTL(n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dilations=nd, **kw)
    if w is not None:
        m.set_weights_dict(w)
    return m


def oracle_forward(x, w, ncls, nb, nd):
    """oracle.b3_mtl.forward at another depth: (outputs [S, M, (N,) R, 3C] concatenated, trunk)."""
    trunk = b3_mtl.tcn_forward(np.asarray(x, np.float32), w, nb, nd)
    return np.concatenate(b3_mtl.mtl_heads(trunk.reshape(trunk.shape[0], -1), w, ncls), axis=1), trunk


def rows_to_check(N, n=8):
    return np.unique(np.r_[0:min(n // 2, N), max(0, N - n // 2):N])


# ---------------------------------------------------------------------------------------------------
# 1. inference forward (smh_model_forward_f32): outputs and trunk tap
# ---------------------------------------------------------------------------------------------------
FORWARD_SHAPES = [  # (n_feat, nb_stacks, n_dilations, W, N, n_classes)
    (20, 3, 8, 25, 3, 3), (40, 3, 8, 50, 307, 5), (60, 3, 6, 75, 1, 3), (80, 3, 3, 100, 3, 5), (100, 1, 1, 68, 307, 3),
    (120, 3, 8, 68, 3, 3), (160, 10, 8, 68, 307, 3), (200, 3, 6, 50, 3, 5), (240, 10, 16, 68, 3, 3), (240, 1, 1, 100, 1, 5),
    (402, 3, 8, 68, 3, 3), (402, 10, 8, 100, 1, 5), (61, 3, 3, 68, 307, 3), (75, 10, 8, 25, 3, 5), (75, 1, 1, 75, 1, 3),
    (61, 10, 16, 50, 3, 3),
]


@pytest.mark.parametrize("F,nb,nd,W,N,ncls", FORWARD_SHAPES)
def test_forward_and_trunk_vs_oracle(F, nb, nd, W, N, ncls):
    w = weights(F, W, ncls, nb, nd)
    m = model(F, W, ncls, nb, nd, w)
    x = np.random.default_rng(F * 7 + W + N).standard_normal((N, W, F)).astype(np.float32)
    trunk = torch.full((N, W, 32), float("nan"), device="cuda")
    out = host(m.forward_device(at_end_of_buffer(x), trunk=trunk))
    m.check_status()
    assert np.isfinite(out).all() and np.isfinite(host(trunk)).all()
    sel = rows_to_check(N)
    ref, ref_trunk = oracle_forward(x[sel], w, ncls, nb, nd)
    np.testing.assert_allclose(host(trunk)[sel], ref_trunk, atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out[sel], ref, atol=1e-4)
    assert np.array_equal(out[sel][:, -ncls:].argmax(1), ref[:, -ncls:].argmax(1))


@pytest.mark.parametrize("F,nb,nd,expect_skew", [(120, 10, 8, 1), (61, 10, 16, 0)])
def test_deep_block_schedules_agree_bit_for_bit(F, nb, nd, expect_skew, monkeypatch):
    """SMH_TCN_SKEW=0 (barrier per block) against =2 (the skewed task list whenever it can run) at 80 and 160 blocks, W = 68 with
    four patches per workgroup (17 column tiles): 80 x 17 < 2048 tasks runs the skew schedule, 160 x 17 falls back to the barrier
    schedule (smh_tcn.hip: the task decode is exact below 2048).  Same bits either way, both within 1e-4 of the oracle."""
    W, N, ncls = 68, 1030, 3
    w = weights(F, W, ncls, nb, nd, seed=5)
    m = model(F, W, ncls, nb, nd, w)
    x = at_end_of_buffer(np.random.default_rng(3).standard_normal((N, W, F)).astype(np.float32))
    sched = m.lib.smh_internal_tcn_schedule  # test-only export, not in include/smh.h
    sched.restype, sched.argtypes = C.c_int, [C.c_void_p, C.c_int]
    outs = {}
    for skew in ("2", "0"):
        monkeypatch.setenv("SMH_TCN_SKEW", skew)
        assert sched(m._h, N) == (expect_skew if skew == "2" else 0)
        trunk = torch.empty((N, W, 32), device="cuda")
        outs[skew] = (host(m.forward_device(x, trunk=trunk)), host(trunk))
        m.check_status()
    assert np.array_equal(outs["2"][0], outs["0"][0]) and np.array_equal(outs["2"][1], outs["0"][1])
    sel = rows_to_check(N)
    ref, _ = oracle_forward(host(x)[sel], w, ncls, nb, nd)
    np.testing.assert_allclose(outs["0"][0][sel], ref, atol=1e-4)
    assert np.array_equal(outs["0"][0][sel][:, -ncls:].argmax(1), ref[:, -ncls:].argmax(1))


# ---------------------------------------------------------------------------------------------------
# 2. cascaded model
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,nb,nd,W,N,ncls", [(61, 3, 8, 50, 7, 5), (120, 10, 8, 68, 307, 3), (40, 1, 1, 25, 1, 3)])
def test_cascaded_forward_vs_reference(F, nb, nd, W, N, ncls):
    from sm_hpss_mtl_amd.lib.proposed_architectures import get_Lemaire_Cascaded_MTL_model
    from sm_hpss_mtl_amd.model import CascadedMTL
    if (nb, nd) == (3, 8):
        m, _ = get_Lemaire_Cascaded_MTL_model(TR_STEPS=10, N_MELS=F, n_classes=ncls, patch_size=W, seed=0)
    else:  # the factory builds the reference's default depth; the class takes the tuned ones
        m = CascadedMTL(n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dilations=nd, seed=0)
    w = cref.init_weights(seed=3, n_feat=F, patch_size=W, n_classes=ncls)
    w.update((k, v) for k, v in weights(F, W, 3, nb, nd, seed=3).items() if k.startswith("tcn/"))
    w = {name: w[name] for name, _, _, _ in m._spec}
    m.set_weights_dict(w)
    x = np.random.default_rng(W + N).standard_normal((N, W, F)).astype(np.float32)
    out = host(m.forward_device(at_end_of_buffer(x)))
    m.check_status()
    sel = rows_to_check(N)
    trunk = b3_mtl.tcn_forward(x[sel], w, nb, nd)
    ref = np.concatenate(cref.heads_forward(trunk.reshape(len(sel), -1), w, ncls), axis=1)
    assert np.abs(out[sel] - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())  # tests/test_cascaded_gpu.py
    assert np.array_equal(out[sel][:, -ncls:].argmax(1), ref[:, -ncls:].argmax(1))


# ---------------------------------------------------------------------------------------------------
# 3. dense file-level inference and the split-bf16 forward at the same widths
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,nb,nd,W,shift,Tc", [(40, 3, 8, 25, 1, 300), (80, 3, 6, 68, 3, 517), (160, 10, 8, 50, 7, 400),
                                                (200, 1, 1, 100, 1, 180)])
def test_dense_forward_vs_built_patches_and_oracle(F, nb, nd, W, shift, Tc):
    """forward_dense (layer 0 once per frame, every patch a window of it) against forward_device on the patches it implies,
    gathered here in numpy, within 2e-5 (tests/test_inference_gpu.py), and a few patches against the oracle at 1e-4."""
    w = weights(F, W, 3, nb, nd, seed=5)
    m = model(F, W, 3, nb, nd, w)
    fv = np.random.default_rng(F + Tc).standard_normal((F, Tc)).astype(np.float32)
    got = m.forward_dense(at_end_of_buffer(fv), shift)
    starts = ofe.patch_starts(Tc, W, shift)
    x = np.stack([fv[:, s:s + W].T for s in starts])
    assert got.shape == (len(starts), m.out_dim)
    ref = m.forward_device(at_end_of_buffer(x))
    m.check_status()
    assert float((got - ref).abs().max()) <= 2e-5
    sel = rows_to_check(len(starts), 4)
    np.testing.assert_allclose(host(got)[sel], oracle_forward(x[sel], w, 3, nb, nd)[0], atol=1e-4)


@pytest.mark.parametrize("F", [20, 60, 100, 61])
def test_dense_forward_refuses_widths_off_the_8_grid(F):
    m = model(F, 68, 3, 3, 8, seed=0)
    with pytest.raises(ValueError, match="must be a multiple of 8"):
        m.forward_dense(torch.zeros((F, 200), device="cuda"), 1)


@pytest.mark.parametrize("F,nb,nd,W,N,ncls", [(20, 3, 8, 68, 301, 3), (61, 3, 6, 50, 7, 5), (100, 10, 8, 68, 37, 3),
                                              (200, 1, 1, 25, 1, 3), (256, 3, 3, 100, 3, 5), (40, 10, 16, 75, 5, 3)])
def test_split_bf16_forward_vs_f32_and_oracle(F, nb, nd, W, N, ncls):
    w = weights(F, W, ncls, nb, nd, seed=1)
    m = model(F, W, ncls, nb, nd, w)
    x_np = np.random.default_rng(F + N).standard_normal((N, W, F)).astype(np.float32)
    x = at_end_of_buffer(x_np)
    ref = m.forward_device(x)
    got = m.forward_device(x, dtype="bf16")
    m.check_status()
    assert torch.isfinite(got).all()
    # Finding: split operands carry ~1e-5 RELATIVE error per block, so the distance to f32 grows with depth and with the size of
    # the output.  Up to 24 blocks it stays inside test_bf16_gpu.py's absolute 1e-4; at 80 / 160 blocks the linear R outputs
    # reach 10-14 and the distance 1.5-3e-4 (measured; the f32 forward stays within 1e-5 of the oracle there): above 24 blocks
    # the bound is 1e-4 of the output's scale.  A wrong index or mask moves outputs by O(1), far beyond either.
    tol = TOL_SPLIT * (1.0 if nb * nd <= 24 else max(1.0, float(ref.abs().max())))
    assert float((got - ref).abs().max()) <= tol
    assert float((got[:, -ncls:].argmax(1) == ref[:, -ncls:].argmax(1)).float().mean()) >= MIN_AGREE
    sel = rows_to_check(N)
    assert np.max(np.abs(host(got)[sel] - oracle_forward(x_np[sel], w, ncls, nb, nd)[0])) <= tol


def test_split_bf16_forward_refuses_402_features():
    m = model(402, 68, 3, 3, 8, seed=0)
    with pytest.raises(ValueError, match="n_feat=402 exceeds the 256 features"):
        m.forward_device(torch.zeros((2, 68, 402), device="cuda"), dtype="bf16")


# ---------------------------------------------------------------------------------------------------
# 4. training step
# ---------------------------------------------------------------------------------------------------
def problem(F, W, ncls, nb, nd, N, seed=0):
    rng = np.random.default_rng(seed)
    w = b3_mtl.init_weights(seed=3, n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dil=nd, randomize_bn=True)
    x = rng.standard_normal((N, W, F)).astype(np.float32)
    heads = b3_mtl.head_spec(ncls)
    y = {n: ((rng.random((N, od)) > 0.5).astype(np.float32) if act == "sigmoid" else rng.random((N, od)).astype(np.float32))
         for n, od, act in heads}
    y["3C"] = np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, N)]
    drop_tcn = ((rng.random((N, nb * nd, 32)) > 0.2) / 0.8).astype(np.float32)
    drop_heads = ((rng.random((N, len(heads), 16)) > 0.4) / 0.6).astype(np.float32)
    return w, x, y, drop_tcn, drop_heads


def flat_to_dict(m, flat):
    out, o = {}, 0
    for name, shape, _, _ in m._spec:
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    return out


TRAIN_SHAPES = [  # (n_feat, nb_stacks, n_dilations, W, N, n_classes)
    (20, 1, 1, 68, 5, 3), (61, 3, 6, 68, 1, 3), (120, 10, 8, 68, 5, 5), (402, 3, 6, 50, 5, 3), (61, 10, 8, 68, 301, 3),
    (20, 3, 6, 25, 5, 5),
]


@pytest.mark.parametrize("schedule", ["default", "skew", "bf16"])
@pytest.mark.parametrize("F,nb,nd,W,N,ncls", TRAIN_SHAPES)
def test_gradients_and_losses_vs_oracle(F, nb, nd, W, N, ncls, schedule, monkeypatch):
    """train_on_batch(apply=False) with fixed dropout masks against oracle.b3_mtl_train.forward_backward at the same depth:
    losses and every gradient tensor (tests/test_training_gpu.py: test_gradients_and_losses_vs_oracle for small batches,
    test_gradients_and_losses_at_the_config4_batch for the batch of ~300).

    The bf16 step: its backward against the f32 backward on the same split-bf16 forward (SMH_BWD_BF16=0, 2e-4 relative L2:
    test_bf16_backward_equals_the_f32_backward_on_the_same_forward), and every gradient tensor against the oracle in relative L2.
    Finding: the per-element bounds of the 240 / 24-block tests do not hold there.  The channel maximum of some rows has its top
    two channels within 5.6e-6 (n_feat 20, W 25) to 8.3e-6 (80 blocks) of each other, relative; the forward's ~1e-5 error hands
    the maximum to the other channel, and that block's kernel and bias move by up to 16 % of their maximum.  Measured against
    the oracle: the whole TCN gradient within 1.2e-2 relative L2, the worst single tensor 7.6e-2 (80 blocks, 5 patches), shapes
    without such a tie 4e-5.  The bounds: 3e-2 on the whole TCN gradient (the config-4 bf16 bound of one tensor), 1e-1 on each
    tensor.  Saving the gates of 80 blocks with a 24-block stride moves the whole TCN gradient by 0.9-1.0 relative L2."""
    if schedule == "bf16" and F > 256:
        pytest.skip("the split-bf16 forward has n_feat <= 256 (refusal: test_bf16_training_refuses_402_features)")
    if schedule == "skew":
        monkeypatch.setenv("SMH_TCN_SKEW", "2")
    w, x, y, drop_tcn, drop_heads = problem(F, W, ncls, nb, nd, N, seed=F + N)
    lw = {"S": 0.7, "R": 1.3}
    m = model(F, W, ncls, nb, nd, w, loss_weights=lw)
    if schedule == "bf16":
        m.train_dtype = "bf16"
        assert m.train_dtype == "bf16"
    heads = [n for n, _, _ in b3_mtl.head_spec(ncls)]
    got = m.train_on_batch(at_end_of_buffer(x), y, drop_tcn=torch.from_numpy(drop_tcn).cuda(),
                           drop_heads=torch.from_numpy(drop_heads).cuda(), apply=False)
    ref = tr.forward_backward(x, y, w, ncls, drop_tcn, {h: drop_heads[:, i] for i, h in enumerate(heads)}, lw,
                              nb_stacks=nb, n_dil=nd)
    assert abs(got[0] - ref["loss"]) < 2e-4 * max(1.0, abs(ref["loss"]))
    for i, name in enumerate(heads + ["3C"]):
        assert abs(got[1 + i] - ref["losses"][name]) < 2e-4 * max(1.0, abs(ref["losses"][name])), name
    assert abs(got[-1] - ref["acc"]) < 1e-6
    g = flat_to_dict(m, host(m._grad_tensor()))
    assert set(g) - set(ref["grads"]) == set()
    if schedule == "bf16":
        monkeypatch.setenv("SMH_BWD_BF16", "0")
        m.train_on_batch(at_end_of_buffer(x), y, drop_tcn=torch.from_numpy(drop_tcn).cuda(),
                         drop_heads=torch.from_numpy(drop_heads).cuda(), apply=False)
        g32 = flat_to_dict(m, host(m._grad_tensor()).astype(np.float64))
        for name, gref in g32.items():
            if name.endswith(tr.TRAINABLE_SKIP):
                continue
            rel = np.linalg.norm(g[name] - gref) / max(np.linalg.norm(gref), 1e-12)
            assert rel <= 2e-4 or np.abs(gref).max() < 1e-5, (name, rel)
        dev_tcn, ref_tcn = [], []
        for name, gref in ref["grads"].items():
            if name.endswith(tr.TRAINABLE_SKIP) or name.endswith("/dense/bias"):  # (dense/bias: analytically zero, see below)
                continue
            gg = g[name].astype(np.float64) + (2 * tr.L2 * w[name] if name.endswith("/dense/kernel") else 0.0)
            rel = np.linalg.norm(gg - gref) / max(np.linalg.norm(gref), 1e-12)
            assert rel <= 1e-1, (name, rel)
            if name.startswith("tcn/"):
                dev_tcn.append((gg - gref).ravel())
                ref_tcn.append(gref.ravel())
        rel_tcn = np.linalg.norm(np.concatenate(dev_tcn)) / np.linalg.norm(np.concatenate(ref_tcn))
        assert rel_tcn <= 3e-2, rel_tcn
        return
    for name, gref in ref["grads"].items():
        if name.endswith(tr.TRAINABLE_SKIP):
            continue
        gg = g[name].astype(np.float64)
        if name.endswith("/dense/kernel"):
            gg = gg + 2 * tr.L2 * w[name]  # the l2 term is added at apply time on the device
        scale = max(np.abs(gref).max(), 1e-6)
        atol = 2e-5 if name.endswith("/dense/bias") else 1e-6
        err = np.abs(gg - gref).max()
        if N < 100:
            # test_gradients_and_losses_vs_oracle: a forward eps from the oracle's flips a fraction ~ eps of the relu / channel-max
            # gates; the gradient moves by ~ sqrt(eps): 2e-3 (f32 forward)
            assert err <= 2e-3 * scale + atol, (name, err, scale)
        else:
            # test_gradients_and_losses_at_the_config4_batch: with hundreds of patches a handful of rows sit within float32
            # rounding of a gate; tensor-level agreement (relative L2) stays tight, single elements may move further.
            # Finding: at 80 blocks x 301 patches one kernel sits at 3.8e-3 relative L2 (8.3e-3 of its maximum per element;
            # n_feat 240 at the same depth: 2.9e-3).  The same batch at 24 blocks agrees to 1.2e-6: the extra 56 blocks' gates
            # include channel maxima tied within float32 rounding.  Above 24 blocks the tensor bound is 5e-3.
            rel_l2 = np.linalg.norm(gg - gref) / max(np.linalg.norm(gref), 1e-12)
            assert rel_l2 <= (2e-3 if nb * nd <= 24 else 5e-3) or name.endswith("/dense/bias"), (name, rel_l2)
            assert err <= 1e-2 * scale + atol, (name, err, scale)


def test_deterministic_gradients_bit_reproducible_deep_and_narrow():
    """deterministic_gradients at 80 blocks, n_feat = 61, 301 patches: three runs give identical buckets (gradient and BN batch
    statistics), equal to the float-atomic gradient up to summation noise (tests/test_training_gpu.py)."""
    if os.environ.get("SMH_DETERMINISTIC"):
        pytest.skip("the mode under test is forced on by SMH_DETERMINISTIC: nothing to compare it with")
    F, nb, nd, W, N = 61, 10, 8, 68, 301
    w, x, y, drop_tcn, drop_heads = problem(F, W, 3, nb, nd, N, seed=21)
    m = model(F, W, 3, nb, nd, w)
    xd, dt, dh = torch.from_numpy(x).cuda(), torch.from_numpy(drop_tcn).cuda(), torch.from_numpy(drop_heads).cuda()

    def grad():
        m.train_on_batch(xd, y, drop_tcn=dt, drop_heads=dh, apply=False)
        torch.cuda.synchronize()
        return m._bucket_tensor().clone()
    free = grad()
    m.deterministic_gradients = True
    det = [grad() for _ in range(3)]
    assert torch.equal(det[0], det[1]) and torch.equal(det[0], det[2])
    n = m.count_params()
    assert float((det[0][:n] - free[:n]).abs().max()) <= 2e-6 * float(free[:n].abs().max())


def test_sgd_steps_match_oracle_at_another_shape():
    """Two applied SGD steps (momentum, clipnorm, BN moving statistics) at n_feat = 61, 18 blocks, W = 50 against
    oracle.b3_mtl_train.sgd_step: the optimiser's weight-offset tables at another n_feat / n_blocks (test_sgd_step_matches_oracle)."""
    F, nb, nd, W, ncls, N = 61, 3, 6, 50, 5, 8
    w, x, y, drop_tcn, drop_heads = problem(F, W, ncls, nb, nd, N, seed=5)
    m = model(F, W, ncls, nb, nd, w, TR_STEPS=10)
    heads = [n for n, _, _ in b3_mtl.head_spec(ncls)]
    wd, vel = {k: v.astype(np.float64) for k, v in w.items()}, {}
    for step in range(2):
        m.train_on_batch(x, y, drop_tcn=torch.from_numpy(drop_tcn).cuda(), drop_heads=torch.from_numpy(drop_heads).cuda())
        ref = tr.forward_backward(x, y, wd, ncls, drop_tcn, {h: drop_heads[:, i] for i, h in enumerate(heads)},
                                  nb_stacks=nb, n_dil=nd)
        wd, vel = tr.sgd_step(wd, ref["grads"], vel, ref["bn_batch"], tr.exponential_decay(step, 0.002, 30, 0.1))
    got = m.get_weights_dict()
    for k, v in wd.items():
        delta = np.abs(v - w[k]).max()
        assert np.abs(got[k] - v).max() <= 2e-3 * max(delta, 1e-7) + 1e-7, k


def test_bf16_training_refuses_402_features():
    """smh_trainer_set_dtype(1) refuses a model the split-bf16 forward cannot run -- at train_dtype = 'bf16', not at the first
    step; the model keeps training in f32."""
    from sm_hpss_mtl_amd import _lib
    w, x, y, _, _ = problem(402, 50, 3, 3, 6, 4)
    m = model(402, 50, 3, 3, 6, w)
    with pytest.raises(ValueError, match="n_feat=402 exceeds the 256 features"):
        m.train_dtype = "bf16"
    assert m.train_dtype == "f32"
    assert np.isfinite(m.train_on_batch(x, y, apply=False)).all()
    assert m._trainer is not None
    assert m.lib.smh_trainer_set_dtype(m._trainer, 1) == _lib.SMH_E_INVALID
    assert b"n_feat=402" in m.lib.smh_last_error()
    with pytest.raises(ValueError, match="n_feat=402"):
        m.train_dtype = "bf16"
    assert np.isfinite(m.train_on_batch(x, y, apply=False)).all()


# ---------------------------------------------------------------------------------------------------
# 5. front end at other n_mels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [20, 40, 80])
@pytest.mark.parametrize("n_samples,W,shift", [(16000, 50, 25), (160000, 68, 34)])
def test_frontend_and_fused_layer0_at_other_n_mels(n_mels, n_samples, W, shift):
    """LogMelHarmPercSpec with n_mels != 120: featuregram against the oracle on the device's own S (1e-3 dB, every bin), the
    patches against the oracle's standardise + gather of the device's fv (2e-4), then the fused layer-0 path
    (features_l0 -> forward_from_x0, 2 n_mels features) against features -> forward_device (2e-5) and the oracle (1e-4)
    (tests/test_parity_gpu.py: test_frontend_randomised_lengths_and_feature_names, test_layer0_fused_into_features_...)."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.synth import synth_clips
    fe = Frontend(FrontendConfig(n_mels=n_mels))
    y = synth_clips(2, seed=40 + n_mels, n_samples=n_samples)
    audio = torch.from_numpy(y).cuda()
    res = fe.run(audio, W=W, shift=shift)
    S = fe.stft_mag(audio)
    fv, patches, Sh = host(res["fv"]), host(res["patches"]), host(S)
    T = 1 + (n_samples - 400) // 160
    nP = res["n_patches"]
    assert fv.shape == (2, 2 * n_mels, T) and patches.shape == (2 * nP, W, 2 * n_mels)
    for i in range(2):
        ref = ofe.featuregram_from_S(Sh[i], "LogMelHarmPercSpec", n_mels=n_mels)
        assert np.max(np.abs(fv[i] - ref)) <= 1e-3, (i, float(np.max(np.abs(fv[i] - ref))))
        refp = ofe.tcn_input(ofe.feature_patches(fv[i], W, shift))
        assert refp.shape[0] == nP
        np.testing.assert_allclose(patches[i * nP:(i + 1) * nP], refp, atol=2e-4)
    F = 2 * n_mels
    w = weights(F, W, 3, 3, 8, seed=4)
    m = model(F, W, 3, 3, 8, w)
    harm, perc = fe.hpss_median(S)
    two = fe.features(S, harm, perc, W=W, shift=shift)
    ref = m.forward_device(two["patches"])
    sel = rows_to_check(2 * nP)
    oracle = oracle_forward(host(two["patches"])[sel], w, 3, 3, 8)[0]
    assert np.max(np.abs(host(ref)[sel] - oracle)) <= 1e-4
    if 4 * n_mels * ((T | 1) + 3) > 150 * 1024:
        # the fused kernel keeps a whole featuregram half in LDS (smh_feat.hip launch_std_patch): 998 frames of 40 or more mel
        # rows are refused with a clear error, not run
        with pytest.raises(ValueError, match="fits one LDS tile"):
            fe.features_l0(S, harm, perc, 0, W, shift, m, patches=True)
        return
    fused = fe.features_l0(S, harm, perc, 0, W, shift, m, patches=True)
    got = m.forward_from_x0(fused["x0p"])
    m.check_status()
    torch.cuda.synchronize()
    assert torch.equal(fused["fv"], two["fv"]) and torch.equal(fused["patches"], two["patches"])
    assert float((got - ref).abs().max()) <= 2e-5
    assert np.max(np.abs(host(got)[sel] - oracle)) <= 1e-4


# ---------------------------------------------------------------------------------------------------
# 6. refusals at construction
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,msg", [(dict(nb_filters=16), "nb_filters=32"), (dict(kernel_size=5), "kernel_size=3"),
                                    (dict(n_dilations=17), "stacks/dilations"), (dict(patch_size=513), "n_feat/patch_size")])
def test_unsupported_configurations_are_refused_at_construction(kw, msg):
    from sm_hpss_mtl_amd.model import B3MTL
    args = dict(n_feat=120, patch_size=68, n_classes=3)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        B3MTL(**args)
    m = model(120, 68, 3, 3, 8, seed=0)  # the library is still usable
    assert torch.isfinite(m.forward_device(torch.zeros((1, 68, 120), device="cuda"))).all()
