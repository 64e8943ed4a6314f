"""GPU: the SMH_HEADS_SINGLE head kind through the C ABI directly -- sizes, the weight round trip, the d_losses layout of a training
step, and the refusals' error codes and messages."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import single_task_ref as sref
from tests.test_single_task_ref import train_problem

pytestmark = pytest.mark.gpu

SINGLE = 3
SMH_E_INVALID = None


def _lib():
    from sm_hpss_mtl_amd import _lib
    return _lib, _lib.require_gpu()


def _create(heads, ncls, W=68, F=80, block=0):
    _l, lib = _lib()
    cfg = _l.ModelCfg(F, W, ncls, 32, 3, 3, 8, block)
    h = C.c_void_p()
    rc = lib.smh_model_create_heads(C.byref(cfg), heads, C.byref(h))
    return rc, h


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("ncls", [2, 3, 5])
def test_sizes_weights_and_losses_layout(ncls):
    _l, lib = _lib()
    rc, h = _create(SINGLE, ncls)
    assert rc == 0
    try:
        n = 80 * 32 + 32 + 24 * (3 * 32 * 32 + 32 + 32 * 32 + 32) + 68 * 32 * ncls + ncls
        assert lib.smh_model_out_dim(h) == ncls and lib.smh_model_num_params(h) == n
        w = sref.init_weights(seed=5, n_classes=ncls)
        flat = np.concatenate([v.ravel() for v in w.values()]).astype(np.float32)
        assert flat.size == n
        st = _l.current_stream()
        assert lib.smh_model_set_weights(h, flat.ctypes.data_as(C.c_void_p), n, st) == 0
        back = np.zeros(n, np.float32)
        assert lib.smh_model_get_weights(h, back.ctypes.data_as(C.c_void_p), n, st) == 0
        assert np.array_equal(back, flat)
        N = 6
        x, y, drop = train_problem(N, ncls)
        tr = C.c_void_p()
        assert lib.smh_trainer_create(h, 8, C.byref(tr)) == 0
        try:
            assert lib.smh_trainer_bucket_floats(tr) == n
            xd, yd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(drop).cuda()
            losses = torch.full((4,), -1.0, device="cuda")
            assert lib.smh_train_step_f32(tr, _p(xd), _p(yd), N, _p(dd), None, None, _p(losses), st) == 0, _l.last_error()
            torch.cuda.synchronize()
            lv = losses.cpu().numpy()
            ref = sref.torch_forward_backward(x, y, w, ncls, drop)
            assert lv[0] == lv[1] and lv[3] == 0.0  # [loss, loss (weight 1), accuracy, 0]
            assert abs(lv[0] - ref["loss"]) <= 2e-4 * max(1.0, abs(ref["loss"])) and abs(lv[2] - ref["acc"]) <= 1e-6
            lw = (C.c_float * 1)(0.5)
            assert lib.smh_train_step_f32(tr, _p(xd), _p(yd), N, _p(dd), None, lw, _p(losses), st) == 0
            torch.cuda.synchronize()
            lv2 = losses.cpu().numpy()
            assert lv2[0] == lv[0] and lv2[1] == np.float32(0.5) * lv[0]
            assert lib.smh_trainer_set_dtype(tr, 1) < 0 and "smh_trainer_set_dtype" in _l.last_error()
        finally:
            lib.smh_trainer_destroy(tr)
    finally:
        lib.smh_model_destroy(h)


def test_refusals_name_their_entry():
    _l, lib = _lib()
    rc, h = _create(SINGLE, 2)
    rc2, h2 = _create(SINGLE, 2)
    assert rc == 0 and rc2 == 0
    try:
        st = _l.current_stream()
        x0 = torch.zeros((1, 2, 68, 32), device="cuda")
        x = torch.zeros((1, 68, 80), device="cuda")
        out = torch.zeros((1, 2), device="cuda")
        work = torch.zeros((1 << 16,), device="cuda")
        inval = lib.smh_model_forward_x0_f32(h, _p(x0), 1, _p(out), None, st)
        assert inval < 0 and "smh_model_forward_x0_f32" in _l.last_error() and "single-task" in _l.last_error()
        for entry, args in [("smh_model_forward_bf16", (h, _p(x), 1, _p(out), st)),
                            ("smh_model_forward_bf16_ex", (h, _p(x), 1, _p(out), 1, st)),
                            ("smh_model_forward_x0_bf16", (h, _p(x0), 1, _p(out), 1, st))]:
            assert getattr(lib, entry)(*args) == inval and "smh_model_forward_bf16" in _l.last_error(), entry
        assert lib.smh_model_check_train_dtype(h, 1) == inval and "smh_trainer_set_dtype" in _l.last_error()
        assert lib.smh_fusion_forward_f32(h, _p(x), _p(x), 1, _p(out), _p(work), work.numel() * 4, st) == inval
        assert "smh_fusion_forward_f32" in _l.last_error()
        assert lib.smh_fusion_forward_x0_f32(h, _p(x0), 1, _p(work), work.numel() * 4, _p(out), st) == inval
        assert "smh_fusion_forward_x0_f32" in _l.last_error()
        e = C.c_void_p()
        assert lib.smh_late_fusion_create(h, h2, C.byref(e)) == inval and "smh_late_fusion_create" in _l.last_error()
        torch.cuda.synchronize()
    finally:
        lib.smh_model_destroy(h)
        lib.smh_model_destroy(h2)
    rc, h = _create(SINGLE, 2, block=1)
    assert rc == inval and "block_variant" in _l.last_error()
    rc, h = _create(SINGLE, 4)
    assert rc == inval and "n_classes" in _l.last_error()


@pytest.mark.parametrize("heads", [0, 1, 2])
def test_the_mtl_kinds_still_refuse_two_classes(heads):
    _l, lib = _lib()
    rc, h = _create(heads, 2, F=80)
    assert rc < 0 and "n_classes must be 3 or 5" in _l.last_error()
    rc, h = _create(4, 3)
    assert rc < 0 and "smh_model_create_heads" in _l.last_error()
