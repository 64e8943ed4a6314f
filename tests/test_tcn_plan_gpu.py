"""GPU (no kernel is launched): the library's own plan of the network forward (smh_internal_tcn_plan, the function the launcher
calls) equals the restatement of tests/tcn_plans.py on all eight values, and smh_internal_tcn_schedule agrees with its mode --
over patch lengths on both sides of every LDS step, feature widths up to the one whose layer-0 staging costs the weight slots,
depths on both sides of the skew schedule's task bound, batch sizes around every patches-per-workgroup step, the two switches the
tests flip, and the training forward."""
import ctypes as C

import pytest

from tests import tcn_plans as P

pytestmark = pytest.mark.gpu

MODELS = [  # (n_feat, nb_stacks, n_dilations, W)
    (240, 3, 8, 68), (240, 3, 8, 99), (240, 3, 8, 249), (240, 3, 8, 500), (240, 3, 8, 5), (20, 1, 1, 16), (20, 3, 8, 30),
    (402, 10, 8, 68), (240, 10, 16, 68), (480, 3, 8, 68), (240, 1, 1, 417), (402, 3, 8, 512),
]
BATCHES = (1, 2, 37, 255, 256, 257, 510, 512, 768, 1024, 1030)
SWITCHES = [{"SMH_TCN_SKEW": k, "SMH_TCN_SPLIT": s} for k in (None, "0", "2") for s in (None, "0")]


def test_models_cover_the_issue_s_shapes():
    assert {m[3] for m in MODELS} == {5, 16, 30, 68, 99, 249, 417, 500, 512} and {m[0] for m in MODELS} == {20, 240, 402, 480}
    assert {m[1:3] for m in MODELS} == {(1, 1), (3, 8), (10, 8), (10, 16)}


@pytest.mark.parametrize("F,nb,nd,W", MODELS)
def test_library_plan_equals_the_restatement(F, nb, nd, W, monkeypatch):
    from sm_hpss_mtl_amd import _lib
    lib = _lib.load()
    query, sched = lib.smh_internal_tcn_plan, lib.smh_internal_tcn_schedule  # test-only exports, not in include/smh.h
    query.restype, query.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int * 8)]
    sched.restype, sched.argtypes = C.c_int, [C.c_void_p, C.c_int]
    for name in P.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    cfg, h = _lib.ModelCfg(F, W, 3, 32, 3, nb, nd, 0), C.c_void_p()
    created = lib.smh_model_create(C.byref(cfg), C.byref(h)) == 0
    try:
        n = 0
        for env in SWITCHES:
            for k, v in env.items():
                monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
            set_ = {k: v for k, v in env.items() if v is not None}
            for N in BATCHES:
                for train in (0, 1):
                    try:
                        want = P.plan(W, F, nb * nd, N, bool(train), set_)
                    except P.Refused:
                        want = None
                    if not created:  # the library refuses the model itself: so must the restatement
                        assert want is None, (N, env)
                        continue
                    got = (C.c_int * 8)()
                    rc = query(h, N, train, C.byref(got))
                    assert (rc, None if rc else tuple(got)) == ((-1, None) if want is None else (0, tuple(want))), (N, train, env)
                    if not train:
                        assert sched(h, N) == (-1 if want is None else int(want.mode in (P.SKEW, P.SKEW16))), (N, env)
                    n += 1
        assert n == len(SWITCHES) * len(BATCHES) * 2 or not created
    finally:
        if created:
            lib.smh_model_destroy(h)
