"""GPU (no GEMM is launched): the library's own launch plans of the Conv2D models (smh_internal_cnn_plan: the plan functions and the
switches the launchers use) equal the restatement of tests/cnn_plans.py on every value the restatement returns -- for every
Conv2D / Dense layer of the smallest shapes the other Conv2D cases use, at batches on both sides of every step of a plan, under no
switch and each forced one, with the partial buffer a trainer of that batch would own and with one too small for every split."""
import ctypes as C

import pytest

from tests import cnn_plans as P
from tests.test_cnn_train_plans_gpu import FORCED

pytestmark = pytest.mark.gpu

FWD_F32, FWD_BF16, TRAIN_FWD, WGRAD, DGRAD, COL_REDUCE = range(6)  # `what` of smh_internal_cnn_plan

MODELS = [  # (kind, H, W, fc, single)
    ("Doukhan", 30, 68, 0, False), ("Doukhan", 40, 68, 0, False), ("Doukhan", 64, 80, 0, False),
    ("Papakostas", 61, 68, 64, False), ("Papakostas", 61, 68, 100, False), ("Papakostas", 66, 40, 64, False),
    ("Jang", 514, 1, 0, False), ("Jang", 514, 4, 0, False), ("Jang", 514, 12, 0, False),
    ("Doukhan", 21, 68, 0, True), ("Papakostas", 61, 68, 64, True), ("Jang", 257, 12, 0, True),
]
BATCHES = (1, 2, 3, 5, 6, 8, 40, 63, 64, 65, 70, 160, 190)  # 65 and 70: queried as their passes [64, 1] and [64, 6]
WORKSPACE_BATCHES = BATCHES + (130,)
SWITCHES = [None] + [(var, val) for var, val, _ in FORCED]
SMALL_CAP = 10000  # floats: below one slice pair of every split GEMM of Doukhan 30 x 68 at N = 8 (see test_a_small_cap_...)
KINDS = {"Doukhan": 0, "Papakostas": 1, "Jang": 2}


def _lib():
    from sm_hpss_mtl_amd import _lib
    lib = _lib.load()
    query, floats = lib.smh_internal_cnn_plan, lib.smh_internal_cnn_partial_floats  # test-only exports, not in include/smh.h
    query.restype, query.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int * 8)]
    floats.restype, floats.argtypes = C.c_size_t, [C.c_void_p, C.c_int]
    return _lib, lib


def _create(_lib, lib, kind, H, W, fc, single):
    cfg, h = _lib.CnnCfg(KINDS[kind] + (3 if single else 0), H, W, 3, 0, 512, fc, 16000.0), C.c_void_p()
    _lib.check(lib.smh_cnn_create(C.byref(cfg), C.byref(h)), "smh_cnn_create")
    return h


def _ask(lib, h, index, what, N, cap):
    got = (C.c_int * 8)()
    rc = lib.smh_internal_cnn_plan(h, index, what, N, cap, C.byref(got))
    return tuple(got) if rc == 0 else None


def _gemm(rows, cols, p, partial):
    return P.tiles(rows, cols) + (p["ksteps"], p["ksplit"], p["ksteps_per"], partial, 0)


def want_forward(L, n, bf16, single):
    p = P.forward_plan(L, n, bf16=bf16, single=single)
    return _gemm(p["M"], L["OC"], p, p["ksplit"] * p["M"] * L["OC"] if p["ksplit"] > 1 else 0)


def want_train_forward(L, N, cap):
    p = P.train_forward_plan(L, N, cap)
    return _gemm(p["M"], L["OC"], p, p["partial"])


def want_wgrad(L, N, cap, switch):
    var, val = switch or (None, None)
    p = P.wgrad_plan(L, N, cap, env=val if var == "SMH_CNN_WSPLIT" else None, mfma=var == "SMH_CNN_WGRAD_MFMA")
    if p["kind"] == "smallk":
        return (0, 0, 0, 0, p["blocks"], p["rows_per_block"], p["partial"], 1)
    return _gemm(L["K"], L["OC"], p, p["partial"])


def want_dgrad(L, N, cap, switch):
    if L["index"] == 0:
        return None
    var, val = switch or (None, None)
    p = P.dgrad_plan(L, N, cap, env=val if var == "SMH_CNN_DSPLIT" else None)
    return _gemm(p["M"], p["ldc"], p, p["partial"])


def want_col_reduce(L, N):
    p = P.col_reduce_plan(N * L["OH"] * L["OW"], L["OC"])
    return (int(p["vec"]), p["slabs"], p["rows_per_pass"], p["rows_per_block"], p["blocks"], 0, 0, 0)


def _check_training(lib, h, layers, N, cap, switch):
    for L in layers:
        i = L["index"]
        assert _ask(lib, h, i, TRAIN_FWD, N, cap) == want_train_forward(L, N, cap), (L["name"], N, cap, switch)
        assert _ask(lib, h, i, WGRAD, N, cap) == want_wgrad(L, N, cap, switch), (L["name"], N, cap, switch)
        assert _ask(lib, h, i, DGRAD, N, cap) == want_dgrad(L, N, cap, switch), (L["name"], N, cap, switch)
        assert _ask(lib, h, i, COL_REDUCE, N, cap) == want_col_reduce(L, N), (L["name"], N)


@pytest.mark.parametrize("kind,H,W,fc,single", MODELS, ids=["%s-%dx%d-fc%d%s" % (m[:4] + ("-single" * m[4],)) for m in MODELS])
def test_library_plans_equal_the_restatement(kind, H, W, fc, single, monkeypatch):
    _l, lib = _lib()
    for var, _, _ in FORCED:
        monkeypatch.delenv(var, raising=False)
    layers = P.graph(kind, H, W, fc=fc or 4096, single=single)
    conv = {L["index"] for L in layers}
    h = _create(_l, lib, kind, H, W, fc, single)
    try:
        # a layer that is not Conv2D / Dense has no GEMM plan (Jang: the mel-scale layer at 0; everywhere: the pools between)
        for i in range(-1, max(conv) + 3):
            if i not in conv:
                assert all(_ask(lib, h, i, what, 8, 1 << 20) is None for what in range(6)), i
        for N in BATCHES:
            for n in sorted(set(P.passes(N))):
                for L in layers:
                    for what, bf16 in ((FWD_F32, False), (FWD_BF16, True)):
                        assert _ask(lib, h, L["index"], what, n, 0) == want_forward(L, n, bf16, single), (L["name"], n, bf16)
            cap = lib.smh_internal_cnn_partial_floats(h, P.trainer_cap(N))
            assert cap == P.trainer_partial_floats(layers, P.trainer_cap(N))
            for switch in SWITCHES:
                if switch:
                    monkeypatch.setenv(*switch)
                _check_training(lib, h, layers, N, cap, switch)
                if switch:
                    monkeypatch.delenv(switch[0])
        for N in WORKSPACE_BATCHES:
            assert lib.smh_cnn_workspace_bytes(h, N) == P.workspace_bytes(layers, H, W, N, single), N
    finally:
        lib.smh_cnn_destroy(h)


def test_a_small_cap_cuts_the_forward_the_weight_gradient_and_the_data_gradient_split(monkeypatch):
    """Doukhan 30 x 68 at N = 8 with room for SMALL_CAP floats of partials: fc1's training forward (6 slices of 4096 floats), conv2's
    weight gradient (10 slices of 73 728) and conv2's data gradient (9 slices of 212 992) each lose slices to the cap, in the
    restatement and, value for value, in the library -- also under every forced switch."""
    _l, lib = _lib()
    for var, _, _ in FORCED:
        monkeypatch.delenv(var, raising=False)
    layers, N = P.graph("Doukhan", 30, 68), 8
    big = P.trainer_partial_floats(layers, P.trainer_cap(N))
    fc1, c2 = (next(L for L in layers if L["name"] == n) for n in ("fc1", "conv2"))
    assert (P.train_forward_plan(fc1, N, big)["ksplit"], P.train_forward_plan(fc1, N, SMALL_CAP)["ksplit"]) == (6, 2)
    assert (P.wgrad_plan(c2, N, big)["ksplit"], P.wgrad_plan(c2, N, SMALL_CAP)["ksplit"]) == (10, 1)
    assert (P.dgrad_plan(c2, N, big)["ksplit"], P.dgrad_plan(c2, N, SMALL_CAP)["ksplit"]) == (9, 1)
    h = _create(_l, lib, "Doukhan", 30, 68, 0, False)
    try:
        for switch in SWITCHES:
            if switch:
                monkeypatch.setenv(*switch)
            _check_training(lib, h, layers, N, SMALL_CAP, switch)
            if switch:
                monkeypatch.delenv(switch[0])
    finally:
        lib.smh_cnn_destroy(h)
