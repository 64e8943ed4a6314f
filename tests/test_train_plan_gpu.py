"""GPU (no kernel of the step is launched, no trainer is created): the library's own plan of a TCN training step
(smh_internal_train_plan: plan_train of smh_train_plan.h under the switches the step reads) equals the restatement of
tests/train_plans.py on every value -- for the four model kinds at 3 and 5 classes, patch lengths on both sides of every route
boundary, batch sizes on both sides of every heads boundary, both dtypes, under no switch and each forced one.  A step the library
refuses is refused by the restatement, and the other way round.  One stack of one dilation: creation is cheap, and the depth enters
the plan through the bf16 pack's size alone."""
import ctypes as C

import pytest

from tests import train_plans as P

pytestmark = pytest.mark.gpu

HEADS = {"B3_MTL": 0, "cascaded": 1, "fusion": 2, "single": 3}  # include/smh.h: SMH_HEADS_*
WIDTHS = (15, 32, 33, 64, 65, 68, 96, 97, 128, 129, 234, 235, 249, 256, 257, 264, 265)
BATCHES = (1, 2, 390, 391, 512, 513, 538, 539, 903, 904, 1616, 1617)
FORCED = (None, ("SMH_TRAIN_VALU", "1"), ("SMH_BWD_BF16", "0"), ("SMH_DWH_VALU", "1"), ("SMH_HEADS_GLOBAL", "1"))
N_FEAT, N_BLOCKS = 20, 1


def _lib():
    from sm_hpss_mtl_amd import _lib
    return _lib, _lib.require_gpu()


_ask = P.ask_library


def _want(kind, W, ncls, N, dtype, env):
    try:
        return P.ints(P.plan(kind, W, N_BLOCKS, ncls, N, dtype, env))
    except P.Refused:
        return None


@pytest.mark.parametrize("ncls", [3, 5])
@pytest.mark.parametrize("kind", P.KINDS)
def test_library_plan_equals_the_restatement(kind, ncls, monkeypatch):
    _l, lib = _lib()
    for var in P.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    refused = 0
    for W in WIDTHS:
        cfg, h = _l.ModelCfg(N_FEAT, W, ncls, 32, 3, 1, 1, 0), C.c_void_p()
        _l.check(lib.smh_model_create_heads(C.byref(cfg), HEADS[kind], C.byref(h)), "smh_model_create_heads")
        try:
            for switch in FORCED:
                if switch:
                    monkeypatch.setenv(*switch)
                env = dict([switch]) if switch else {}
                for dtype in (0, 1):
                    for N in BATCHES:
                        got, want = _ask(lib, h, N, dtype), _want(kind, W, ncls, N, dtype, env)
                        assert got == want, (kind, ncls, W, N, dtype, switch,
                                             [(f, g, w) for f, g, w in zip(P.FIELDS, got or (), want or ()) if g != w])
                        refused += got is None
                if switch:
                    monkeypatch.delenv(switch[0])
        finally:
            lib.smh_model_destroy(h)
    # what is refused: W = 265 (fusion: 257, 264, 265) at dtype 0, and for dtype 1 everything but B3_MTL below 265 frames
    per_w = len(FORCED) * len(BATCHES)
    f32 = (3 if kind == "fusion" else 1) * per_w
    assert refused == f32 + (per_w if kind == "B3_MTL" else len(WIDTHS) * per_w)


def test_the_query_follows_the_switches_between_calls(monkeypatch):
    """The switches are read per query, as they are per step: one model, the switch flipped between two calls."""
    _l, lib = _lib()
    for var in P.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    cfg, h = _l.ModelCfg(N_FEAT, 68, 3, 32, 3, 1, 1, 0), C.c_void_p()
    _l.check(lib.smh_model_create_heads(C.byref(cfg), HEADS["B3_MTL"], C.byref(h)), "smh_model_create_heads")
    try:
        route = P.FIELDS.index("route")
        assert P.ROUTES[_ask(lib, h, 6, 1)[route]] == "bf16"
        monkeypatch.setenv("SMH_BWD_BF16", "0")
        assert P.ROUTES[_ask(lib, h, 6, 1)[route]] == "mfma_short"
        monkeypatch.setenv("SMH_TRAIN_VALU", "1")
        assert P.ROUTES[_ask(lib, h, 6, 1)[route]] == "scalar"
        monkeypatch.delenv("SMH_TRAIN_VALU")
        monkeypatch.delenv("SMH_BWD_BF16")
        assert P.ROUTES[_ask(lib, h, 6, 1)[route]] == "bf16"
    finally:
        lib.smh_model_destroy(h)
