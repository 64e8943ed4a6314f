"""CPU: the C ABI and the Python surface of dense file-level inference on split bf16 operands -- smh_model_forward_dense_bf16 is
declared once in include/smh.h, bound in _lib.SIGNATURES with the argument types of its declaration and exported by libsmh.so;
every model's `forward_dense` and `inference.patch_probabilities` take `dtype`.  Nothing needs a GPU to import."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

ENTRY = "smh_model_forward_dense_bf16"


def _declared_args(hdr, name):
    """Arguments of the one prototype of `name` in the header (comments removed)."""
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), code)
    assert len(protos) == 1, (name, protos)
    return [a.strip() for a in protos[0].split(",")]


def test_entry_declared_and_bound():
    from sm_hpss_mtl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    args = _declared_args(hdr, ENTRY)
    assert len(args) == 8, args
    # the same arguments as the f32 entry (which takes the model as const: it has no operand cache to rebuild)
    f32 = [a.replace("const smh_model", "smh_model") for a in _declared_args(hdr, "smh_model_forward_dense_f32")]
    assert args == f32, (args, f32)
    assert ENTRY in _lib.SIGNATURES
    res, argtypes = _lib.SIGNATURES[ENTRY]
    vp = C.c_void_p
    assert res is C.c_int and argtypes == [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp], (res, argtypes)
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["smh_model_forward_dense_f32"]


def test_entry_exported():
    from sm_hpss_mtl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    assert hasattr(_lib.load(), ENTRY), "declared in smh.h but not exported: " + ENTRY


def test_python_surface():
    from sm_hpss_mtl_amd import inference
    from sm_hpss_mtl_amd.late_fusion import LateFusion
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL, FusionMTL, SingleTaskTCN
    for cls in (B3MTL, CascadedMTL, FusionMTL, SingleTaskTCN, LateFusion):
        p = inspect.signature(cls.forward_dense).parameters
        names = list(p)
        assert names[:4] == ["self", "fv", "shift", "out"], (cls.__name__, names)
        assert "dtype" in names[4:] and p["dtype"].default == "f32", (cls.__name__, names)
    assert list(inspect.signature(B3MTL.forward_dense).parameters) == ["self", "fv", "shift", "out", "dtype"]
    p = inspect.signature(inference.patch_probabilities).parameters
    assert list(p)[:6] == ["fv", "model", "W", "W_shift", "output", "batch_frames"]
    assert list(p)[-1] == "dtype" and p["dtype"].default == "f32"
    assert "HeadModel" in (inference.patch_probabilities.__doc__ or "")
