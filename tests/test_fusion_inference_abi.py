"""CPU: the C ABI of the fusion model's inference from the layer-0 partials and of its dense file-level forward -- every new symbol
is declared in include/smh.h, exported by libsmh.so and bound in _lib.SIGNATURES with the argument count of its declaration."""
import ctypes as C
import os
import re

import pytest

from tests.conftest import ROOT

NEW = {  # name -> (arguments, returns a pointer / a size / an int status)
    "smh_fusion_w0_ptr": (1, C.c_void_p),
    "smh_fusion_x0_workspace_bytes": (2, C.c_size_t),
    "smh_fusion_forward_x0_f32": (7, C.c_int),
    "smh_fusion_dense_workspace_bytes": (3, C.c_size_t),
    "smh_fusion_forward_dense_f32": (8, C.c_int),
}


def _declared_args(hdr, name):
    """Arguments of the one prototype of `name` in the header (comments removed)."""
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), code)
    assert len(protos) == 1, (name, protos)
    return [a.strip() for a in protos[0].split(",")]


def test_new_symbols_declared_bound_and_exported():
    from sm_hpss_mtl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    for name, (nargs, res) in NEW.items():
        args = _declared_args(hdr, name)
        assert len(args) == nargs, (name, args)
        assert name in _lib.SIGNATURES, name
        got_res, got_args = _lib.SIGNATURES[name]
        assert len(got_args) == nargs and got_res is res, (name, got_res, got_args)
        # pointers travel as void*, integers as int, sizes as size_t
        for decl, ct in zip(args, got_args):
            want = C.c_void_p if "*" in decl else (C.c_size_t if decl.startswith("size_t") else C.c_int)
            assert ct is want, (name, decl, ct)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), "declared in smh.h but not exported: " + name


def test_python_surface_names_the_new_entry_points():
    import inspect

    from sm_hpss_mtl_amd import inference, pipeline
    from sm_hpss_mtl_amd.model import B3MTL, FusionMTL
    assert callable(getattr(FusionMTL, "forward_from_x0_halves", None))
    assert FusionMTL.forward_dense is not B3MTL.forward_dense and list(inspect.signature(FusionMTL.forward_dense).parameters) == \
        list(inspect.signature(B3MTL.forward_dense).parameters)
    assert "forward_from_x0_halves" in inspect.getsource(pipeline.HotPath.step)
    assert "FusionMTL" in (inference.patch_probabilities.__doc__ or "")
