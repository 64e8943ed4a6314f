"""CPU: the C ABI and the Python surface of the late-fusion ensemble -- every new symbol is declared in include/smh.h, exported by
libsmh.so and bound in _lib.SIGNATURES with the argument types of its declaration; the host module and the hooks in the existing
modules exist; nothing needs a GPU to import."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

NEW = {  # name -> (arguments, result type)
    "smh_late_fusion_create": (3, C.c_int),
    "smh_late_fusion_destroy": (1, None),
    "smh_late_fusion_w0_ptr": (2, C.c_void_p),
    "smh_late_fusion_workspace_bytes": (2, C.c_size_t),
    "smh_late_fusion_forward_f32": (11, C.c_int),
    "smh_late_fusion_x0_workspace_bytes": (2, C.c_size_t),
    "smh_late_fusion_forward_x0_f32": (10, C.c_int),
    "smh_late_fusion_dense_workspace_bytes": (3, C.c_size_t),
    "smh_late_fusion_forward_dense_f32": (11, C.c_int),
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
        # pointers travel as void* (the handle's out-parameter as a pointer to one), alpha as double, integers as int, sizes as size_t
        for decl, ct in zip(args, got_args):
            if "**" in decl:
                want = C.POINTER(C.c_void_p)
            elif "*" in decl:
                want = C.c_void_p
            else:
                want = {"size_t": C.c_size_t, "double": C.c_double}.get(decl.split()[0], C.c_int)
            assert ct is want or (want is C.POINTER(C.c_void_p) and ct == want), (name, decl, ct)
    for name in ("smh_late_fusion_forward_f32", "smh_late_fusion_forward_x0_f32", "smh_late_fusion_forward_dense_f32"):
        assert sum(a.startswith("double alpha") for a in _declared_args(hdr, name)) == 1
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), "declared in smh.h but not exported: " + name


def test_python_surface():
    from sm_hpss_mtl_amd import frontend, inference, late_fusion, pipeline
    LF = late_fusion.LateFusion
    for name in ("forward_device", "forward_from_x0_halves", "forward_dense", "w0_ptr", "check_status", "predict", "predict_classes",
                 "predict_heads", "split_outputs", "_sync_weights"):
        assert callable(getattr(LF, name, None)), name
    assert isinstance(LF.alpha, property) and LF.alpha.fset is not None
    assert LF.output_names == ["3C"]
    assert list(inspect.signature(LF.__init__).parameters) == ["self", "model_H", "model_P", "alpha"]
    assert inspect.signature(LF.__init__).parameters["alpha"].default == 0.5
    assert list(inspect.signature(LF.forward_device).parameters) == ["self", "x", "out", "labels", "heads"]
    assert list(inspect.signature(LF.forward_dense).parameters)[:4] == ["self", "fv", "shift", "out"]
    assert list(inspect.signature(late_fusion.predict_file).parameters) == ["PARAMS", "ensemble", "file_name_sp", "file_name_mu", "target_dB"]
    assert list(inspect.signature(late_fusion.test_model).parameters) == ["PARAMS", "ensemble", "target_dB"]
    assert "LATE_FUSION" in inspect.getsource(pipeline.HotPath.__init__) and "w0_ptr" in inspect.getsource(pipeline.HotPath.step)
    assert "LATE_FUSION" in inspect.getsource(frontend._l0_kernel)
    assert "LateFusion" in (inference.patch_probabilities.__doc__ or "")


def test_confusion_matrix_counts():
    import numpy as np

    from sm_hpss_mtl_amd.late_fusion import confusion_matrix
    cm = confusion_matrix([0, 1, 1, 2, 2, 2, 0], [0, 1, 2, 2, 2, 0, 0], 3)
    assert cm.tolist() == [[2, 0, 1], [0, 1, 0], [0, 1, 2]] and cm.dtype == np.int64
    assert confusion_matrix([], [], 3).tolist() == [[0] * 3] * 3
