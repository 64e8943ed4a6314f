"""CPU: the C ABI of the fine-tuning feed -- smh_gather_windows_f32 is declared once in include/smh.h, bound in _lib.SIGNATURES
with the argument types of its declaration and exported by libsmh.so; sm_hpss_mtl_amd.dafx has the driver's names.  Nothing
needs a GPU to import."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

ENTRY = "smh_gather_windows_f32"

CTYPE = {"const smh_ctx *": C.c_void_p, "const float *": C.c_void_p, "float *": C.c_void_p, "void *": C.c_void_p,
         "const int *": C.POINTER(C.c_int), "int": C.c_int, "long long": C.c_longlong, "float": C.c_float,
         "unsigned long long": C.c_ulonglong}


def _declared_args(hdr, name):
    """Arguments of the one prototype of `name` in the header (comments removed)."""
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), code)
    assert len(protos) == 1, (name, protos)
    return [" ".join(a.split()) for a in protos[0].split(",")]


def _type_of(arg):
    m = re.match(r"(.*?)(\w+)$", arg)
    return m.group(1).strip(), m.group(2)


def test_entry_declared_and_bound():
    from sm_hpss_mtl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    args = [_type_of(a) for a in _declared_args(hdr, ENTRY)]
    assert [n for _, n in args] == ["ctx", "d_FV", "F", "T", "h_desc", "N", "W", "patch_layout", "noise_scale", "seed", "offset",
                                    "d_out", "stream"], args
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, hdr)
    assert ENTRY in _lib.SIGNATURES
    res, argtypes = _lib.SIGNATURES[ENTRY]
    assert res is C.c_int
    assert argtypes == [CTYPE[t] for t, _ in args], (argtypes, args)


def test_entry_exported():
    from sm_hpss_mtl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    assert hasattr(_lib.load(), ENTRY), "declared in smh.h but not exported: " + ENTRY


def test_python_surface():
    from sm_hpss_mtl_amd import dafx
    want = {"get_annotations": ["folder", "fl", "nFrames", "opDir"],
            "load_data": ["PARAMS", "folder", "file_list"],
            "generator": ["PARAMS", "FV", "labels_mu", "labels_sp", "batchSize"],
            "patch_labels": ["marker", "W", "shift"],
            "getPerformance": ["PtdLabels", "GroundTruths", "labels"],
            "evaluate_file": ["PARAMS", "fl", "Train_Params"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(dafx, name)).parameters) == params, name
    assert inspect.signature(dafx.getPerformance).parameters["labels"].default is None
