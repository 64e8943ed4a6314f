"""CPU: the C ABI of HPSS audio separation -- smh_hpss_resynth_f32, smh_hpss_audio_workspace_bytes and smh_hpss_audio_f32 are each
declared once in include/smh.h, bound in _lib.SIGNATURES with the argument types of their declarations and exported by libsmh.so;
the test query smh_internal_resynth_plan is bound and exported; Frontend has `separate` and `resynth`.  Nothing needs a GPU to
import."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

ENTRIES = {
    "smh_hpss_resynth_f32": ("int", ["ctx", "d_audio", "B", "n_samples", "d_harm", "d_perc", "d_y_harm", "d_y_perc", "stream"]),
    "smh_hpss_audio_workspace_bytes": ("size_t", ["ctx", "B", "n_samples"]),
    "smh_hpss_audio_f32": ("int", ["ctx", "d_audio", "B", "n_samples", "d_y_harm", "d_y_perc", "d_work", "work_bytes", "stream"]),
}
CTYPE = {"const smh_ctx *": C.c_void_p, "const float *": C.c_void_p, "float *": C.c_void_p, "void *": C.c_void_p, "int": C.c_int,
         "size_t": C.c_size_t}


def _declared_args(hdr, name):
    """Arguments of the one prototype of `name` in the header (comments removed)."""
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), code)
    assert len(protos) == 1, (name, protos)
    return [" ".join(a.split()) for a in protos[0].split(",")]


def _type_of(arg):
    m = re.match(r"(.*?)(\w+)$", arg)
    return m.group(1).strip(), m.group(2)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_declared_and_bound(entry):
    from sm_hpss_mtl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    restype, names = ENTRIES[entry]
    args = [_type_of(a) for a in _declared_args(hdr, entry)]
    assert [n for _, n in args] == names, args
    assert re.search(r"\b%s\s+%s\s*\(" % (restype, entry), hdr)
    assert entry in _lib.SIGNATURES
    res, argtypes = _lib.SIGNATURES[entry]
    assert res is CTYPE[restype]
    assert argtypes == [CTYPE[t] for t, _ in args], (argtypes, args)


def test_plan_query_bound():
    from sm_hpss_mtl_amd import _lib
    res, argtypes = _lib.INTERNAL_SIGNATURES["smh_internal_resynth_plan"]
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int)]


def test_entries_exported():
    from sm_hpss_mtl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for entry in list(ENTRIES) + ["smh_internal_resynth_plan"]:
        assert hasattr(lib, entry), "not exported: " + entry


def test_python_surface():
    from sm_hpss_mtl_amd.frontend import Frontend
    assert list(inspect.signature(Frontend.separate).parameters) == ["self", "audio", "out"]
    assert list(inspect.signature(Frontend.resynth).parameters) == ["self", "audio", "harm", "perc", "out"]
    assert inspect.signature(Frontend.separate).parameters["out"].default is None
