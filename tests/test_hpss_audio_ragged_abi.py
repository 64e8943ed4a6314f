"""CPU: the C ABI of HPSS audio separation for clips of different lengths -- smh_hpss_audio_ragged_sizes and smh_hpss_audio_ragged_f32
are each declared once in include/smh.h, bound in _lib.SIGNATURES with the argument types of their declarations and exported by
libsmh.so; the test query smh_internal_hpss_audio_ragged_route is bound with the other smh_internal_* entries that the header does not
declare, and exported; Frontend has `separate_ragged` and `separate` is as it was.  Nothing needs a GPU to import."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT
from tests.test_hpss_audio_abi import _declared_args, _type_of

ENTRIES = {
    "smh_hpss_audio_ragged_sizes": ("int", ["ctx", "h_offsets", "h_lengths", "B", "h_T", "work_bytes"]),
    "smh_hpss_audio_ragged_f32": ("int", ["ctx", "d_audio", "h_offsets", "h_lengths", "B", "d_y_harm", "d_y_perc", "d_work", "work_bytes",
                                          "stream"]),
}
QUERY = "smh_internal_hpss_audio_ragged_route"
CTYPE = {"const smh_ctx *": C.c_void_p, "const float *": C.c_void_p, "float *": C.c_void_p, "void *": C.c_void_p, "int": C.c_int,
         "size_t": C.c_size_t, "const long long *": C.POINTER(C.c_longlong), "const int *": C.POINTER(C.c_int), "int *": C.POINTER(C.c_int),
         "size_t *": C.POINTER(C.c_size_t)}


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


def test_route_query_bound_and_kept_out_of_the_header():
    from sm_hpss_mtl_amd import _lib
    res, argtypes = _lib.INTERNAL_SIGNATURES[QUERY]
    assert res is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    assert QUERY not in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    assert not re.search(r"\b%s\s*\(" % QUERY, hdr)  # tests/test_host_logic.py holds the header and SIGNATURES equal


def test_entries_exported():
    from sm_hpss_mtl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for entry in list(ENTRIES) + [QUERY]:
        assert hasattr(lib, entry), "not exported: " + entry


def test_python_surface():
    from sm_hpss_mtl_amd.frontend import Frontend
    assert list(inspect.signature(Frontend.separate_ragged).parameters) == ["self", "signals", "out"]
    assert inspect.signature(Frontend.separate_ragged).parameters["out"].default is None
    assert list(inspect.signature(Frontend.separate).parameters) == ["self", "audio", "out"]
