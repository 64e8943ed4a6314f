"""CPU: the C ABI of frame-level scaling -- smh_row_moments_f64 and smh_scaled_patches_f32 (and the patch count that sizes the
latter's buffer) are declared once in include/smh.h next to smh_scale_data_f64, bound in _lib.SIGNATURES with the argument types of
their declarations and exported by libsmh.so; Frontend, lib.preprocessing and generators have the Python names.  Nothing needs a GPU
to import."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

CTYPE = {"const smh_ctx *": C.c_void_p, "const float *const *": C.POINTER(C.c_void_p), "const int *": C.POINTER(C.c_int),
         "const double *": C.c_void_p, "double *": C.c_void_p, "int32_t *": C.c_void_p, "float *": C.c_void_p, "void *": C.c_void_p,
         "long long *": C.POINTER(C.c_longlong), "int": C.c_int}

ENTRIES = {
    "smh_row_moments_f64": ("int", C.c_int, ["ctx", "h_fv", "h_T", "B", "rows", "d_moments", "d_nonfinite", "stream"]),
    "smh_scaled_patches_count": ("long long", C.c_longlong, ["h_T", "B", "W", "shift", "h_patch_off"]),
    "smh_scaled_patches_f32": ("int", C.c_int, ["ctx", "h_fv", "h_T", "B", "rows", "d_mean", "d_stdev", "W", "shift", "patch_layout",
                                                "d_patches", "stream"]),
}


def _declared_args(hdr, name):
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
    ret, res_type, names = ENTRIES[entry]
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    args = [_type_of(a) for a in _declared_args(hdr, entry)]
    assert [n for _, n in args] == names, args
    assert re.search(r"\b%s\s+%s\s*\(" % (re.escape(ret), entry), hdr)
    assert hdr.index("smh_scale_data_f64(") < hdr.index(entry + "(") < hdr.index("typedef struct smh_model_cfg")
    res, argtypes = _lib.SIGNATURES[entry]
    assert res is res_type
    assert argtypes == [CTYPE[t] for t, _ in args], (argtypes, args)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_exported(entry):
    from sm_hpss_mtl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    assert hasattr(_lib.load(), entry), "declared in smh.h but not exported: " + entry


def test_patch_count_is_the_integer_contract():
    """smh_scaled_patches_count runs on the host: the running sums of smh_num_patches(smh_tiled_frames(T, W), W, shift)."""
    from sm_hpss_mtl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    Ts = [3, 8, 9, 64, 65, 137, 700]
    for W, shift in ((8, 8), (8, 3), (5, 2), (68, 68), (99, 34)):
        off = (C.c_longlong * (len(Ts) + 1))()
        total = lib.smh_scaled_patches_count((C.c_int * len(Ts))(*Ts), len(Ts), W, shift, off)
        want = [lib.smh_num_patches(lib.smh_tiled_frames(T, W), W, shift) for T in Ts]
        assert total == sum(want) and (want[1] == 0) == (W == 8)  # T = W = 8: range(4, 4, shift) is empty
        assert [off[i + 1] - off[i] for i in range(len(Ts))] == want and off[0] == 0
    assert lib.smh_scaled_patches_count((C.c_int * 1)(0), 1, 8, 8, None) < 0
    assert lib.smh_scaled_patches_count((C.c_int * 1)(5), 1, 0, 8, None) < 0


def test_python_surface():
    from sm_hpss_mtl_amd import generators as gen
    from sm_hpss_mtl_amd.frontend import Frontend
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    assert list(inspect.signature(Frontend.row_moments).parameters) == ["self", "fvs"]
    p = inspect.signature(Frontend.scaled_patches).parameters
    assert list(p) == ["self", "fvs", "mean", "stdev", "W", "shift", "layout"] and p["layout"].default == "time_major"
    assert list(inspect.signature(pp.get_data_stats).parameters)[:2] == ["PARAMS", "files"]
    assert list(inspect.signature(pp.scale_data).parameters) == ["FV", "mean", "stdev"]
    assert list(inspect.signature(gen.data_stats_for_fold).parameters)[0] == "PARAMS"
    import lib.preprocessing as top
    assert top.get_data_stats is pp.get_data_stats and top.scale_data is pp.scale_data
