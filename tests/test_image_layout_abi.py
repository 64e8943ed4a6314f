"""CPU: the C ABI and the Python surface of the image patch layout -- the three `*_layout_f32` entries are declared in include/smh.h
with one `int patch_layout` more than the entries they extend (which keep their signatures), bound in _lib.SIGNATURES with the
argument types of their declarations and exported by libsmh.so; `frontend.LAYOUTS` numbers the layouts as
smh_extract_patches_f32 does; the `layout` arguments exist and an unknown layout is a ValueError.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

PAIRS = {"smh_features_layout_f32": "smh_features_ex_f32", "smh_frontend_layout_f32": "smh_frontend_f32",
         "smh_frontend_ragged_layout_f32": "smh_frontend_ragged_f32"}


def _declared_args(hdr, name):
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), code)
    assert len(protos) == 1, (name, protos)
    return [" ".join(a.split()) for a in protos[0].split(",")]


def test_layout_entries_declared_bound_and_exported():
    from sm_hpss_mtl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    for new, old in PAIRS.items():
        a_new, a_old = _declared_args(hdr, new), _declared_args(hdr, old)
        assert "int patch_layout" in a_new and [a for a in a_new if a != "int patch_layout"] == a_old, (new, a_new, a_old)
        assert a_new.index("int patch_layout") == a_new.index("int shift") + 1
        res, args = _lib.SIGNATURES[new]
        res_old, args_old = _lib.SIGNATURES[old]
        assert res is C.c_int is res_old and len(args) == len(a_new) == len(args_old) + 1
        for decl, ct in zip(a_new, args):
            if decl.startswith("const long long *"):
                want = C.POINTER(C.c_longlong)
            elif decl.startswith("const int *"):
                want = C.POINTER(C.c_int)
            elif "*" in decl:
                want = C.c_void_p
            else:
                want = {"size_t": C.c_size_t}.get(decl.split()[0], C.c_int)
            assert ct is want or ct == want, (new, decl, ct)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in list(PAIRS) + list(PAIRS.values()):
        assert hasattr(lib, name), "declared in smh.h but not exported: " + name


def test_python_surface():
    from sm_hpss_mtl_amd import frontend as fe
    # numbered as smh_extract_patches_f32 numbers its layout argument: 0 = (nP, F, W), 1 = (nP, W, F)
    assert fe.LAYOUTS == {"image": 0, "time_major": 1}
    assert fe._patch_shape(5, 68, 240, "image") == (5, 240, 68) and fe._patch_shape(5, 68, 240, "time_major") == (5, 68, 240)
    for bad in ("nhwc", 0, None, "Image"):
        with pytest.raises(ValueError, match="layout"):
            fe._layout(bad)
    for name in ("features", "run", "run_ragged", "patches_from_featuregram"):
        assert inspect.signature(getattr(fe.Frontend, name)).parameters["layout"].default == "time_major", name
    for name in ("features_l0", "plain_features"):  # time-major only
        assert "layout" not in inspect.signature(getattr(fe.Frontend, name)).parameters, name
