"""CPU: the C ABI and the Python surface of the plain front end's image patch layout -- the three `smh_plain_*_layout_f32` entries
are declared in include/smh.h with one `int patch_layout` directly behind `int shift`, the entries they extend keep their
declarations, the new ones are bound in _lib.SIGNATURES with the argument types of their declarations and exported by libsmh.so;
`Frontend.run / run_ragged / plain_features` take layout="image" on a plain configuration.  Nothing here needs a GPU.
(The pattern of tests/test_image_layout_abi.py, which pins the harmonic-percussive entries.)"""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

PAIRS = {"smh_plain_features_layout_f32": "smh_plain_features_f32", "smh_plain_frontend_layout_f32": "smh_plain_frontend_f32",
         "smh_plain_frontend_ragged_layout_f32": "smh_plain_frontend_ragged_f32"}
# the old entries, as they were declared before the layout entries came
OLD_DECLS = {
    "smh_plain_features_f32": ["const smh_ctx *ctx", "const float *d_S", "int B", "int T", "int W", "int shift", "float *d_fv",
                               "float *d_patches", "int32_t *d_maxkeys", "void *stream"],
    "smh_plain_frontend_f32": ["const smh_ctx *ctx", "const float *d_audio", "int B", "int n_samples", "int W", "int shift",
                               "float *d_fv", "float *d_patches", "void *d_work", "size_t work_bytes", "float *d_S", "void *stream"],
    "smh_plain_frontend_ragged_f32": ["const smh_ctx *ctx", "const float *d_audio", "const long long *h_offsets",
                                      "const int *h_lengths", "int B", "int W", "int shift", "float *d_fv", "float *d_patches",
                                      "void *d_work", "size_t work_bytes", "void *stream"],
}


def _declared_args(hdr, name):
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), code)
    assert len(protos) == 1, (name, protos)
    return [" ".join(a.split()) for a in protos[0].split(",")]


def _ctype_of(decl):
    if decl.startswith("const long long *"):
        return C.POINTER(C.c_longlong)
    if decl.startswith("const int *"):
        return C.POINTER(C.c_int)
    if "*" in decl:
        return C.c_void_p
    return {"size_t": C.c_size_t}.get(decl.split()[0], C.c_int)


def test_plain_layout_entries_declared_bound_and_exported():
    from sm_hpss_mtl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smh.h")).read()
    for new, old in PAIRS.items():
        a_new, a_old = _declared_args(hdr, new), _declared_args(hdr, old)
        assert a_old == OLD_DECLS[old], (old, a_old)
        assert [a for a in a_new if a != "int patch_layout"] == a_old, (new, a_new, a_old)
        assert a_new.count("int patch_layout") == 1 and a_new.index("int patch_layout") == a_new.index("int shift") + 1
        res, args = _lib.SIGNATURES[new]
        res_old, args_old = _lib.SIGNATURES[old]
        assert res is C.c_int is res_old and len(args) == len(a_new) == len(args_old) + 1
        for name, decls, cts in ((new, a_new, args), (old, a_old, args_old)):
            for decl, ct in zip(decls, cts):
                want = _ctype_of(decl)
                assert ct is want or ct == want, (name, decl, ct)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in list(PAIRS) + list(PAIRS.values()):
        assert hasattr(lib, name), "declared in smh.h but not exported: " + name


def test_plain_python_surface():
    from sm_hpss_mtl_amd import frontend as fe
    fams = fe._FAMILIES
    assert fams[False].equal == "smh_plain_frontend_layout_f32" and fams[False].ragged == "smh_plain_frontend_ragged_layout_f32"
    assert fams[True].equal == "smh_frontend_layout_f32" and fams[True].ragged == "smh_frontend_ragged_layout_f32"
    # one geometry for both families: (W, shift, patch_layout), and an unknown layout is a ValueError before anything else
    geometry = fe.Frontend._geometry
    assert geometry(None, 68, 34, "image") == (68, 34, 0) and geometry(None, None, None, "time_major") == (0, 0, 1)
    for bad in ("nhwc", 0, None, "Image"):
        with pytest.raises(ValueError, match="layout"):
            geometry(None, 68, 34, bad)
    # plain_features takes the layout as a keyword option (its named parameters are pinned by tests/test_image_layout_abi.py)
    assert inspect.signature(fe.Frontend.plain_features).parameters["options"].kind is inspect.Parameter.VAR_KEYWORD
    src = inspect.getsource(fe.Frontend.plain_features)
    assert "smh_plain_features_layout_f32" in src and "_patch_shape" in src


def test_device_generator_no_longer_refuses_the_plain_names():
    """`generators._device_patches_for` used to raise for a Conv2D model with a plain feature name; the three single-task baselines'
    configurations (Baseline_Results.py: MelSpec / Spec / LogSpec) now go to the front end with layout="image"."""
    from sm_hpss_mtl_amd import _lib, generators as gen
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmh.so not built (run __graft_entry__.build())")
    for model, feat, n_fft, n_mels in (("Doukhan_et_al", "MelSpec", 400, 21), ("Papakostas_et_al", "Spec", 400, 0),
                                       ("Jang_et_al", "LogSpec", 512, 0)):
        P = {"Model": model, "Tw": 25, "Ts": 10, "feature_opDir": "unused"}
        try:  # no files: with a GPU an empty list, without one the front end's "no HIP device" -- never the old refusal
            assert gen._device_patches_for(P, [], feat, n_fft, n_mels, 68, 34) == []
        except RuntimeError as e:
            assert "no HIP device" in str(e), e
