"""The router's predicate and the launcher agree: `smh_features_blocked_ok(ctx, T, with_l0)` says exactly which clips the single-kernel
feature path (`harm_layout = 2` of `smh_features_layout_f32` / `smh_features_l0_f32`) accepts.  Both are written on one budget function
(smh_feat::clip_image_bytes); this test holds them together at the last T that fits and the first that does not, in three contexts:
the default one (120 mels, 240 rows), and the mel-less ones of n_fft 400 and 512 (402 and 514 rows, where layer 0 never qualifies).
No length is written down here: every T comes from the library's own predicate."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B, W, SHIFT = 2, 4, 2
FILL = -7.0
CONTEXTS = {"default": {}, "rows201": {"n_mels": 0}, "rows257": {"n_mels": 0, "n_fft": 512, "win_length": 512}}


def _skip_if_forced(*names):
    """Which path takes a clip is what this test is about: it has nothing to say when a switch forces another one."""
    forced = [n for n in names if os.environ.get(n)]
    if forced:
        pytest.skip("implementation forced by " + ", ".join(forced))


@pytest.fixture(scope="module")
def frontends():
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    return {name: Frontend(FrontendConfig(**kw)) for name, kw in CONTEXTS.items()}


def _lengths(fe, with_l0):
    """1, 2 and the four T around the last one in 1..400 the predicate takes (none is allowed)."""
    ok = [T for T in range(1, 401) if fe.lib.smh_features_blocked_ok(fe._h, T, with_l0)]
    Ts = {1, 2}
    if ok:
        T_last = ok[-1]
        assert T_last < 400, "the budget ends inside the scanned range"
        Ts |= {T for T in range(T_last - 1, T_last + 3) if T >= 1}
    return ok[-1] if ok else None, sorted(Ts)


@pytest.mark.parametrize("with_l0", [0, 1])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_predicate_and_launcher_agree(frontends, name, with_l0):
    _skip_if_forced("SMH_FEAT_TWO_KERNELS", "SMH_FEAT_TAPS")
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import _ptr, _stream
    fe = frontends[name]
    lib, h, K, R2 = fe.lib, fe._h, fe.K, 2 * fe.rows
    torch.manual_seed(0)
    T_last, Ts = _lengths(fe, with_l0)
    print("%s (%d rows), with_l0=%d: T_last = %s, testing T in %s" % (name, R2, with_l0, T_last, Ts))
    if with_l0 and fe.rows > 128:
        assert T_last is None, "layer 0 needs at most 128 rows per half"
    w0 = torch.zeros((R2, 32), device="cuda")
    accepted = 0
    for T in Ts:
        want = lib.smh_features_blocked_ok(h, T, with_l0)
        nP = lib.smh_num_patches(lib.smh_tiled_frames(T, W), W, SHIFT)
        assert nP >= 1
        S = torch.rand((B, K, T), device="cuda") + 0.1
        perc = torch.rand((B, K, T), device="cuda") + 0.1
        harm = torch.rand((B, lib.smh_harm_buffer_floats(K, T)), device="cuda") + 0.1
        keys = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
        for patch_layout in ((1,) if with_l0 else (0, 1)):
            fv = torch.full((B, R2, T), FILL, device="cuda")
            patches = torch.full((B * nP * W * R2,), FILL, device="cuda")
            x0p = torch.full((B * nP, 2, W, 32), FILL, device="cuda")
            if with_l0:
                rc = lib.smh_features_l0_f32(h, _ptr(S), _ptr(harm), _ptr(perc), 2, B, T, W, SHIFT, _ptr(fv), _ptr(patches), _ptr(w0),
                                             _ptr(x0p), _ptr(keys), _stream())
            else:
                rc = lib.smh_features_layout_f32(h, _ptr(S), _ptr(harm), _ptr(perc), 2, B, T, W, SHIFT, patch_layout, _ptr(fv),
                                                 _ptr(patches), _ptr(keys), _stream())
            err = _lib.last_error() if rc < 0 else "ok"
            torch.cuda.synchronize()
            print("  T=%d layout=%d: predicate %d, rc %d (%s)" % (T, patch_layout, want, rc, err))
            if want:
                assert rc == nP, "the predicate takes T=%d, the launcher answered %d (%s)" % (T, rc, err)
                assert bool((fv != FILL).all()) and bool((patches != FILL).all())
                accepted += 1
            else:
                assert rc == _lib.SMH_E_INVALID, "the predicate refuses T=%d, the launcher answered %d" % (T, rc)
                assert "smh_features_blocked_ok" in err
                # nothing was launched
                assert bool((fv == FILL).all()) and bool((patches == FILL).all()) and bool((x0p == FILL).all())
    assert (accepted > 0) == (T_last is not None)
