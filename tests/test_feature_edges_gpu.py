"""The LDS-image feature kernels (csrc/smh_feat.hip: features_half_kernel, features_clip_kernel) and the two-kernel path beside them
(hp_feat_walk_kernel + std_patch_kernel) at signal edges and short lengths, compared value by value.

Direct part: the crafted (S, harm, perc) of tests/feature_cases.py go through `smh_features_layout_f32` / `smh_features_l0_f32`, and
every output is held against a reference of its own:
  * the featuregram against `feature_cases.reference_from_parts` (the functions of oracle/frontend.py behind the medians) at the
    project's bounds (SURVEY 8d'): dB features abs 1e-3 dB on every bin; HarmPercSpec abs 1e-6 max|S|; MelHarmPercSpec rel 1e-5 +
    abs 1e-6 max|S|.  In dB each half's maximum within 1e-3 and its minimum >= its maximum - 80 - 1e-3;
  * the time-major patches against `oracle.frontend.feature_patches` of the device's own featuregram, abs 1e-4; the image patches
    `torch.equal` to their transpose;
  * the layer-0 partials x0p against the float64 product of the device's own patches with the layer-0 kernel, within `_x0p_bound`.
Which kernel a call reaches follows from its arguments, and every test's docstring says how: harm_layout 2 takes the LDS-image
kernels, an even T features_half_kernel, an odd T -- or any T under SMH_FEAT_NOPAIR -- features_clip_kernel; harm_layout 0 takes
hp_feat_walk_kernel + std_patch_kernel.

From audio: `Frontend.run` / `Frontend.run_ragged` on routes 0 and 1 (asserted with `smh_internal_frontend_route`), which reach
the equal-length and the RAG instantiations, on the signal edges tests/test_streaming_frontend_gpu.py holds route 2 to.

The bank sweep at the end asks every Slaney bank's context for its bin-walk plan (`smh_internal_feat_plan`).

Every direct test prints `edge:` lines, the largest error of each (context, case) next to its bound.

A finding these cases made: where own^2 underflows, `mixed` leaves linear mel rows of f32 denormals whose standard deviation is below
1 / FLT_MAX; the scaler's f32 reciprocal scale was inf there and the patches inf / NaN (first seen at T = 2, MelHarmPercSpec, on
features_half_kernel).  `centre_denormal_row` in smh_feat.hip is the fix; the patch check against the oracle holds it.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import feature_cases as FC
from tests.frontend_helpers import _dev, _host, _music, _n_samples, _quiet, _route, _run_both, _t_star, _tone

pytestmark = pytest.mark.gpu

W, SHIFT = FC.W, FC.SHIFT
U = 2.0 ** -24
CONTEXTS = {
    "default": dict(),                               # LogMelHarmPercSpec, 120 rows per half: layer0_mtile
    "MelHarmPercSpec": dict(log_db=False),           # linear, 120 rows
    "LogHarmPercSpec": dict(n_mels=0),               # 201 rows: no layer 0
    "HarmPercSpec": dict(n_mels=0, log_db=False),
    "mel40": dict(n_mels=40),                        # 40 rows per half: the generic layer0
}
_FE, _REF, _W0 = {}, {}, {}


def _skip_if_forced(*names):
    """Which kernel takes a call is what these tests are about: they have nothing to say when a switch forces another one."""
    forced = [n for n in names if os.environ.get(n)]
    if forced:
        pytest.skip("implementation forced by " + ", ".join(forced))


def _frontend(name):
    if name not in _FE:
        from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
        _FE[name] = Frontend(FrontendConfig(**CONTEXTS[name]))
    return _FE[name]


def _reference(name, case, T):
    """[(2 * rows, T) per clip], computed once per (context, case, T) and left unchanged."""
    key = (name, case, T)
    if key not in _REF:
        fe = _frontend(name)
        S, harm, perc = FC.build(case, fe.K, T)
        _REF[key] = [FC.reference_from_parts(S[b], harm[b], perc[b], fe.cfg.n_mels, fe.cfg.log_db) for b in range(S.shape[0])]
        for r in _REF[key]:
            assert np.isfinite(r).all()
            r.setflags(write=False)
    return _REF[key]


def _w0(rows):
    """A layer-0 kernel (2 * rows, 32): Gaussian, a tenth of the rows zero, one column of one sign."""
    if rows not in _W0:
        rng = np.random.default_rng(rows)
        w = (0.2 * rng.standard_normal((2 * rows, 32))).astype(np.float32)
        w[::10] = 0.0
        w[:, 7] = np.abs(w[:, 7])
        _W0[rows] = w
    return _W0[rows]


def _launch(fe, case, T, harm_layout, patch_layout, with_l0):
    """One call of smh_features_layout_f32 / smh_features_l0_f32 on the case's clips; outputs start as NaN.  Returns
    (fv (B, 2 rows, T), patches, x0p or None) on the host."""
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import _ptr, _stream
    lib, h, R2 = fe.lib, fe._h, 2 * fe.rows
    S, harm, perc = FC.build(case, fe.K, T)
    B = S.shape[0]
    nP = lib.smh_num_patches(lib.smh_tiled_frames(T, W), W, SHIFT)
    assert nP >= 1
    hb = FC.blocked(harm) if harm_layout == 2 else harm
    assert harm_layout != 2 or hb[0].size == lib.smh_harm_buffer_floats(fe.K, T)
    dS, dH, dP = _dev(S), _dev(hb), _dev(perc)
    keys = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
    nan = float("nan")
    fv = torch.full((B, R2, T), nan, device="cuda")
    shape = (B * nP, R2, W) if patch_layout == 0 else (B * nP, W, R2)
    patches = torch.full(shape, nan, device="cuda")
    x0p = None
    if with_l0:
        assert patch_layout == 1
        x0p = torch.full((B * nP, 2, W, 32), nan, device="cuda")
        w0 = _dev(_w0(fe.rows))
        rc = lib.smh_features_l0_f32(h, _ptr(dS), _ptr(dH), _ptr(dP), harm_layout, B, T, W, SHIFT, _ptr(fv), _ptr(patches), _ptr(w0),
                                     _ptr(x0p), _ptr(keys), _stream())
    else:
        rc = lib.smh_features_layout_f32(h, _ptr(dS), _ptr(dH), _ptr(dP), harm_layout, B, T, W, SHIFT, patch_layout, _ptr(fv),
                                         _ptr(patches), _ptr(keys), _stream())
    assert rc == nP, (case, T, harm_layout, patch_layout, with_l0, rc, _lib.last_error() if rc < 0 else "")
    torch.cuda.synchronize()
    return _host(fv), _host(patches).reshape((B, nP) + shape[1:]), None if x0p is None else _host(x0p).reshape(B, nP, 2, W, 32)


def _check_fv(fe, fv, ref, smax, tag):
    """One clip's featuregram at the stated bounds; returns (largest error, its bound)."""
    cfg, rows = fe.cfg, fe.rows
    assert fv.shape == ref.shape and np.isfinite(fv).all(), tag
    diff = np.abs(fv.astype(np.float64) - ref.astype(np.float64))
    err = float(diff.max())
    where = tuple(int(i) for i in np.unravel_index(np.argmax(diff), diff.shape))
    print("  fv %s: max err %.3g at %s" % (tag, err, where))
    if cfg.log_db:
        assert err <= 1e-3, (tag, err, where, float(fv[where]), float(ref[where]))
        for g, r in ((fv[:rows], ref[:rows]), (fv[rows:], ref[rows:])):
            assert abs(float(g.max()) - float(r.max())) <= 1e-3, (tag, float(g.max()), float(r.max()))
            assert float(g.min()) >= float(g.max()) - 80.0 - 1e-3, (tag, float(g.min()), float(g.max()))
        return err, 1e-3
    if not cfg.n_mels:
        assert err <= 1e-6 * smax, (tag, err, smax, where)
        return err, 1e-6 * smax
    np.testing.assert_allclose(fv, ref, rtol=1e-5, atol=1e-6 * smax, err_msg=str(tag))
    slack = float((diff - 1e-5 * np.abs(ref)).max())  # what the absolute term has to cover
    return max(slack, 0.0), 1e-6 * smax


def _row_scaler(fv):
    """(largest |value|, 1 / scale) per row of one clip's featuregram, as oracle.frontend.standardize_rows scales it."""
    x = fv.astype(np.float64)
    n = x.shape[1]
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.where(constant | (var == 0.0), 1.0, np.sqrt(var))
    return np.abs(x).max(axis=1), 1.0 / scale


def _x0p_bound(fv, patches, w0, rows):
    """x0p[p][half][j][c] is the f32 sum over this half's rows r of b_r w_rc, b_r the kernel's own standardised value, against
    ref = sum_r p_r w_rc in float64, p_r the stored patch value.  With u = 2^-24:

      |x0p - ref| <= (rows + 6) u sum_r |p_r w_rc|  +  2^-47 sum_r M_r inv_r |w_rc|,      M_r = max |row r|, inv_r = 1 / scale_r.

    The sum: `rows` products accumulated in f32, in whatever order (k steps of four rows, two chains added at the end): the
    classical bound is gamma_n sum |b w| with n = rows, (rows) u to first order.
    The terms: with d = x - (hi + lo) exactly, the patch writer stores p = fl(fl(d) inv) -- (float)((double)x - (hi + lo)) rounds d
    once, up to an f64 rounding of hi + lo and of the difference, each <= 2^-53 (|x| + |hi|) -- and the layer-0 loop forms
    b = fl(fl(fl(x - hi) - lo) inv): fl(x - hi) = (x - hi)(1 + e1), then minus lo and (1 + e2), so
    fl(fl(x - hi) - lo) = d (1 + e2) + (x - hi) e1 (1 + e2) with |x - hi| <= |d| + |lo|, |lo| <= u |hi| / 2.  Hence
      |fl(fl(x - hi) - lo) - fl(d)| <= 3 u |d| + (u^2 + 2^-51) M  <  3 u |d| + 2^-47 M,
    and after the multiplication by inv (one more rounding on either side) |b - p| <= 5 u |p| + 2^-47 M inv.  The 5 joins the
    `rows` of the sum; the sixth unit covers the second-order terms ((rows + 5) u < 2^-16 here).  (std_patch_kernel<true> forms
    b the patch writer's way: its error is inside this bound.)
    fv (2 rows, T) is the device's featuregram of the clip, patches (nP, W, 2 rows), w0 (2 rows, 32).  Returns (nP, 2, W, 32)."""
    M, inv = _row_scaler(fv)
    p = np.abs(patches.astype(np.float64))
    w = np.abs(w0.astype(np.float64))
    out = np.empty(patches.shape[:1] + (2, patches.shape[1], 32))
    for half in range(2):
        sl = slice(half * rows, (half + 1) * rows)
        out[:, half] = (rows + 6) * U * (p[:, :, sl] @ w[sl]) + 2.0 ** -47 * ((M[sl] * inv[sl]) @ w[sl])
    return out


def _x0p_reference(patches, w0, rows):
    p, w = patches.astype(np.float64), w0.astype(np.float64)
    return np.stack([p[:, :, half * rows:(half + 1) * rows] @ w[half * rows:(half + 1) * rows] for half in range(2)], axis=1)


def _lengths(fe, parity=None):
    """The lengths of the case table for this context, with and without layer 0 (T_last differs: the weights share the LDS)."""
    Ts = sorted(set(FC.lengths(fe.rows, False)) | set(FC.lengths(fe.rows, True)))
    return [T for T in Ts if parity is None or T % 2 == parity]


def _patch_condition_bound(fa, fb, p):
    """How far two kernels' standardised values may lie apart given how far their featuregrams do.  With d_r = max_t |fa - fb| on row r,
    the row means differ by <= d_r and the deviations by <= d_r (the standard deviation is 1-Lipschitz in the sup norm), so
    (x - mean) / scale moves by <= (2 d_r + |p| d_r) / scale: the bound is 1e-4 + 3 d_r (1 + |p|) / min(scale_a, scale_b) per value.
    d_r = 0 leaves the 1e-4 both hold against the oracle.  fa, fb (2 rows, T); p (nP, W, 2 rows), the larger |patch value|."""
    d = np.abs(fa.astype(np.float64) - fb.astype(np.float64)).max(axis=1)
    inv = np.maximum(_row_scaler(fa)[1], _row_scaler(fb)[1])
    return 1e-4 + 3.0 * (d * inv)[None, None, :] * (1.0 + p.astype(np.float64))


def _variants(fe, T):
    """(patch layout, with layer 0) of one length: both layouts, and layer 0 where the context and the budget have it."""
    v = [(1, False), (0, False)]
    tl0 = FC.t_last(fe.rows, True)
    if tl0 is not None and T <= tl0:
        v.append((1, True))
    return v


class _Worst:
    """The largest error per (case, figure) next to its bound, printed as `edge:` lines."""

    def __init__(self, ctx, route):
        self.ctx, self.route, self.rows = ctx, route, {}

    def add(self, case, figure, err, bound):
        key = (case, figure)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if key not in self.rows or ratio >= self.rows[key][2]:
            self.rows[key] = (err, bound, ratio)

    def report(self):
        for (case, figure), (err, bound, ratio) in sorted(self.rows.items()):
            print("edge: %-16s %-14s %-11s %-8s err %.3e  bound %.3e  (%.3f of it)" % (self.ctx, case, self.route, figure, err, bound, ratio))


def _run_case(fe, name, case, T, harm_layout, worst, keep=None, check=True):
    """Every variant of one (case, T) on the kernels the current arguments and switches select; all the value checks.
    keep: a dict that receives {(b, variant): (fv, patches, x0p)} for a comparison between kernels; check=False: only that."""
    S = FC.build(case, fe.K, T)[0]
    refs = _reference(name, case, T)
    name_f = FC.feat_name(fe.cfg.n_mels, fe.cfg.log_db)
    tm = None
    for patch_layout, with_l0 in _variants(fe, T):
        fv, patches, x0p = _launch(fe, case, T, harm_layout, patch_layout, with_l0)
        if not check:
            for b in range(S.shape[0]):
                keep[(b, patch_layout, with_l0)] = (fv[b], patches[b], x0p[b] if with_l0 else None)
            continue
        for b in range(S.shape[0]):
            tag = (name, case, "T=%d" % T, "clip %d" % b, "layout %d" % patch_layout, "l0" if with_l0 else "")
            err, bound = _check_fv(fe, fv[b], refs[b], float(S[b].max()), tag)
            worst.add(case, "fv", err, bound)
            assert np.isfinite(patches[b]).all(), tag
            if patch_layout == 1:
                pref = ofe.tcn_input(ofe.feature_patches(fv[b], W, SHIFT, name_f))
                assert pref.shape == patches[b].shape, (tag, pref.shape, patches[b].shape)
                perr = float(np.max(np.abs(patches[b] - pref)))
                worst.add(case, "patches", perr, 1e-4)
                assert perr <= 1e-4, (tag, perr)
            if case == "all_zero":
                if fe.cfg.log_db:
                    assert np.all(np.abs(fv[b] + 100.0) <= 1e-3), tag
                else:
                    assert np.all(fv[b] == 0.0), tag
            if case in ("all_zero", "flat"):
                assert np.all(patches[b] == 0.0), tag
            if with_l0:
                w0 = _w0(fe.rows)
                xref, xb = _x0p_reference(patches[b], w0, fe.rows), _x0p_bound(fv[b], patches[b], w0, fe.rows)
                xerr = np.abs(x0p[b].astype(np.float64) - xref)
                assert np.isfinite(x0p[b]).all(), tag
                i = np.unravel_index(np.argmax(xerr - xb), xerr.shape)
                worst.add(case, "x0p", float(xerr[i]), float(xb[i]))
                assert np.all(xerr <= xb), (tag, float(xerr[i]), float(xb[i]), i)
                if case == "all_zero":
                    assert np.all(x0p[b] == 0.0), tag
            if keep is not None:
                keep[(b, patch_layout, with_l0)] = (fv[b], patches[b], x0p[b] if with_l0 else None)
        if patch_layout == 1 and not with_l0:
            tm = (fv, patches)
        elif patch_layout == 0:  # the same values at other addresses
            assert tm is not None
            assert torch.equal(torch.from_numpy(fv), torch.from_numpy(tm[0])), (name, case, T)
            assert torch.equal(torch.from_numpy(patches).transpose(2, 3), torch.from_numpy(tm[1])), (name, case, T)
        else:  # layer 0 adds outputs, it does not change the others
            assert tm is not None and np.array_equal(fv, tm[0]) and np.array_equal(patches, tm[1]), (name, case, T)


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_half_kernel_even_T(name):
    """features_half_kernel<2, false, false, false, IMAGE>: harm_layout 2, T even, no switch set.  T = 2 is one pair, 16 and 34 end
    a harm block with a full pair and with two frames, T_last - 1 fills the image.  `mixed` takes the wave-uniform fallback to
    the normalised mask in waves that hold normal lanes too; with layer 0 the default and the linear mel context run layer0_mtile
    (120 rows), mel40 the generic layer0."""
    _skip_if_forced("SMH_FEAT_TWO_KERNELS", "SMH_FEAT_TAPS", "SMH_FEAT_NOPAIR")
    fe = _frontend(name)
    Ts = _lengths(fe, 0)
    assert FC.t_last(fe.rows, False) - 1 in Ts and 2 in Ts
    worst = _Worst(name, "half")
    for T in Ts:
        assert fe.lib.smh_features_blocked_ok(fe._h, T, 0), T
        for case in FC.CASES:
            _run_case(fe, name, case, T, 2, worst)
    worst.report()


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_clip_kernel_odd_T(name):
    """features_clip_kernel<false, IMAGE>: harm_layout 2, T odd (its scalar store branch).  T = 1 is one lane, 15 and 17 sit on either
    side of a harm block, 33 ends in a block of one frame, T_last is the last length the image fits -- and the first the predicate
    refuses comes right after it."""
    _skip_if_forced("SMH_FEAT_TWO_KERNELS", "SMH_FEAT_TAPS")
    fe = _frontend(name)
    for with_l0 in (False, True):  # the budget restated for the case table is the library's
        ok = [T for T in range(1, 600) if fe.lib.smh_features_blocked_ok(fe._h, T, int(with_l0))]
        assert (ok[-1] if ok else None) == FC.t_last(fe.rows, with_l0), (name, with_l0, ok[-1:])
    Ts = _lengths(fe, 1)
    assert FC.t_last(fe.rows, False) in Ts and 1 in Ts
    worst = _Worst(name, "clip")
    for T in Ts:
        for case in FC.CASES:
            _run_case(fe, name, case, T, 2, worst)
    worst.report()


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_clip_kernel_even_T_under_nopair_against_the_half_kernel(name, monkeypatch):
    """features_clip_kernel's even-T store branch (float2 rows), reached only with SMH_FEAT_NOPAIR set: harm_layout 2, T even.  The
    same inputs went through features_half_kernel first (the switch unset); the two kernels agree within the 1e-4 dB
    tests/test_parity_gpu.py allows between feature paths and their patches within 1e-4 (layer-0 partials: 1e-4 sum |w|).
    Linear features have no dB figure: the featuregrams agree at the bounds each holds against the reference, and the patches
    within what that difference explains (`_patch_condition_bound`) -- where own^2 underflows the two mask forms quantise a
    denormal differently, and a row of such values standardises to anything."""
    _skip_if_forced("SMH_FEAT_TWO_KERNELS", "SMH_FEAT_TAPS", "SMH_FEAT_NOPAIR")
    fe = _frontend(name)
    Ts = _lengths(fe, 0)
    worst = _Worst(name, "clip_even")
    for T in Ts:
        for case in FC.CASES:
            half, clip = {}, {}
            monkeypatch.delenv("SMH_FEAT_NOPAIR", raising=False)
            _run_case(fe, name, case, T, 2, None, keep=half, check=False)
            monkeypatch.setenv("SMH_FEAT_NOPAIR", "1")
            _run_case(fe, name, case, T, 2, worst, keep=clip)
            monkeypatch.delenv("SMH_FEAT_NOPAIR")
            smax = float(FC.build(case, fe.K, T)[0].max())
            for key in half:
                (fh, ph, xh), (fc, pc, xc) = half[key], clip[key]
                tag = (name, case, T, key)
                if fe.cfg.log_db:
                    d = float(np.max(np.abs(fh - fc)))
                    worst.add(case, "half-clip", d, 1e-4)
                    assert d <= 1e-4, (tag, d)
                elif not fe.cfg.n_mels:
                    assert float(np.max(np.abs(fh - fc))) <= 1e-6 * smax, tag
                else:
                    np.testing.assert_allclose(fh, fc, rtol=1e-5, atol=1e-6 * smax, err_msg=str(tag))
                if key[1] == 0:  # image patches: compared time-major
                    ph, pc = ph.transpose(0, 2, 1), pc.transpose(0, 2, 1)
                pd = np.abs(ph.astype(np.float64) - pc)
                if fe.cfg.log_db:
                    worst.add(case, "half-clip p", float(pd.max()), 1e-4)
                    assert float(pd.max()) <= 1e-4, (tag, float(pd.max()))
                    if xh is not None:  # sums of those patch values: |w| times their bound
                        xb = 1e-4 * np.abs(_w0(fe.rows).astype(np.float64)).reshape(2, fe.rows, 32).sum(axis=1)
                        assert np.all(np.abs(xh.astype(np.float64) - xc) <= xb[None, :, None, :]), tag
                else:
                    pb = _patch_condition_bound(fh, fc, np.maximum(np.abs(ph), np.abs(pc)))
                    assert np.all(pd <= pb), (tag, float((pd - pb).max()))
                    worst.add(case, "loose p", float(np.mean(pb > 2e-4)), 1.0)  # the share of values the bound says little about
    worst.report()


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_two_kernel_path(name):
    """hp_feat_walk_kernel + std_patch_kernel<L0, IMAGE>: harm_layout 0 (bin-major harm, no LDS copy), every length of either parity;
    with layer 0 std_patch_kernel<true>, with image patches std_patch_kernel<false, true>.  The same cases, the same bounds: the
    top-dB floor arrives through the atomicMax keys here."""
    _skip_if_forced("SMH_FEAT_TAPS")
    fe = _frontend(name)
    worst = _Worst(name, "two_kernel")
    for T in _lengths(fe):
        for case in FC.CASES:
            _run_case(fe, name, case, T, 0, worst)
    worst.report()


# ---------------------------------------------------------------------------------------------------------------------------
# from audio: routes 0 and 1 of Frontend.run and Frontend.run_ragged
# ---------------------------------------------------------------------------------------------------------------------------
GEOM = ((68, 34),)


def _last_frame_burst(cfg, T, odd, seed):
    """Near-silence with a two-tone burst in the samples that belong to frame T - 1 only."""
    n = _n_samples(cfg, T, odd)
    y = _quiet(n, seed)
    s0, s1 = cfg.hop * (T - 1) + (cfg.n_fft - cfg.hop), cfg.hop * (T - 1) + cfg.n_fft
    y[s0:s1] += _tone(s1 - s0, 1000.0, 0.5) + _tone(s1 - s0, 3100.0, 0.3)
    return y


def _tiny_bursts(cfg, T, odd):
    """Digital silence with 1e-19 tone bursts of 800 samples every 3100, each at the centre of an FFT bin of its own (see
    tests/test_streaming_frontend_gpu.py: three non-zero bins per frame inside a burst, everything else exactly 0; the frames that
    straddle a burst's edge are non-zero on every bin, so bursts keep the harmonic window's 21 frames apart)."""
    n = _n_samples(cfg, T, odd)
    y = np.zeros(n, np.float32)
    t = np.arange(800) / 16000.0
    for j, start in enumerate(range(300, n - 900, 3100)):
        k = 5 + 9 * j
        y[start:start + 800] = (1e-19 * np.sin(2 * np.pi * 40.0 * k * t)).astype(np.float32)
    return y


def _both_layouts(fe, clips):
    """The image patches of run and run_ragged are the time-major ones transposed, bit for bit."""
    Wg, sg = GEOM[0]
    rag_t, rag_i = fe.run_ragged(clips, W=Wg, shift=sg), fe.run_ragged(clips, W=Wg, shift=sg, layout="image")
    for i, c in enumerate(clips):
        one_t, one_i = fe.run(_dev(c)[None], W=Wg, shift=sg), fe.run(_dev(c)[None], W=Wg, shift=sg, layout="image")
        torch.cuda.synchronize()
        assert torch.equal(one_i["fv"], one_t["fv"]) and torch.equal(one_i["patches"].transpose(1, 2), one_t["patches"]), i
        assert torch.equal(rag_i["fv"][i], one_t["fv"][0]) and torch.equal(rag_i["patches"][i], one_i["patches"]), i
        assert torch.equal(rag_t["patches"][i], one_t["patches"]), i


def test_signal_edges_from_audio_on_the_lds_image_routes():
    """Default context, routes 0 and 1 asserted: `run` reaches features_half_kernel<2> / features_clip_kernel<false>, `run_ragged`
    the RAG instantiations (<2, false, false, true, IMAGE> and <true, IMAGE>), both with time-major and with image patches.  One ragged
    call mixes an all-zero clip, near-silence with a burst confined to the last frame (the lone frame of odd T, the .y of the last
    pair of even T) and music, in even and odd lengths from 40 frames to T*; every clip equals its own `run` bit for bit and
    the oracle from the device's S at the stated bounds."""
    _skip_if_forced("SMH_FEAT_TWO_KERNELS", "SMH_FEAT_TAPS", "SMH_FEAT_NOPAIR")
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    cfg = FrontendConfig()
    fe = Frontend(cfg)
    ts = _t_star(fe)
    assert ts >= 99 and ts % 2 == 1
    plan = [("zero", 40), ("zero", 41), ("burst", 98), ("burst", 99), ("burst", ts - 1), ("burst", ts), ("music", 64), ("music", 65),
            ("music", ts - 1), ("music", ts)]
    clips = []
    for i, (kind, T) in enumerate(plan):
        odd = i % 3 == 1
        if kind == "zero":
            clips.append(np.zeros(_n_samples(cfg, T, odd), np.float32))
        elif kind == "burst":
            clips.append(_last_frame_burst(cfg, T, odd, seed=10 + i))
        else:
            clips.append(_music(_n_samples(cfg, T, odd), seed=20 + i))
    S = _run_both(fe, clips, GEOM, [T & 1 for _, T in plan])
    _both_layouts(fe, clips)
    for i, (kind, T) in enumerate(plan):
        r = fe.run(_dev(clips[i])[None], W=GEOM[0][0], shift=GEOM[0][1])
        fv, pt = _host(r["fv"][0]), _host(r["patches"])
        if kind == "zero":  # every row constant at -100 dB: left unscaled, standardised to exactly 0
            assert np.all(np.abs(fv + 100.0) <= 1e-3) and pt.shape[0] > 0 and np.all(pt == 0.0), T
        if kind == "burst":
            # the premise: the P array's maximum lies in the last frame only and the floor decides most bins (a one-frame burst has
            # no harmonic part above amin: the H array is -100 dB throughout)
            ref = ofe.featuregram_from_S(S[i], "LogMelHarmPercSpec")
            h = ref[120:]
            assert h[:, T - 1:].max() > h[:, :T - 1].max() + 10.0, (T, float(h[:, T - 1:].max()), float(h[:, :T - 1].max()))
            assert np.mean(h <= h.max() - 80.0 + 1e-4) > 0.5
            g = fv[120:]
            assert abs(float(g.max()) - float(h.max())) <= 1e-3 and float(g.min()) >= float(g.max()) - 80.0 - 1e-3


@pytest.mark.parametrize("kw", [dict(n_mels=0, log_db=False), dict(log_db=False)], ids=["HarmPercSpec", "MelHarmPercSpec"])
def test_tiny_tone_bursts_take_the_split_zeros_rule_on_the_lds_image_routes(kw):
    """Linear features, routes 0 and 1 asserted (features_half_kernel<2> and its RAG form for even T, features_clip_kernel for odd T):
    digital silence with 1e-19 bursts, where S > 0 at three bins of a frame and both medians are 0 -- librosa's split_zeros gives
    both masks 0.5, and in features_half_kernel that is the fallback branch (den = 0 < 2^-100).  A mask of 0 would show: the
    bound is 1e-6 max|S| (rel 1e-5 with mel) and the values are max|S| / 2.  The premise, on the device's own S: at least 18 such bins
    per clip (two or three frames of three bins in each of at least four bursts).  A music clip rides in the same ragged call."""
    _skip_if_forced("SMH_FEAT_TWO_KERNELS", "SMH_FEAT_TAPS", "SMH_FEAT_NOPAIR")
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    cfg = FrontendConfig(**kw)
    fe = Frontend(cfg)
    ts = _t_star(fe)
    Ts = [ts - 1, ts, 80, 81]
    clips = [_tiny_bursts(cfg, T, odd=i % 2 == 1) for i, T in enumerate(Ts)] + [_music(_n_samples(cfg, 66, False), seed=31)]
    S = _run_both(fe, clips, GEOM, [T & 1 for T in Ts] + [0])
    _both_layouts(fe, clips)
    for i, T in enumerate(Ts):
        harm, perc = ofe.median_time(S[i], cfg.l_harm), ofe.median_freq(S[i], cfg.l_perc)
        split = (S[i] > 0) & (harm < FC.TINY) & (perc < FC.TINY)
        print("T=%d: %d split_zeros bins, max|S| %.3g" % (T, int(split.sum()), float(S[i].max())))
        assert split.sum() >= 18, (T, int(split.sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# which Slaney banks reach the four-accumulator instantiations
# ---------------------------------------------------------------------------------------------------------------------------
def test_no_slaney_bank_reaches_the_four_accumulator_kernels():
    """Context creation only, no launch: smh_internal_feat_plan for n_mels 1 .. 256 x n_fft {400, 512} x mel_sr {16000, 22050} (and the
    mel-less contexts).  pick_half_kernel takes features_half_kernel<4, ...> when feat_pend > 2; every bank here has feat_pend <= 2
    and a walkable plan, so those four instantiations are reached by no test -- and, with Slaney banks, by no user.  If a bank
    ever reports more, this test names it: add that context to CONTEXTS above."""
    from sm_hpss_mtl_amd import _lib
    lib = _lib.require_gpu()
    out = (C.c_int * 4)()
    assert lib.smh_internal_feat_plan(None, out) == _lib.SMH_E_INVALID
    over, unwalkable, seen = [], [], set()
    for n_fft in (400, 512):
        for mel_sr in (16000.0, 22050.0):
            for n_mels in range(0, 257):
                c = _lib.FrontendCfg(n_fft, n_fft, 160, n_mels, 21, 11, 1, mel_sr)
                h = C.c_void_p()
                _lib.check(lib.smh_ctx_create(C.byref(c), C.byref(h)), "smh_ctx_create")
                try:
                    assert lib.smh_internal_feat_plan(h, out) == 0
                    walk_ok, pend, nseg0, nseg1 = out[0], out[1], out[2], out[3]
                finally:
                    lib.smh_ctx_destroy(h)
                assert 1 <= pend <= 4 and 1 <= nseg0 <= 4 and 1 <= nseg1 <= 8, (n_fft, mel_sr, n_mels, list(out))
                seen.add(pend)
                if pend > 2:
                    over.append((n_fft, mel_sr, n_mels, pend))
                if not walk_ok:
                    unwalkable.append((n_fft, mel_sr, n_mels))
    print("feat_pend values seen: %s; banks over two: %s; banks without a walk plan: %s" % (sorted(seen), over[:8], unwalkable[:8]))
    assert not unwalkable, unwalkable[:8]
    assert not over, over[:8]
    assert seen == {1, 2}, seen
