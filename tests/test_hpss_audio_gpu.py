"""GPU: the HPSS resynthesis kernel (smh_hpss_resynth_f32) on caller-supplied medians against the float64 restatement
(tests/hpss_audio_ref.py), at the lengths where it can go wrong: a single frame, fewer frames than the overlap depth, a tail of zeros,
the tile edges read from smh_internal_resynth_plan, odd lengths and unaligned clips (the scalar store path), every configuration the
kernel claims to serve or refuse.  Every output lies inside a sentinel-filled buffer whose sentinels must survive on both sides, and
every audio buffer ends with NaN directly behind its last sample.

Error measure: d(a, b) = max_n |a[n] - b[n]| * wss[n] / max|x| (the overlap-add numerators; hpss_audio_ref.distance).  Bound, per
case and per component: d(device, f64 restatement) <= 8 * d_ref with d_ref = d(f32 restatement, f64 restatement) on the case's own
inputs -- 8 for a different summation order in two transforms of about 9 stages each.  On samples without window weight
(wss <= FLT_MIN) the device is within 1e-6 * max|x| of the restatement (0 there).

Measured on an MI355X (d_dev / d_ref against the bound 8): the two reference configurations over all cases of this module, 56 (clip,
component) figures: d_dev 3.9e-8 .. 1.4e-7, d_ref 3.5e-8 .. 1.7e-7, ratio 0.59 .. 1.96 (the largest at T = 2); the five other
configurations: d_dev 4.6e-8 .. 1.3e-7, ratio 0.65 .. 1.43; (84, 84, 28), the radix-7 row added later: d_dev 7.2e-8 .. 1.1e-7, d_ref
7.8e-8 .. 1.1e-7, ratio 0.83 .. 1.17; samples without window weight: 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import hpss_audio_ref as ref

pytestmark = pytest.mark.gpu

SENT = 12345.0
GUARD = 64  # sentinel floats on either side of an output (a multiple of 4: the output's first clip keeps the buffer's alignment)
CONFIGS = [(400, 400, 160), (512, 400, 160)]  # the reference's two
# other configurations the kernel serves: radix 8 x 8 x 2 with win_length < n_fft; radices 8, 5, 3; an odd M = 45 (5 x 3 x 3);
# hop = n_fft (no halo); a hop that 16-byte alignment does not divide; M = 42 = 2 × 3 × 7
OTHER = [(256, 200, 64), (240, 240, 80), (90, 90, 30), (64, 64, 64), (400, 400, 150), (84, 84, 28)]
# ... and refuses, with the limit its message names
REFUSED = [((64, 64, 65), "hop=65 > n_fft=64"), ((400, 400, 16), "more than 17 overlapping frames"), ((2048, 2048, 512), "bytes of LDS")]

_FES = {}


def _fe(cfg, precision="f32"):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    key = (cfg, precision)
    if key not in _FES:
        _FES[key] = Frontend(FrontendConfig(n_fft=cfg[0], win_length=cfg[1], hop=cfg[2], stft_precision=precision))
    return _FES[key]


def _plan(fe, N):
    from sm_hpss_mtl_amd import _lib
    out = (C.c_int * 4)()
    _lib.check(fe.lib.smh_internal_resynth_plan(fe._h, N, out), "smh_internal_resynth_plan")
    return list(out)  # frames per workgroup, halo frames, threads, LDS bytes


def _audio_dev(x, front=0):
    """x (B, N) -> a device view (B, N) whose buffer holds NaN directly behind the last sample (`front` floats precede it)."""
    B, N = x.shape
    buf = torch.full((front + B * N + 1,), float("nan"), dtype=torch.float32, device="cuda")
    buf[front:front + B * N] = torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(-1)
    return buf[front:front + B * N].view(B, N)


def _guarded(B, N, front=GUARD):
    buf = torch.full((front + B * N + GUARD,), SENT, dtype=torch.float32, device="cuda")
    return buf, buf[front:front + B * N].view(B, N)


def _sentinels_intact(buf, B, N, front=GUARD):
    h = buf.cpu().numpy()
    return bool((h[:front] == SENT).all() and (h[front + B * N:] == SENT).all())


def run_kernel(fe, x, harm, perc, front=GUARD):
    """x (B, N), harm / perc (B, K, T) numpy -> y_harm, y_perc (B, N) numpy; asserts the sentinels."""
    B, N = x.shape
    bh, yh = _guarded(B, N, front)
    bp, yp = _guarded(B, N, front)
    fe.resynth(_audio_dev(x), torch.from_numpy(harm).cuda(), torch.from_numpy(perc).cuda(), out={"harmonic": yh, "percussive": yp})
    torch.cuda.synchronize()
    assert _sentinels_intact(bh, B, N, front) and _sentinels_intact(bp, B, N, front), "the kernel wrote outside its outputs"
    return yh.cpu().numpy(), yp.cpu().numpy()


def _inputs(cfg, N, B, seed):
    n_fft, wl, hop = cfg
    K, T = 1 + n_fft // 2, 1 + (N - n_fft) // hop
    x = ref.noise_tone(N, seed, B=B)
    hp = [ref.random_medians(K, T, seed * 100 + b) for b in range(B)]
    return x, np.stack([h for h, _ in hp]), np.stack([p for _, p in hp])


def check_against_ref(cfg, x, harm, perc, yh, yp, what):
    n_fft, wl, hop = cfg
    worst = 0.0
    for b in range(x.shape[0]):
        r64 = ref.resynth(x[b], harm[b], perc[b], n_fft, wl, hop, np.float64)
        r32 = ref.resynth(x[b], harm[b], perc[b], n_fft, wl, hop, np.float32)
        xmax = float(np.abs(x[b]).max())
        unc = ref.uncovered(r64["wss"])
        for c, y in (("harmonic", yh[b]), ("percussive", yp[b])):
            assert np.isfinite(y).all(), (what, b, c)
            d_ref = ref.distance(r32[c], r64[c], r64["wss"], xmax)
            d_dev = ref.distance(y, r64[c], r64["wss"], xmax)
            print("%s clip %d %s: d_dev = %.3g, d_ref = %.3g, ratio %.2f" % (what, b, c, d_dev, d_ref, d_dev / d_ref))
            assert d_dev <= 8 * d_ref, (what, b, c, d_dev, d_ref)
            assert np.abs(y[unc] - r64[c][unc]).max() <= 1e-6 * xmax, (what, b, c)
            worst = max(worst, d_dev / d_ref)
    return worst


def _lengths(cfg):
    """case name -> N"""
    n_fft, wl, hop = cfg
    tile, halo, _, _ = _plan(_fe(cfg), n_fft)
    assert halo == -(-n_fft // hop) - 1 and tile >= 1
    cases = {"single frame": n_fft, "T=2": n_fft + hop, "T=3": n_fft + 2 * hop, "tail of zeros": n_fft + 3 * hop + 77}
    for name, T in (("T=tile-1", tile - 1), ("T=tile", tile), ("T=tile+1", tile + 1), ("T=2*tile+1", 2 * tile + 1)):
        cases[name] = n_fft + (T - 1) * hop
    return cases


CASES = ["single frame", "T=2", "T=3", "tail of zeros", "T=tile-1", "T=tile", "T=tile+1", "T=2*tile+1"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_lengths(cfg, case):
    N = _lengths(cfg)[case]
    x, harm, perc = _inputs(cfg, N, 1, seed=CASES.index(case) + 1)
    yh, yp = run_kernel(_fe(cfg), x, harm, perc)
    check_against_ref(cfg, x, harm, perc, yh, yp, "%s %s N=%d" % (cfg, case, N))
    cov = cfg[0] + cfg[2] * ((N - cfg[0]) // cfg[2])
    assert not yh[:, cov:].any() and not yp[:, cov:].any()  # behind the last frame: exactly 0


@pytest.mark.parametrize("front", [GUARD, GUARD + 1])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_odd_length_unaligned_clips(cfg, front):
    """B = 3 with an odd N: clips 1 and 2 start off 16-byte boundaries (with front = GUARD + 1 clip 0 does too): scalar stores."""
    N = cfg[0] + 17 * cfg[2] + 33
    assert N % 2 == 1
    x, harm, perc = _inputs(cfg, N, 3, seed=11)
    yh, yp = run_kernel(_fe(cfg), x, harm, perc, front=front)
    check_against_ref(cfg, x, harm, perc, yh, yp, "%s odd N=%d front=%d" % (cfg, N, front))


@pytest.mark.parametrize("N_extra", [0, 33])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_batch_independence(cfg, N_extra):
    """The middle clip of a B = 3 batch is bit-identical to the same clip at B = 1 (aligned and unaligned); two calls are
    bit-identical."""
    N = cfg[0] + 18 * cfg[2] + N_extra
    x, harm, perc = _inputs(cfg, N, 3, seed=12)
    fe = _fe(cfg)
    yh3, yp3 = run_kernel(fe, x, harm, perc)
    yh1, yp1 = run_kernel(fe, x[1:2], harm[1:2], perc[1:2])
    np.testing.assert_array_equal(yh3[1], yh1[0])
    np.testing.assert_array_equal(yp3[1], yp1[0])
    yh3b, yp3b = run_kernel(fe, x, harm, perc)
    np.testing.assert_array_equal(yh3, yh3b)
    np.testing.assert_array_equal(yp3, yp3b)


@pytest.mark.parametrize("cfg", OTHER)
def test_other_configurations(cfg):
    fe = _fe(cfg)
    tile = _plan(fe, cfg[0])[0]
    N = cfg[0] + (tile + 1) * cfg[2] + 5
    x, harm, perc = _inputs(cfg, N, 2, seed=13)
    yh, yp = run_kernel(fe, x, harm, perc)
    check_against_ref(cfg, x, harm, perc, yh, yp, "%s N=%d" % (cfg, N))


@pytest.mark.parametrize("cfg,text", REFUSED)
def test_refused_configurations(cfg, text):
    fe = _fe(cfg)
    N = 2 * cfg[0] + 3 * cfg[2]
    x, harm, perc = _inputs(cfg, N, 1, seed=14)
    bh, yh = _guarded(1, N)
    bp, yp = _guarded(1, N)
    with pytest.raises(ValueError, match=text):
        fe.resynth(_audio_dev(x), torch.from_numpy(harm).cuda(), torch.from_numpy(perc).cuda(), out={"harmonic": yh, "percussive": yp})
    with pytest.raises(ValueError, match=text):
        fe.separate(_audio_dev(x), out={"harmonic": yh, "percussive": yp})
    with pytest.raises(ValueError, match=text):
        _plan(fe, N)
    torch.cuda.synchronize()
    assert (bh == SENT).all() and (bp == SENT).all()


def test_refusals():
    """Every SMH_REQUIRE of the two entries, each with its message; B = 0 touches nothing."""
    from sm_hpss_mtl_amd import _lib
    cfg = CONFIGS[0]
    fe = _fe(cfg)
    lib, h = fe.lib, fe._h
    N = cfg[0] + 4 * cfg[2]
    x, harm, perc = _inputs(cfg, N, 2, seed=15)
    a = _audio_dev(x)
    hm, pc = torch.from_numpy(harm).cuda(), torch.from_numpy(perc).cuda()
    bh, yh = _guarded(2, N)
    bp, yp = _guarded(2, N)
    need = lib.smh_hpss_audio_workspace_bytes(h, 2, N)
    assert need >= 3 * 4 * 2 * fe.K * fe.num_frames(N)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def refused(rc, code, text):
        assert rc == code, (rc, _lib.last_error())
        assert text in _lib.last_error(), _lib.last_error()

    good = [h, p(a), 2, N, p(hm), p(pc), p(yh), p(yp), None]
    for i in (0, 1, 4, 5, 6, 7):  # null pointers
        args = list(good)
        args[i] = None
        refused(lib.smh_hpss_resynth_f32(*args), _lib.SMH_E_INVALID, "null argument")
    good2 = [h, p(a), 2, N, p(yh), p(yp), p(work), need, None]
    for i in (0, 1, 4, 5):
        args = list(good2)
        args[i] = None
        refused(lib.smh_hpss_audio_f32(*args), _lib.SMH_E_INVALID, "null argument")
    args = list(good2)
    args[6] = None
    refused(lib.smh_hpss_audio_f32(*args), _lib.SMH_E_INVALID, "null workspace")
    for fn, g in ((lib.smh_hpss_resynth_f32, good), (lib.smh_hpss_audio_f32, good2)):
        args = list(g)
        args[2] = -1
        refused(fn(*args), _lib.SMH_E_INVALID, "B=-1 is negative")
        args[2] = 65536
        refused(fn(*args), _lib.SMH_E_INVALID, "exceeds the grid limit of 65535")
        args = list(g)
        args[3] = cfg[0] - 1
        refused(fn(*args), _lib.SMH_E_INVALID, "shorter than n_fft=400")
    # outputs aliasing each other, the input, a median, the workspace
    args = list(good)
    args[7] = C.c_void_p(yh.data_ptr() + 4 * N)
    refused(lib.smh_hpss_resynth_f32(*args), _lib.SMH_E_INVALID, "d_y_harm and d_y_perc overlap")
    args = list(good)
    args[6] = C.c_void_p(a.data_ptr() + 4 * (2 * N - 1))
    refused(lib.smh_hpss_resynth_f32(*args), _lib.SMH_E_INVALID, "an output overlaps an input")
    args = list(good)
    args[7] = p(hm)
    refused(lib.smh_hpss_resynth_f32(*args), _lib.SMH_E_INVALID, "an output overlaps an input")
    args = list(good2)
    args[5] = p(yh)
    refused(lib.smh_hpss_audio_f32(*args), _lib.SMH_E_INVALID, "d_y_harm and d_y_perc overlap")
    args = list(good2)
    args[4] = p(a)
    refused(lib.smh_hpss_audio_f32(*args), _lib.SMH_E_INVALID, "overlaps an input or the workspace")
    args = list(good2)
    args[5] = p(work)
    refused(lib.smh_hpss_audio_f32(*args), _lib.SMH_E_INVALID, "overlaps an input or the workspace")
    args = list(good2)
    args[7] = need - 1
    refused(lib.smh_hpss_audio_f32(*args), _lib.SMH_E_WORKSPACE, "%d needed" % need)
    # B = 0: SMH_OK, nothing touched
    args = list(good)
    args[2] = 0
    assert lib.smh_hpss_resynth_f32(*args) == _lib.SMH_OK
    args = list(good2)
    args[2] = 0
    assert lib.smh_hpss_audio_f32(*args) == _lib.SMH_OK
    assert lib.smh_hpss_audio_workspace_bytes(h, 0, N) == 0
    torch.cuda.synchronize()
    assert (bh == SENT).all() and (bp == SENT).all()
    # and the good arguments work
    assert lib.smh_hpss_resynth_f32(*good) == _lib.SMH_OK
    assert lib.smh_hpss_audio_f32(*good2) == _lib.SMH_OK
    torch.cuda.synchronize()
    assert _sentinels_intact(bh, 2, N) and _sentinels_intact(bp, 2, N)
    assert torch.isfinite(yh).all() and torch.isfinite(yp).all()
