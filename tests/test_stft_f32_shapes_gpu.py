"""GPU: the f32 STFT (csrc/smh_stft.hip) on every radix, hop, window and alignment route, against oracle.frontend.stft_mag.

The library takes any even n_fft >= 8 whose half factors over {8, 4, 2, 5, 3, 7}, any win_length <= n_fft and any hop >= 1; the
other suites run (400, 400, 160) and (512, 400, 160) only.  Here:

1. the generic kernel (stft_mag_kernel), one geometry per radix chain: radix 2 / 3 / 7 stages, the Winograd radix 5 on a planned
   route, the reciprocal-multiply index arithmetic at nb, Ns and nf that are no powers of two, four stages, hop 1 and odd hops;
   (980, 800, 245) is one of the three sizes up to 1024 (756, 972, 980) at which fdiv's + 0.5f decides an index
   (test_where_the_reciprocal_multiply_needs_its_half);
2. n_fft = 400, every route to either kernel, asserted with the test-only query `smh_internal_stft_route` (1 specialised, 0 generic,
   2 f64), which evaluates the predicate `smh_stft_mag_f32` dispatches on: odd hops, odd lengths with B = 1 and B > 1, a clip off an
   8-byte boundary, SMH_STFT_GENERIC; zero-padded centred windows, even hops from 2 to beyond n_fft, and frame counts at the edges
   of both tile plans (specialised: F = ceil(T / ceil(T / 20)); generic: tt = ceil(T / ceil(T / 16)));
3. what is refused, at context creation and -- for n_fft > 1024 -- by the clip's frame count;
4. the front end behind the STFT at K = 161 and K = 513: mel tables, segment plans, the plain projection's LDS rule.

Every STFT case: clips of n = n_fft + (T - 1) hop + r samples with r in {0, 1, hop - 1} (so that the floor of the frame count
matters), one of them with digital silence over whole frames (exactly 0 out where the oracle gives 0); the audio sits in a buffer
with NaN directly in front of and behind it (in bounds: a read outside a clip turns outputs into NaN, nothing faults); the output
goes through the C ABI into a buffer with one guard clip of a sentinel behind the batch.  Where a case asserts the specialised
route, an odd r runs as a single clip (B = 1) and B = 3 runs the even r in {0, hop - 2}: an odd length with B > 1 is, by the
predicate, a generic-route call (its own case below).

Bound: max |S - ref| <= 1e-5 max(ref) per clip (include/smh.h).  Measured on an MI355X, worst |S - ref| / max(ref) over the clips
of a case:

    generic kernel (route 0), T = 41 (and 1 at n_fft = 8, 16 at n_fft = 1024), radices of n_fft / 2:
      (8, 8, 3)          4          1.77e-7      (140, 100, 35)     2x5x7      1.79e-7
      (16, 11, 4)        8          1.50e-7      (320, 320, 160)    8x4x5      1.74e-7
      (20, 20, 5)        2x5        1.14e-7      (600, 400, 160)    4x5x5x3    1.61e-7
      (84, 80, 37)       2x3x7      2.13e-7      (980, 800, 245)    2x5x7x7    1.79e-7
      (96, 96, 1)        8x2x3      2.27e-7      (1000, 1000, 250)  4x5x5x5    1.95e-7
      (2048, 1600, 400)  8x8x8x2    2.50e-7 (3 frames)   (1024, 1000, 256)  8x8x8  2.02e-7
    n_fft = 400, hop 160, win_length 400 unless named:         specialised (route 1)    generic (route 0)
      T = 41, B = 3, even n / SMH_STFT_GENERIC=1 (8x5x5)       1.71e-7                  2.17e-7
      odd hop 161                                                                       2.11e-7
      odd n_samples: B = 1 / B = 3                             1.55e-7                  2.17e-7
      data_ptr % 8 == 4, B = 1                                                          1.55e-7
      win_length 399 / 320 / 2 / 1                             1.72e-7 / 1.79e-7 / 2.36e-8 / 0
      hop 2 / 80 / 200 / 400 / 402                             2.29e-7 / 2.67e-7 / 1.71e-7 / 1.67e-7 / 1.73e-7
      T = 1 / 19 / 20 / 21                                     1.16e-7 / 1.87e-7 (x3)   2.29e-7 (x4)
      T = 40 / 41 / 61                                         1.71e-7 / 1.71e-7 / 1.70e-7    2.17e-7 / 2.17e-7 / 1.90e-7
      32-frame tiles (SMH_STFT_FRAMES=32,256), T = 30 / 31 / 32 / 63: 1.71e-7 / 1.71e-7 / 1.71e-7 / 1.70e-7
    behind the STFT, worst |fv - ref| in dB: K = 161: 7.6e-6 (no mel), 1.1e-5 (40 mels); K = 513: 1.1e-5, 7.6e-6

Every figure is between 2.4e-8 and 2.7e-7: some 40 times inside the bound, and where an independent f32 FFT lands.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import plain_ref as pr
from tests import stft_plans as sp

pytestmark = pytest.mark.gpu

TOL = 1e-5      # include/smh.h: |S| within 1e-5 of max|S| of the reference's, per clip
SENTINEL = -7.0
LDS_LIMIT = sp.LDS_LIMIT  # the generic kernel's launch refuses more dynamic LDS
_FES, _BASE = {}, {}


def _fe(**kw):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    cfg = FrontendConfig(**kw)
    if cfg not in _FES:
        _FES[cfg] = Frontend(cfg)
    return _FES[cfg]


def _base():
    """Three synth_clips clips, computed once; every case cuts its clips from them."""
    if "y" not in _BASE:
        from sm_hpss_mtl_amd.synth import synth_clips
        _BASE["y"] = synth_clips(3, seed=41, n_samples=18200)
    return _BASE["y"]


def _clips(geom, T, r, B=3):
    """B clips of n_fft + (T - 1) hop + r samples; clip 1 (of three) silent over frames 2..4 (all of it when T < 5)."""
    n_fft, _, hop = geom
    n = n_fft + (T - 1) * hop + r
    assert ofe.num_frames(n, n_fft, hop) == T and (r == 0 or ofe.num_frames(n + hop - r, n_fft, hop) == T + 1)
    y = _base()[:B, :n].copy()
    if B == 3:
        if T >= 5:
            y[1, 2 * hop:2 * hop + n_fft + 2 * hop] = 0.0
        else:
            y[1] = 0.0
    return y


def _place(y, front):
    """y on the device with NaN in the `front` floats before it and in the 64 behind it (both inside the allocation).  The allocation
    starts on a 512-byte boundary: an even `front` keeps the clip on an 8-byte boundary, an odd one puts it 4 bytes off."""
    y = np.ascontiguousarray(y, np.float32)
    buf = torch.full((front + y.size + 64,), float("nan"), dtype=torch.float32, device="cuda")
    buf[front:front + y.size] = torch.from_numpy(y.ravel()).cuda()
    x = buf[front:front + y.size].view(y.shape)
    assert x.data_ptr() % 8 == (4 * front) % 8 and x.is_contiguous()
    return x


def _route(fe, x, B, n):
    f = fe.lib.smh_internal_stft_route  # test-only export, not in include/smh.h
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return f(fe._h, C.c_void_p(x.data_ptr()), B, n)


def _stft(fe, y, front=1022):
    """smh_stft_mag_f32 on y (B, n) -> (S on the host, route).  Asserts the shape, the dtype, finiteness, the guard clip, and that
    Frontend.stft_mag gives the same bits."""
    from sm_hpss_mtl_amd import _lib
    B, n = y.shape
    cfg = fe.cfg
    T, K = ofe.num_frames(n, cfg.n_fft, cfg.hop), 1 + cfg.n_fft // 2
    x = _place(y, front)
    buf = torch.full((B + 1, K, T), SENTINEL, dtype=torch.float32, device="cuda")  # one guard clip behind the batch
    route = _route(fe, x, B, n)
    _lib.check(fe.lib.smh_stft_mag_f32(fe._h, C.c_void_p(x.data_ptr()), B, n, C.c_void_p(buf.data_ptr()), _lib.current_stream()),
               "smh_stft_mag_f32")
    S2 = fe.stft_mag(x)
    torch.cuda.synchronize()
    assert bool((buf[B] == SENTINEL).all()), "the guard clip behind the batch was written"
    assert S2.shape == (B, K, T) and S2.dtype == torch.float32 and torch.equal(S2, buf[:B])
    S = buf[:B].cpu().numpy()
    assert S.shape == (B, K, T) and S.dtype == np.float32 and np.isfinite(S).all(), "NaN: a read outside a clip"
    return S, route


def _worst(S, y, geom, tag):
    """Asserts the bound per clip; returns the worst |S - ref| / max(ref)."""
    n_fft, wl, hop = geom
    worst = 0.0
    for i in range(len(y)):
        ref = ofe.stft_mag(y[i], n_fft=n_fft, win_length=wl, hop=hop)
        assert S[i].shape == ref.shape
        m = float(ref.max())
        err = float(np.max(np.abs(S[i].astype(np.float64) - ref.astype(np.float64))))
        ratio = err / m if m > 0 else (0.0 if err == 0 else np.inf)
        assert err <= TOL * m, (tag, i, ratio)
        assert (S[i][ref == 0] == 0).all(), (tag, i, "nonzero where the oracle gives 0")
        worst = max(worst, ratio)
    return worst


def _silence_covers_frames(y, geom, T):
    n_fft, wl, hop = geom
    ref = ofe.stft_mag(y[1], n_fft=n_fft, win_length=wl, hop=hop)
    assert (ref[:, 2:5] == 0).all() if T >= 5 else (ref == 0).all()


def _rs(hop):
    return sorted({0, min(1, hop - 1), hop - 1})


def _run_generic(fe, geom, T, tag):
    """B = 3 at every r; the route must be the generic kernel's."""
    worst = 0.0
    for r in _rs(geom[2]):
        y = _clips(geom, T, r)
        if r == 0:
            _silence_covers_frames(y, geom, T)
        S, route = _stft(fe, y)
        assert route == 0, (tag, T, r, route)
        worst = max(worst, _worst(S, y, geom, (tag, T, r)))
    return worst


def _run_specialised(fe, geom, T, tag):
    """The specialised route: B = 3 at the even r in {0, hop - 2}, B = 1 (clip 0, then the silent clip) at the odd r in {1, hop - 1}."""
    hop = geom[2]
    assert hop % 2 == 0
    worst = 0.0
    for r in sorted({0, hop - 2}):
        y = _clips(geom, T, r)
        if r == 0:
            _silence_covers_frames(y, geom, T)
        S, route = _stft(fe, y)
        assert route == 1, (tag, T, r, route)
        worst = max(worst, _worst(S, y, geom, (tag, T, r)))
    for r in sorted({1, hop - 1}):
        y = _clips(geom, T, r)
        for i in (0, 1):
            S, route = _stft(fe, y[i:i + 1])
            assert route == 1, (tag, T, r, route)
            worst = max(worst, _worst(S, y[i:i + 1], geom, (tag, T, r, "B=1", i)))
    return worst


def _report(tag, geom, route, worst):
    print("f32 STFT %-34s %-16s route %d: worst |S - ref| / max(ref) = %.3g" % (tag, geom, route, worst))


# ---------------------------------------------------------------------------------------------------
# 1. generic kernel, one geometry per radix chain
# ---------------------------------------------------------------------------------------------------
def _factor(M):
    """factor_radices of csrc/smh_ctx.hip: the radices in the preference order 8, 4, 2, 5, 3, 7."""
    out = []
    for p in (8, 4, 2, 5, 3, 7):
        while M % p == 0 and M > 1:
            out.append(p)
            M //= p
    return out if M == 1 else None


GENERIC = [  # (n_fft, win_length, hop), the radices of n_fft / 2
    ((8, 8, 3), [4]),                 # the smallest accepted size
    ((16, 11, 4), [8]),               # odd win_length: lpad = 2
    ((20, 20, 5), [2, 5]),
    ((84, 80, 37), [2, 3, 7]),        # odd hop
    ((96, 96, 1), [8, 2, 3]),         # hop 1
    ((140, 100, 35), [2, 5, 7]),
    ((320, 320, 160), [8, 4, 5]),     # a 20 ms window at 16 kHz
    ((600, 400, 160), [4, 5, 5, 3]),  # four stages
    ((980, 800, 245), [2, 5, 7, 7]),  # nb = 245 in stage 0: test_where_the_reciprocal_multiply_needs_its_half
    ((1000, 1000, 250), [4, 5, 5, 5]),
    ((1024, 1000, 256), [8, 8, 8]),   # at the LDS limit with 16 frames per workgroup
]


@pytest.mark.parametrize("geom,radices", GENERIC, ids=lambda v: "-".join(map(str, v)))
def test_generic_kernel_on_every_radix_chain(geom, radices):
    n_fft, wl, hop = geom
    assert _factor(n_fft // 2) == radices, "the preference order of factor_radices changed: this case covers other stages now"
    fe = _fe(n_fft=n_fft, win_length=wl, hop=hop, n_mels=0)
    # T = 41: three tiles of 14, 14 and 13 frames (tt = ceil(41 / ceil(41 / 16))), the last one short
    Ts = [41]
    if n_fft == 8:
        Ts.append(1)
    if n_fft == 1024:
        Ts.append(16)  # one tile of 16 frames: the 147 976 bytes of test_lds_need_of_the_generic_kernel
    worst = max(_run_generic(fe, geom, T, "generic") for T in Ts)
    _report("radices " + "x".join(map(str, radices)), geom, 0, worst)


def test_where_the_reciprocal_multiply_needs_its_half():
    """fdiv(it, inv) = (int)((it + 0.5f) * inv) stands for it / n in the work-item maps.  Without the + 0.5f it is one short
    wherever fl(q n * fl(1 / n)) < q -- which no n of the other geometries does: not their nb = M / R, not their Ns, not a frame
    count nf <= 16 (1 / nf against the bins of a tile).  Below n_fft = 1024 only nb = 189, 243 and 245 do (n_fft = 756, 972, 980):
    hence (980, 800, 245) in the list above, whose first stage maps item 245 to frame 1."""
    f32 = np.float32

    def short(n, inv, items):
        it = np.arange(items, dtype=np.int64)
        exact = ((it.astype(f32) + f32(0.5)) * inv).astype(np.int64)
        assert np.array_equal(exact, it // n), "fdiv itself"
        return np.nonzero((it.astype(f32) * inv).astype(np.int64) != it // n)[0]

    hit = {}
    for (n_fft, _, _), radices in GENERIC + [((400, 400, 160), [8, 5, 5])]:
        M, Ns = n_fft // 2, 1
        for s, R in enumerate(radices):
            nb = M // R
            for nf in range(1, 17):
                if len(short(nb, f32(R) / f32(M), nf * nb)):
                    hit.setdefault(n_fft, set()).add(("nb", nb))
            if s and len(short(Ns, f32(1) / f32(Ns), nb)):
                hit.setdefault(n_fft, set()).add(("Ns", Ns))
            Ns *= R
        for nf in range(1, 17):
            if len(short(nf, f32(1) / f32(nf), nf * (M + 1))):
                hit.setdefault(n_fft, set()).add(("nf", nf))
    assert hit == {980: {("nb", 245)}}
    assert short(245, f32(2) / f32(490), 16 * 245)[0] == 245


# ---------------------------------------------------------------------------------------------------
# 2. n_fft = 400: every route to either kernel
# ---------------------------------------------------------------------------------------------------
G400 = (400, 400, 160)


def _fe400(wl=400, hop=160):
    return _fe(n_fft=400, win_length=wl, hop=hop, n_mels=0)


@pytest.fixture
def default_route(monkeypatch):
    """The dispatch as a caller without tuning switches gets it."""
    for name in ("SMH_STFT_GENERIC", "SMH_STFT_FRAMES", "SMH_STFT_ROW"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_400_specialised_and_forced_generic(default_route):
    fe = _fe400()
    y = _clips(G400, 41, 0)
    assert y.shape[1] % 2 == 0
    S1, route = _stft(fe, y)
    assert route == 1
    w1 = _worst(S1, y, G400, "specialised")
    default_route.setenv("SMH_STFT_GENERIC", "1")
    S0, route = _stft(fe, y)
    assert route == 0
    w0 = _worst(S0, y, G400, "forced generic")
    _report("default", G400, 1, w1)
    _report("SMH_STFT_GENERIC=1 (8x5x5)", G400, 0, w0)
    assert _factor(200) == [8, 5, 5]


def test_400_odd_hop_takes_the_generic_kernel(default_route):
    geom = (400, 400, 161)
    _report("odd hop", geom, 0, _run_generic(_fe400(hop=161), geom, 41, "odd hop"))


def test_400_odd_length_single_clip_keeps_the_specialised_kernel(default_route):
    fe = _fe400()
    n = 400 + 40 * 160 + 1
    y = _base()[:3, :n].copy()
    S1, route = _stft(fe, y[:1])
    assert route == 1, "B = 1: the next clip's start does not matter"
    w1 = _worst(S1, y[:1], G400, "odd n, B = 1")
    S3, route = _stft(fe, y)
    assert route == 0, "B = 3: clips 1 and 2 start off an 8-byte boundary"
    w3 = _worst(S3, y, G400, "odd n, B = 3")
    _report("odd n_samples, B = 1", G400, 1, w1)
    _report("odd n_samples, B = 3", G400, 0, w3)


def test_400_clip_off_an_8_byte_boundary_takes_the_generic_kernel(default_route):
    fe = _fe400()
    y = _clips(G400, 41, 0, B=1)
    S, route = _stft(fe, y, front=1021)  # data_ptr() % 8 == 4 (asserted in _place)
    assert route == 0
    w = _worst(S, y, G400, "off8")
    S, route = _stft(fe, y, front=1022)
    assert route == 1
    _worst(S, y, G400, "on8")
    _report("data_ptr % 8 == 4, B = 1", G400, 0, w)


@pytest.mark.parametrize("wl,lpad", [(399, 0), (320, 40), (2, 199), (1, 199)])
def test_400_short_windows_on_the_specialised_kernel(wl, lpad, default_route):
    # the oracle pads like the context: 0.5 - 0.5 cos(2 pi n / win_length) placed at (n_fft - win_length) // 2
    assert lpad == (400 - wl) // 2
    w = np.zeros(400)
    w[lpad:lpad + wl] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wl) / wl)
    np.testing.assert_allclose(ofe.hann_window(wl, 400), w, rtol=0, atol=1e-15)
    assert np.array_equal(ofe.hann_window(wl, 400) == 0, np.abs(w) < 1e-15)
    geom = (400, wl, 160)
    _report("win_length %d (lpad %d)" % (wl, lpad), geom, 1, _run_specialised(_fe400(wl=wl), geom, 41, "win"))


@pytest.mark.parametrize("hop", [2, 80, 200, 400, 402])
def test_400_even_hops_on_the_specialised_kernel(hop, default_route):
    geom = (400, 400, hop)  # 402: the hop exceeds n_fft, frames skip samples
    _report("even hop %d" % hop, geom, 1, _run_specialised(_fe400(hop=hop), geom, 41, "hop"))


# tiles of F = ceil(T / ceil(T / 20)) frames: 1 | 19 | 20 | 11 + 10 | 20 + 20 | 14 + 14 + 13 | 16 + 16 + 16 + 13
# generic (tt = ceil(T / ceil(T / 16))):      1 | 10 + 9 | 10 + 10 | 11 + 10 | 14 + 14 + 12 | 14 + 14 + 13 | 16 + 16 + 16 + 13
FRAME_COUNTS = [1, 19, 20, 21, 40, 41, 61]


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("T", FRAME_COUNTS)
def test_400_frame_counts_at_the_tile_plans_edges(T, generic, default_route):
    fe = _fe400()
    if generic:
        default_route.setenv("SMH_STFT_GENERIC", "1")
        w = _run_generic(fe, G400, T, "T")
    else:
        w = _run_specialised(fe, G400, T, "T")
    _report("T = %d" % T, G400, 0 if generic else 1, w)


@pytest.mark.parametrize("T,plain_loop", [(30, False), (31, True), (32, True), (63, True)])
def test_400_phase_1_without_look_ahead(T, plain_loop, default_route):
    """stft400_kernel requests phase 1's audio ahead of the table loads when `25 * nf <= kRounds1 * blockDim.x` (nf: the frames of
    the tile; 3 * 256 = 768: nf <= 30), else it runs the plain loop.  The default plan gives F <= 20, so no T alone flips it: the
    tuning override SMH_STFT_FRAMES=32,256 raises the tile to 32 frames.  T = 30 still looks ahead, 31 and 32 do not; T = 63 is a
    tile of 32 and one of 31."""
    default_route.setenv("SMH_STFT_FRAMES", "32,256")
    F = -(-T // -(-T // 32))
    assert (25 * min(F, T) > 3 * 256) == plain_loop
    _report("T = %d, 32-frame tiles" % T, G400, 1, _run_specialised(_fe400(), G400, T, "plain loop"))


# ---------------------------------------------------------------------------------------------------
# 3. what is refused, and when
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,cause", [
    (dict(n_fft=44, win_length=44, hop=11), "prime factor"),     # n_fft / 2 = 22 = 2 x 11
    (dict(n_fft=402, win_length=400, hop=160), "prime factor"),  # 201 = 3 x 67
    (dict(n_fft=6, win_length=6, hop=2), "n_fft must be even and >= 8"),
    (dict(n_fft=400, win_length=401, hop=160), "win_length must be in"),
    (dict(n_fft=400, win_length=400, hop=0), "hop must be >= 1"),
])
def test_refused_at_context_creation(kw, cause):
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    with pytest.raises(ValueError, match=cause):
        Frontend(FrontendConfig(n_mels=0, **kw))
    lib = _lib.require_gpu()
    c = _lib.FrontendCfg(kw["n_fft"], kw["win_length"], kw["hop"], 0, 21, 11, 1, 22050.0)
    h = C.c_void_p()
    assert lib.smh_ctx_create_ex(C.byref(c), _lib.SMH_STFT_F32, C.byref(h)) == _lib.SMH_E_INVALID
    assert not h.value and cause in _lib.last_error()


def _generic_lds(n_fft, tt):
    """The launcher's formula (smh_stft_mag_f32): M twiddles, M + 1 untangle twiddles, two buffers of tt padded frames, 8 bytes each."""
    M = n_fft // 2
    MP = M + (M >> 4) + 2
    return 8 * (M + (M + 1) + 2 * tt * MP)


def _generic_tt(T):
    return -(-T // -(-T // 16))


def test_lds_need_of_the_generic_kernel():
    assert _generic_lds(1024, 16) == 147976 <= LDS_LIMIT  # 5 624 bytes under the limit
    # n_fft = 2048 at 16 frames per workgroup: 295 432 bytes by the launcher's formula (padded frame stride M + M / 16 + 2 = 1090;
    # 279 048 would be the figure with an unpadded stride of 1026)
    assert _generic_lds(2048, 16) == 295432 > LDS_LIMIT
    assert _generic_tt(40) == 14 and _generic_lds(2048, 14) == 260552 > LDS_LIMIT  # the 40-frame clip below
    assert _generic_tt(3) == 3 and _generic_lds(2048, 3) == 68712 <= LDS_LIMIT     # the 3-frame clip below
    assert max(tt for tt in range(1, 17) if _generic_lds(2048, tt) <= LDS_LIMIT) == 7


def test_n_fft_2048_is_accepted_or_refused_by_the_clips_frame_count(default_route):
    from sm_hpss_mtl_amd import _lib
    geom = (2048, 1600, 400)
    assert _factor(1024) == [8, 8, 8, 2]
    fe = _fe(n_fft=2048, win_length=1600, hop=400, n_mels=0)
    _report("3 frames", geom, 0, _run_generic(fe, geom, 3, "2048"))
    y = _clips(geom, 40, 0)
    x = _place(y, 1022)
    buf = torch.full((4, 1025, 40), SENTINEL, dtype=torch.float32, device="cuda")
    rc = fe.lib.smh_stft_mag_f32(fe._h, C.c_void_p(x.data_ptr()), 3, y.shape[1], C.c_void_p(buf.data_ptr()), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == _lib.SMH_E_INVALID and "too large for the LDS FFT" in _lib.last_error()
    assert bool((buf == SENTINEL).all()), "nothing was launched"
    with pytest.raises(ValueError, match="too large for the LDS FFT"):
        fe.stft_mag(x)
    # the refusal leaves nothing behind: the same context on a short clip, and another context
    _run_generic(fe, geom, 3, "2048 again")
    y = _clips(G400, 41, 0)
    S, route = _stft(_fe400(), y)
    assert route == 1
    _worst(S, y, G400, "after the refusal")


# ---------------------------------------------------------------------------------------------------
# 4. behind the STFT at another K
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [0, 40])
@pytest.mark.parametrize("geom", [(320, 320, 160), (1024, 1000, 256)], ids=["K161", "K513"])
def test_front_end_behind_the_stft_at_another_K(geom, n_mels, clips4):
    """Medians, masks, mel projection and dB at K = 161 and K = 513, judged on the device's own S (the method of
    tests/test_bench_path_gpu.py): 1e-3 dB on every bin."""
    n_fft, wl, hop = geom
    fe = _fe(n_fft=n_fft, win_length=wl, hop=hop, n_mels=n_mels, l_harm=21, l_perc=11, log_db=True)
    K, T = 1 + n_fft // 2, ofe.num_frames(16000, n_fft, hop)
    x = torch.from_numpy(clips4).cuda()
    S = fe.stft_mag(x)
    fv = fe.run(x)["fv"]
    torch.cuda.synchronize()
    rows = n_mels if n_mels else K
    assert S.shape == (4, K, T) and fv.shape == (4, 2 * rows, T) and fe.rows == rows
    S, fv = S.cpu().numpy(), fv.cpu().numpy()
    assert np.isfinite(fv).all()
    name = "LogMelHarmPercSpec" if n_mels else "LogHarmPercSpec"
    worst = 0.0
    for i in range(4):
        _worst(S[i:i + 1], clips4[i:i + 1], geom, ("front end", i))
        ref = ofe.featuregram_from_S(S[i], name, n_mels=n_mels, l_harm=21, l_perc=11)
        assert fv[i].shape == ref.shape
        err = float(np.max(np.abs(fv[i] - ref)))
        assert err <= 1e-3, (geom, n_mels, i, err)
        worst = max(worst, err)
    print("front end %s n_mels=%d: worst |fv - ref| = %.3g dB" % (geom, n_mels, worst))
    if n_mels:
        B = fe.mel_basis()
        ref = ofe.mel_basis(22050, n_fft, n_mels)
        assert B.shape == ref.shape == (n_mels, K)
        np.testing.assert_allclose(B, ref, rtol=2e-7, atol=0)  # tests/test_parity_gpu.py: test_mel_basis_and_projection
        assert np.array_equal(B == 0, ref == 0)


def test_plain_projection_runs_at_n_fft_1024_and_refuses_1200(clips4):
    """include/smh.h: the plain mel projection keeps a K x 64-frame image in LDS, n_fft <= 1198 with a filterbank."""
    fe = _fe(hpss=False, n_mels=120, n_fft=1024, win_length=1000, hop=256, mel_sr=16000.0)
    x = torch.from_numpy(clips4).cuda()
    S = fe.stft_mag(x)
    fv = fe.run(x)["fv"]
    assert torch.equal(fe.plain_features(S)["fv"], fv)
    S, fv = S.cpu().numpy(), fv.cpu().numpy()
    assert fv.shape == (4, 120, ofe.num_frames(16000, 1024, 256))
    for i in range(4):
        ref = pr.featuregram_from_S(S[i], "LogMelSpec", 120, 16000)
        err = float(np.max(np.abs(fv[i] - ref)))
        assert err <= 1e-3, (i, err)  # tests/test_plain_gpu.py: dB features abs 1e-3 on every bin
    # n_fft = 1200: n_fft / 2 = 600 = 8 x 5 x 5 x 3, the context is valid; 601 bins x 64 frames x 4 bytes > 150 KB
    assert _factor(600) == [8, 5, 5, 3] and 4 * 601 * 64 > 150 * 1024 >= 4 * 600 * 64
    big = _fe(hpss=False, n_mels=120, n_fft=1200, win_length=1000, hop=256, mel_sr=16000.0)
    y = clips4[:2, :1200 + 9 * 256]  # 10 frames: the generic STFT's own LDS need at n_fft = 1200 stays under its limit up to 14
    assert _generic_lds(1200, 14) <= LDS_LIMIT < _generic_lds(1200, 15)
    S = big.stft_mag(torch.from_numpy(np.ascontiguousarray(y)).cuda())
    _worst(S.cpu().numpy(), y, (1200, 1000, 256), "n_fft 1200")
    with pytest.raises(ValueError, match="LDS image"):
        big.plain_features(S)
    with pytest.raises(ValueError, match="LDS image"):
        big.run(torch.from_numpy(np.ascontiguousarray(y)).cuda())
    # without a filterbank the rule does not apply
    spec = _fe(hpss=False, n_mels=0, n_fft=1200, win_length=1000, hop=256, log_db=False)
    got = spec.plain_features(S)["fv"]
    assert torch.equal(got, S)
