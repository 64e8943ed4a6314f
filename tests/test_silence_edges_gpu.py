"""GPU tests of smh_silence.hip where its paths and its runs change: the cases of tests/silence_cases.py (each shown on the CPU, by
tests/test_silence_cases.py, to reach the branch it names) against oracle/silence.py and the results of the compiled reference
(tests/golden/silence_runs_golden.npz).

Bars.  The silence decision is integer work on given float32 energies: markers, n_keep and the compacted output are BIT-equal.
`preprocess_signal` carries the 1e-6 of tests/test_silence_gpu.py (two normalisations and an rms whose sums run in another order; the
audio cases keep every energy >= 1 % away from the threshold, so the decision itself cannot differ).  normalize / rms / mix_signals:
see the tests.  Every test prints the largest error it saw before it asserts (pytest -s shows it).

Device inputs are views into a larger allocation, fenced by NaN in front and behind (the last sample of the last clip is followed
by 64 NaN and the end of the allocation): a load outside the clip shows as NaN in the output instead of going unnoticed.  The fence
in front is a multiple of four floats, the 16-byte alignment the float4 load of the LDS kernel is entitled to."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from oracle import silence as osil
from tests import silence_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT, BACK = 1024, 64


@pytest.fixture(scope="module")
def sil():
    from sm_hpss_mtl_amd import silence
    return silence


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "silence_runs_golden.npz"))


@pytest.fixture(scope="module")
def route_query():
    from sm_hpss_mtl_amd import _lib
    fn = _lib.load().smh_internal_preprocess_route  # test-only export, not in include/smh.h
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]
    return fn


def fenced(a):
    """`a` as a contiguous float32 device tensor inside an allocation of NaN: FRONT NaN before it, BACK NaN behind it."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((FRONT + a.size + BACK,), float("nan"), dtype=torch.float32, device="cuda")
    buf[FRONT:FRONT + a.size] = torch.from_numpy(a.ravel()).cuda()
    return buf[FRONT:FRONT + a.size].view(a.shape)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- remove_silence: the crafted energies -------------------------------------------------------------------------------------------
def _remove(sil, cases):
    c = cases[0]
    x = np.stack([sc.crafted_signal(k) for k in cases])
    e = np.stack([k.energy for k in cases])
    out, n_keep, sm, fm = sil.remove_silence(fenced(x), fenced(e), c.fs, c.Tw, c.Ts, alpha=c.alpha, beta=c.beta, markers=True)
    return x, host(out), host(n_keep), host(sm), host(fm)


def _check_row(c, x, out, n_keep, sm, fm, golden=None):
    o_ref, sm_ref, fm_ref, _ = osil.remove_silence(x, c.energy, c.fs, c.Tw, c.Ts, c.alpha, c.beta)
    assert np.array_equal(fm, fm_ref)
    assert np.array_equal(sm, sm_ref)
    assert n_keep == (c.N if o_ref is x else int(sm_ref.sum()))
    assert out.dtype == np.float32 and np.array_equal(out, o_ref)
    if golden is not None:
        n, kept, untouched, _ = golden[c.name + "_meta"]
        assert np.array_equal(golden[c.name + "_x_sha"], sc.sha(x)) and np.array_equal(golden[c.name + "_energy_sha"], sc.sha(c.energy))
        assert np.array_equal(fm, golden[c.name + "_frame_marker"])
        assert np.array_equal(np.packbits(sm), golden[c.name + "_sample_marker"])
        assert n_keep == (n if untouched else kept)
        assert np.array_equal(sc.sha(out), golden[c.name + "_out_sha"])


@pytest.mark.parametrize("c", sc.CRAFTED, ids=lambda c: c.name)
def test_remove_silence_crafted(sil, golden, c):
    """Alone, then as row 1 of a batch of three whose rows 0 and 2 are other cases of the same shape: bit-equal to the compiled
    reference's results and to the oracle, and row 1 is what the case gave alone."""
    x, out, n_keep, sm, fm = _remove(sil, [c])
    _check_row(c, x[0], out[0], int(n_keep[0]), sm[0], fm[0], golden)
    a, b = sc.neighbours(c)
    x3, out3, n_keep3, sm3, fm3 = _remove(sil, [a, c, b])
    assert np.array_equal(out3[1], out[0]) and n_keep3[1] == n_keep[0]
    assert np.array_equal(sm3[1], sm[0]) and np.array_equal(fm3[1], fm[0])
    for i, k in enumerate((a, c, b)):
        _check_row(k, x3[i], out3[i], int(n_keep3[i]), sm3[i], fm3[i])


# ---- preprocess_signal: the audio cases on both routes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audio_refs():
    """(raw clip, oracle output, oracle n_keep) per audio case, computed once for both routes."""
    cache = {}

    def get(a, n):
        if (a.name, n) not in cache:
            raw = sc.audio_clip(a, n)
            ref = osil.load_and_preprocess_from_samples(raw, a.fs, a.Tw, a.Ts)
            cache[(a.name, n)] = (raw, ref, sc.audio_facts(raw, a.fs, a.Tw, a.Ts)["n_keep"])
        return cache[(a.name, n)]
    return get


@pytest.mark.parametrize("multipass", [False, True], ids=["default", "multipass"])
@pytest.mark.parametrize("p", sc.AUDIO_PARAMS, ids=sc.audio_id)
def test_preprocess_signal_audio(sil, route_query, audio_refs, p, multipass, monkeypatch):
    a, n = p
    if multipass:
        monkeypatch.setenv("SMH_SILENCE_MULTIPASS", "1")
    else:
        monkeypatch.delenv("SMH_SILENCE_MULTIPASS", raising=False)
    assert route_query(n, a.fs, a.Tw, a.Ts) == sc.route(n, a.fs, a.Tw, a.Ts, multipass)
    raw, ref, keep_ref = audio_refs(a, n)
    out, n_keep = sil.preprocess_signal(fenced(raw), a.fs, a.Tw, a.Ts)
    out, n_keep = host(out)[0], int(host(n_keep)[0])
    if n / a.fs < 0.1:  # the oracle goes on to duplicate a clip below 0.1 s (preprocessing.py:343-346), the caller's job here
        assert len(ref) % n == 0 and len(ref) > n
        ref = ref[:n]
    assert out.shape == ref.shape == (n,)
    err = float(np.max(np.abs(out - ref)))  # NaN (a load outside the clip) fails the comparison below
    print("preprocess_signal %s route %d: n_keep %d, max |out - oracle| = %.3g" % (sc.audio_id(p), route_query(n, a.fs, a.Tw, a.Ts), n_keep, err))
    assert n_keep == keep_ref
    assert err <= 1e-6
    assert np.all(out[n_keep:] == out[n_keep:n_keep + 1])  # the tail of the compaction is one value
    assert np.max(np.abs(out)) == 1.0


@pytest.mark.parametrize("multipass", [False, True], ids=["default", "multipass"])
def test_preprocess_signal_mixed_batch(sil, route_query, multipass, monkeypatch):
    """Clips with different outcomes side by side (in the LDS kernel every clip is its own workgroup with its own run table): every row
    of B = 8 and of B = 136 is bit-equal to the same clip processed alone on the same route, n_keep is the oracle's."""
    if multipass:
        monkeypatch.setenv("SMH_SILENCE_MULTIPASS", "1")
    else:
        monkeypatch.delenv("SMH_SILENCE_MULTIPASS", raising=False)
    fs, Tw, Ts = sc.MIXED_FS, sc.MIXED_TW, sc.MIXED_TS
    assert route_query(sc.MIXED_N, fs, Tw, Ts) == (0 if multipass else 1)
    x = sc.mixed_batch()
    keep_ref = np.array([sc.audio_facts(r, fs, Tw, Ts)["n_keep"] for r in x])
    alone = []
    for r in x:
        o, k = sil.preprocess_signal(fenced(r), fs, Tw, Ts)
        alone.append((host(o)[0], int(host(k)[0])))
    assert [k for _, k in alone] == list(keep_ref)
    alone_out = np.stack([o for o, _ in alone])
    assert not np.isnan(alone_out).any()
    worst = 0.0
    for row, o in zip(x, alone_out):
        worst = max(worst, float(np.max(np.abs(o - osil.load_and_preprocess_from_samples(row, fs, Tw, Ts)))))
    print("mixed batch, route %d: max |out - oracle| = %.3g" % (0 if multipass else 1, worst))
    assert worst <= 1e-6
    for rep in (1, sc.MIXED_REPEAT):
        out, n_keep = sil.preprocess_signal(fenced(np.tile(x, (rep, 1))), fs, Tw, Ts)
        out, n_keep = host(out), host(n_keep)
        assert out.shape == (8 * rep, sc.MIXED_N)
        assert np.array_equal(n_keep, np.tile(keep_ref, rep))
        assert np.array_equal(out, np.tile(alone_out, (rep, 1)))


# ---- normalize ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8191, 8192, 8193, 16385])
def test_normalize_chunk_edges_and_dc(sil, n):
    """Rows: zero-mean noise, noise + 0.05, and 1000 + 1e-3 * noise (a DC offset 10^5 times the signal).
    Reference: (x - mean) / max |x - mean| in float64 on the float32 input.
    Bound, absolute (|out| <= 1): 2^-23 * (1 + |mean| / m), m = max |x - mean|.  The kernel sums in float64 and rounds the mean to
    float32: mean error <= 2^-24 |mean|.  That error moves every difference x - mean, and the maximum m with it: each is a relative
    error of 2^-24 |mean| / m in the quotient, 2 * 2^-24 |mean| / m together.  The float32 subtraction rounds by <= 2^-24 of the
    difference (<= 2^-24 relative to m) and the IEEE division by <= 2^-24 of a quotient <= 1.  Sum: 2^-24 (2 + 2 |mean| / m).
    For the zero-mean rows at N >= 8191 (|mean| <= 0.05 + 4 / sqrt(N) < 0.1, m > 2) this is 1.2e-7 (1 + small), inside the 2e-7 of
    tests/test_silence_gpu.py.  Two samples are never zero-mean next to their own spread (m = |a - b| / 2), so at N = 2 only the
    formula holds."""
    rng = np.random.default_rng(n)
    noise = rng.standard_normal((3, n)).astype(np.float32)
    x = np.stack([noise[0], noise[1] + np.float32(0.05), np.float32(1000.0) + np.float32(1e-3) * noise[2]]).astype(np.float32)
    out = host(sil.normalize(fenced(x)))
    assert out.dtype == np.float32 and out.shape == x.shape
    for i in range(3):
        x64 = x[i].astype(np.float64)
        d = x64 - x64.mean()
        m = np.max(np.abs(d))
        bound = 2.0 ** -23 * (1.0 + abs(x64.mean()) / m)
        err = float(np.max(np.abs(out[i] - d / m)))
        print("normalize N=%d row %d: max err %.3g, bound %.3g" % (n, i, err, bound))
        assert err <= bound
        if i < 2 and n >= 8191:
            assert bound <= 2e-7  # a property of the input: here the formula is the existing bound
        assert np.max(np.abs(out[i])) == 1.0  # the peak sample divides to exactly +-1


# ---- rms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fl,hop", [(201, 400, 160), (1000, 401, 160), (1000, 33, 7), (1000, 64, 200), (8193, 512, 128),
                                      (22050, 551, 220)])
def test_rms_frame_edges(sil, n, fl, hop):
    """A frame that reflects at both ends (N just above frame / 2), odd frames, a frame below one wavefront, a hop beyond the frame.
    Against the float64 rms of the float32 input, relative 1e-6 (the bound of tests/test_silence_gpu.py for frames <= 512: a float32
    sum of up to 551 squares, 9 per lane and a 6-step tree, stays below 16 roundings of 6e-8; the square root halves it)."""
    y = np.random.default_rng(n + fl).standard_normal((3, n)).astype(np.float32)
    e = host(sil.rms(fenced(y), fl, hop))
    worst = 0.0
    for i in range(3):
        ref = osil.rms(y[i].astype(np.float64), fl, hop)
        assert e.shape == (3, len(ref)) and ref.dtype == np.float64
        worst = max(worst, float(np.max(np.abs(e[i] - ref) / ref)))
    print("rms N=%d frame=%d hop=%d: %d frames, max rel err %.3g" % (n, fl, hop, e.shape[1], worst))
    assert worst <= 1e-6


# ---- mix_signals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nmu", [(8192, 1), (8193, 8194), (16385, 5000)])
def test_mix_signals_loop_edges(sil, n, nmu):
    """Music of one sample (a constant, looped N times), music one sample longer than the speech (cut), and a speech length one
    sample into its third chunk with the music looped 3.3 times; against oracle.frontend.mix_signals within the 2e-6 of
    tests/test_silence_gpu.py."""
    rng = np.random.default_rng(n + nmu)
    sp = (0.3 * rng.standard_normal((3, n))).astype(np.float32)
    mu = (0.1 * rng.standard_normal((3, nmu)) + 0.02).astype(np.float32)
    db = np.array([-5.0, 0.0, 20.0], np.float32)
    out = host(sil.mix_signals(fenced(sp), fenced(mu), db))
    worst = 0.0
    for i in range(3):
        ref = ofe.mix_signals(sp[i], mu[i], float(db[i]))
        assert out[i].shape == ref.shape
        worst = max(worst, float(np.max(np.abs(out[i] - ref))))
    print("mix_signals N=%d N_mu=%d: max err %.3g" % (n, nmu, worst))
    assert worst <= 2e-6
