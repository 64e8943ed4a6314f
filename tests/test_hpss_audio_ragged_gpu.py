"""GPU: HPSS audio separation for clips of different lengths in one call (smh_hpss_audio_ragged_f32, `Frontend.separate_ragged`).

The contract: every clip's two components are bit for bit what smh_hpss_audio_f32 (`Frontend.separate`) gives that clip alone,
whatever else is in the call, whatever the sub-batching, in every run.  Clips are N(T, r) = n_fft + hop * (T - 1) + r samples of
tests/hpss_audio_ref.noise_tone; SHAPES covers a resynthesis tile boundary with and without a one-frame last tile (T = 16, 17, 33),
a halo that reaches into the previous 16-frame harm block (every T > 16), the 76-frame median tile boundary (T = 76, 77, 153), odd
sample counts and tails no frame covers (r > 0).

Which clips the ragged kernels take (route 0) and which go alone through smh_hpss_audio_f32 (route -1) is the rule of smh_rag.h:
the context has a block-split median kernel (both windows <= 21), the clip has T > l_harm / 2 + 4 frames (smh_median_plan.h: fast_ok;
T >= 15 at l_harm = 21, so T = 1 and T = 2 of SHAPES go alone and every T >= 2 * l_harm is taken), and it starts on an 8-byte
boundary where the f32 STFT reads float2 (n_fft = 400 with an even hop).  The reference of a clip that starts off a 16-byte boundary
is `separate` of that clip alone AT THE SAME ALIGNMENT: the f32 STFT picks its kernel by where a clip starts (include/smh.h), which is
what the contract's "alone" means.

Against the float64 restatement (tests/hpss_audio_ref.py), error measure and bound of tests/test_hpss_audio_frontend_gpu.py:
d(device, f64 restatement) <= 8 * d(f32 restatement, f64 restatement), uncovered samples within 1e-6 * max|x|.

Measured on an MI355X, test_against_f64_restatement, six (clip, component) figures: d_dev 8.2e-8 .. 1.5e-7, d_ref 7.5e-8 .. 1.2e-7,
ratio 0.70 .. 1.43 against the bound 8; uncovered samples 0.  The 26 cases of this module take 2.8 s."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import hpss_audio_ref as ref
from tests.test_hpss_audio_gpu import CONFIGS, _audio_dev, _fe

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (2, 159), (15, 0), (16, 1), (17, 0), (33, 77), (76, 0), (77, 3), (153, 158)]
SHUFFLED = [4, 8, 0, 6, 2, 7, 1, 5, 3]
NAN_BITS = 0x7FC00DAD  # a quiet NaN with a payload of its own: the pre-fill of every output
PRECISIONS = ["f32", "f64"]
L_HARM = 21  # FrontendConfig's default

_SIGNALS, _ALONE = {}, {}


def _n(cfg, T, r):
    return cfg[0] + cfg[2] * (T - 1) + r


def _signals(cfg):
    """The clips of SHAPES for this configuration: computed once, shared, left unchanged."""
    if cfg not in _SIGNALS:
        _SIGNALS[cfg] = [ref.noise_tone(_n(cfg, T, r), seed=100 + i) for i, (T, r) in enumerate(SHAPES)]
    return _SIGNALS[cfg]


def _alone(cfg, precision, i, misalign=0):
    """`separate` of clip i alone, `misalign` floats off a 16-byte boundary: (harmonic, percussive) as numpy, computed once."""
    key = (cfg, precision, i, misalign)
    if key not in _ALONE:
        x = _signals(cfg)[i]
        got = _fe(cfg, precision).separate(_audio_dev(x[None], front=misalign)[0])
        _ALONE[key] = (got["harmonic"].cpu().numpy(), got["percussive"].cpu().numpy())
    return _ALONE[key]


def _skip_if_forced():
    """A test that asserts WHICH kernels ran has nothing to say when an environment switch forces another route."""
    forced = [n for n in os.environ if n.startswith("SMH_MEDIAN_") or n == "SMH_RAGGED_PERFILE"]
    if forced:
        pytest.skip("implementation forced by " + ", ".join(forced))


def _filled(n):
    return torch.full((n,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


class Call:
    """One layout of clips for the C ABI: the audio buffer (NaN in every gap), host tables, pre-filled outputs."""

    def __init__(self, fe, xs, offs, slack=16):
        self.fe, self.xs, self.offs, self.lens = fe, xs, list(offs), [len(x) for x in xs]
        self.B = len(xs)
        self.total = max(o + n for o, n in zip(self.offs, self.lens)) + slack
        host = np.full(self.total, np.nan, np.float32)
        for x, o in zip(xs, self.offs):
            host[o:o + len(x)] = x
        self.audio = torch.from_numpy(host).cuda()
        self.h_off, self.h_len = (C.c_longlong * self.B)(*self.offs), (C.c_int * self.B)(*self.lens)
        self.fresh()

    def fresh(self):
        self.yh, self.yp = _filled(self.total), _filled(self.total)

    def sizes(self):
        hT, work = (C.c_int * self.B)(), C.c_size_t()
        rc = self.fe.lib.smh_hpss_audio_ragged_sizes(self.fe._h, self.h_off, self.h_len, self.B, hT, C.byref(work))
        assert rc == 0
        return list(hT), work.value

    def routes(self):
        out = (C.c_int * self.B)()
        rc = self.fe.lib.smh_internal_hpss_audio_ragged_route(self.fe._h, C.c_void_p(self.audio.data_ptr()), self.h_off, self.h_len, self.B, out)
        assert rc == 0
        return list(out)

    def args(self, work, work_bytes=None):
        from sm_hpss_mtl_amd import _lib
        p = lambda t: C.c_void_p(t.data_ptr())
        return [self.fe._h, p(self.audio), self.h_off, self.h_len, self.B, p(self.yh), p(self.yp), p(work),
                work.numel() if work_bytes is None else work_bytes, _lib.current_stream()]

    def run(self, work=None, work_bytes=None):
        if work is None:
            work = torch.empty(max(self.sizes()[1], 16), dtype=torch.uint8, device="cuda")
        return self.fe.lib.smh_hpss_audio_ragged_f32(*self.args(work, work_bytes))

    def untouched(self):
        return bool((_bits(self.yh) == NAN_BITS).all() and (_bits(self.yp) == NAN_BITS).all())

    def component(self, b):
        o, n = self.offs[b], self.lens[b]
        return self.yh[o:o + n].cpu().numpy(), self.yp[o:o + n].cpu().numpy()


def _packed(lens, gap=0, first=0):
    """offsets: multiples of 4, `gap` extra floats (a multiple of 4) between clips"""
    offs, o = [], first
    for n in lens:
        offs.append(o)
        o += (n + 3) // 4 * 4 + gap
    return offs


def _gapped(lens):
    """offsets that are multiples of 4 with 4 .. 12 floats between clips"""
    offs, o = [], 8
    for i, n in enumerate(lens):
        offs.append(o)
        o = (o + n + (4, 8, 9)[i % 3] + 3) // 4 * 4
        assert 4 <= o - (offs[-1] + n) <= 12 and o % 4 == 0
    return offs


def _equal_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


@pytest.mark.parametrize("order", ["listed", "shuffled"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_bit_identity(cfg, precision, order):
    """1: one call of `separate_ragged` on all of SHAPES: every component torch.equal to `separate` of that clip alone."""
    fe = _fe(cfg, precision)
    idx = list(range(len(SHAPES))) if order == "listed" else SHUFFLED
    got = fe.separate_ragged([_signals(cfg)[i] for i in idx])
    assert len(got["harmonic"]) == len(got["percussive"]) == len(idx)
    for pos, i in enumerate(idx):
        wh, wp = _alone(cfg, precision, i)
        assert torch.equal(got["harmonic"][pos].cpu(), torch.from_numpy(wh)), (cfg, precision, SHAPES[i], "harmonic")
        assert torch.equal(got["percussive"][pos].cpu(), torch.from_numpy(wp)), (cfg, precision, SHAPES[i], "percussive")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_the_ragged_kernels_ran(cfg, precision):
    """2: at default switches every clip of test 1 with T >= 2 * l_harm is on route 0, and the batch holds both routes: route 0 from
    T = l_harm / 2 + 5 = 15 on (fast_ok), route -1 for T = 1 and T = 2.  Without this an all-fallback implementation passes test 1."""
    _skip_if_forced()
    fe = _fe(cfg, precision)
    xs = _signals(cfg)
    call = Call(fe, xs, _packed([len(x) for x in xs]))
    routes = call.routes()
    assert set(routes) == {0, -1}, routes
    for (T, r), route in zip(SHAPES, routes):
        assert route == (0 if T > L_HARM // 2 + 4 else -1), (T, r, route)
        if T >= 2 * L_HARM:
            assert route == 0
    assert call.sizes()[0] == [T for T, _ in SHAPES]


@pytest.mark.parametrize("cfg", CONFIGS)
def test_nothing_else_is_written(cfg):
    """3: through the C ABI, outputs pre-filled with a NaN pattern, 4 .. 12 floats between clips and slack behind the last: every gap
    and the slack keep the pattern; inside a clip every sample from n_fft + hop * (T - 1) on is +0.0, everything before it finite."""
    fe = _fe(cfg)
    xs = _signals(cfg)
    call = Call(fe, xs, _gapped([len(x) for x in xs]), slack=40)
    assert call.run() == 0, fe.lib.smh_last_error()
    torch.cuda.synchronize()
    for y in (call.yh, call.yp):
        bits = _bits(y)
        inside = np.zeros(call.total, bool)
        for (T, r), o, n in zip(SHAPES, call.offs, call.lens):
            inside[o:o + n] = True
            cov = cfg[0] + cfg[2] * (T - 1)
            assert np.isfinite(y[o:o + cov].cpu().numpy()).all(), (T, r)
            assert (bits[o + cov:o + n] == 0).all(), (T, r)  # +0.0, not -0.0
            assert n - cov == r
        assert (bits[~inside] == NAN_BITS).all()
        assert (~inside).sum() >= 40 + 4 * (len(xs) - 1)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_misaligned_starts(cfg, precision):
    """4: one clip at an offset = 1 and one at = 2 (mod 4) among aligned ones, all of an even sample count.  Bit-equal to `separate` of
    the clip alone at that alignment.  Where the f32 STFT reads float2 (n_fft = 400) the clip at 1 (mod 4) starts off an 8-byte
    boundary and goes alone; the clip at 2 (mod 4) and every clip of the other contexts are taken."""
    fe = _fe(cfg, precision)
    idx = [2, 4, 6, 7]  # (15, 0), (17, 0), (76, 0) and (77, 3) cut to an even length below
    xs = [_signals(cfg)[i] for i in idx]
    xs[3] = xs[3][:len(xs[3]) - 1]
    assert all(len(x) % 2 == 0 for x in xs)
    mis = [0, 1, 2, 0]
    offs, o = [], 0
    for x, m in zip(xs, mis):
        offs.append(o + m)
        o = (o + m + len(x) + 3) // 4 * 4 + 4
    call = Call(fe, xs, offs)
    assert [o % 4 for o in call.offs] == mis and call.audio.data_ptr() % 16 == 0
    if not [n for n in os.environ if n.startswith("SMH_MEDIAN_") or n in ("SMH_RAGGED_PERFILE", "SMH_STFT_GENERIC")]:
        need8 = precision == "f32" and cfg[0] == 400
        assert call.routes() == [0, -1 if need8 else 0, 0, 0]
    assert call.run() == 0, fe.lib.smh_last_error()
    torch.cuda.synchronize()
    for b, (x, m) in enumerate(zip(xs, mis)):
        want = fe.separate(_audio_dev(x[None], front=m)[0])
        gh, gp = call.component(b)
        assert _equal_bits(gh, want["harmonic"].cpu().numpy()), (cfg, precision, b, m)
        assert _equal_bits(gp, want["percussive"].cpu().numpy()), (cfg, precision, b, m)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_sub_batches(cfg):
    """5: a workspace of exactly the single-clip minimum -- the largest answer of _sizes for each clip alone -- runs the call in
    sub-batches with the same bits as the full workspace; one byte less is SMH_E_WORKSPACE and the outputs keep their pre-fill."""
    from sm_hpss_mtl_amd import _lib
    fe = _fe(cfg)
    xs = _signals(cfg)
    call = Call(fe, xs, _packed([len(x) for x in xs]))
    least = max(Call(fe, [x], [0]).sizes()[1] for x in xs)
    full = call.sizes()[1]
    if call.routes().count(0) > 1:  # (a switch that sends every clip alone leaves nothing to split)
        assert least < full
    assert call.run() == 0, fe.lib.smh_last_error()
    torch.cuda.synchronize()
    want = (_bits(call.yh), _bits(call.yp))
    call.fresh()
    work = torch.empty(least, dtype=torch.uint8, device="cuda")
    assert call.run(work) == 0, fe.lib.smh_last_error()
    torch.cuda.synchronize()
    assert (_bits(call.yh) == want[0]).all() and (_bits(call.yp) == want[1]).all()
    for b in range(call.B):
        gh, gp = call.component(b)
        wh, wp = _alone(cfg, "f32", b)
        assert _equal_bits(gh, wh) and _equal_bits(gp, wp), SHAPES[b]
    call.fresh()
    assert call.run(work, least - 1) == _lib.SMH_E_WORKSPACE
    assert "smh_hpss_audio_ragged_f32" in _lib.last_error()
    torch.cuda.synchronize()
    assert call.untouched()


def test_fallback_context():
    """6: l_harm = 31 has no block-split median kernel: every clip is on route -1 and the result is bit-equal to `separate` alone."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    cfg = CONFIGS[0]
    fe = Frontend(FrontendConfig(n_fft=cfg[0], win_length=cfg[1], hop=cfg[2], l_harm=31))
    xs = [_signals(cfg)[i] for i in (0, 4, 5, 7)]
    call = Call(fe, xs, _packed([len(x) for x in xs]))
    assert call.routes() == [-1] * 4
    got = fe.separate_ragged(xs)
    for b, x in enumerate(xs):
        want = fe.separate(torch.from_numpy(x).cuda())
        assert torch.equal(got["harmonic"][b], want["harmonic"]) and torch.equal(got["percussive"][b], want["percussive"]), b


def test_against_f64_restatement():
    """7: an f64-STFT context at CONFIGS[0], clips (17, 0), (33, 77), (77, 3) from one ragged call, against the float64 restatement --
    not only against the device's own other path.  d(device, f64) <= 8 * d(f32 restatement, f64 restatement)."""
    cfg = CONFIGS[0]
    fe = _fe(cfg, "f64")
    idx = [SHAPES.index(s) for s in ((17, 0), (33, 77), (77, 3))]
    xs = [_signals(cfg)[i] for i in idx]
    got = fe.separate_ragged(xs)
    for b, x in enumerate(xs):
        harm, perc = ref.medians(x, *cfg, 21, 11)
        r64, r32 = ref.resynth(x, harm, perc, *cfg, np.float64), ref.resynth(x, harm, perc, *cfg, np.float32)
        xmax = float(np.abs(x).max())
        unc = ref.uncovered(r64["wss"])
        for c in ("harmonic", "percussive"):
            y = got[c][b].cpu().numpy()
            d_ref = ref.distance(r32[c], r64[c], r64["wss"], xmax)
            d_dev = ref.distance(y, r64[c], r64["wss"], xmax)
            print("ragged %s clip %s %s: d_dev = %.3g, d_ref = %.3g, ratio %.2f" % (cfg, SHAPES[idx[b]], c, d_dev, d_ref, d_dev / d_ref))
            assert d_dev <= 8 * d_ref, (SHAPES[idx[b]], c, d_dev, d_ref)
            assert np.abs(y[unc] - r64[c][unc]).max() <= 1e-6 * xmax


@pytest.mark.parametrize("precision", PRECISIONS)
def test_repeats_and_stream_order(precision):
    """8: the same call twice gives the same bits; four calls in flight (the four staging slots) give the same bits as one."""
    cfg = CONFIGS[0]
    fe = _fe(cfg, precision)
    xs = _signals(cfg)
    call = Call(fe, xs, _packed([len(x) for x in xs]))
    work = torch.empty(call.sizes()[1], dtype=torch.uint8, device="cuda")
    assert call.run(work) == 0
    torch.cuda.synchronize()
    want = (_bits(call.yh), _bits(call.yp))
    call.fresh()
    assert call.run(work) == 0
    torch.cuda.synchronize()
    assert (_bits(call.yh) == want[0]).all() and (_bits(call.yp) == want[1]).all()
    outs = []
    for _ in range(4):  # no synchronisation in between
        call.fresh()
        assert call.run(work) == 0
        outs.append((call.yh, call.yp))
    torch.cuda.synchronize()
    for yh, yp in outs:
        assert (_bits(yh) == want[0]).all() and (_bits(yp) == want[1]).all()


def test_refusals():
    """9: every refusal, its code and a text that names the clip where one is at fault; the outputs stay untouched.  All host-side."""
    from sm_hpss_mtl_amd import _lib
    cfg = CONFIGS[0]
    fe = _fe(cfg)
    lib = fe.lib
    xs = [_signals(cfg)[i] for i in (2, 4, 3)]
    call = Call(fe, xs, _packed([len(x) for x in xs]))
    need = call.sizes()[1]
    work = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 16 == 0

    def refused(rc, code, text):
        assert rc == code, (rc, _lib.last_error())
        assert text in _lib.last_error(), _lib.last_error()

    good = call.args(work, need)
    for i in (0, 1, 2, 3, 5, 6):  # null pointers
        args = list(good)
        args[i] = None
        refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "null argument")
    args = list(good)
    args[7] = None
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "null workspace")
    args = list(good)
    args[4] = -1
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "B=-1 is negative")
    refused(lib.smh_hpss_audio_ragged_sizes(fe._h, call.h_off, call.h_len, -1, None, None), _lib.SMH_E_INVALID, "B=-1 is negative")
    args = list(good)
    args[3] = (C.c_int * 3)(call.lens[0], cfg[0] - 1, call.lens[2])
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "clip 1 of 399 samples is shorter than n_fft=400")
    refused(lib.smh_hpss_audio_ragged_sizes(fe._h, call.h_off, args[3], 3, None, None), _lib.SMH_E_INVALID, "clip 1 of 399 samples")
    args = list(good)
    args[2] = (C.c_longlong * 3)(call.offs[0], -4, call.offs[2])
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "clip 1 has a negative offset")
    args = list(good)
    args[2] = (C.c_longlong * 3)(call.offs[0], call.offs[1], call.offs[1] + call.lens[1] - 1)
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "clip 1 and clip 2 overlap")
    args[2] = (C.c_longlong * 3)(call.offs[2], call.offs[1], call.offs[2])  # the same clip twice, out of order
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "clip 0 and clip 2 overlap")
    args = list(good)
    args[6] = C.c_void_p(call.yh.data_ptr() + 4 * (call.total - 20))
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "d_y_harm and d_y_perc overlap")
    args = list(good)
    args[5] = C.c_void_p(call.audio.data_ptr() + 4 * call.lens[0])
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "an output overlaps the audio or the workspace")
    args = list(good)
    args[6] = C.c_void_p(work.data_ptr())
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "an output overlaps the audio or the workspace")
    args = list(good)
    args[7] = C.c_void_p(work.data_ptr() + 4)
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_INVALID, "not 16-byte aligned")
    args = list(good)
    args[8] = 1024
    refused(lib.smh_hpss_audio_ragged_f32(*args), _lib.SMH_E_WORKSPACE, "needed by the largest single clip")
    # a capturing stream: refused before anything is enqueued; nothing is launched inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.smh_hpss_audio_ragged_f32(*call.args(work, need))
        err = _lib.last_error()
    torch.cuda.synchronize()
    assert rc == _lib.SMH_E_INVALID and "smh_hpss_audio_ragged_f32" in err and "cannot be captured in a graph" in err
    # B = 0: SMH_OK, nothing touched
    args = list(good)
    args[4] = 0
    assert lib.smh_hpss_audio_ragged_f32(*args) == _lib.SMH_OK
    work_bytes = C.c_size_t(7)
    assert lib.smh_hpss_audio_ragged_sizes(fe._h, call.h_off, call.h_len, 0, None, C.byref(work_bytes)) == _lib.SMH_OK and work_bytes.value == 0
    torch.cuda.synchronize()
    assert call.untouched()
    # and the good arguments work
    assert lib.smh_hpss_audio_ragged_f32(*good) == _lib.SMH_OK, _lib.last_error()
    torch.cuda.synchronize()
    for b, i in enumerate((2, 4, 3)):
        gh, gp = call.component(b)
        wh, wp = _alone(cfg, "f32", i)
        assert _equal_bits(gh, wh) and _equal_bits(gp, wp)


def test_python_refusals():
    """9, Python: an empty list, a 2-D entry and a short entry naming its index; `out` carries the two flat buffers; a plain
    configuration is refused as `separate` refuses it."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    cfg = CONFIGS[0]
    fe = _fe(cfg)
    assert fe.separate_ragged([]) == {"harmonic": [], "percussive": []}
    xs = [_signals(cfg)[2], _signals(cfg)[3]]
    with pytest.raises(ValueError, match=r"signals\[1\] must be 1-D"):
        fe.separate_ragged([xs[0], xs[1][None]])
    with pytest.raises(ValueError, match=r"signals\[1\] of 399 samples is shorter than n_fft=400"):
        fe.separate_ragged([xs[0], xs[1][:399]])
    total = sum((len(x) + 3) // 4 * 4 for x in xs)
    out = {"harmonic": torch.empty(total, device="cuda"), "percussive": torch.empty(total, device="cuda")}
    got = fe.separate_ragged([torch.from_numpy(xs[0]).cuda(), xs[1]], out=out)
    assert got["harmonic"][0].data_ptr() == out["harmonic"].data_ptr() and got["percussive"][1].shape == (len(xs[1]),)
    for b, i in enumerate((2, 3)):
        wh, wp = _alone(cfg, "f32", i)
        assert torch.equal(got["harmonic"][b].cpu(), torch.from_numpy(wh)) and torch.equal(got["percussive"][b].cpu(), torch.from_numpy(wp))
    with pytest.raises(ValueError, match="has shape"):
        fe.separate_ragged(xs, out={"harmonic": torch.empty(total + 4, device="cuda")})
    plain = Frontend(FrontendConfig(hpss=False, n_mels=0))
    with pytest.raises(ValueError, match="plain configuration"):
        plain.separate_ragged(xs)
