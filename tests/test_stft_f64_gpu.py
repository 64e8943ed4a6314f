"""GPU: the f64 STFT mode (FrontendConfig(stft_precision="f64"), csrc/smh_stft_f64.hip) against the oracle.

In f64 mode |S| must equal oracle.frontend.stft_mag (np.abs of librosa's complex64 STFT) bit for bit: the bound is >= 99.99 % of
the bins bit-equal, every other bin within 1 ulp and exactly 0 where the oracle gives 0; the fraction measured is reported in the
assertion messages.  Bins more than 100 dB below their frame's maximum (near-pure tones only) are held to the f64 noise floor
instead: no f64 transform but pocketfft's own summation order reproduces their last bits (_compare_S).  With that S, the whole front end meets from the AUDIO the bounds tests/test_streaming_frontend_gpu.py holds
it to from the device's own S, on every bin: 1e-3 dB (Log*), 1e-6 max|S| (HarmPercSpec), rel 1e-5 (MelHarmPercSpec).
The default (f32) mode is unchanged: its outputs equal those of a context made by the old smh_ctx_create.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import frontend as ofe

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float32).tiny

NAMES = {  # feature name -> FrontendConfig fields
    "LogMelHarmPercSpec": dict(),
    "MelHarmPercSpec": dict(log_db=False),
    "LogHarmPercSpec": dict(n_mels=0),
    "HarmPercSpec": dict(n_mels=0, log_db=False),
}
_FES = {}


def _fe(**kw):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    cfg = FrontendConfig(**kw)
    if cfg not in _FES:
        _FES[cfg] = Frontend(cfg)
    return _FES[cfg]


def _f64(**kw):
    return _fe(stft_precision="f64", **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _music(n, seed, silent=None):
    """Tones with a tremolo, gated noise and clicks (peak about 1); `silent` = (start, end): digital silence there."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    f0 = 110.0 * 2.0 ** (rng.integers(0, 24) / 12.0)
    y = np.zeros(n)
    for h in range(1, 7):
        y += 0.2 / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi))
    y *= 0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t)
    gate = (rng.random(n // 1600 + 1) > 0.7).repeat(1600)[:n]
    y += 0.1 * rng.standard_normal(n) * gate
    y[rng.integers(0, n, n // 8000 + 1)] += 0.5
    if silent is not None:
        y[silent[0]:silent[1]] = 0.0
    return y.astype(np.float32)


DEEP_DB = 100.0  # bins this far below their frame's largest: f64 rounding noise of ANY summation order reaches their f32 ulp


def _compare_S(S, ref, tag):
    """The f64 bound on |S|; returns (bit-equal bins, bins).  Bins within DEEP_DB of their frame's maximum: >= 99.99 % bit-equal.
    Every bin: within 1 ulp, or within the f64 noise floor of 1e-11 of its frame's maximum.  The floor is for the deep bins -- the
    sidelobe nulls of near-pure tones, down to -200 dB; synth_clips, with a dynamic range of 67-83 dB, has none -- where two f64
    FFTs of different summation order round to different f32 values (numpy's own rfft against a DFT product as well).  Exactly 0
    where the oracle gives 0."""
    assert S.shape == ref.shape and S.dtype == np.float32, (tag, S.shape, ref.shape)
    eq = S.view(np.uint32) == ref.view(np.uint32)
    ulps = np.abs(S.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    fmax = np.broadcast_to(ref.max(axis=0, keepdims=True), ref.shape).astype(np.float64)
    top = ref >= fmax * 10.0 ** (-DEEP_DB / 20)
    n_eq, n = int(eq.sum()), eq.size
    n_top, n_top_eq = int(top.sum()), int(eq[top].sum())
    rel = np.abs(S.astype(np.float64) - ref) / np.maximum(fmax, TINY)
    off = (ulps > 1) & (rel > 1e-11)
    msg = "%s: %d of %d bins bit-equal (%.6f %%); within %g dB of the frame max %d of %d (%.6f %%); max %d ulp, %d bins beyond " \
          "1 ulp and 1e-11 of the frame max (worst %.3g)" % (tag, n_eq, n, 100.0 * n_eq / n, DEEP_DB, n_top_eq, n_top,
                                                             100.0 * n_top_eq / max(n_top, 1), int(ulps.max()), int(off.sum()),
                                                             float(rel.max()))
    assert n_top_eq >= 0.9999 * n_top, msg
    assert not off.any() and (S >= 0).all(), msg
    assert (S[ref == 0] == 0).all(), msg + "; nonzero where the oracle gives 0"
    return n_eq, n


def _synth(n, seed, silent=None):
    """One synth_clips clip of n samples (the kind bench.py runs); `silent` = (start, end): digital silence there."""
    from sm_hpss_mtl_amd.synth import synth_clips
    y = synth_clips(1, seed=seed, n_samples=n)[0].copy()
    if silent is not None:
        y[silent[0]:silent[1]] = 0.0
    return y


def _clip_set(n_fft):
    from sm_hpss_mtl_amd.synth import bench_clips, synth_clips
    return {
        "clips4": synth_clips(4, seed=0),
        "bench64": bench_clips(64),
        "odd": _synth(16001, 3)[None],
        "silent": _synth(24000, 4, silent=(5000, 9000 + n_fft))[None],
        "tones": np.stack([_music(24000, 5), _music(24000, 6)]),  # near-pure tones: bins down to -200 dB (the deep-bin rule)
    }


@pytest.mark.parametrize("n_fft,win_length", [(400, 400), (512, 400)])
def test_stft_mag_equals_the_oracle_bit_for_bit(n_fft, win_length):
    fe = _f64(n_fft=n_fft, win_length=win_length, n_mels=0)
    tot_eq = tot = 0
    for tag, clips in _clip_set(n_fft).items():
        S = _host(fe.stft_mag(_dev(clips)))
        for i, y in enumerate(clips):
            ref = ofe.stft_mag(y, n_fft=n_fft, win_length=win_length, hop=160)
            e, n = _compare_S(S[i], ref, (n_fft, tag, i))
            tot_eq, tot = tot_eq + e, tot + n
            if tag == "silent":
                assert (ref == 0).sum() >= 10 * ref.shape[0], "the silent stretch covers whole frames"
    # a clip starting off an 8-byte boundary (data_ptr % 8 == 4), of odd length
    y = _synth(20001, 5)
    buf = torch.zeros(len(y) + 1, dtype=torch.float32, device="cuda")
    buf[1:] = _dev(y)
    x = buf[1:][None]
    assert x.data_ptr() % 8 == 4
    e, n = _compare_S(_host(fe.stft_mag(x))[0], ofe.stft_mag(y, n_fft=n_fft, win_length=win_length, hop=160), (n_fft, "off8"))
    tot_eq, tot = tot_eq + e, tot + n
    print("f64 STFT n_fft=%d: %d of %d bins bit-equal (%.6f %%)" % (n_fft, tot_eq, tot, 100.0 * tot_eq / tot))


@pytest.mark.parametrize("n_fft,win_length,hop", [(84, 80, 37), (96, 96, 1), (1024, 1000, 256), (2048, 1600, 400)])
def test_stft_mag_other_radices_hops_and_windows(n_fft, win_length, hop):
    """n_fft / 2 = 42 (2 x 3 x 7), 48 (8 x 2 x 3), 512 (8 x 8 x 8), 1024 (beyond the f32 kernel's LDS); hop 1 and odd hops."""
    fe = _f64(n_fft=n_fft, win_length=win_length, hop=hop, n_mels=0)
    n = n_fft + 40 * hop + 3
    clips = np.stack([_synth(n, 7), _synth(n, 8, silent=(0, n_fft + 2 * hop)), _music(n, 9)])
    S = _host(fe.stft_mag(_dev(clips)))
    for i, y in enumerate(clips):
        _compare_S(S[i], ofe.stft_mag(y, n_fft=n_fft, win_length=win_length, hop=hop), (n_fft, win_length, hop, i))


def test_plain_grid_gives_the_bits_of_the_per_xcd_grid(monkeypatch):
    """SMH_STFT_XCD=0 (the (tile, clip) grid) against the default 1-D grid: B = 3, T = 41 (three tiles of 14, 14 and 13 frames)."""
    monkeypatch.delenv("SMH_STFT_XCD", raising=False)
    fe = _f64(n_mels=0)
    n = 400 + 40 * 160
    clips = np.stack([_synth(n, 51), _synth(n, 52, silent=(0, 400 + 2 * 160)), _music(n, 53)])
    x = _dev(clips)
    from tests import stft_plans as P
    grid = lambda: P.ask_library(fe.lib, fe._h, x.data_ptr(), 3, n)[P.FIELDS.index("grid_x"):P.FIELDS.index("pairs")]
    S = fe.stft_mag(x)
    assert grid() == (16, 1, 3)
    monkeypatch.setenv("SMH_STFT_XCD", "0")
    S_plain = fe.stft_mag(x)
    assert grid() == (3, 3, 0)
    assert S.shape == (3, 201, 41) and torch.equal(S, S_plain)
    _compare_S(_host(S_plain)[0], ofe.stft_mag(clips[0], n_fft=400, win_length=400, hop=160), "plain grid")


def _window_ok(Sok, h, axis):
    """bins whose median window (half width h along `axis`, reflect boundary) holds bit-equal S only"""
    bad = ~Sok
    out = bad.copy()
    n = bad.shape[axis]
    for d in range(1, h + 1):
        sl_a = [slice(None)] * 2
        sl_b = [slice(None)] * 2
        sl_a[axis], sl_b[axis] = slice(d, n), slice(0, n - d)
        out[tuple(sl_a)] |= bad[tuple(sl_b)]
        out[tuple(sl_b)] |= bad[tuple(sl_a)]
    return ~out


def _check_fv(fe, fv, S_ref, tag):
    cfg = fe.cfg
    name = ("Log" if cfg.log_db else "") + ("Mel" if cfg.n_mels else "") + "HarmPercSpec"
    ref = ofe.featuregram_from_S(S_ref, name, n_mels=cfg.n_mels, l_harm=cfg.l_harm, l_perc=cfg.l_perc)
    assert fv.shape == ref.shape, (tag, fv.shape, ref.shape)
    smax = float(S_ref.max())
    if cfg.log_db:
        err = float(np.max(np.abs(fv - ref)))
        assert err <= 1e-3, (tag, err)
    elif not cfg.n_mels:
        err = float(np.max(np.abs(fv - ref)))
        assert err <= 1e-6 * smax, (tag, err, smax)
    else:
        np.testing.assert_allclose(fv, ref, rtol=1e-5, atol=1e-6 * smax, err_msg=str(tag))


@pytest.mark.parametrize("name", sorted(NAMES))
def test_end_to_end_from_the_audio_with_taps(clips4, name):
    fe = _f64(**NAMES[name])
    cfg = fe.cfg
    for tag, clips in (("clips4", clips4), ("odd", _synth(16001, 11)[None]), ("silent", _synth(30000, 12, silent=(4000, 12000))[None]),
                       ("tones", _music(30001, 13)[None])):
        res = fe.run(_dev(clips), W=68, shift=68, taps=True)
        S, harm, perc, fv = (_host(res[k]) for k in ("S", "harm", "perc", "fv"))
        for i, y in enumerate(clips):
            ref_S = ofe.stft_mag(y, n_fft=cfg.n_fft, win_length=cfg.win_length, hop=cfg.hop)
            _compare_S(S[i], ref_S, (name, tag, i, "S tap"))
            ok = S[i].view(np.uint32) == ref_S.view(np.uint32)
            mh = _window_ok(ok, cfg.l_harm // 2, 1)
            mp = _window_ok(ok, cfg.l_perc // 2, 0)
            rh, rp = ofe.median_time(ref_S, cfg.l_harm), ofe.median_freq(ref_S, cfg.l_perc)
            assert np.array_equal(harm[i][mh], rh[mh]), (name, tag, i, "harm")
            assert np.array_equal(perc[i][mp], rp[mp]), (name, tag, i, "perc")
            _check_fv(fe, fv[i], ref_S, (name, tag, i))


@pytest.mark.parametrize("name", ["LogMelHarmPercSpec", "HarmPercSpec"])
def test_ragged_files_and_a_long_clip_from_the_audio(name):
    fe = _f64(**NAMES[name])
    cfg = fe.cfg
    lens = [16000, 16001, 32161, 47999, 80000, 113337, 160000, 24001]
    clips = [_music(n, 100 + i, silent=(3000, 7000) if i == 2 else None) for i, n in enumerate(lens)]
    T_long = ofe.num_frames(160000, cfg.n_fft, cfg.hop)
    assert fe.lib.smh_internal_frontend_route(fe._h, T_long) == 2, "the 10 s clip takes the streaming kernels"
    rag = fe.run_ragged(clips, W=68, shift=34)
    torch.cuda.synchronize()
    for i, y in enumerate(clips):
        one = fe.run(_dev(y)[None], W=68, shift=34)
        torch.cuda.synchronize()
        assert torch.equal(rag["fv"][i], one["fv"][0]), (name, len(y))
        assert torch.equal(rag["patches"][i], one["patches"]), (name, len(y))
        ref_S = ofe.stft_mag(y, n_fft=cfg.n_fft, win_length=cfg.win_length, hop=cfg.hop)
        _check_fv(fe, _host(one["fv"][0]), ref_S, (name, len(y)))
    # the long clip alone, equal-length route, against its own stft_mag
    S = _host(fe.stft_mag(_dev(clips[6])[None]))[0]
    _compare_S(S, ofe.stft_mag(clips[6], n_fft=cfg.n_fft, win_length=cfg.win_length, hop=cfg.hop), (name, "long"))


def test_featuregram_from_signal_reads_the_params_key():
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    PARAMS = {"Model": "Lemaire_et_al", "Tw": 25, "Ts": 10, "l_harm": {"Lemaire_et_al": 21}, "l_perc": {"Lemaire_et_al": 11}}
    y = _music(27001, 21)
    fv = pp.featuregram_from_signal(PARAMS | {"stft_precision": "f64"}, y, 400, 120, "LogMelHarmPercSpec")
    ref = ofe.featuregram(y, "LogMelHarmPercSpec", n_fft=400, n_mels=120)
    err = float(np.max(np.abs(fv - ref)))
    assert fv.shape == ref.shape and err <= 1e-3, err
    # without the key: the f32 front end, bit for bit what FrontendConfig() gives
    fv32 = pp.featuregram_from_signal(PARAMS, y, 400, 120, "LogMelHarmPercSpec")
    assert np.array_equal(fv32, _host(_fe().run(_dev(y)[None])["fv"][0]))


def test_invalid_precisions_are_rejected():
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    with pytest.raises(ValueError):
        FrontendConfig(stft_precision="f16")
    lib = _lib.require_gpu()
    c = _lib.FrontendCfg(400, 400, 160, 120, 21, 11, 1, 22050.0)
    for p in (-1, 2, 64):
        h = C.c_void_p()
        assert lib.smh_ctx_create_ex(C.byref(c), p, C.byref(h)) == _lib.SMH_E_INVALID
        assert not h.value and "stft_precision" in _lib.last_error()
    # an n_fft whose f64 frame does not fit the kernel's LDS: rejected when the context is created, not run in f32
    with pytest.raises(ValueError, match="f64"):
        Frontend(FrontendConfig(n_fft=4000, win_length=4000, n_mels=0, stft_precision="f64"))


def test_f32_mode_is_the_old_context(clips4):
    """FrontendConfig() and stft_precision="f32" give what a context made by smh_ctx_create gives, on every output."""
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    new = Frontend(FrontendConfig(stft_precision="f32"))
    old = Frontend(FrontendConfig())
    lib = old.lib
    lib.smh_ctx_destroy(old._h)
    c = _lib.FrontendCfg(400, 400, 160, 120, 21, 11, 1, 22050.0)
    h = C.c_void_p()
    _lib.check(lib.smh_ctx_create(C.byref(c), C.byref(h)), "smh_ctx_create")
    old._h = h
    x = _dev(np.concatenate([clips4, _music(16000, 31)[None]]))
    a, b = new.run(x, W=68, shift=68, taps=True), old.run(x, W=68, shift=68, taps=True)
    for k in ("S", "harm", "perc", "fv", "patches"):
        assert torch.equal(a[k], b[k]), k
    clips = [_music(n, 40 + n) for n in (16000, 40001, 120000)]
    ra, rb = new.run_ragged(clips, W=68, shift=68), old.run_ragged(clips, W=68, shift=68)
    for i in range(len(clips)):
        assert torch.equal(ra["fv"][i], rb["fv"][i]) and torch.equal(ra["patches"][i], rb["patches"][i]), i
