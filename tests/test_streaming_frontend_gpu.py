"""The front end's long-clip path against the oracle on every bin.

Clips whose featuregram does not fit one LDS image (T > T*, about 1.6 s at 240 rows) take the three streaming kernels of
csrc/smh_ragged.hip (rag_walk_kernel, rag_stats_kernel, rag_final_kernel), in `Frontend.run` (equal clips, smh_rag::run_equal)
and in `Frontend.run_ragged` alike.  Every case here asserts the route it claims with `smh_internal_frontend_route` and compares
both calls with `oracle.frontend.featuregram_from_S` started from the device's own S of the clip (`Frontend.stft_mag`: the kernel
the fused calls use), so the medians are selections of identical values and what remains is the arithmetic of masks, mel, dB,
top-dB floor and scaler:
  * dB features: abs 1e-3 dB on every bin;
  * HarmPercSpec (H, P themselves): abs 1e-6 max|S|;
  * MelHarmPercSpec: rel 1e-5 of the value, abs 1e-6 max|S|;
  * patches: against the oracle's scaler and patch grid on the device's featuregram, abs 1e-4.
The audio is written here and in tests/frontend_helpers.py (tones, noise bursts, clicks, bursts placed on chunk boundaries,
near-silence, digital silence); the helpers are shared with tests/test_feature_edges_gpu.py, which holds routes 0 and 1.
"""
import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests.frontend_helpers import _check, _dev, _host, _music, _n_samples, _quiet, _route, _run_both, _t_star, _tone

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float32).tiny


def _frontend(cfg):
    from sm_hpss_mtl_amd.frontend import Frontend
    return Frontend(cfg)


# ---------------------------------------------------------------------------------------------------------------------------
# boundary and chunk lengths across configurations
# ---------------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from sm_hpss_mtl_amd.frontend import FrontendConfig
    return FrontendConfig(**kw)


CONFIGS = {
    "default": (dict(), ((68, 34), (99, 34), (5, 1))),
    "17x17": (dict(l_harm=17, l_perc=17), ((68, 68),)),
    "LogHarmPercSpec": (dict(n_mels=0), ((68, 34),)),
    "MelHarmPercSpec": (dict(log_db=False), ((68, 68),)),
    "HarmPercSpec": (dict(n_mels=0, log_db=False), ((68, 34),)),
    "n_fft512": (dict(n_fft=512, n_mels=0), ((68, 68),)),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_boundary_and_chunk_lengths_against_the_oracle(name):
    """T*-1 .. T*+2 (both parities across the switch to the streaming kernels), the 128-frame walk and 64-frame final chunk
    boundaries 255-257 and 383-385, T = 1 (mod 64) and a clip of a few thousand frames; odd and even numbers of samples."""
    kw, geoms = CONFIGS[name]
    cfg = _cfg(**kw)
    fe = _frontend(cfg)
    ts = _t_star(fe)
    Ts = [ts - 1, ts, ts + 1, ts + 2, 255, 256, 257, 383, 384, 385, 449, 3009 if name == "default" else 2113]
    assert all(T % 64 == 1 for T in Ts[-2:])
    clips = [_music(_n_samples(cfg, T, odd=i % 2 == 1), seed=100 + i) for i, T in enumerate(Ts)]
    routes = [(_route(fe, T) if _route(fe, T) == 3 else T & 1) if T <= ts else 2 for T in Ts]  # (3 only as _t_star allows it)
    _run_both(fe, clips, geoms, routes)


def test_window_pair_without_a_streaming_kernel_takes_the_two_kernel_path():
    """(l_harm, l_perc) = (11, 31) has a pair median kernel but no block-split one: no ragged median, no LDS-image features, so
    every length takes route 3 (launch_hp_feat + launch_std_patch over the whole clip) -- in run_ragged clip by clip."""
    cfg = _cfg(l_harm=11, l_perc=31)
    fe = _frontend(cfg)
    Ts = [60, 165, 166, 257, 385, 1025]
    clips = [_music(_n_samples(cfg, T, odd=i % 2 == 0), seed=200 + i) for i, T in enumerate(Ts)]
    _run_both(fe, clips, ((68, 34), (99, 34)), [3] * len(Ts))


def test_tile_if_short_and_dense_patches_on_streamed_clips():
    """W = 249 on clips of T* < T < 249 frames: tile-if-short inside rag_final_kernel (a frame sits in the tiled featuregram more than
    once); W = 5, shift = 1: every frame belongs to five patches (rag_final_kernel's p_lo / p_hi bounds)."""
    cfg = _cfg()
    fe = _frontend(cfg)
    ts = _t_star(fe)
    Ts = [ts + 1, ts + 2, 200, 247, 248]
    assert all(ts < T < 249 for T in Ts)
    clips = [_music(_n_samples(cfg, T, odd=i % 2 == 0), seed=300 + i) for i, T in enumerate(Ts)]
    _run_both(fe, clips, ((249, 24), (5, 1)), [2] * len(Ts))


# ---------------------------------------------------------------------------------------------------------------------------
# signal edges
# ---------------------------------------------------------------------------------------------------------------------------


def test_burst_in_the_lone_last_frame_and_in_the_last_walk_chunk():
    """The maximum of each half's array sits in the last frame of an odd-T clip -- the lone frame the walk pairs with itself, alone in
    the last 128-frame chunk (T = 385) -- or inside the last partial chunk of an even-T clip (T = 300).  Everything else is 100 dB
    down, so the top-dB floor (which follows the per-array atomicMax over the chunks) decides almost every bin."""
    cfg = _cfg()
    fe = _frontend(cfg)
    clips = []
    T = 385
    n = _n_samples(cfg, T, odd=True)
    y = _quiet(n, 1)
    s0 = cfg.hop * (T - 1) + (cfg.n_fft - cfg.hop)  # samples from here on belong to frame T - 1 only
    s1 = cfg.hop * (T - 1) + cfg.n_fft
    y[s0:s1] += _tone(s1 - s0, 1000.0, 0.5)[:s1 - s0] + _tone(s1 - s0, 3100.0, 0.3)
    clips.append(y)
    T2 = 300
    n2 = _n_samples(cfg, T2, odd=False)
    y2 = _quiet(n2, 2)
    a, b = cfg.hop * 270, cfg.hop * 280
    y2[a:b] += _tone(b - a, 440.0, 0.5) + _tone(b - a, 2500.0, 0.2)
    y2[cfg.hop * 275] += 0.8  # and a click
    clips.append(y2)
    S = _run_both(fe, clips, ((68, 34),), [2, 2])
    # the premise: the array's maximum lies in the last frame / the last walk chunk only (the one-frame burst has no harmonic part
    # above amin: its H array is -100 dB throughout, so only its P array counts)
    for i, (Ti, lo, halves) in enumerate(((T, T - 1, (1,)), (T2, 256, (0, 1)))):
        ref = ofe.featuregram_from_S(S[i], "LogMelHarmPercSpec")
        for h in (ref[120 * k:120 * (k + 1)] for k in halves):
            assert h[:, lo:].max() > h[:, :lo].max() + 10.0, (Ti, float(h[:, lo:].max()), float(h[:, :lo].max()))
            assert np.mean(h <= h.max() - 80.0 + 1e-4) > 0.5  # the floor is active on most bins


def test_near_silence_with_one_loud_second_activates_the_top_db_floor():
    cfg = _cfg()
    fe = _frontend(cfg)
    T = 601
    n = _n_samples(cfg, T, odd=True)
    y = _quiet(n, 3, amp=1e-6)
    a = cfg.hop * 250
    y[a:a + 16000] += _music(16000, seed=4)
    S = _run_both(fe, [y], ((68, 34),), [2])
    fv = _host(fe.run(_dev(y)[None])["fv"][0])
    ref = ofe.featuregram_from_S(S[0], "LogMelHarmPercSpec")
    for g, r in ((fv[:120], ref[:120]), (fv[120:], ref[120:])):
        assert np.mean(r <= r.max() - 80.0 + 1e-4) > 0.3  # the premise: the floor is active on many bins
        assert float(g.min()) >= float(g.max()) - 80.0 - 1e-3
        assert abs(float(g.max()) - float(r.max())) <= 1e-3


@pytest.mark.parametrize("kw", [dict(n_mels=0, log_db=False), dict(log_db=False)], ids=["HarmPercSpec", "MelHarmPercSpec"])
def test_tiny_tone_bursts_in_digital_silence_take_the_split_zeros_rule(kw):
    """Digital silence with 20 bursts of 1e-19 amplitude, 800 samples each, every one a tone at the centre of an FFT bin.  In a frame
    that lies inside a burst the Hann-windowed tone has three non-zero bins (k - 1, k, k + 1, about 1e-17); the rest is rounding
    noise whose square underflows in the STFT's |re + i im|, so S is exactly 0 there.  At those three bins S > 0 while both medians
    are 0 (8 of 11 bins and more than 10 of 21 frames are 0): librosa's softmask gives both masks 0.5 (split_zeros).  Linear
    features, so a mask of 0 instead would show."""
    cfg = _cfg(**kw)
    fe = _frontend(cfg)
    T = 401
    n = _n_samples(cfg, T, odd=True)
    y = np.zeros(n, np.float32)
    t = np.arange(800) / 16000.0
    for j, start in enumerate(range(2000, n - 2000, 3100)):
        k = 5 + 9 * j  # bin k: 40 k Hz
        y[start:start + 800] = (1e-19 * np.sin(2 * np.pi * 40.0 * k * t)).astype(np.float32)
    S = _run_both(fe, [y], ((68, 34),), [2])[0]
    harm, perc = ofe.median_time(S, cfg.l_harm), ofe.median_freq(S, cfg.l_perc)
    split = (S > 0) & (harm < TINY) & (perc < TINY)
    assert split.sum() >= 100, int(split.sum())  # the premise, on the device's own S


def test_all_zero_clip_gives_constant_rows_and_zero_patches():
    """Every row is -100 dB: constant, so the scaler leaves it unscaled (sklearn's _is_constant_feature / _handle_zeros_in_scale,
    what the oracle restates) and every standardised value is exactly 0."""
    cfg = _cfg()
    fe = _frontend(cfg)
    T = 300
    y = np.zeros(_n_samples(cfg, T, odd=True), np.float32)
    _run_both(fe, [y], ((68, 34),), [2])
    r = fe.run(_dev(y)[None], W=68, shift=34)
    rag = fe.run_ragged([y], W=68, shift=34)
    fv, pt = _host(r["fv"]), _host(r["patches"])
    assert np.all(np.abs(fv + 100.0) <= 1e-3)
    assert pt.shape[0] > 0 and np.all(pt == 0.0) and np.all(_host(rag["patches"][0]) == 0.0)


def test_unaligned_equal_batch_matches_each_clip_alone():
    """B = 3 equal clips of an odd number of samples: clips 1 and 2 start on 4-byte boundaries, so the batch takes the generic STFT
    kernel (aligned8 = false).  Every clip is bit-equal to its own B = 1 run on a clip that starts 4 bytes past an 8-byte boundary
    (the same STFT kernel; the specialised kernel an aligned clip gets differs from it in the last bits of S) and within tolerance of
    the oracle from the batch's own S."""
    cfg = _cfg()
    fe = _frontend(cfg)
    T = 1001
    n = _n_samples(cfg, T, odd=True)
    y = np.stack([_music(n, seed=400 + i) for i in range(3)])
    assert _route(fe, T) == 2
    res = fe.run(_dev(y), W=68, shift=34)
    S = _host(fe.stft_mag(_dev(y)))
    nP = res["n_patches"]
    fv, pt = _host(res["fv"]), _host(res["patches"])
    for i in range(3):
        buf = torch.zeros(n + 1, device="cuda")
        clip = buf[1:]
        clip.copy_(_dev(y[i]))
        assert clip.data_ptr() % 8 == 4
        one = fe.run(clip[None], W=68, shift=34)
        assert torch.equal(one["fv"][0], res["fv"][i]) and torch.equal(one["patches"], res["patches"][i * nP:(i + 1) * nP]), i
        _check(fe, S[i], fv[i], pt[i * nP:(i + 1) * nP], 68, 34, ("batch", i))


def test_sixty_second_clip_against_the_oracle():
    """T = 5998: the f64 row statistics over thousands of frames under the 1e-4 patch check, 47 walk chunks, 94 final chunks."""
    cfg = _cfg()
    fe = _frontend(cfg)
    y = _music(960000, seed=500)
    _run_both(fe, [y], ((68, 34),), [2])


def test_route_beyond_the_streaming_kernels_offset_bound():
    """rag_clip_ok keeps a clip's rows within 32-bit offsets: K * T and 2 * rows * T below 2^29 elements.  Beyond it the route is 3
    (not allocated here: several hours of audio)."""
    fe = _frontend(_cfg())
    K, rows = fe.K, fe.rows
    T_max = min(((1 << 29) - 1) // (K + 16), ((1 << 29) - 1) // (2 * rows))
    assert _route(fe, T_max) == 2 and _route(fe, T_max + 1) == 3 and _route(fe, 1 << 30) == 3
    assert _route(fe, 0) == -1
