"""What the front end's GPU tests share -- TEST INFRASTRUCTURE, a plain module like tests/median_cases.py: the audio written for them
(tones, noise bursts, clicks, near-silence), clip lengths of an exact frame count, and the comparison of `Frontend.run` /
`Frontend.run_ragged` with `oracle.frontend.featuregram_from_S` started from the device's own S at the project's bounds (SURVEY 8d'):
dB features abs 1e-3 dB on every bin; HarmPercSpec abs 1e-6 max|S|; MelHarmPercSpec rel 1e-5 + abs 1e-6 max|S|; patches against the
oracle's scaler and patch grid on the device's featuregram, abs 1e-4.  tests/test_streaming_frontend_gpu.py (routes 2 and 3) and
tests/test_feature_edges_gpu.py (routes 0 and 1) import it."""
import numpy as np
import torch

from oracle import frontend as ofe


def _feat_name(cfg):
    return ("Log" if cfg.log_db else "") + ("Mel" if cfg.n_mels else "") + "HarmPercSpec"


def _route(fe, T):
    return fe.lib.smh_internal_frontend_route(fe._h, T)


def _t_star(fe):
    """The last T before the streaming kernels: from 40 frames up, the route query reports the LDS image (0 / 1) or -- where the
    block-split median has no wave budget for the tile, n_fft = 512 with odd T -- the two-kernel path (3), then 2 from T* + 1 on."""
    routes = {T: _route(fe, T) for T in range(40, 400)}
    assert routes[40] == 0, routes[40]
    first2 = min(T for T, r in routes.items() if r == 2)
    assert all(r in (T & 1, 3) for T, r in routes.items() if T < first2), routes
    assert all(r == 2 for T, r in routes.items() if T >= first2), routes
    return first2 - 1


def _n_samples(cfg, T, odd):
    """A clip length of exactly T frames; `odd` picks an odd number of samples."""
    extra = (37 * T) % (cfg.hop // 2 - 1) * 2 + (1 if odd else 0)
    n = cfg.n_fft + cfg.hop * (T - 1) + extra
    assert ofe.num_frames(n, cfg.n_fft, cfg.hop) == T and n % 2 == (1 if odd else 0)
    return n


def _music(n, seed):
    """Harmonic tone with a tremolo, gated noise bursts and a few clicks (peak about 1)."""
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
    return y.astype(np.float32)


def _quiet(n, seed, amp=1e-5):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _tone(n, f, amp):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / 16000.0)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _check(fe, S, fv, patches, W, shift, tag):
    """fv (2*rows, T) from the device's S (K, T); patches (nP, W, 2*rows) from the device's fv."""
    cfg, name = fe.cfg, _feat_name(fe.cfg)
    ref = ofe.featuregram_from_S(S, name, n_mels=cfg.n_mels, l_harm=cfg.l_harm, l_perc=cfg.l_perc)
    assert fv.shape == ref.shape, (tag, fv.shape, ref.shape)
    smax = float(S.max())
    if cfg.log_db:
        err = float(np.max(np.abs(fv - ref)))
        assert err <= 1e-3, (tag, err, np.unravel_index(np.argmax(np.abs(fv - ref)), fv.shape))
    elif not cfg.n_mels:
        err = float(np.max(np.abs(fv - ref)))
        assert err <= 1e-6 * smax, (tag, err, smax)
    else:
        np.testing.assert_allclose(fv, ref, rtol=1e-5, atol=1e-6 * smax, err_msg=str(tag))
    if W:
        pref = ofe.tcn_input(ofe.feature_patches(fv.astype(np.float32), W, shift, name))
        assert pref.shape == patches.shape, (tag, pref.shape, patches.shape)
        if pref.size:
            err = float(np.max(np.abs(patches - pref)))
            assert err <= 1e-4, (tag, W, shift, err)
    return ref


def _run_both(fe, clips, geoms, routes):
    """Every clip through run_ragged (all at once) and run (alone), for every patch geometry; both against the oracle from the
    clip's own device S.  routes: the route each clip must take."""
    for c, r in zip(clips, routes):
        T = ofe.num_frames(len(c), fe.cfg.n_fft, fe.cfg.hop)
        assert _route(fe, T) == r, (fe.cfg, T, _route(fe, T), r)
    S = [_host(fe.stft_mag(_dev(c)[None]))[0] for c in clips]
    for W, shift in geoms:
        rag = fe.run_ragged(clips, W=W, shift=shift)
        torch.cuda.synchronize()
        for i, c in enumerate(clips):
            one = fe.run(_dev(c)[None], W=W, shift=shift)
            torch.cuda.synchronize()
            assert torch.equal(rag["fv"][i], one["fv"][0]), (fe.cfg, W, len(c))
            assert torch.equal(rag["patches"][i], one["patches"]), (fe.cfg, W, len(c))
            _check(fe, S[i], _host(one["fv"][0]), _host(one["patches"]), W, shift, (fe.cfg, W, shift, len(c)))
    return S
