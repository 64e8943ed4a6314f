"""The image patch layout of the harmonic-percussive front end: `layout="image"` on `Frontend.run`, `features`, `run_ragged` and
`patches_from_featuregram` (patch_layout 0 of smh_frontend_layout_f32 / smh_features_layout_f32 / smh_frontend_ragged_layout_f32).

The yardstick is the unchanged time-major output, which the existing suites pin against the oracle: a patch value is the same f32
number in either layout, so every case asserts `torch.equal(image, time_major.permute(0, 2, 1))` -- no tolerance -- and a
bit-identical featuregram.  One anchor against the oracle's get_feature_patches restatement, at the tolerance
tests/test_parity_gpu.py::test_fused_patches_vs_oracle applies to the time-major patches of the same configuration (atol 1e-4).

Shapes: the smallest at which each store loop can go wrong -- overlapping and abutting patches, T < W (frame index modulo T), W well
above 64, 120 / 201 / 257 / 40 rows per half (201 and 257: no multiple of 64 or of 4), even and odd T (one workgroup per clip half /
per clip), clips beyond the LDS image (the streaming kernels; a last 64-frame chunk that is partial) and the long-clip route of
`features` (a featuregram half beyond one LDS tile)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import frontend as ofe

pytestmark = pytest.mark.gpu

_FES = {}


def _fe(**kw):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    key = tuple(sorted(kw.items()))
    if key not in _FES:
        _FES[key] = Frontend(FrontendConfig(**kw))
    return _FES[key]


def _clips(B, n, seed):
    from sm_hpss_mtl_amd.synth import synth_clips
    return synth_clips(B, seed=seed, n_samples=n)


def _same(img, tm, fv_img, fv_tm, what, n_min=1):
    assert img.shape == (tm.shape[0], tm.shape[2], tm.shape[1]) and img.is_contiguous(), (what, tuple(img.shape), tuple(tm.shape))
    assert img.shape[0] >= n_min, what
    assert torch.equal(fv_img, fv_tm), ("fv", what)
    assert torch.equal(img, tm.permute(0, 2, 1)), ("patches", what)


MEL120, HP400 = dict(), dict(n_mels=0, n_fft=400, log_db=False)
LOGHP512, MEL40 = dict(n_mels=0, n_fft=512, log_db=True), dict(n_mels=40)
# (configuration, samples per clip, W, shift)
EQUAL_CASES = [
    pytest.param(MEL120, 16000, 68, 34, id="1s-mel120-W68-s34"),      # the Doukhan shape: overlapping patches
    pytest.param(MEL120, 16000, 68, 68, id="1s-mel120-W68-s68"),
    pytest.param(MEL120, 16160, 68, 34, id="oddT-mel120-W68-s34"),    # T = 99: one workgroup per clip
    pytest.param(MEL120, 8000, 68, 34, id="0.5s-mel120-tiled"),       # T = 48 < W: tiling, frame index modulo T
    pytest.param(MEL120, 48000, 249, 24, id="3s-mel120-W249-s24"),    # the driver's shape; beyond the LDS image: streaming kernels
    pytest.param(HP400, 16000, 68, 34, id="1s-HarmPercSpec-201rows"),
    pytest.param(LOGHP512, 16000, 68, 34, id="1s-LogHarmPercSpec-257rows"),
    pytest.param(MEL40, 16000, 68, 34, id="1s-mel40"),
]


@pytest.mark.parametrize("cfg,n,W,shift", EQUAL_CASES)
def test_run_image_equals_time_major_transposed(cfg, n, W, shift):
    fe = _fe(**cfg)
    audio = torch.from_numpy(_clips(3, n, seed=11)).cuda()
    tm = fe.run(audio, W=W, shift=shift)
    img = fe.run(audio, W=W, shift=shift, layout="image")
    torch.cuda.synchronize()
    assert img["n_patches"] == tm["n_patches"] and img["patches"].shape == (3 * tm["n_patches"], 2 * fe.rows, W)
    _same(img["patches"], tm["patches"], img["fv"], tm["fv"], (cfg, n, W, shift))


# the stage-by-stage entry (medians as the reference returns them): std_patch_kernel, and -- the last case -- the long-clip route of a
# featuregram half beyond one LDS tile (257 rows x 298 frames)
@pytest.mark.parametrize("cfg,n,W,shift", EQUAL_CASES + [pytest.param(LOGHP512, 48000, 68, 34, id="3s-LogHarmPercSpec-long-clip-route")])
def test_features_image_equals_time_major_transposed(cfg, n, W, shift):
    fe = _fe(**cfg)
    S = fe.stft_mag(torch.from_numpy(_clips(3, n, seed=12)).cuda())
    harm, perc = fe.hpss_median(S)
    tm = fe.features(S, harm, perc, W=W, shift=shift)
    img = fe.features(S, harm, perc, W=W, shift=shift, layout="image")
    torch.cuda.synchronize()
    assert img["n_patches"] == tm["n_patches"]
    _same(img["patches"], tm["patches"], img["fv"], tm["fv"], (cfg, n, W, shift))


def _ragged_lengths(fe, n_fft, W, all_classes):
    """Sample counts of one ragged call, read from the planner (none written down): LDS image with even T and with odd T (both
    longer than a patch; all_classes: the configuration must have them, else they are taken where the planner offers them),
    streaming with a partial last 64-frame chunk, even and odd T; plus a 0.4 s clip (T < W) and a clip of exactly W frames (which
    holds no patch: tools.extract_patches' range(W/2, T - W/2, shift) is empty -- its slot in the buffers stays empty in both
    layouts).  Returns (lens, Ts, number of clips in front of the W-frame one)."""
    lib, h = fe.lib, fe._h
    route = lambda T: lib.smh_internal_frontend_route(h, T)
    first = lambda pred: next((T for T in range(W + 1, 4096) if pred(T)), None)
    image = [T for T in (first(lambda T: route(T) == 0), first(lambda T: route(T) == 1)) if T is not None]
    assert len(image) == 2 or not all_classes, "this configuration must have both LDS-image classes"
    T_long = first(lambda T: not lib.smh_features_blocked_ok(h, T, 0) and T % 64 not in (0, 63))
    Ts = image + [T_long, T_long + 1, lib.smh_num_frames(6400, n_fft, 160), W]
    assert route(T_long) == 2 and route(T_long + 1) == 2, "the long clips must take the streaming kernels"
    assert T_long % 64 != 0 and (T_long + 1) % 64 != 0 and Ts[-2] < W
    assert {route(T) for T in Ts} >= ({0, 1, 2} if all_classes else {2})
    lens = [n_fft + (T - 1) * 160 for T in Ts]
    assert [lib.smh_num_frames(n, n_fft, 160) for n in lens] == Ts
    return lens, Ts, len(Ts) - 1


@pytest.mark.parametrize("cfg,shift", [pytest.param(MEL120, 34, id="mel120-s34"), pytest.param(MEL120, 68, id="mel120-s68"),
                                       pytest.param(LOGHP512, 34, id="LogHarmPercSpec512-s34")])
def test_ragged_image_equals_time_major_and_every_clip_alone(cfg, shift):
    W = 68
    fe = _fe(**cfg)
    lens, Ts, n_full = _ragged_lengths(fe, fe.cfg.n_fft, W, all_classes=cfg is MEL120)
    clips = [_clips(1, n, seed=70 + i)[0] for i, n in enumerate(lens)]
    tm = fe.run_ragged(clips, W=W, shift=shift)
    img = fe.run_ragged(clips, W=W, shift=shift, layout="image")
    torch.cuda.synchronize()
    assert img["T"] == tm["T"] == Ts and img["n_patches"] == tm["n_patches"]
    assert min(tm["n_patches"][:n_full]) >= 1 and tm["n_patches"][n_full] == 0
    for i, c in enumerate(clips):
        _same(img["patches"][i], tm["patches"][i], img["fv"][i], tm["fv"][i], (cfg, shift, i, Ts[i]), n_min=1 if i < n_full else 0)
        one = fe.run(torch.from_numpy(c).cuda()[None], W=W, shift=shift, layout="image")
        assert torch.equal(img["patches"][i], one["patches"]) and torch.equal(img["fv"][i], one["fv"][0]), (cfg, shift, i, Ts[i])


def test_patches_from_featuregram_image():
    fe = _fe()
    fv = fe.run(torch.from_numpy(_clips(1, 20000, seed=5)).cuda())["fv"][0]
    for W, shift in ((68, 34), (249, 24)):  # (the second: T = 123 < W, tiled)
        tm = fe.patches_from_featuregram(fv, W, shift)
        img = fe.patches_from_featuregram(fv, W, shift, layout="image")
        assert img.shape == (tm.shape[0], 240, W) and tm.shape[0] > 0 and torch.equal(img, tm.permute(0, 2, 1))


def test_no_patches_and_invalid_layout():
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import _ptr, _stream
    fe = _fe()
    clips = _clips(2, 16000, seed=3)
    audio = torch.from_numpy(clips).cuda()
    ref = fe.run(audio)
    res = fe.run(audio, layout="image")  # no W: no patches
    assert res["n_patches"] == 0 and "patches" not in res and torch.equal(res["fv"], ref["fv"])
    rag = fe.run_ragged([clips[0], clips[1][:9000]], layout="image")
    assert rag["n_patches"] == [0, 0] and "patches" not in rag and torch.equal(rag["fv"][0], ref["fv"][0])
    S = fe.stft_mag(audio)
    harm, perc = fe.hpss_median(S)
    assert fe.features(S, harm, perc, layout="image")["patches"] is None
    for call in (lambda: fe.run(audio, W=68, shift=34, layout="nhwc"), lambda: fe.run_ragged([clips[0]], W=68, shift=34, layout=0),
                 lambda: fe.features(S, harm, perc, W=68, shift=34, layout="images"),
                 lambda: fe.patches_from_featuregram(ref["fv"][0], 68, 34, layout=None)):
        with pytest.raises(ValueError, match="layout"):
            call()
    # the C entries: SMH_E_INVALID with a text, and nothing launched -- the outputs keep their fill
    lib, h = fe.lib, fe._h
    B, N, T, W = 2, 16000, 98, 68
    nP = fe.num_patches(T, W, 34)
    fv = torch.full((B, 240, T), -7.0, device="cuda")
    pt = torch.full((B * nP, W, 240), -7.0, device="cuda")
    wk = torch.empty(lib.smh_frontend_workspace_bytes(h, B, N), dtype=torch.uint8, device="cuda")
    keys = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
    h_off, h_len = (C.c_longlong * B)(0, N), (C.c_int * B)(N, N)
    for bad in (2, -1):
        rcs = [lib.smh_frontend_layout_f32(h, _ptr(audio), B, N, W, 34, bad, _ptr(fv), _ptr(pt), _ptr(wk), wk.numel(), None, None, None,
                                           _stream()),
               lib.smh_features_layout_f32(h, _ptr(S), _ptr(harm), _ptr(perc), 0, B, T, W, 34, bad, _ptr(fv), _ptr(pt), _ptr(keys),
                                           _stream()),
               lib.smh_frontend_ragged_layout_f32(h, _ptr(audio), h_off, h_len, B, W, 34, bad, _ptr(fv), _ptr(pt), _ptr(wk), wk.numel(),
                                                  _stream())]
        for rc in rcs:
            assert rc == _lib.SMH_E_INVALID
        assert "patch_layout" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((fv == -7.0).all()) and bool((pt == -7.0).all())


def test_image_patches_against_the_oracle():
    """One-second clips, 120 mels: the image patches against oracle.frontend.feature_patches -- get_feature_patches' '*HarmPerc*'
    branch, (nP, 2F, W) -- on the device's own featuregram, at test_fused_patches_vs_oracle's atol of 1e-4."""
    fe = _fe()
    W, shift = 68, 34
    res = fe.run(torch.from_numpy(_clips(3, 16000, seed=11)).cuda(), W=W, shift=shift, layout="image")
    torch.cuda.synchronize()
    fv, patches, nP = res["fv"].cpu().numpy(), res["patches"].cpu().numpy(), res["n_patches"]
    assert patches.shape == (3 * nP, 240, W)
    for i in range(3):
        ref = ofe.feature_patches(fv[i], W, shift, "LogMelHarmPercSpec")
        assert ref.shape == (nP, 240, W)
        np.testing.assert_allclose(patches[i * nP:(i + 1) * nP], ref, atol=1e-4)
