"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on identical seeded inputs,
against the committed golden vectors, and -- at BASELINE's full batch -- through size-independent
properties.  Tolerances are SURVEY 8(d'): bit-exact for selection/indexing, stated fp32 bounds elsewhere."""
import numpy as np
import pytest
import torch

from oracle import b3_mtl, frontend as ofe
from tests.conftest import checks

pytestmark = pytest.mark.gpu


def _skip_if_forced(*names):
    """A test that asserts WHICH implementation ran (not what it computed) has nothing to say when an environment switch forces
    another one (tools/gpu/r*_variants.sh run the suites under such switches): skipped there, not failed."""
    import os
    forced = [n for n in names if os.environ.get(n)]
    if forced:
        pytest.skip("implementation forced by " + ", ".join(forced))


@pytest.fixture(scope="module")
def fe():
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    return Frontend(FrontendConfig())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------
# a1 STFT
# ---------------------------------------------------------------------------------------------------
def test_stft_mag_vs_oracle(fe, clips4, golden_fe):
    S = host(fe.stft_mag(dev(clips4)))
    assert S.shape == (4, 201, 98) and S.dtype == np.float32  # frame count is an integer contract
    for i in range(4):
        ref = ofe.stft_mag(clips4[i])
        assert np.max(np.abs(S[i] - ref)) <= 1e-5 * ref.max()  # rel 1e-5 of max|S| per clip
    assert np.max(np.abs(S[0] - golden_fe["S"])) <= 1e-5 * golden_fe["S"].max()


@pytest.mark.parametrize("n_fft", [400, 512])
@pytest.mark.parametrize("B", [1, 3, 8, 9, 21, 67])
def test_stft_xcd_grid_equals_plain_grid_at_any_batch(B, n_fft, monkeypatch):
    """The 1-D grid that keeps neighbouring frame tiles on one XCD (csrc/smh_stft.hip) decodes (clip, tile) from the workgroup index:
    the (clip, tile) items are cut into 8 contiguous ranges, and item counts that are not multiples of 8 leave workgroups without an
    item.  Same bits as the plain (tile, clip) grid, every clip within 1e-5 max|S| of the oracle, nothing written behind the batch."""
    import ctypes as C
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.synth import synth_clips
    y = synth_clips(B, seed=77)[:, :7000 + 160 * (B % 5)]  # 40-44 frames: 2-4 tiles, the last one short
    f = Frontend(FrontendConfig() if n_fft == 400 else FrontendConfig(n_fft=512, win_length=400, n_mels=0, log_db=True))  # 512: the generic kernel
    T = f.num_frames(y.shape[1])
    buf = torch.full((B + 1, f.K, T), -7.0, device="cuda")  # one guard clip behind the batch
    lib, st = f.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ya = dev(y)

    def run():
        buf.fill_(-7.0)
        _lib.check(lib.smh_stft_mag_f32(f._h, C.c_void_p(ya.data_ptr()), B, y.shape[1], C.c_void_p(buf.data_ptr()), st))
        return buf.clone()

    monkeypatch.setenv("SMH_STFT_XCD", "1")
    got = run()
    monkeypatch.setenv("SMH_STFT_XCD", "0")
    plain = run()
    assert torch.equal(got, plain)
    assert bool((got[B] == -7.0).all())
    Sh = host(got[:B])
    for i in range(B):
        ref = ofe.stft_mag(y[i]) if n_fft == 400 else ofe.stft_mag(y[i], n_fft=512, win_length=400, hop=160)
        assert Sh[i].shape == ref.shape and np.max(np.abs(Sh[i] - ref)) <= 1e-5 * ref.max()


def test_stft_other_lengths_and_nfft(clips4):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    f512 = Frontend(FrontendConfig(n_fft=512, win_length=400, n_mels=0, log_db=True))  # Jang: zero-padded window
    y = clips4[:2, :5000]
    S = host(f512.stft_mag(dev(y)))
    assert S.shape == (2, 257, 1 + (5000 - 512) // 160)
    for i in range(2):
        ref = ofe.stft_mag(y[i], n_fft=512, win_length=400, hop=160)
        assert np.max(np.abs(S[i] - ref)) <= 1e-5 * ref.max()
    with pytest.raises(ValueError):
        f512.stft_mag(dev(clips4[:1, :300]))  # shorter than n_fft


# ---------------------------------------------------------------------------------------------------
# a2 median filters: bit-exact selection
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lh,lp", [(21, 11), (17, 17), (11, 51), (31, 31), (13, 7), (3, 63)])
def test_hpss_median_bit_exact(fe, clips4, lh, lp):
    S = np.stack([ofe.stft_mag(c) for c in clips4])
    harm, perc = fe.hpss_median(dev(S), lh, lp)
    harm, perc = host(harm), host(perc)
    for i in range(4):
        assert np.array_equal(harm[i], ofe.median_time(S[i], lh)), "harm differs"
        assert np.array_equal(perc[i], ofe.median_freq(S[i], lp)), "perc differs"


@pytest.mark.parametrize("lh,lp,B,persist", [(17, 17, 1024, None), (21, 11, 1024, None), (17, 17, 515, "1"),
                                              (11, 21, 700, None), (21, 21, 513, None), (21, 11, 1024, "0")])
def test_hpss_median_large_batch_bit_exact(fe, lh, lp, B, persist, monkeypatch):
    """Batches of at least two clips per CU: windows above 17 take the persistent double-buffered kernel (LDS-DMA
    tile loads, clips that start on 8-byte boundaries, uneven clips per workgroup), the others the ordinary
    block-split kernel; SMH_MEDIAN_PERSIST forces either.  Every clip must be bit-exact."""
    if persist is not None:
        monkeypatch.setenv("SMH_MEDIAN_PERSIST", persist)
    from sm_hpss_mtl_amd.synth import synth_clips
    base = synth_clips(24, seed=77)
    Sb = np.stack([ofe.stft_mag(c) for c in base])
    idx = (np.arange(B) * 7) % 24  # clip b is base clip idx[b]
    S = dev(Sb[idx])
    harm, perc = fe.hpss_median(S, lh, lp)
    ref_h = dev(np.stack([ofe.median_time(x, lh) for x in Sb]))
    ref_p = dev(np.stack([ofe.median_freq(x, lp) for x in Sb]))
    sel = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    assert torch.equal(harm, ref_h[sel]), "harm differs"
    assert torch.equal(perc, ref_p[sel]), "perc differs"
    # time-major harmonic output of the fused pipeline
    h2, p2 = torch.empty_like(S), torch.empty_like(S)
    import ctypes as C
    from sm_hpss_mtl_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lay = _lib.check(fe.lib.smh_hpss_median_ex_f32(fe._h, ptr(S), B, 201, 98, lh, lp, ptr(h2), ptr(p2), 1,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert lay == 1
    assert torch.equal(h2.view(B, 98, 201), ref_h[sel].transpose(1, 2)) and torch.equal(p2, ref_p[sel])


def test_median_golden_scipy(fe, golden_fe):
    S = golden_fe["S"][None]
    harm, perc = fe.hpss_median(dev(S), 21, 11)
    assert np.array_equal(host(harm)[0], golden_fe["harm_21"])  # scipy.ndimage.median_filter outputs
    assert np.array_equal(host(perc)[0], golden_fe["perc_11"])
    h17, p17 = fe.hpss_median(dev(S), 17, 17)
    assert np.array_equal(host(h17)[0][::25], golden_fe["harm_17_rows"])
    assert np.array_equal(host(p17)[0][::25], golden_fe["perc_17_rows"])
    assert np.allclose(checks(host(h17)[0]), golden_fe["harm_17_check"], rtol=1e-12)


@pytest.mark.parametrize("K,T", [(201, 98), (257, 97), (201, 1000), (201, 37), (40, 300), (201, 5), (3, 98), (1, 1)])
def test_median_ragged_shapes_ties_and_tiny_axes(fe, K, T):
    """Long files (frame tiling + halo), odd sizes, heavy ties and axes shorter than the window."""
    rng = np.random.default_rng(K * 1000 + T)
    S = np.abs(rng.standard_normal((2, K, T))).astype(np.float32)
    S[0] = np.round(S[0] * 4) / 4  # many exact ties
    S[1, : max(1, K // 3)] = 0.0  # zero rows (split_zeros territory)
    for w in (21, 11):
        ht = host(fe.median_time(dev(S), w))
        pf = host(fe.median_freq(dev(S), w))
        for i in range(2):
            assert np.array_equal(ht[i], ofe.median_time(S[i], w)), ("time", K, T, w)
            assert np.array_equal(pf[i], ofe.median_freq(S[i], w)), ("freq", K, T, w)


def test_median_randomised_shapes_and_windows(fe):
    """40 seeded random (K, T, l_harm, l_perc, B) draws: pairs and single filters, block-split / persistent / delete-
    insert / rank-counting kernels, one- and multi-tile clips, batches on both sides of the persistent threshold."""
    rng = np.random.default_rng(2024)
    wins = [3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 31, 41, 63]
    for trial in range(40):
        K, T = int(rng.integers(2, 300)), int(rng.integers(2, 420))
        lh, lp = int(rng.choice(wins)), int(rng.choice(wins))
        if trial % 5 == 0:
            lh, lp = [(21, 11), (17, 17), (11, 21), (21, 21), (11, 11)][(trial // 5) % 5]  # fused pair kernels
        B = int(rng.choice([1, 2, 3, 600])) if K * T < 12000 else int(rng.choice([1, 2]))
        S = np.abs(rng.standard_normal((min(B, 3), K, T))).astype(np.float32)
        if trial % 3 == 0:
            S = np.round(S * 3) / 3  # ties
        Sd = dev(S[np.arange(B) % S.shape[0]])
        harm, perc = fe.hpss_median(Sd, lh, lp)
        harm, perc = host(harm), host(perc)
        for i in {0, B // 2, B - 1}:
            ref = S[i % S.shape[0]]
            assert np.array_equal(harm[i], ofe.median_time(ref, lh)), ("harm", trial, K, T, lh, lp, B, i)
            assert np.array_equal(perc[i], ofe.median_freq(ref, lp)), ("perc", trial, K, T, lh, lp, B, i)


def test_median_rejects_bad_windows(fe):
    S = dev(np.ones((1, 20, 20), np.float32))
    with pytest.raises(ValueError):
        fe.median_time(S, 4)  # even
    with pytest.raises(ValueError):
        fe.median_freq(S, 65)  # > SMH_MAX_MEDIAN
    assert fe.median_time(torch.empty((0, 20, 20), device="cuda"), 5).shape == (0, 20, 20)  # empty batch


# ---------------------------------------------------------------------------------------------------
# a3-a6 masks, mel, dB, featuregram
# ---------------------------------------------------------------------------------------------------
def test_softmask_bit_exact_given_inputs(fe, golden_fe):
    S, harm, perc = golden_fe["S"], golden_fe["harm_21"], golden_fe["perc_11"]
    S2 = np.stack([S, S]); h2 = np.stack([harm, harm]); p2 = np.stack([perc, perc])
    h2[1, :3] = 0; p2[1, :3] = 0  # both below tiny -> mask 0.5 each
    H, P = fe.softmask(dev(S2), dev(h2), dev(p2))
    H, P = host(H), host(P)
    for i in range(2):
        mh, mp = ofe.softmask(h2[i], p2[i]), ofe.softmask(p2[i], h2[i])
        assert np.array_equal(H[i], S2[i] * mh) and np.array_equal(P[i], S2[i] * mp)  # same f32 op order
    assert np.array_equal(H[0], golden_fe["H"]) and np.array_equal(P[0], golden_fe["P"])
    assert np.all(np.abs(H + P - S2) <= 2 * np.spacing(S2) + 1e-30)


def test_mel_basis_and_projection(fe, golden_fe):
    B = fe.mel_basis()
    assert B.shape == (120, 201)
    np.testing.assert_allclose(B, golden_fe["mel_basis"], rtol=2e-7, atol=0)  # same float64 construction
    assert np.array_equal(B == 0, golden_fe["mel_basis"] == 0)
    Y = host(fe.mel(dev(golden_fe["H"][None])))[0]
    ref = ofe.mel_project(golden_fe["H"], 120)
    np.testing.assert_allclose(Y, ref, rtol=1e-5, atol=1e-6 * ref.max())


def test_power_to_db(fe):
    rng = np.random.default_rng(2)
    X = np.abs(rng.standard_normal((3, 120, 98))).astype(np.float32) * np.float32(10.0) ** rng.uniform(-8, 2, (3, 1, 1)).astype(np.float32)
    X[0, 0] = 0  # hits amin
    Y = host(fe.power_to_db_sq(dev(X)))
    for i in range(3):
        ref = ofe.power_to_db(X[i] ** 2)
        np.testing.assert_allclose(Y[i], ref, atol=1e-3)  # abs 1e-3 dB
        assert abs(Y[i].min() - (Y[i].max() - 80)) < 1e-3 or Y[i].min() > Y[i].max() - 80


@pytest.mark.parametrize("feat", ["LogMelHarmPercSpec", "MelHarmPercSpec", "HarmPercSpec", "LogHarmPercSpec"])
def test_featuregram_fused_vs_oracle(clips4, feat):
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    PARAMS = {"Tw": 25, "Ts": 10, "Model": "Lemaire_et_al_MTL", "l_harm": {"Lemaire_et_al_MTL": 21},
              "l_perc": {"Lemaire_et_al_MTL": 11}, "frame_level_scaling": False}
    res = pp.featuregram_batch(PARAMS, dev(clips4), 400, 120, feat, taps=True)
    fv, S, harm, perc = host(res["fv"]), host(res["S"]), host(res["harm"]), host(res["perc"])
    for i in range(4):
        ref, p = ofe.featuregram(clips4[i], feat, return_parts=True)
        assert fv[i].shape == ref.shape and fv.dtype == np.float32
        # medians are exact selections of the GPU's own S
        assert np.array_equal(harm[i], ofe.median_time(S[i], 21)) and np.array_equal(perc[i], ofe.median_freq(S[i], 11))
        if feat.startswith("Log"):
            # (1) SURVEY 8(d'): abs 1e-3 dB on EVERY bin against the oracle started from the device's own S -- the medians are
            # then selections of identical values, what remains is the arithmetic of masks / mel / dB
            ref_s = ofe.featuregram_from_S(S[i], feat, n_mels=120, l_harm=21, l_perc=11)
            assert np.max(np.abs(fv[i] - ref_s)) <= 1e-3, (feat, float(np.max(np.abs(fv[i] - ref_s))))
            # (2) end to end from the audio (oracle: numpy's f64 FFT): the device's f32 STFT differs in the last bits, a few
            # medians then select a neighbouring value and those bins move by up to 2e-2 dB; 98 % of the bins stay within 1e-3
            half = ref.shape[0] // 2
            for a, b in ((fv[i][:half], ref[:half]), (fv[i][half:], ref[half:])):
                floor = b.max() - 80
                free = (b > floor + 0.05) & (a > floor + 0.05)
                assert np.max(np.abs(a[free] - b[free])) < 2e-2, feat
                assert np.mean(np.abs(a - b) < 1e-3) > 0.98
                assert abs(a.max() - b.max()) < 1e-3
        else:
            # the three non-log feature names (the inputs of Doukhan / Papakostas / Jang).  (1) SURVEY 8(d') from the DEVICE's
            # own S (identical median selections): masks / H / P abs 1e-6 max|S| ("HarmPercSpec" = H, P themselves), mel rel
            # 1e-5 (of the row scale: a mel row sums up to 11 masked bins)
            ref_s = ofe.featuregram_from_S(S[i], feat, n_mels=120, l_harm=21, l_perc=11)
            smax = float(S[i].max())
            if feat == "HarmPercSpec":
                assert np.max(np.abs(fv[i] - ref_s)) <= 1e-6 * smax, (feat, float(np.max(np.abs(fv[i] - ref_s))) / smax)
            else:
                np.testing.assert_allclose(fv[i], ref_s, rtol=1e-5, atol=1e-6 * smax)
            # (2) end to end from the audio (a few medians select a neighbouring value of the f32 STFT)
            np.testing.assert_allclose(fv[i], ref, rtol=2e-4, atol=2e-5 * p["S"].max())


def test_featuregram_golden_and_per_file_wrapper(clips4, golden_fe, tmp_path):
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    PARAMS = {"Tw": 25, "Ts": 10, "Model": "Lemaire_et_al_MTL", "l_harm": {"Lemaire_et_al_MTL": 21},
              "l_perc": {"Lemaire_et_al_MTL": 11}, "frame_level_scaling": False}
    fv = pp.featuregram_from_signal(PARAMS, clips4[0], 400, 120, "LogMelHarmPercSpec")
    assert fv.shape == (240, 98) and fv.dtype == np.float32
    # end to end from the audio against the committed oracle featuregram: the same pair of bounds as
    # test_featuregram_fused_vs_oracle (2): 98 % of the bins within 1e-3 dB, every bin off the top-dB floor within 2e-2 dB
    g = golden_fe["fv"]
    assert np.mean(np.abs(fv - g) < 1e-3) > 0.98
    for a, b in ((fv[:120], g[:120]), (fv[120:], g[120:])):
        floor = b.max() - 80
        free = (b > floor + 0.05) & (a > floor + 0.05)
        assert np.max(np.abs(a[free] - b[free])) < 2e-2 and abs(a.max() - b.max()) < 1e-3
    # file-based call + the reference's .npy cache layout
    wav = tmp_path / "clipA.npy"
    np.save(wav, clips4[0])
    a = pp.get_featuregram(PARAMS, "music", str(tmp_path / "feat"), "", str(wav), None, 400, 120, "LogMelHarmPercSpec")
    assert (tmp_path / "feat" / "music" / "clipA.npy").exists()
    b = pp.get_featuregram(PARAMS, "music", str(tmp_path / "feat"), "", str(wav), None, 400, 120, "LogMelHarmPercSpec")
    assert np.array_equal(a, b) and np.max(np.abs(a - fv)) < 1e-3


# ---------------------------------------------------------------------------------------------------
# a7-a9 standardise + patches
# ---------------------------------------------------------------------------------------------------
def test_standardize_rows(fe, golden_fe):
    fv = golden_fe["fv"]
    Y = host(fe.standardize_rows(dev(fv)))
    np.testing.assert_allclose(Y[:120], golden_fe["std_H"], atol=1e-4)  # sklearn StandardScaler outputs
    np.testing.assert_allclose(Y[120:], golden_fe["std_P"], atol=1e-4)
    const = np.full((2, 50), 3.25, np.float32)
    assert np.all(host(fe.standardize_rows(dev(const))) == 0)


@pytest.mark.parametrize("W,shift", [(68, 68), (68, 34), (99, 34), (249, 24), (5, 1)])
def test_extract_patches_indexing_bit_exact(fe, golden_fe, W, shift):
    fv = golden_fe["fv"][:120]
    ref = ofe.extract_patches(ofe.tile_if_short(fv, W), W, shift)  # == compiled tools.pyx (pinned on CPU)
    got = host(fe.extract_patches(dev(fv[None]), W, shift))
    assert got.shape == ref.shape and np.array_equal(got.astype(np.float64), ref)
    tm = host(fe.extract_patches(dev(fv[None]), W, shift, time_major=True))
    assert np.array_equal(tm, np.transpose(got, (0, 2, 1)))
    key = "patches_W%d_s%d_shape" % (W, shift)
    if key in golden_fe:
        assert tuple(golden_fe[key]) == got.shape
        assert np.allclose(checks(got), golden_fe["patches_W%d_s%d_check" % (W, shift)], rtol=1e-6)


@pytest.mark.parametrize("W,shift", [(68, 68), (68, 34), (99, 34), (249, 24)])
def test_get_feature_patches_wrapper_vs_oracle(golden_fe, W, shift):
    from sm_hpss_mtl_amd.lib import preprocessing as pp
    from sm_hpss_mtl_amd.lib.cython_impl import tools
    fv = golden_fe["fv"]
    PARAMS = {"frame_level_scaling": False, "Model": "Lemaire_et_al_MTL"}
    got = pp.get_feature_patches(PARAMS, fv.copy(), W, shift, "LogMelHarmPercSpec")
    ref = ofe.feature_patches(fv, W, shift, "LogMelHarmPercSpec")
    assert got.dtype == np.float64 and got.shape == ref.shape
    np.testing.assert_allclose(got, ref, atol=1e-4)
    got4 = pp.get_feature_patches({"frame_level_scaling": False, "Model": "Doukhan_et_al_MTL"}, fv.copy(), W, shift, "MelHarmPercSpec")
    assert got4.shape == ref.shape + (1,)
    p = tools.extract_patches(fv, fv.shape, 68, 34)
    assert p.dtype == np.float64 and np.array_equal(p, ofe.extract_patches(fv, 68, 34))
    if (W, shift) == (68, 34):
        assert np.array_equal(p[:, :8, :].astype(np.float32), golden_fe["patches_W68_s34_first8rows"])  # compiled tools.pyx


@pytest.mark.parametrize("W,shift", [(68, 68), (99, 34), (249, 24)])
def test_fused_patches_vs_oracle(fe, clips4, W, shift):
    res = fe.run(dev(clips4), W=W, shift=shift)
    fv, patches = host(res["fv"]), host(res["patches"])
    nP = res["n_patches"]
    assert patches.shape == (4 * nP, W, 240)
    for i in range(4):
        ref = ofe.tcn_input(ofe.feature_patches(fv[i], W, shift, "LogMelHarmPercSpec"))  # from the GPU's own fv
        np.testing.assert_allclose(patches[i * nP:(i + 1) * nP], ref, atol=1e-4)


# ---------------------------------------------------------------------------------------------------
# a10-a12 B3_MTL forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls,W,N", [(3, 68, 6), (5, 68, 6), (3, 99, 6), (3, 249, 3), (3, 68, 1030), (5, 68, 1030), (5, 99, 700),
                                      (3, 500, 2)])  # 500 frames: no LDS left for the weight slots (per-wave weight reads)
def test_b3mtl_forward_vs_oracle(golden_model, ncls, W, N):
    from sm_hpss_mtl_amd.model import B3MTL
    w = b3_mtl.init_weights(seed=7, n_feat=240, patch_size=W, n_classes=ncls, randomize_bn=True)
    m = B3MTL(n_feat=240, patch_size=W, n_classes=ncls)
    m.set_weights_dict(w)
    x = np.random.default_rng(11).standard_normal((N, W, 240)).astype(np.float32)
    trunk = torch.empty((N, W, 32), device="cuda")
    out = host(m.forward_device(dev(x), trunk=trunk))
    n_ref = min(N, 12)
    sel = np.r_[0:n_ref // 2, N - (n_ref - n_ref // 2):N]
    ref_outs, ref_trunk = b3_mtl.forward(x[sel], w, n_classes=ncls, return_trunk=True)
    ref = np.concatenate(ref_outs, axis=1)
    np.testing.assert_allclose(host(trunk)[sel], ref_trunk, atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out[sel], ref, atol=1e-4)  # SURVEY 8(d'): abs 1e-4
    assert np.array_equal(out[sel][:, -ncls:].argmax(1), ref[:, -ncls:].argmax(1))
    key = "out_c%d_W%d" % (ncls, W)
    if N == 6 and key in golden_model:
        np.testing.assert_allclose(out, golden_model[key], atol=1e-4)
    outs = m.predict(x[:5])
    assert [o.shape[1] for o in outs] == ([1, 1, 2, 3] if ncls == 3 else [1, 1, 1, 3, 5])
    assert np.allclose(outs[-1].sum(1), 1, atol=1e-5)


@pytest.mark.parametrize("W,N", [(68, 1024), (68, 37), (99, 301), (249, 9), (30, 64), (8, 70), (16, 33), (68, 1), (5, 3)])
def test_b3mtl_block_schedules_agree(W, N, monkeypatch):
    """The two schedules of the 24 residual blocks (smh_tcn.hip) -- a barrier per block, and the skewed task list with tile
    flags that large batches run by default -- hold the same network: outputs equal bit for bit, both within 1e-4 of the
    oracle, identical argmax; a partial last workgroup and short patches included."""
    from sm_hpss_mtl_amd.model import B3MTL
    w = b3_mtl.init_weights(seed=5, n_feat=240, patch_size=W, n_classes=3, randomize_bn=True)
    m = B3MTL(n_feat=240, patch_size=W, n_classes=3)
    m.set_weights_dict(w)
    x = dev(np.random.default_rng(3).standard_normal((N, W, 240)).astype(np.float32))
    outs = {}
    # 2: the skew schedule whenever it can run (by default only where it is the faster one); "16": its 16-wave form with the
    # block weights in an LDS ring instead of registers (opt-in, SMH_TCN_SKEW16=1)
    # (the 16-wave form only exists in a lab build of the library: python -m sm_hpss_mtl_amd.build --lab)
    variants = ("2", "0", "16") if m.lib.smh_internal_lab() else ("2", "0")
    for skew in variants:
        monkeypatch.setenv("SMH_TCN_SKEW", "2" if skew == "16" else skew)
        monkeypatch.setenv("SMH_TCN_SKEW16", "1" if skew == "16" else "0")
        trunk = torch.empty((N, W, 32), device="cuda")
        outs[skew] = (host(m.forward_device(x, trunk=trunk)), host(trunk))
        m.check_status()
    # bit for bit: all add the same products in the same order (centre tap first), so a patch's outputs do not depend on the
    # schedule its batch size selects
    assert np.array_equal(outs["2"][0], outs["0"][0]) and np.array_equal(outs["2"][1], outs["0"][1])
    if "16" in outs:
        assert np.array_equal(outs["16"][0], outs["0"][0]) and np.array_equal(outs["16"][1], outs["0"][1])
    # the barrier schedule gives a lone last-round tile to two waves, 16 output channels each (5, 9, 13, 17 tiles): without the
    # split (SMH_TCN_SPLIT=0) the same bits
    monkeypatch.setenv("SMH_TCN_SKEW", "0")
    monkeypatch.setenv("SMH_TCN_SPLIT", "0")
    trunk = torch.empty((N, W, 32), device="cuda")
    whole = (host(m.forward_device(x, trunk=trunk)), host(trunk))
    m.check_status()
    monkeypatch.delenv("SMH_TCN_SPLIT")
    assert np.array_equal(whole[0], outs["0"][0]) and np.array_equal(whole[1], outs["0"][1])
    sel = np.unique(np.r_[0:min(4, N), max(0, N - 4):N])
    ref = np.concatenate(b3_mtl.forward(host(x)[sel], w, n_classes=3), axis=1)
    for skew in ("2", "0"):
        np.testing.assert_allclose(outs[skew][0][sel], ref, atol=1e-4)
        assert np.array_equal(outs[skew][0][sel][:, -3:].argmax(1), ref[:, -3:].argmax(1))


def test_skew_give_up_is_reported(monkeypatch):
    """Error contract of the stream-ordered forward (include/smh.h: smh_model_status).  The skewed block schedule bounds every
    spin; a wave whose dependency never arrives gives up, its workgroup's outputs are zero-filled and the model's device error
    word is set -- `predict` raises RuntimeError instead of handing the caller numbers.  Forced here by the debug knob
    SMH_TCN_TUNE=256 (wave 1 withholds its flags, the spin limit drops to 2^10), which only exists under SMH_ENABLE_PROBES=1."""
    from sm_hpss_mtl_amd.model import B3MTL
    w = b3_mtl.init_weights(seed=5, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True)
    m = B3MTL(n_feat=240, patch_size=68, n_classes=3)
    m.set_weights_dict(w)
    x = np.random.default_rng(3).standard_normal((64, 68, 240)).astype(np.float32)
    monkeypatch.setenv("SMH_TCN_SKEW", "2")
    good = m.predict(x)
    m.check_status()  # clean
    monkeypatch.setenv("SMH_TCN_TUNE", "256")   # without SMH_ENABLE_PROBES the knob is ignored: same results, no error
    again = m.predict(x)
    assert all(np.array_equal(a, b) for a, b in zip(good, again))
    monkeypatch.setenv("SMH_ENABLE_PROBES", "1")
    with pytest.raises(RuntimeError, match="gave up"):
        m.predict(x)
    m.check_status()  # reading the word cleared it
    monkeypatch.delenv("SMH_TCN_TUNE")
    monkeypatch.delenv("SMH_ENABLE_PROBES")
    after = m.predict(x)
    assert all(np.array_equal(a, b) for a, b in zip(good, after))
    # the same contract on the other entries that only enqueue a forward: dense file-level inference (patch_probabilities) and the
    # training step (train_on_batch(sync=True); fit checks once per epoch where it reads the losses back)
    from sm_hpss_mtl_amd import inference
    fv = np.random.default_rng(4).standard_normal((240, 700)).astype(np.float32)
    track = inference.patch_probabilities(fv, m, 68, 1, "M")
    rng = np.random.default_rng(6)
    y = {"S": rng.integers(0, 2, (64, 1)).astype(np.float32), "M": rng.integers(0, 2, (64, 1)).astype(np.float32),
         "R": rng.random((64, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[rng.integers(0, 3, 64)]}
    losses = m.train_on_batch(x, y, apply=False)
    assert np.isfinite(losses).all()
    monkeypatch.setenv("SMH_TCN_TUNE", "256")
    monkeypatch.setenv("SMH_ENABLE_PROBES", "1")
    with pytest.raises(RuntimeError, match="gave up"):
        inference.patch_probabilities(fv, m, 68, 1, "M")
    with pytest.raises(RuntimeError, match="gave up"):
        m.train_on_batch(x, y, apply=False)
    monkeypatch.delenv("SMH_TCN_TUNE")
    monkeypatch.delenv("SMH_ENABLE_PROBES")
    assert np.array_equal(inference.patch_probabilities(fv, m, 68, 1, "M"), track)


def test_get_lemaire_model_surface(tmp_path):
    from sm_hpss_mtl_amd.lib.proposed_architectures import get_Lemaire_MTL_model
    model, lr = get_Lemaire_MTL_model(TR_STEPS=100, N_MELS=240, n_classes=3, patch_size=68, seed=3)
    assert lr == 0.002 and model.count_params() == 218743 + 96
    assert model.metrics_names == ["loss", "S_loss", "M_loss", "R_loss", "3C_loss", "3C_accuracy"]
    lines = []
    model.summary(print_fn=lines.append)
    assert any("Total params" in s for s in lines) and "B3_MTL" in model.to_json()
    x = np.random.default_rng(0).standard_normal((4, 68, 240))
    a = model.predict(x)
    model.save_weights(str(tmp_path / "w"))
    m2, _ = get_Lemaire_MTL_model(100, 240, 3, 68, seed=99)
    m2.load_weights(str(tmp_path / "w"))
    for u, v in zip(a, m2.predict(x)):
        assert np.array_equal(u, v)
    with pytest.raises(ValueError):
        model.predict(np.zeros((2, 67, 240), np.float32))


# ---------------------------------------------------------------------------------------------------
# full BASELINE size: properties that do not need the oracle
# ---------------------------------------------------------------------------------------------------
def test_full_batch_properties(fe):
    from sm_hpss_mtl_amd.synth import synth_clips
    B = 1024
    clips = synth_clips(64, seed=1)
    audio = dev(np.tile(clips, (B // 64, 1)))
    res = fe.run(audio, W=68, shift=68, taps=True)
    S, harm, perc, fv, patches = res["S"], res["harm"], res["perc"], res["fv"], res["patches"]
    torch.cuda.synchronize()
    assert patches.shape == (B, 68, 240) and torch.isfinite(patches).all() and torch.isfinite(fv).all()
    # replicas of the same clip give identical bits wherever they sit in the batch
    for t in (S, harm, perc, fv, patches):
        v = t.view(B // 64, 64, -1)
        assert torch.equal(v[0], v[-1]) and torch.equal(v[0], v[7])
    # medians are selections: every output value occurs in its input row / column window range
    assert (harm <= S.amax(dim=2, keepdim=True)).all() and (harm >= S.amin(dim=2, keepdim=True)).all()
    assert (perc <= S.amax(dim=1, keepdim=True)).all() and (perc >= S.amin(dim=1, keepdim=True)).all()
    # median filtering commutes with positive scaling, bit for bit (power of two)
    h2, p2 = fe.hpss_median(S * 4.0)
    assert torch.equal(h2, harm * 4.0) and torch.equal(p2, perc * 4.0)
    # top-dB: each half spans at most 80 dB; standardised patches have ~zero mean / unit variance per row
    assert float((fv[:, :120].amax(dim=(1, 2)) - fv[:, :120].amin(dim=(1, 2))).max()) <= 80.0 + 1e-3
    # bit-exact against the oracle on a handful of clips spread over the batch
    Sh, hh, ph = host(S), host(harm), host(perc)
    for i in (0, 63, 511, 1023):
        assert np.array_equal(hh[i], ofe.median_time(Sh[i], 21)) and np.array_equal(ph[i], ofe.median_freq(Sh[i], 11))


def test_long_clips_take_the_streaming_paths(fe):
    """Whole files, not one-second clips: 10 s (T = 998: frame-tiled medians, slab feature kernel, streaming
    clip / standardise / patch kernels) against the oracle; 60 s for shape, finiteness and the patch contract."""
    from sm_hpss_mtl_amd.synth import synth_clips
    y = synth_clips(2, seed=21, n_samples=160000)
    res = fe.run(torch.from_numpy(y).cuda(), W=68, shift=34)
    S = host(fe.stft_mag(torch.from_numpy(y).cuda()))  # the same kernel: the S the fused call worked on
    fv, patches = host(res["fv"]), host(res["patches"])
    nP = len(ofe.patch_starts(998, 68, 34))
    assert fv.shape == (2, 240, 998) and patches.shape == (2 * nP, 68, 240)
    for i in range(2):
        ref_s = ofe.featuregram_from_S(S[i], "LogMelHarmPercSpec")
        assert np.max(np.abs(fv[i] - ref_s)) <= 1e-3          # dB, every bin, from the device's own S
        ref = ofe.featuregram(y[i], "LogMelHarmPercSpec")
        assert np.max(np.abs(fv[i] - ref)) <= 2e-3            # dB, end to end from the audio (STFT-ulp median flips included)
        refp = ofe.tcn_input(ofe.feature_patches(fv[i], 68, 34))
        assert np.max(np.abs(patches[i * nP:(i + 1) * nP] - refp)) <= 2e-4  # standardisation + patch gather of the device's fv
    y60 = synth_clips(1, seed=22, n_samples=960000)
    r60 = fe.run(torch.from_numpy(y60).cuda(), W=68, shift=68)
    torch.cuda.synchronize()
    assert r60["fv"].shape == (1, 240, 5998) and r60["patches"].shape[0] == len(ofe.patch_starts(5998, 68, 68))
    assert torch.isfinite(r60["fv"]).all() and torch.isfinite(r60["patches"]).all()
    assert float(r60["fv"][0, :120].max() - r60["fv"][0, :120].min()) <= 80.0 + 1e-3  # top_db span of the H array


def test_odd_large_batch_end_to_end(fe):
    """5001 clips (not a multiple of anything): every clip equals its replica computed in a batch of 8."""
    from sm_hpss_mtl_amd.model import B3MTL
    from sm_hpss_mtl_amd.synth import synth_clips
    base = synth_clips(8, seed=31)
    B = 5001
    idx = (np.arange(B) * 5) % 8
    audio = torch.from_numpy(base[idx]).cuda()
    m = B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=3)
    out = m.forward_device(fe.run(audio, W=68, shift=68)["patches"])
    ref = m.forward_device(fe.run(torch.from_numpy(base).cuda(), W=68, shift=68)["patches"])
    torch.cuda.synchronize()
    assert out.shape == (B, 7) and torch.equal(out, ref[torch.from_numpy(idx).cuda()])


@pytest.mark.parametrize("W,shift,ncls", [(68, 68, 3), (68, 34, 5), (99, 34, 3)])
def test_layer0_fused_into_features_matches_the_two_step_path(fe, clips4, W, shift, ncls):
    """smh_features_l0_f32 + smh_model_forward_x0_f32 (the bench fast path) against features -> patches -> forward and
    against the oracle; W = 99 exercises tile-if-short (98 frames)."""
    from sm_hpss_mtl_amd.model import B3MTL
    w = b3_mtl.init_weights(seed=4, n_feat=240, patch_size=W, n_classes=ncls, randomize_bn=True)
    m = B3MTL(n_feat=240, patch_size=W, n_classes=ncls, seed=0)
    m.set_weights_dict(w)
    S = fe.stft_mag(dev(clips4))
    harm, perc = fe.hpss_median(S)
    two = fe.features(S, harm, perc, W=W, shift=shift)
    ref = m.forward_device(two["patches"])
    fused = fe.features_l0(S, harm, perc, 0, W, shift, m, patches=True)
    got = m.forward_from_x0(fused["x0p"])
    torch.cuda.synchronize()
    assert torch.equal(fused["fv"], two["fv"]) and torch.equal(fused["patches"], two["patches"])
    assert float((got - ref).abs().max()) <= 2e-5
    oracle = np.concatenate(b3_mtl.forward(host(two["patches"]), w, ncls), axis=1)
    assert np.max(np.abs(host(got) - oracle)) <= 1e-4


@pytest.mark.parametrize("W,shift,ncls", [(68, 68, 3), (68, 5, 3), (99, 34, 5)])
def test_single_feature_kernel_on_blocked_harm_matches_the_two_step_path(fe, clips4, W, shift, ncls):
    """The bench fast path end to end: median with harm_layout = 2 (16-frame blocks) -> features_clip_kernel with the
    layer-0 partials -> smh_model_forward_x0_f32, against (B,K,T) medians -> features -> patches -> forward."""
    import ctypes as C
    from sm_hpss_mtl_amd import _lib
    from sm_hpss_mtl_amd.model import B3MTL
    w = b3_mtl.init_weights(seed=5, n_feat=240, patch_size=W, n_classes=ncls, randomize_bn=True)
    m = B3MTL(n_feat=240, patch_size=W, n_classes=ncls, seed=0)
    m.set_weights_dict(w)
    S = fe.stft_mag(dev(clips4))
    B, K, T = S.shape
    harm0, perc0 = fe.hpss_median(S)
    two = fe.features(S, harm0, perc0, W=W, shift=shift)
    ref = m.forward_device(two["patches"])
    _skip_if_forced("SMH_FEAT_TWO_KERNELS", "SMH_FEAT_TAPS", "SMH_MEDIAN_NOSPLIT")
    assert fe.lib.smh_features_blocked_ok(fe._h, T, 1) == 1
    harm2 = torch.empty((B, fe.lib.smh_harm_buffer_floats(K, T)), device="cuda")
    perc2 = torch.empty_like(S)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lay = _lib.check(fe.lib.smh_hpss_median_ex_f32(fe._h, ptr(S), B, K, T, fe.cfg.l_harm, fe.cfg.l_perc, ptr(harm2), ptr(perc2), 2, st))
    assert lay == 2 and torch.equal(perc2, perc0)
    G = (T + 15) // 16
    dec = harm2.view(B, G, K, 16).permute(0, 2, 1, 3).reshape(B, K, G * 16)[:, :, :T]
    assert torch.equal(dec, harm0)  # bit-exact medians in the blocked layout
    fused = fe.features_l0(S, harm2, perc2, 2, W, shift, m, patches=True)
    got = m.forward_from_x0(fused["x0p"])
    torch.cuda.synchronize()
    assert fused["n_patches"] == two["n_patches"]
    assert float((fused["fv"] - two["fv"]).abs().max()) <= 1e-4       # dB: other summation order over the taps
    assert float((fused["patches"] - two["patches"]).abs().max()) <= 1e-4
    assert float((got - ref).abs().max()) <= 5e-5
    oracle = np.concatenate(b3_mtl.forward(host(two["patches"]), w, ncls), axis=1)
    assert np.max(np.abs(host(got) - oracle)) <= 1e-4


def test_frontend_randomised_lengths_and_feature_names():
    """12 seeded draws of (clip length, feature name, n_fft, windows, patch geometry): odd sample counts (generic STFT
    kernel), T below and above one wave, every featName of SURVEY 8a (mel / no mel, dB / magnitude), Jang's n_fft = 512;
    featuregram and patches from the fused entry point against the oracle."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig, FEATS
    from sm_hpss_mtl_amd.synth import synth_clips
    rng = np.random.default_rng(7)
    names = sorted(FEATS)
    for trial in range(12):
        name = names[trial % 4]
        use_mel, log = FEATS[name]
        n_fft = 512 if (trial % 6 == 5) else 400
        n = int(rng.integers(3000, 30000)) | (trial & 1)           # odd lengths every other trial
        lh, lp = [(21, 11), (17, 17), (11, 21), (5, 31)][trial % 4]
        W, shift = [(68, 34), (20, 7), (99, 50)][trial % 3]
        cfg = FrontendConfig(n_fft=n_fft, win_length=400, n_mels=120 if use_mel else 0, l_harm=lh, l_perc=lp, log_db=log)
        fe_t = Frontend(cfg)
        y = synth_clips(2, seed=100 + trial, n_samples=n)
        res = fe_t.run(dev(y), W=W, shift=shift)
        S = host(fe_t.stft_mag(dev(y)))  # the same kernel: the S the fused call worked on
        fv, patches = host(res["fv"]), host(res["patches"])
        T = 1 + (n - n_fft) // 160
        rows = 120 if use_mel else n_fft // 2 + 1
        assert fv.shape == (2, 2 * rows, T), (trial, fv.shape)
        for i in range(2):
            ref = ofe.featuregram(y[i], name, n_fft=n_fft, n_mels=120, l_harm=lh, l_perc=lp)
            tol = 2e-3 if log else 2e-5 * max(1.0, float(np.abs(ref).max()))
            assert np.max(np.abs(fv[i] - ref)) <= tol, (trial, name, n, float(np.max(np.abs(fv[i] - ref))))
            if log:  # SURVEY 8(d'): abs 1e-3 dB on every bin once the STFT's last bits are taken out of the comparison
                ref_s = ofe.featuregram_from_S(S[i], name, n_mels=120, l_harm=lh, l_perc=lp)
                assert np.max(np.abs(fv[i] - ref_s)) <= 1e-3, (trial, name, n, float(np.max(np.abs(fv[i] - ref_s))))
            nP = res["n_patches"]
            refp = ofe.tcn_input(ofe.feature_patches(fv[i], W, shift, name))  # from the GPU's own fv
            assert refp.shape[0] == nP
            np.testing.assert_allclose(patches[i * nP:(i + 1) * nP], refp, atol=2e-4)


def test_reload_of_keras_written_artifacts(tmp_path):
    """Proposed_Work_Results.py:376-384 on files laid out the way Keras writes them (auto-generated layer names, Functional
    JSON): model_from_json(architecture) -> load_weights(weights) -> predict equals the oracle on the original weights."""
    import json
    from collections import OrderedDict
    from sm_hpss_mtl_amd import h5io
    from sm_hpss_mtl_amd.lib.proposed_architectures import model_from_json
    from tests.test_host_logic import _keras_style_artifacts
    if not h5io.available():
        pytest.skip("libhdf5 not found on this machine")
    w = OrderedDict((k, np.asarray(v, np.float32)) for k, v in b3_mtl.init_weights(seed=8, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True).items())
    layers, arch = _keras_style_artifacts(w, 3, 68, 240)
    weightFile, architechtureFile = str(tmp_path / "m.h5"), str(tmp_path / "m.json")
    h5io.write_layers(weightFile, layers)
    json.dump(arch, open(architechtureFile, "w"))
    with open(architechtureFile, "r") as f:
        model = model_from_json(f.read())
    model.load_weights(weightFile)
    assert (model.patch_size, model.n_feat, model.n_classes, model.dropout_rate) == (68, 240, 3, 0.25)
    x = np.random.default_rng(0).standard_normal((5, 68, 240)).astype(np.float32)
    ref = b3_mtl.forward(x, w)
    for a, b in zip(model.predict(x), ref):
        np.testing.assert_allclose(a, b, atol=1e-4)


def test_preallocated_outputs_are_validated(fe, clips4):
    """The C ABI takes raw pointers without sizes: an `out` dict kept from a smaller batch must be refused, not written past."""
    S = fe.stft_mag(dev(clips4))
    harm, perc = fe.hpss_median(S)
    small = fe.features(S[:2], harm[:2], perc[:2], W=68, shift=68)
    with pytest.raises(ValueError, match="shape"):
        fe.features(S, harm, perc, W=68, shift=68, out=small)
    with pytest.raises(ValueError, match="maxkeys"):
        fe.features(S, harm, perc, W=68, shift=68, out={"maxkeys": torch.empty(2, dtype=torch.int32, device="cuda")})
    with pytest.raises(ValueError, match="float32|torch.float32"):
        fe.features(S, harm, perc, out={"fv": torch.empty((4, 240, 98), dtype=torch.float64, device="cuda")})
    ok = fe.features(S, harm, perc, W=68, shift=68)
    again = fe.features(S, harm, perc, W=68, shift=68, out=ok)  # the right shapes are reused in place
    assert again["fv"].data_ptr() == ok["fv"].data_ptr() and again["patches"].data_ptr() == ok["patches"].data_ptr()


@pytest.mark.parametrize("ncls,W,N", [(3, 68, 6), (5, 68, 7), (3, 99, 5), (3, 68, 1030), (3, 249, 3)])
def test_b3mtl_two_conv_block_variant_vs_oracle(ncls, W, N, tmp_path):
    """smh_model_cfg.block_variant = 1 (the residual block of keras-tcn >= 2.8: two dilated convolutions, relu each, identity
    / 1x1 'matching' shortcut, relu of the sum; no initial convolution) against oracle.b3_mtl.tcn_forward_v2."""
    from sm_hpss_mtl_amd.lib.proposed_architectures import get_Lemaire_MTL_model, model_from_json
    w = b3_mtl.init_weights_v2(seed=9, n_feat=240, patch_size=W, n_classes=ncls, randomize_bn=True)
    for k in w:  # keep the un-normalised trunk in a sane range (24 blocks without 'norm_relu')
        if "/conv" in k and k.endswith("kernel"):
            w[k] = (w[k] * 0.5).astype(np.float32)
    m, _ = get_Lemaire_MTL_model(10, N_MELS=240, n_classes=ncls, patch_size=W, tcn_block="2.8")
    assert [n for n, _, _, _ in m._spec] == list(w) and m.count_params() == sum(v.size for v in w.values())
    m.set_weights_dict(w)
    x = np.random.default_rng(12).standard_normal((N, W, 240)).astype(np.float32)
    trunk = torch.empty((N, W, 32), device="cuda")
    out = host(m.forward_device(dev(x), trunk=trunk))
    sel = np.r_[0:min(N, 6) // 2 + 1, N - 2:N] if N > 6 else np.arange(N)
    ref_outs, ref_trunk = b3_mtl.forward(x[sel], w, n_classes=ncls, return_trunk=True)
    scale = max(1.0, float(np.abs(ref_trunk).max()))
    np.testing.assert_allclose(host(trunk)[sel], ref_trunk, atol=2e-4 * scale)
    ref = np.concatenate(ref_outs, axis=1)
    np.testing.assert_allclose(out[sel], ref, atol=2e-4)
    assert np.array_equal(out[sel][:, -ncls:].argmax(1), ref[:, -ncls:].argmax(1))
    if N == 6:
        m.save_weights(str(tmp_path / "v2.h5"))
        m2 = model_from_json(m.to_json())
        assert m2.tcn_block == "2.8"
        m2.load_weights(str(tmp_path / "v2.h5"))
        assert np.array_equal(m2.predict(x)[-1], m.predict(x)[-1])
        # n_feat == nb_filters: Keras builds no 'matching' convolution (identity shortcut in the first block); a model saved
        # from one instance reloads and predicts the same bits in another
        from sm_hpss_mtl_amd.model import B3MTL
        m32 = B3MTL(n_feat=32, patch_size=W, n_classes=ncls, seed=4, tcn_block="2.8")
        assert not any("/matching/" in n for n in m32.weight_names()) and any("/matching/" in n for n in m.weight_names())
        x32 = np.random.default_rng(13).standard_normal((N, W, 32)).astype(np.float32)
        m32.save_weights(str(tmp_path / "v2_32.h5"))
        m3 = model_from_json(m32.to_json())
        assert (m3.n_feat, m3.tcn_block, m3.weight_names()) == (32, "2.8", m32.weight_names())
        m3.load_weights(str(tmp_path / "v2_32.h5"))
        for a, b in zip(m3.predict(x32), m32.predict(x32)):
            assert np.array_equal(a, b) and np.isfinite(a).all()
        with pytest.raises(NotImplementedError):
            m.train_on_batch(x, {"S": np.zeros((N, 1)), "M": np.zeros((N, 1)), "R": np.zeros((N, 2)), "3C": np.eye(3)[np.zeros(N, int)]})
        with pytest.raises(ValueError):
            m.forward_from_x0(torch.zeros((N, 2, W, 32), device="cuda"))
