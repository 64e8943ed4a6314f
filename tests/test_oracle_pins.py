"""CPU: pin the oracle against the boundary routines the reference delegates to and against the
committed golden vectors.  No GPU, no product code."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from oracle import b3_mtl, frontend as ofe
from tests.conftest import ROOT, checks


def test_median_vs_scipy_bit_exact():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    S = np.abs(rng.standard_normal((201, 98))).astype(np.float32)
    S[5:9, 10:40] = 0.25  # ties
    for w in (3, 11, 17, 21, 51):
        assert np.array_equal(ofe.median_time(S, w), ndi.median_filter(S, size=(1, w), mode="reflect"))
        assert np.array_equal(ofe.median_freq(S, w), ndi.median_filter(S, size=(w, 1), mode="reflect"))
    # window longer than the axis (multiple reflections)
    small = np.abs(rng.standard_normal((7, 5))).astype(np.float32)
    assert np.array_equal(ofe.median_time(small, 21), ndi.median_filter(small, size=(1, 21), mode="reflect"))
    assert np.array_equal(ofe.median_freq(small, 21), ndi.median_filter(small, size=(21, 1), mode="reflect"))


def test_c_oracle_median_and_patches():
    so = os.path.join(ROOT, "oracle", "_build", "libsmh_oracle.so")
    if not os.path.exists(so):
        pytest.skip("oracle C library not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(so)
    rng = np.random.default_rng(4)
    S = np.abs(rng.standard_normal((40, 33))).astype(np.float32)
    out = np.empty_like(S)
    fp = ctypes.POINTER(ctypes.c_float)
    for w in (5, 11, 21):
        assert lib.orc_median_time(S.ctypes.data_as(fp), out.ctypes.data_as(fp), 40, 33, w) == 0
        assert np.array_equal(out, ofe.median_time(S, w))
        assert lib.orc_median_freq(S.ctypes.data_as(fp), out.ctypes.data_as(fp), 40, 33, w) == 0
        assert np.array_equal(out, ofe.median_freq(S, w))
    FV = rng.standard_normal((6, 120)).astype(np.float32)
    for W, shift in ((68, 34), (99, 24), (5, 1)):
        nP = lib.orc_num_patches(120, W, shift)
        po = np.empty((nP, 6, W))
        assert lib.orc_extract_patches(FV.ctypes.data_as(fp), po.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 6, 120, W, shift) == nP
        assert np.array_equal(po, ofe.extract_patches(FV, W, shift))


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


@pytest.fixture(scope="module")
def ref_tools_golden():
    """Outputs of the reference's compiled tools module on the inputs below (tests/golden/make_ref_tools_golden.py)."""
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_tools_golden.npz"))


def test_patches_vs_compiled_reference_module(ref_tools_golden):
    g = ref_tools_golden
    rng = np.random.default_rng(5)
    for T in (69, 98, 137, 300):
        FV = rng.standard_normal((9, T)).astype(np.float32)
        assert np.array_equal(_sha(FV), g["patches_T%d_in_sha" % T]), T
        for W, shift in ((68, 68), (68, 34), (99, 34), (249, 24)):
            FVt = ofe.tile_if_short(FV, W)
            got = ofe.extract_patches(FVt, W, shift)
            key = "patches_T%d_W%d_s%d" % (T, W, shift)
            assert got.dtype == np.float64 and got.shape == tuple(g[key + "_shape"]), (T, W, shift)
            assert np.array_equal(_sha(got), g[key + "_sha"]), (T, W, shift)


def test_npatch_table_golden(golden_fe):
    for T, W, shift, nP in golden_fe["npatch_table"]:
        assert len(ofe.patch_starts(int(T), int(W), int(shift))) == nP, (T, W, shift)


def test_standardize_vs_sklearn(golden_fe):
    skp = pytest.importorskip("sklearn.preprocessing")
    fv = golden_fe["fv"]
    half = fv.shape[0] // 2
    for rows in (fv[:half], fv[half:]):
        ref = skp.StandardScaler(copy=True).fit_transform(rows.T.copy()).T
        got = ofe.standardize_rows(rows)
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, ref, atol=2e-6, rtol=0)
    # constant row (the empty mel filter) -> zeros
    const = np.full((1, 98), -37.5, np.float32)
    assert np.all(ofe.standardize_rows(const) == 0)


def test_frontend_golden_roundtrip(golden_fe, clips4):
    """The committed vectors are what the oracle produces today (guards against silent oracle drift)."""
    assert np.allclose(checks(clips4[0]), golden_fe["audio0_check"], rtol=1e-12)
    fv, p = ofe.featuregram(clips4[0], "LogMelHarmPercSpec", return_parts=True)
    assert np.array_equal(p["harm"], golden_fe["harm_21"]) and np.array_equal(p["perc"], golden_fe["perc_11"])
    np.testing.assert_allclose(p["S"], golden_fe["S"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(fv, golden_fe["fv"], atol=1e-4)
    np.testing.assert_allclose(ofe.standardize_rows(fv[:120]), golden_fe["std_H"], atol=1e-5)


def test_closed_form_identities(clips4):
    fv, p = ofe.featuregram(clips4[1], "LogMelHarmPercSpec", return_parts=True)
    S, H, P = p["S"], p["H"], p["P"]
    assert S.shape == (201, 98) and fv.shape == (240, 98) and fv.dtype == np.float32
    assert np.all(np.abs(H + P - S) <= 2 * np.spacing(S) + 1e-30)  # masks sum to one
    assert np.all(H >= 0) and np.all(P >= 0)
    for half in (fv[:120], fv[120:]):
        assert half.max() - half.min() <= 80.0 + 1e-4  # top_db clip per array
    B = ofe.mel_basis()
    assert B.shape == (120, 201) and np.all(B >= 0)
    assert np.count_nonzero(B) == 393 and (B.sum(axis=1) == 0).sum() == 1  # 393 nnz, 1 empty filter
    # frames: T = 1 + (N - n_fft)//hop
    assert ofe.num_frames(16000, 400, 160) == 98 and ofe.num_frames(399, 400, 160) == 0
    # tile-if-short quirk: T < W tiles until T > W (98 -> 294 for W=249, 98 -> 196 for W=99)
    assert ofe.tile_if_short(np.zeros((2, 98)), 249).shape[1] == 294
    assert ofe.tile_if_short(np.zeros((2, 98)), 99).shape[1] == 196
    assert ofe.tile_if_short(np.zeros((2, 98)), 98).shape[1] == 98


def test_b3mtl_golden_and_shapes(golden_model):
    for ncls, W in ((3, 68), (5, 68), (3, 99)):
        w = b3_mtl.init_weights(seed=7, n_feat=240, patch_size=W, n_classes=ncls, randomize_bn=True)
        x = np.random.default_rng(11).standard_normal((6, W, 240)).astype(np.float32)
        outs = b3_mtl.forward(x, w, n_classes=ncls)
        got = np.concatenate(outs, axis=1)
        np.testing.assert_allclose(got, golden_model["out_c%d_W%d" % (ncls, W)], atol=1e-5)
        assert np.allclose(outs[-1].sum(axis=1), 1, atol=1e-6) and outs[-1].shape == (6, ncls)
    n3 = sum(v.size for v in b3_mtl.init_weights(patch_size=68).values())
    # 218 743 params at W=68 of which 3*16*2 are non-trainable BN moving statistics
    assert n3 - 3 * 32 == 218743
    assert abs(b3_mtl.flops_per_patch() - 14.64e6) < 0.01e6


def test_b3mtl_dilated_conv_matches_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 30, 8)).astype(np.float32)
    k = rng.standard_normal((3, 8, 5)).astype(np.float32)
    b = rng.standard_normal(5).astype(np.float32)
    for d in (1, 4, 16, 64):
        ref = torch.nn.functional.conv1d(torch.from_numpy(x).permute(0, 2, 1), torch.from_numpy(k).permute(2, 1, 0),
                                         torch.from_numpy(b), padding=d, dilation=d).permute(0, 2, 1).numpy()
        np.testing.assert_allclose(b3_mtl.conv1d_same(x, k, b, d), ref, atol=1e-5)


def _silence_case(c):
    from oracle import silence as sil
    from sm_hpss_mtl_amd.synth import gappy_clip
    x = sil.normalize_signal(gappy_clip(c))
    return x, sil.rms(x, 400, 160)


@pytest.mark.parametrize("case", range(7))
def test_remove_silence_vs_compiled_reference(case, ref_tools_golden):
    from oracle import silence as sil
    from sm_hpss_mtl_amd.synth import SILENCE_CASES
    g = ref_tools_golden
    gaps = SILENCE_CASES[case][1]
    x, energy = _silence_case(case)
    assert energy.shape == (1 + len(x) // 160,) and energy.dtype == np.float32
    assert np.array_equal(_sha(np.concatenate([x, energy])), g["silence_c%d_in_sha" % case])
    ref_len, ref_untouched, ref_n_sm, ref_tot = g["silence_c%d_meta" % case]
    ref_sm = np.unpackbits(g["silence_c%d_sample_marker" % case])[:ref_n_sm]
    out, sm, fm, tot = sil.remove_silence(x, energy, 16000, 25, 10)
    assert tot == ref_tot
    assert np.array_equal(fm, g["silence_c%d_frame_marker" % case]) and len(sm) == ref_n_sm and np.array_equal(sm, ref_sm)
    assert out.dtype == np.dtype(str(g["silence_c%d_out_dtype" % case])) and len(out) == ref_len
    assert np.array_equal(_sha(out), g["silence_c%d_out_sha" % case]) and int(out is x) == ref_untouched
    if out is not x:  # >= 2 qualifying runs: the reference's tail of ones
        n_keep = int(sm.sum())
        assert n_keep < len(x) and np.all(out[n_keep:] == 1.0)
    else:  # 0 or 1 qualifying runs: input returned untouched, even though sample_marker may hold zeros
        assert sum(b - a > 0.1 for a, b in gaps) < 2


@pytest.mark.parametrize("case", range(7))
def test_remove_silence_vs_golden(case):
    """The committed outputs of the compiled reference (tests/golden/make_silence_golden.py)."""
    from oracle import silence as sil
    g = np.load(os.path.join(ROOT, "tests", "golden", "silence_golden.npz"))
    x, energy = _silence_case(case)
    assert hashlib.sha256(x.tobytes()).digest() == g["c%d_x_sha" % case].tobytes()
    assert np.array_equal(energy, g["c%d_energy" % case])
    out, sm, fm, tot = sil.remove_silence(x, energy, 16000, 25, 10)
    n, n_keep, untouched, ref_tot = g["c%d_meta" % case]
    assert (len(x), int(sm.sum()), int(out is x), tot) == (n, n_keep, untouched, ref_tot)
    assert np.array_equal(fm, g["c%d_frame_marker" % case])
    assert np.array_equal(np.packbits(sm.astype(np.uint8)), g["c%d_sample_marker" % case])
    assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).digest() == g["c%d_out_sha" % case].tobytes()


def test_rms_closed_form():
    from oracle import silence as sil
    rng = np.random.default_rng(0)
    y = rng.standard_normal(1000).astype(np.float32)
    e = sil.rms(y, 400, 160)
    yp = np.concatenate([y[200:0:-1], y, y[-2:-202:-1]])  # numpy 'reflect': no edge repeat
    for t in (0, 3, len(e) - 1):
        assert abs(e[t] - np.sqrt(np.mean(yp[t * 160:t * 160 + 400].astype(np.float64) ** 2))) < 1e-6


@pytest.mark.parametrize("n,k", [(40, 5), (1000, 501), (300, 501), (7, 9), (64, 1)])
def test_oracle_medfilt_vs_scipy(n, k):
    """scipy.signal.medfilt is the routine DAFx12...:96 calls."""
    ss = pytest.importorskip("scipy.signal")
    from oracle import inference as oinf
    x = np.random.default_rng(n + k).random(n).astype(np.float32)
    x[::7] = x[0]
    assert np.array_equal(oinf.medfilt(x, k), ss.medfilt(x, k))


def test_scale_data_vs_compiled_reference(ref_tools_golden):
    from oracle import tools_stats
    g = ref_tools_golden
    rng = np.random.default_rng(3)
    for dt in (np.float32, np.float64):
        FV = rng.normal(size=(42, 68)).astype(dt) * 7 - 3
        name = np.dtype(dt).name
        assert np.array_equal(_sha(FV), g["scale_%s_in_sha" % name]), name
        mean, std = FV.mean(axis=1), FV.std(axis=1)
        got = tools_stats.scale_data(FV, mean, std)
        assert got.dtype == np.float64 and got.shape == tuple(g["scale_%s_shape" % name])
        assert np.array_equal(_sha(got), g["scale_%s_sha" % name]), name


@pytest.mark.parametrize("stat", ["mean", "variance", "skew", "kurtosis"])
@pytest.mark.parametrize("axis", [0, 1])
def test_data_statistics_vs_compiled_reference(stat, axis, ref_tools_golden):
    from oracle import tools_stats
    g = ref_tools_golden
    rng = np.random.default_rng(11)
    FV = rng.gamma(2.0, size=(5, 21, 34)) - rng.normal(size=(5, 21, 34)) ** 2
    assert np.array_equal(_sha(FV), g["stats_in_sha"])
    ref = g["stats_%s_%d" % (stat, axis)]
    got = tools_stats.get_data_statistics(FV, stat, axis)
    assert got.shape == ref.shape == (5, 34 if axis == 0 else 21)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-13)


def test_data_statistics_constant_rows():
    from oracle import tools_stats
    FV = np.ones((2, 4, 6))
    assert np.all(tools_stats.get_data_statistics(FV, "skew", 0) == 0.0)
    assert np.all(tools_stats.get_data_statistics(FV, "kurtosis", 1) == -3.0)


# ---------------------------------------------------------------------------------------------------
# Cross-checks of the UNPINNED half of the oracle against independent implementations available in this container
# (VERDICT r2 item 5).  None of these is the reference (librosa / Keras / keras-tcn are absent): they lower the risk of a
# restatement error, they do not turn "parity unpinned" into "pinned".
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [400, 512])
def test_hann_window_vs_scipy_get_window(n):
    """librosa.filters.get_window delegates to scipy.signal.get_window('hann', n, fftbins=True) -- the very routine (SURVEY 8c
    lists it as an in-container boundary oracle).  Bit-exact: the oracle evaluates the window the way scipy does."""
    sig = pytest.importorskip("scipy.signal")
    ref = sig.get_window("hann", n, fftbins=True)
    got = ofe.hann_window(n, n)
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.array_equal(got, ref)
    assert np.max(np.abs(got - (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)))) < 1e-15   # = SURVEY a1's closed form
    # win_length < n_fft (Jang: window 400 in n_fft 512): librosa's util.pad_center puts (n_fft - win) // 2 zeros in front
    padded = ofe.hann_window(400, 512)
    assert padded.shape == (512,) and np.all(padded[:56] == 0) and np.all(padded[456:] == 0)
    assert np.array_equal(padded[56:456], sig.get_window("hann", 400, fftbins=True))


@pytest.mark.parametrize("n_fft,win,hop", [(400, 400, 160), (512, 400, 160)])
def test_stft_mag_vs_torch_stft_and_scipy(clips4, n_fft, win, hop):
    """|STFT| of the oracle against two independent implementations of the same transform: torch.stft(center=False, periodic
    Hann, float64) and scipy.signal.ShortTimeFFT.  1e-6 of max|S| (the oracle rounds its f64 spectrum to complex64 as librosa
    does: 6e-8 relative); frame count = 1 + (N - n_fft) // hop in all three."""
    import torch
    sig = pytest.importorskip("scipy.signal")
    for y in clips4[:2]:
        S = ofe.stft_mag(y, n_fft, win, hop)
        T = 1 + (len(y) - n_fft) // hop
        assert S.shape == (n_fft // 2 + 1, T) and S.dtype == np.float32
        w = torch.hann_window(win, periodic=True, dtype=torch.float64)
        Z = torch.stft(torch.from_numpy(y.astype(np.float64)), n_fft=n_fft, hop_length=hop, win_length=win, window=w, center=False,
                       return_complex=True)
        ref = Z.abs().numpy()
        assert ref.shape == S.shape
        assert np.max(np.abs(S - ref)) <= 1e-6 * ref.max()
        if win == n_fft:
            stft = sig.ShortTimeFFT(sig.get_window("hann", win, fftbins=True), hop=hop, fs=16000, mfft=n_fft, scale_to=None,
                                    phase_shift=None)
            # ShortTimeFFT centres its windows on k * hop: slice k0 is the first whose window starts at sample 0
            Z2 = stft.stft(y.astype(np.float64), p0=0, p1=stft.p_max(len(y)))
            k0 = (win // 2) // hop + (1 if (win // 2) % hop else 0)
            starts = [k * hop - win // 2 for k in range(Z2.shape[1])]
            cols = [i for i, s0 in enumerate(starts) if s0 >= 0 and s0 % hop == 0 and s0 // hop < T and s0 + win <= len(y)]
            if cols:  # only when the two framings coincide (hop | win / 2); otherwise torch.stft above is the check
                ref2 = np.abs(Z2[:, cols])
                ours = S[:, [starts[i] // hop for i in cols]]
                assert np.max(np.abs(ours - ref2)) <= 1e-6 * ref2.max()
            del k0


@pytest.mark.parametrize("ncls,W", [(3, 68), (5, 68), (3, 99)])
def test_b3mtl_forward_outputs_vs_torch_nn(ncls, W):
    """oracle.b3_mtl.forward (numpy) against a torch.nn build of the same graph with the same weights -- OUTPUTS, not only
    gradients (tests/test_oracle_train.py pins the gradients): Conv1d('same', dilation), relu, channel-max normalisation,
    residual 1x1 Conv1d, final relu, Flatten in (time, channel) order, Linear + BatchNorm1d(eval, eps 1e-3) + relu + Linear
    heads, softmax.  Float64 on both sides: 1e-6 (SURVEY d' asks 1e-4 of the device)."""
    import torch
    from torch import nn
    w = b3_mtl.init_weights(seed=3, n_feat=240, patch_size=W, n_classes=ncls, randomize_bn=True)
    x = np.random.default_rng(9).standard_normal((5, W, 240))

    def t(a):
        return torch.tensor(np.asarray(a, np.float64))

    class Block(nn.Module):
        def __init__(self, p, d):
            super().__init__()
            self.conv = nn.Conv1d(32, 32, 3, padding=d, dilation=d)
            self.conv1x1 = nn.Conv1d(32, 32, 1)
            with torch.no_grad():
                self.conv.weight.copy_(t(w[p + "/conv/kernel"]).permute(2, 1, 0))      # Keras (k, in, out) -> torch (out, in, k)
                self.conv.bias.copy_(t(w[p + "/conv/bias"]))
                self.conv1x1.weight.copy_(t(w[p + "/conv1x1/kernel"]).permute(2, 1, 0))
                self.conv1x1.bias.copy_(t(w[p + "/conv1x1/bias"]))

        def forward(self, h):                                                           # h: (N, C, T)
            y = torch.relu(self.conv(h))
            y = y / (y.abs().amax(dim=1, keepdim=True) + 1e-5)                          # keras-tcn 2.3 channel_normalization
            return h + self.conv1x1(y)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.initial = nn.Conv1d(240, 32, 1)
            with torch.no_grad():
                self.initial.weight.copy_(t(w["tcn/initial_conv/kernel"]).permute(2, 1, 0))
                self.initial.bias.copy_(t(w["tcn/initial_conv/bias"]))
            self.blocks = nn.ModuleList([Block("tcn/s%d_d%d" % (s, 2 ** i), 2 ** i) for s in range(3) for i in range(8)])
            D = W * 32
            self.c3 = nn.Linear(D, ncls)
            self.heads = nn.ModuleDict()
            with torch.no_grad():
                self.c3.weight.copy_(t(w["3C/kernel"]).T)
                self.c3.bias.copy_(t(w["3C/bias"]))
                for name, odim, _ in b3_mtl.head_spec(ncls):
                    d, bn, o = nn.Linear(D, 16), nn.BatchNorm1d(16, eps=1e-3), nn.Linear(16, odim)
                    d.weight.copy_(t(w[name + "/dense/kernel"]).T), d.bias.copy_(t(w[name + "/dense/bias"]))
                    bn.weight.copy_(t(w[name + "/bn/gamma"])), bn.bias.copy_(t(w[name + "/bn/beta"]))
                    bn.running_mean.copy_(t(w[name + "/bn/moving_mean"])), bn.running_var.copy_(t(w[name + "/bn/moving_variance"]))
                    o.weight.copy_(t(w[name + "/out/kernel"]).T), o.bias.copy_(t(w[name + "/out/bias"]))
                    self.heads[name] = nn.Sequential(d, bn, nn.ReLU(), nn.Dropout(0.4), o)

        def forward(self, xin):                                                         # (N, T, F) as Keras feeds it
            h = self.initial(xin.permute(0, 2, 1))
            for b in self.blocks:
                h = b(h)
            trunk = torch.relu(h).permute(0, 2, 1)                                      # (N, T, C): Keras Flatten order
            flat = trunk.reshape(trunk.shape[0], -1)
            outs = []
            for name, _, act in b3_mtl.head_spec(ncls):
                z = self.heads[name](flat)
                outs.append(torch.sigmoid(z) if act == "sigmoid" else z)
            outs.append(torch.softmax(self.c3(flat), dim=1))
            return outs, trunk

    net = Net().double().eval()
    with torch.no_grad():
        ref_outs, ref_trunk = net(t(x))
    outs, trunk = b3_mtl.forward(x, w, n_classes=ncls, return_trunk=True)
    np.testing.assert_allclose(trunk, ref_trunk.numpy(), atol=1e-6, rtol=1e-6)
    assert len(outs) == len(ref_outs)
    for a, b in zip(outs, ref_outs):
        assert a.shape == tuple(b.shape)
        np.testing.assert_allclose(a, b.numpy(), atol=1e-6)


def _scaled_v2_weights(F, W, nb, nd, scale=0.5, seed=9):
    """init_weights_v2 with the convolution kernels scaled as the GPU tests of the 2.8 block scale them (no channel normalisation:
    the trunk of unscaled glorot kernels grows with every block)."""
    w = b3_mtl.init_weights_v2(seed=seed, n_feat=F, patch_size=W, n_classes=3, nb_stacks=nb, n_dil=nd, randomize_bn=True)
    for k in w:
        if "/conv" in k and k.endswith("kernel"):
            w[k] = (w[k] * scale).astype(np.float32)
    return w


@pytest.mark.parametrize("F,nb,nd,W", [(240, 3, 8, 68), (32, 1, 1, 25), (61, 3, 3, 50), (32, 3, 8, 68), (20, 1, 1, 25)])
def test_b3mtl_v2_trunk_vs_torch_conv1d(F, nb, nd, W):
    """oracle.b3_mtl.tcn_forward_v2 (the residual block of keras-tcn >= 2.8) against a float64 build of the same trunk from
    torch.nn.functional.conv1d with the same weights: per (stack, dilation d) two Conv1D(32, 3, dilation d, 'same') -- padding d,
    kernels permuted from Keras' (k, cin, cout) to torch's (cout, cin, k) -- each followed by relu, a 1x1 'matching' convolution
    on the shortcut only where the block's input does not have 32 channels (the first block, unless n_feat == 32: identity), relu
    of the sum.  No initial convolution, nothing behind the last block.  The same 1e-6 as the 2.3 cross-check above; the outputs
    are mtl_heads on the flattened trunk, which that cross-check pins."""
    import torch
    import torch.nn.functional as tf
    w = _scaled_v2_weights(F, W, nb, nd)
    assert (("tcn/s0_d1/matching/kernel" in w) == (F != 32)) and not any("/matching/" in k for k in w if not k.startswith("tcn/s0_d1/"))
    x = np.random.default_rng(F + W).standard_normal((4, W, F)).astype(np.float32)

    def t(a):
        return torch.tensor(np.asarray(a, np.float64))

    def conv(h, p, d):                                                                  # h: (N, C, T)
        return tf.conv1d(h, t(w[p + "/kernel"]).permute(2, 1, 0), t(w[p + "/bias"]), padding=d * (w[p + "/kernel"].shape[0] // 2),
                         dilation=d)

    h = t(x).permute(0, 2, 1)
    for s in range(nb):
        for i in range(nd):
            d, p = 2 ** i, "tcn/s%d_d%d" % (s, 2 ** i)
            y = torch.relu(conv(torch.relu(conv(h, p + "/conv0", d)), p + "/conv1", d))
            sc = conv(h, p + "/matching", 1) if h.shape[1] != 32 else h
            h = torch.relu(sc + y)
    ref = h.permute(0, 2, 1).numpy()                                                    # (N, T, C): Keras Flatten order
    got = b3_mtl.tcn_forward_v2(x, w, nb, nd)
    assert got.shape == ref.shape == (4, W, 32) and got.dtype == np.float32
    assert 0.1 <= ref.max() <= 200 and np.mean(ref == 0) <= 0.9                         # a live trunk, not a dead or exploded one
    np.testing.assert_allclose(got, ref, atol=1e-6, rtol=1e-6)


def test_b3mtl_forward_follows_the_weight_dict_to_the_v2_block():
    """b3_mtl.forward (and through it oracle.inference.patch_probabilities) takes the two-convolution trunk for a dict from
    init_weights_v2, identity first block included."""
    for F in (32, 40):
        w = _scaled_v2_weights(F, 25, 3, 8)
        x = np.random.default_rng(F).standard_normal((3, 25, F)).astype(np.float32)
        outs, trunk = b3_mtl.forward(x, w, return_trunk=True)
        assert np.array_equal(trunk, b3_mtl.tcn_forward_v2(x, w))
        for a, b in zip(outs, b3_mtl.mtl_heads(trunk.reshape(3, -1), w, 3)):
            assert np.array_equal(a, b)


# ---- transformers.audio_utils: an independent, librosa-compatible implementation of the mel filter bank, the dB conversion and
# the spectrogram (the feature extraction behind Whisper etc., written to reproduce librosa's numbers) that IS installed here.
def test_mel_basis_vs_transformers_audio_utils():
    """`oracle.frontend.mel_basis(22050, 400, 120)` -- the restatement of librosa.filters.mel(sr=22050, n_fft=400, n_mels=120,
    fmin=0, fmax=sr/2, htk=False, norm='slaney'), the bank the reference gets through its `sr` quirk -- against
    transformers.audio_utils.mel_filter_bank(norm='slaney', mel_scale='slaney'): float32 rounding apart (2.4e-9 absolute), the
    same 393 non-zero taps and the same single all-zero filter (both libraries warn about it, as librosa does)."""
    au = pytest.importorskip("transformers.audio_utils")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = au.mel_filter_bank(201, 120, 0.0, 11025.0, 22050, norm="slaney", mel_scale="slaney").T   # (120, 201) float64
    got = ofe.mel_basis(22050.0, 400, 120)
    assert got.shape == ref.shape == (120, 201) and got.dtype == np.float32
    assert np.max(np.abs(got - ref)) <= 5e-9
    assert np.array_equal(got > 0, ref > 0) and int((got > 0).sum()) == 393
    assert np.array_equal(np.flatnonzero(got.sum(1) == 0), np.flatnonzero(ref.sum(1) == 0)) and int((got.sum(1) == 0).sum()) == 1
    # Jang's bank (librosa.filters.mel(16000, n_fft=512, n_mels=120), lib/proposed_architectures.py:681)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref2 = au.mel_filter_bank(257, 120, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T
    assert np.max(np.abs(ofe.mel_basis(16000.0, 512, 120) - ref2)) <= 5e-9


def test_power_to_db_vs_transformers_audio_utils():
    """librosa.core.power_to_db(x, ref=1.0, amin=1e-10, top_db=80.0) as restated against transformers' power_to_db with the same
    three constants: 1e-5 dB (float32 log10)."""
    au = pytest.importorskip("transformers.audio_utils")
    rng = np.random.default_rng(0)
    x = (np.abs(rng.standard_normal((120, 98))) * 3).astype(np.float32)
    x[5, :7] = 0.0          # below amin
    x[9, 3] = 1e-7          # below the top_db floor of this array
    ref = au.power_to_db(x.astype(np.float64) ** 2, reference=1.0, min_value=1e-10, db_range=80.0)
    got = ofe.power_to_db(x ** 2)
    assert got.dtype == np.float32 and np.max(np.abs(got - ref)) <= 1e-4
    assert abs(float(got.min()) - (float(got.max()) - 80.0)) <= 1e-4


def test_stft_mel_db_chain_vs_transformers_spectrogram(clips4):
    """|STFT| (center=False, periodic Hann 400 / hop 160) -> mel(22050 quirk) -> dB with top_db 80, i.e. the reference's
    LogMel branch WITHOUT the HPSS masks (for which no second implementation exists offline), end to end against
    transformers.audio_utils.spectrogram(power=1, mel_filters=, log_mel='dB', db_range=80): 2e-3 dB on every bin above the
    floor (the two chains round |S| differently: complex64 here, float64 there)."""
    au = pytest.importorskip("transformers.audio_utils")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fb = au.mel_filter_bank(201, 120, 0.0, 11025.0, 22050, norm="slaney", mel_scale="slaney")
    win = au.window_function(400, "hann", periodic=True)
    assert np.array_equal(win, ofe.hann_window(400, 400)) or np.max(np.abs(win - ofe.hann_window(400, 400))) < 1e-15
    for y in clips4[:2]:
        ref = au.spectrogram(y.astype(np.float64), win, frame_length=400, hop_length=160, fft_length=400, power=1.0, center=False,
                             mel_filters=fb, mel_floor=1e-5, log_mel="dB", reference=1.0, min_value=1e-5, db_range=80.0,
                             dtype=np.float64)
        got = ofe.power_to_db(ofe.mel_project(ofe.stft_mag(y), 120) ** 2)
        assert got.shape == ref.shape == (120, 98)
        live = (ref > ref.max() - 79.9) & (got > got.max() - 79.9)   # off both floors (the empty filter row sits on them)
        assert live.mean() > 0.98 and np.max(np.abs(got[live] - ref[live])) <= 2e-3
        assert abs(float(got.max()) - float(ref.max())) <= 1e-3


def test_rms_vs_torch_unfold():
    """`oracle.silence.rms` = librosa.feature.rms(frame_length, hop_length) with librosa 0.8's defaults (center=True,
    pad_mode='reflect') against torch: reflect-pad by frame_length // 2 (no edge repeat), `unfold` into frames, root mean square.
    1 + N // hop frames (101 for the 1 s clip), float32 rounding apart."""
    import torch
    from oracle import silence as osil
    rng = np.random.default_rng(2)
    for n, fl, hop in ((16000, 400, 160), (12345, 400, 160), (4000, 512, 128)):
        y = rng.standard_normal(n).astype(np.float32)
        got = osil.rms(y, fl, hop)
        yp = torch.nn.functional.pad(torch.from_numpy(y).double()[None, None], (fl // 2, fl // 2), mode="reflect")[0, 0]
        ref = yp.unfold(0, fl, hop).pow(2).mean(dim=1).sqrt().numpy()
        assert got.shape == ref.shape == (1 + n // hop,)
        assert np.max(np.abs(got - ref)) <= 2e-6 * ref.max()
