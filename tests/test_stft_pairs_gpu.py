"""GPU: stft400_kernel (csrc/smh_stft.hip) with phase 1 on a fixed column per thread and phase 3 in frame pairs, n_fft 400 and the
default window.

The kernel takes the two forms per tile: phase 1 keeps its window and twiddle column in registers when the tile's frames fit three
rounds of blockDim.x / 25 frame groups (nf <= 30 at 256 threads), and phase 3 handles two neighbouring frames per item when nf, t0
and T are even and the clip's S starts on an 8-byte boundary.  Every other tile runs the round-robin phase 1 with its LDS tables
and one frame per phase-3 item; SMH_STFT_PAIRS=0 forces that on every tile.  Both are re-arrangements: the bits must not move.

Shapes (hop 160, B in {1, 3}): T = 1 (no pair), 2 (one pair), 19 (an odd tile), 20 (one full tile), 21 (an odd and an even tile:
11 + 10), 22 (12 + 10: the launcher keeps tiles even for an even T), 40 (two full tiles), 41 (14 + 14 + 13), 98 (the headline:
5 x 20, the last with 18); T in {20, 21} at hops 2 and 402.  Checked per case:

1. S against oracle.frontend.stft_mag, |S - ref| <= 1e-5 max(ref) per clip (the bound of tests/test_stft_f32_shapes_gpu.py);
2. NaN directly in front of and behind the audio (in bounds: a read outside a clip turns outputs into NaN) and a guard clip of NaN
   behind S that must stay NaN;
3. SMH_STFT_PAIRS=0 gives the same bits, and so does the plain grid (SMH_STFT_XCD=0) against the per-XCD one;
4. 32-frame tiles (SMH_STFT_FRAMES=32,256) at T = 30 (fixed column, pairs), 31 (neither), 32 (LDS tables, pairs), 63 (32 + 31): the
   same bits as the default plan, with and without SMH_STFT_PAIRS=0;
5. one ragged call of clips with T = 20, 21, 98, 1 against the same clips run alone.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import frontend as ofe

pytestmark = pytest.mark.gpu

TOL = 1e-5  # include/smh.h: |S| within 1e-5 of max|S| of the reference's, per clip
K = 201
SWITCHES = ("SMH_STFT_PAIRS", "SMH_STFT_XCD", "SMH_STFT_FRAMES", "SMH_STFT_GENERIC", "SMH_STFT_ROW", "SMH_STFT_PROBE_NOSTORE")
_CACHE = {}


def _fe(hop):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    if ("fe", hop) not in _CACHE:
        _CACHE["fe", hop] = Frontend(FrontendConfig(n_fft=400, win_length=400, hop=hop, n_mels=0))
    return _CACHE["fe", hop]


def _clips(hop, T, B=3):
    """B clips of 400 + (T - 1) hop samples (even: the specialised route at any B), cut from three synthetic clips made once."""
    if "y" not in _CACHE:
        from sm_hpss_mtl_amd.synth import synth_clips
        _CACHE["y"] = synth_clips(3, seed=43, n_samples=16000)
    n = 400 + (T - 1) * hop
    assert n <= 16000 and ofe.num_frames(n, 400, hop) == T
    return np.ascontiguousarray(_CACHE["y"][:B, :n])


def _ref(hop, T, i):
    """oracle.frontend.stft_mag of clip i of _clips(hop, T), computed once."""
    if ("ref", hop, T, i) not in _CACHE:
        _CACHE["ref", hop, T, i] = ofe.stft_mag(_clips(hop, T)[i], n_fft=400, win_length=400, hop=hop)
    return _CACHE["ref", hop, T, i]


def _stft(fe, y):
    """smh_stft_mag_f32 through the C ABI: the audio between NaN, S with a guard clip of NaN behind it -> S (B, K, T) on the device."""
    from sm_hpss_mtl_amd import _lib
    B, n = y.shape
    T = ofe.num_frames(n, 400, fe.cfg.hop)
    front = 1022  # even: the clip stays on an 8-byte boundary
    buf = torch.full((front + y.size + 64,), float("nan"), dtype=torch.float32, device="cuda")
    buf[front:front + y.size] = torch.from_numpy(y.ravel()).cuda()
    x = buf[front:front + y.size].view(B, n)
    assert x.data_ptr() % 8 == 0
    f = fe.lib.smh_internal_stft_route
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert f(fe._h, C.c_void_p(x.data_ptr()), B, n) == 1, "not the specialised kernel"
    out = torch.full((B + 1, K, T), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(fe.lib.smh_stft_mag_f32(fe._h, C.c_void_p(x.data_ptr()), B, n, C.c_void_p(out.data_ptr()), _lib.current_stream()),
               "smh_stft_mag_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B]).all()), "the guard clip behind S was written"
    assert bool(torch.isfinite(out[:B]).all()), "NaN in S: a read outside a clip, or an element left unwritten"
    return out[:B].clone()


@pytest.fixture
def env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _check_oracle(S, hop, T):
    S = S.cpu().numpy()
    worst = 0.0
    for i in range(S.shape[0]):
        ref = _ref(hop, T, i)
        assert S[i].shape == ref.shape
        m = float(ref.max())
        err = float(np.max(np.abs(S[i].astype(np.float64) - ref.astype(np.float64))))
        worst = max(worst, err / m)
        assert err <= TOL * m, (hop, T, i, err / m)
    return worst


CASES = [(160, T, B) for T in (1, 2, 19, 20, 21, 22, 40, 41, 98) for B in (1, 3)] + [(hop, T, 3) for hop in (2, 402) for T in (20, 21)]


@pytest.mark.parametrize("hop,T,B", CASES, ids=lambda v: str(v))
def test_pairs_against_the_oracle_and_the_single_frame_path(hop, T, B, env):
    fe, y = _fe(hop), _clips(hop, T, B)
    S = _stft(fe, y)
    worst = _check_oracle(S, hop, T)
    print("stft pairs hop %d T %d B %d: worst |S - ref| / max(ref) = %.3g" % (hop, T, B, worst))
    env.setenv("SMH_STFT_XCD", "0")
    assert torch.equal(_stft(fe, y), S), "SMH_STFT_XCD=0 against 1"
    env.setenv("SMH_STFT_PAIRS", "0")
    assert torch.equal(_stft(fe, y), S), "SMH_STFT_PAIRS=0, plain grid"
    env.delenv("SMH_STFT_XCD")
    S0 = _stft(fe, y)
    _check_oracle(S0, hop, T)
    assert torch.equal(S0, S), "SMH_STFT_PAIRS=0"


@pytest.mark.parametrize("T", [30, 31, 32, 63])
def test_pairs_under_32_frame_tiles(T, env):
    fe, y = _fe(160), _clips(160, T)
    S = _stft(fe, y)
    _check_oracle(S, 160, T)
    env.setenv("SMH_STFT_FRAMES", "32,256")
    assert torch.equal(_stft(fe, y), S), "SMH_STFT_FRAMES=32,256"
    env.setenv("SMH_STFT_XCD", "0")
    assert torch.equal(_stft(fe, y), S), "SMH_STFT_FRAMES=32,256, SMH_STFT_XCD=0"
    env.setenv("SMH_STFT_PAIRS", "0")
    assert torch.equal(_stft(fe, y), S), "SMH_STFT_FRAMES=32,256, SMH_STFT_XCD=0, SMH_STFT_PAIRS=0"
    env.delenv("SMH_STFT_XCD")
    assert torch.equal(_stft(fe, y), S), "SMH_STFT_FRAMES=32,256, SMH_STFT_PAIRS=0"


def test_pairs_in_a_ragged_call(env):
    """A plain configuration without a filterbank or dB returns S itself as its featuregram, so run_ragged shows the ragged STFT's S."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    fe = Frontend(FrontendConfig(hpss=False, n_fft=400, win_length=400, hop=160, n_mels=0, log_db=False))
    Ts = [20, 21, 98, 1]
    clips = [_clips(160, T)[i % 3].copy() for i, T in enumerate(Ts)]
    alone = []
    for c, T in zip(clips, Ts):
        x = torch.from_numpy(c[None]).cuda()
        S = fe.stft_mag(x)
        assert S.shape == (1, K, T) and torch.equal(fe.plain_features(S)["fv"], S)
        alone.append(S[0])
    for pairs in (None, "0"):
        if pairs is not None:
            env.setenv("SMH_STFT_PAIRS", pairs)
        res = fe.run_ragged(clips)
        torch.cuda.synchronize()
        assert res["T"] == Ts
        for b, T in enumerate(Ts):
            assert res["fv"][b].shape == (K, T)
            assert torch.equal(res["fv"][b], alone[b]), (pairs, b, T)
