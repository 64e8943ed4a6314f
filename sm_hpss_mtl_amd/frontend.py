"""Device-resident batched front end: thin host wrapper over the C ABI (include/smh.h).

torch is plumbing here (device memory + the current HIP stream); every computation happens in
libsmh.so.  Inputs/outputs are float32 CUDA(=HIP) tensors, spectrogram-like tensors are (B, rows, T).
"""
from __future__ import annotations

import collections
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

# featName -> (n_mels used?, log?)   (lib/preprocessing.py:404-444; only the '*HarmPerc*' branches are
# on the hot path -- SURVEY 8a)
FEATS = {
    "MelHarmPercSpec": (True, False),
    "LogMelHarmPercSpec": (True, True),
    "HarmPercSpec": (False, False),
    "LogHarmPercSpec": (False, True),
}
# One-half feature names (the intermediate-fusion driver, Intermediate_Fusion_Results.py:704-706) -> their '*HarmPercSpec' sibling:
# get_featuregram computes the same H||P featuregram for them (lib/preprocessing.py:404-444); get_feature_patches keeps one half.
HALF_FEATS = {h + t: h + "HarmPercSpec" for h in ("Mel", "LogMel", "", "Log") for t in ("HarmSpec", "PercSpec")}
# The four branches without harmonic-percussive separation (lib/preprocessing.py:378-402), same (n_mels used?, log?) meaning.  Their
# mel basis is built for sr = fs and applied to the POWER spectrogram (melspectrogram(y=Xin, sr=fs, ...): include/smh.h, smh_plain_*).
PLAIN_FEATS = {
    "Spec": (False, False),
    "LogSpec": (False, True),
    "MelSpec": (True, False),
    "LogMelSpec": (True, True),
}
# Frontend's `layout` argument -> the C ABI's patch_layout (include/smh.h): "image" (nP, 2*rows, W), what get_feature_patches returns
# and the Conv2D models read; "time_major" (nP, W, 2*rows), the TCN's input.  A plain configuration has rows in place of 2*rows.
LAYOUTS = {"image": 0, "time_major": 1}
# FrontendConfig.stft_precision -> the C ABI's stft_precision (include/smh.h: SMH_STFT_F32 / SMH_STFT_F64)
STFT_PRECISIONS = {"f32": _lib.SMH_STFT_F32, "f64": _lib.SMH_STFT_F64}


def _l0_kernel(model):
    """(device address of the (rows_in, 32) layer-0 kernel the feature kernel multiplies by, rows_in) of a model with a fused
    layer-0 path: B3MTL / cascaded -- its initial-conv kernel, rows_in = n_feat; FusionMTL -- trunk H's kernel followed by trunk
    P's, rows_in = 2 * n_feat; late_fusion.LateFusion -- model H's kernel followed by model P's, rows_in = 2 * n_feat.  Anything else
    raises."""
    from .model import HEADS_FUSION
    if getattr(model, "LATE_FUSION", False):
        return model.w0_ptr(), 2 * model.n_feat
    model._sync_weights()
    fusion = getattr(model, "HEADS", None) == HEADS_FUSION
    w0 = model.lib.smh_fusion_w0_ptr(model._h) if fusion else model.lib.smh_model_w0_ptr(model._h)
    if not w0:
        raise ValueError("the model has no layer-0 kernel the feature kernel could apply (keras-tcn 2.3.x block only)")
    return w0, (2 if fusion else 1) * model.n_feat


@dataclass(frozen=True)
class FrontendConfig:
    n_fft: int = 400
    win_length: int = 400
    hop: int = 160
    n_mels: int = 120
    l_harm: int = 21
    l_perc: int = 11
    log_db: bool = True
    mel_sr: float = 22050.0
    # "f32": the fast STFT (|S| within 1e-5 of max|S| of the reference's); "f64": an f64 transform whose |S| equals
    # np.abs(librosa.core.stft(...)) bit for bit (include/smh.h: smh_ctx_create_ex).  Everything after the STFT is the same.
    stft_precision: str = "f32"
    # False: one of PLAIN_FEATS -- no medians, no soft masks, one featuregram of `rows` rows per clip instead of the H || P pair
    # (l_harm / l_perc are then ignored, and mel_sr is the audio's sampling rate)
    hpss: bool = True

    def __post_init__(self):
        if self.stft_precision not in STFT_PRECISIONS:
            raise ValueError("stft_precision must be one of %s, got %r" % (sorted(STFT_PRECISIONS), self.stft_precision))

    @staticmethod
    def from_params(PARAMS, n_fft, n_mels, featName, fs=16000):
        """Build from the reference's PARAMS dict (Proposed_Work_Results.py:723-807)."""
        if featName in PLAIN_FEATS:  # PARAMS needs no l_harm / l_perc for these
            use_mel, log = PLAIN_FEATS[featName]
            return FrontendConfig(
                n_fft=int(n_fft), win_length=int(PARAMS["Tw"] * fs / 1000), hop=int(PARAMS["Ts"] * fs / 1000),
                n_mels=int(n_mels) if use_mel else 0, log_db=log, mel_sr=float(fs),
                stft_precision=PARAMS.get("stft_precision", "f32"), hpss=False)
        featName = HALF_FEATS.get(featName, featName)
        if featName not in FEATS:
            raise ValueError("featName %r is not one of the feature names %s"
                             % (featName, sorted(FEATS) + sorted(HALF_FEATS) + sorted(PLAIN_FEATS)))
        use_mel, log = FEATS[featName]
        model = PARAMS["Model"]
        return FrontendConfig(
            n_fft=int(n_fft), win_length=int(PARAMS["Tw"] * fs / 1000), hop=int(PARAMS["Ts"] * fs / 1000),
            n_mels=int(n_mels) if use_mel else 0, l_harm=int(PARAMS["l_harm"][model]),
            l_perc=int(PARAMS["l_perc"][model]), log_db=log, stft_precision=PARAMS.get("stft_precision", "f32"))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _layout(layout):
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (sorted(LAYOUTS), layout))
    return LAYOUTS[layout]


def _patch_shape(n, W, F, layout):
    return (n, F, W) if layout == "image" else (n, W, F)


def _stream():
    return _lib.current_stream()


def _out(out, key, shape, dtype, dev):
    """A caller-supplied output tensor (steady-state loops allocate nothing) or a fresh one.  The C ABI receives raw
    pointers without sizes, so a stale `out` dict from a smaller batch must never reach it: wrong shape / dtype / device
    raises here."""
    t = out.get(key) if out else None
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous()):
        raise ValueError("out[%r] must be a contiguous %s tensor on %s" % (key, dtype, dev))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("out[%r] has shape %s, this call writes %s" % (key, tuple(t.shape), tuple(shape)))
    return t


def _maxkeys(out, n, what, dev):
    """The int32 max-key scratch of a features call: out['maxkeys'] if the caller keeps one (at least n entries; `what` names n in
    the error text), else a fresh tensor."""
    keys = (out or {}).get("maxkeys")
    if keys is None:
        return torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if not (keys.is_cuda and keys.dtype == torch.int32 and keys.numel() >= n and keys.is_contiguous()):
        raise ValueError("out['maxkeys'] must be a contiguous int32 device tensor with at least %s = %d entries" % (what, n))
    return keys


def _f32c(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA/HIP torch tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    return t.contiguous()


# What differs between the harmonic-percussive (True) and the plain front end in Frontend.run / run_ragged: featuregram rows per
# feat_rows, taps, the four entries (each takes a patch layout behind `shift`) and the label a ragged error carries.
_Family = collections.namedtuple("_Family", "row_mult taps workspace equal ragged_sizes ragged ragged_label")
_FAMILIES = {
    True: _Family(2, ("S", "harm", "perc"), "smh_frontend_workspace_bytes", "smh_frontend_layout_f32", "smh_frontend_ragged_sizes",
                  "smh_frontend_ragged_layout_f32", "smh_frontend_ragged_f32"),
    False: _Family(1, ("S",), "smh_plain_frontend_workspace_bytes", "smh_plain_frontend_layout_f32", "smh_plain_frontend_ragged_sizes",
                   "smh_plain_frontend_ragged_layout_f32", "smh_plain_frontend_ragged_f32"),
}


class Frontend:
    """Owns one `smh_ctx` (window, FFT twiddles, mel CSR tables) for a fixed configuration."""

    def __init__(self, cfg: FrontendConfig = FrontendConfig()):
        self.lib = _lib.require_gpu()
        self.cfg = cfg
        c = _lib.FrontendCfg(cfg.n_fft, cfg.win_length, cfg.hop, cfg.n_mels, cfg.l_harm, cfg.l_perc,
                             1 if cfg.log_db else 0, cfg.mel_sr)
        h = C.c_void_p()
        _lib.check(self.lib.smh_ctx_create_ex(C.byref(c), STFT_PRECISIONS[cfg.stft_precision], C.byref(h)), "smh_ctx_create_ex")
        self._h = h
        self.K = 1 + cfg.n_fft // 2
        self.rows = self.lib.smh_ctx_feat_rows(self._h)
        self._work = None
        self._family = _FAMILIES[bool(cfg.hpss)]

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.smh_ctx_destroy(h)
            self._h = None

    # ---- integer contracts ----
    def num_frames(self, n_samples: int) -> int:
        return self.lib.smh_num_frames(n_samples, self.cfg.n_fft, self.cfg.hop)

    def num_patches(self, T: int, W: int, shift: int) -> int:
        return _lib.check(self.lib.smh_num_patches(self.lib.smh_tiled_frames(T, W), W, shift), "smh_num_patches")

    def mel_basis(self) -> np.ndarray:
        out = np.empty((self.cfg.n_mels, self.K), np.float32)
        _lib.check(self.lib.smh_ctx_mel_basis(self._h, out.ctypes.data_as(C.c_void_p)), "smh_ctx_mel_basis")
        return out

    # ---- stage-by-stage API (one call per reference call) ----
    def stft_mag(self, audio):
        audio = _f32c(audio, "audio")
        B, N = audio.shape
        T = self.num_frames(N)
        if T < 1:
            raise ValueError("clip of %d samples is shorter than n_fft=%d" % (N, self.cfg.n_fft))
        S = torch.empty((B, self.K, T), dtype=torch.float32, device=audio.device)
        _lib.check(self.lib.smh_stft_mag_f32(self._h, _ptr(audio), B, N, _ptr(S), _stream()), "smh_stft_mag_f32")
        return S

    def _need_hpss(self, what):
        if not self.cfg.hpss:
            raise ValueError("%s belongs to the harmonic-percussive path; this Frontend has a plain configuration (hpss=False): "
                             "use plain_features / run" % what)

    def hpss_median(self, S, l_harm=None, l_perc=None):
        self._need_hpss("hpss_median")
        S = _f32c(S, "S")
        B, K, T = S.shape
        lh = self.cfg.l_harm if l_harm is None else l_harm
        lp = self.cfg.l_perc if l_perc is None else l_perc
        harm, perc = torch.empty_like(S), torch.empty_like(S)
        _lib.check(self.lib.smh_hpss_median_f32(self._h, _ptr(S), B, K, T, lh, lp, _ptr(harm), _ptr(perc), _stream()),
                   "smh_hpss_median_f32")
        return harm, perc

    def median_time(self, S, l_harm):
        S = _f32c(S, "S")
        B, K, T = S.shape
        out = torch.empty_like(S)
        _lib.check(self.lib.smh_median_time_f32(self._h, _ptr(S), B, K, T, l_harm, _ptr(out), _stream()),
                   "smh_median_time_f32")
        return out

    def median_freq(self, S, l_perc):
        S = _f32c(S, "S")
        B, K, T = S.shape
        out = torch.empty_like(S)
        _lib.check(self.lib.smh_median_freq_f32(self._h, _ptr(S), B, K, T, l_perc, _ptr(out), _stream()),
                   "smh_median_freq_f32")
        return out

    def softmask(self, S, harm, perc):
        S, harm, perc = _f32c(S, "S"), _f32c(harm, "harm"), _f32c(perc, "perc")
        if not (S.shape == harm.shape == perc.shape):
            raise ValueError("softmask: shape mismatch %s %s %s" % (S.shape, harm.shape, perc.shape))
        H, P = torch.empty_like(S), torch.empty_like(S)
        _lib.check(self.lib.smh_softmask_f32(self._h, _ptr(S), _ptr(harm), _ptr(perc), S.numel(), _ptr(H), _ptr(P),
                                             _stream()), "smh_softmask_f32")
        return H, P

    # ---- HPSS audio separation (librosa.effects.hpss with this framing; include/smh.h a3') ----
    def _audio_2d(self, audio, who):
        """(audio as (B, N), whether it came 1-D)"""
        audio = _f32c(audio, "audio")
        if audio.dim() not in (1, 2):
            raise ValueError("%s: audio must be (B, N) or (N,), got shape %s" % (who, tuple(audio.shape)))
        one = audio.dim() == 1
        audio = audio[None] if one else audio
        if audio.shape[1] < self.cfg.n_fft:
            raise ValueError("%s: clip of %d samples is shorter than n_fft=%d" % (who, audio.shape[1], self.cfg.n_fft))
        return audio, one

    def resynth(self, audio, harm, perc, out=None):
        """`smh_hpss_resynth_f32`, the resynthesis kernel alone: audio (B, N) or (N,), harm / perc (B, K, T) or (K, T) (the medians of
        |STFT|, or any non-negative pair) -> dict(harmonic, percussive), float32 device tensors of audio's shape:
        istft(stft(audio) * softmask(harm, perc)) and istft(stft(audio) * softmask(perc, harm)).  `out` may carry preallocated
        'harmonic' / 'percussive' tensors."""
        self._need_hpss("resynth")
        audio, one = self._audio_2d(audio, "resynth")
        harm, perc = _f32c(harm, "harm"), _f32c(perc, "perc")
        B, N = audio.shape
        shape = (B, self.K, self.num_frames(N))
        if one and harm.dim() == 2 and perc.dim() == 2:
            harm, perc = harm[None], perc[None]
        if tuple(harm.shape) != shape or tuple(perc.shape) != shape:
            raise ValueError("resynth: harm %s and perc %s must be %s" % (tuple(harm.shape), tuple(perc.shape), shape))
        yshape = (N,) if one else (B, N)
        yh = _out(out, "harmonic", yshape, torch.float32, audio.device)
        yp = _out(out, "percussive", yshape, torch.float32, audio.device)
        _lib.check(self.lib.smh_hpss_resynth_f32(self._h, _ptr(audio), B, N, _ptr(harm), _ptr(perc), _ptr(yh), _ptr(yp), _stream()),
                   "smh_hpss_resynth_f32")
        return {"harmonic": yh, "percussive": yp}

    def separate(self, audio, out=None):
        """`smh_hpss_audio_f32`: audio (B, N) -> dict(harmonic (B, N), percussive (B, N)), float32 device tensors --
        librosa.effects.hpss(y, kernel_size=(l_harm, l_perc)) with this configuration's framing; bit for bit
        resynth(audio, *hpss_median(stft_mag(audio))).  A 1-D input gives 1-D outputs.  A list of 1-D signals of different lengths
        is grouped by length, one call per distinct length (signal by signal for an odd length under the f32 STFT, see below), and
        returns lists in the caller's order, each entry bit for bit what the signal gives alone (`out` is for tensors only)."""
        self._need_hpss("separate")
        if isinstance(audio, (list, tuple)):
            if out is not None:
                raise ValueError("separate: `out` is not supported for a list of signals")
            sigs = [_f32c(s, "audio[%d]" % i) for i, s in enumerate(audio)]
            for i, s in enumerate(sigs):
                if s.dim() != 1:
                    raise ValueError("separate: audio[%d] must be 1-D, got shape %s" % (i, tuple(s.shape)))
            groups = collections.OrderedDict()
            for i, s in enumerate(sigs):
                groups.setdefault(int(s.shape[0]), []).append(i)
            res = {"harmonic": [None] * len(sigs), "percussive": [None] * len(sigs)}
            for n, idx in groups.items():
                # Every signal gets bit for bit what it gets alone.  The resynthesis kernel and the f64 STFT give that in any batch;
                # the f32 STFT picks its kernel by where the clips start (smh_stft_plan.h: frames_aligned8), and in a batch of an odd
                # length all clips but the first start off 8-byte boundaries: such a group goes signal by signal.
                alone = self.cfg.stft_precision == "f32" and n % 2 == 1 and len(idx) > 1
                for part in ([[i] for i in idx] if alone else [idx]):
                    got = self.separate(torch.stack([sigs[i] for i in part]))
                    for row, i in enumerate(part):
                        res["harmonic"][i], res["percussive"][i] = got["harmonic"][row], got["percussive"][row]
            return res
        audio, one = self._audio_2d(audio, "separate")
        B, N = audio.shape
        dev = audio.device
        yshape = (N,) if one else (B, N)
        yh = _out(out, "harmonic", yshape, torch.float32, dev)
        yp = _out(out, "percussive", yshape, torch.float32, dev)
        need = self.lib.smh_hpss_audio_workspace_bytes(self._h, B, N)
        if self._work is None or self._work.numel() < need or self._work.device != dev:
            self._work = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        _lib.check(self.lib.smh_hpss_audio_f32(self._h, _ptr(audio), B, N, _ptr(yh), _ptr(yp), _ptr(self._work), self._work.numel(),
                                               _stream()), "smh_hpss_audio_f32")
        return {"harmonic": yh, "percussive": yp}

    def separate_ragged(self, signals, out=None):
        """`smh_hpss_audio_ragged_f32`: signals of DIFFERENT lengths in one call, one launch per stage for all of them.  signals: list
        of 1-D float32 arrays / tensors -> dict(harmonic=[...], percussive=[...]) in the caller's order, each entry a 1-D view of one
        flat buffer per component and bit for bit what `separate` gives that signal alone.  The signals are packed at offsets that
        are multiples of 4 samples, as `run_ragged` packs them; `out` may carry the two flat float32 buffers 'harmonic' /
        'percussive' (sum of the lengths, each rounded up to 4; the floats between signals are not written)."""
        self._need_hpss("separate_ragged")
        B = len(signals)
        if B == 0:
            return {"harmonic": [], "percussive": []}
        for i, s in enumerate(signals):
            if s.ndim != 1:
                raise ValueError("separate_ragged: signals[%d] must be 1-D, got shape %s" % (i, tuple(s.shape)))
            if s.shape[0] < self.cfg.n_fft:
                raise ValueError("separate_ragged: signals[%d] of %d samples is shorter than n_fft=%d" % (i, s.shape[0], self.cfg.n_fft))
        dev = torch.device("cuda", torch.cuda.current_device())
        lens = [int(s.shape[0]) for s in signals]
        offs, o = [], 0
        for n in lens:
            offs.append(o)
            o += (n + 3) // 4 * 4  # next signal starts on a 16-byte boundary
        if all(isinstance(s, np.ndarray) for s in signals):
            # host signals: laid out in ONE host buffer and uploaded by ONE copy
            host = np.zeros(o, dtype=np.float32)
            for s, n, of in zip(signals, lens, offs):
                host[of:of + n] = s
            audio = torch.from_numpy(host).to(device=dev)
        else:
            audio = torch.zeros(o, dtype=torch.float32, device=dev)
            for s, n, of in zip(signals, lens, offs):
                t = s if isinstance(s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32))
                audio[of:of + n] = t.to(device=dev, dtype=torch.float32)
        yh = _out(out, "harmonic", (o,), torch.float32, dev)
        yp = _out(out, "percussive", (o,), torch.float32, dev)
        h_off, h_len = (C.c_longlong * B)(*offs), (C.c_int * B)(*lens)
        work = C.c_size_t()
        _lib.check(self.lib.smh_hpss_audio_ragged_sizes(self._h, h_off, h_len, B, None, C.byref(work)), "smh_hpss_audio_ragged_sizes")
        if self._work is None or self._work.numel() < work.value or self._work.device != dev:
            self._work = torch.empty(max(work.value, 1), dtype=torch.uint8, device=dev)
        _lib.check(self.lib.smh_hpss_audio_ragged_f32(self._h, _ptr(audio), h_off, h_len, B, _ptr(yh), _ptr(yp), _ptr(self._work),
                                                      self._work.numel(), _stream()), "smh_hpss_audio_ragged_f32")
        return {"harmonic": [yh[of:of + n] for of, n in zip(offs, lens)], "percussive": [yp[of:of + n] for of, n in zip(offs, lens)]}

    def mel(self, X):
        X = _f32c(X, "X")
        B, K, T = X.shape
        if K != self.K:
            raise ValueError("mel: expected %d bins, got %d" % (self.K, K))
        Y = torch.empty((B, self.cfg.n_mels, T), dtype=torch.float32, device=X.device)
        _lib.check(self.lib.smh_mel_f32(self._h, _ptr(X), B, T, _ptr(Y), _stream()), "smh_mel_f32")
        return Y

    def power_to_db_sq(self, X):
        """power_to_db(X**2) with the top_db max taken per leading-axis entry."""
        X = _f32c(X, "X")
        n = X.shape[0]
        Y = torch.empty_like(X)
        _lib.check(self.lib.smh_power_to_db_sq_f32(self._h, _ptr(X), n, X.numel() // max(n, 1), _ptr(Y), _stream()),
                   "smh_power_to_db_sq_f32")
        return Y

    def standardize_rows(self, X):
        X = _f32c(X, "X")
        T = X.shape[-1]
        Y = torch.empty_like(X)
        _lib.check(self.lib.smh_standardize_rows_f32(self._h, _ptr(X), X.numel() // T, T, _ptr(Y), _stream()),
                   "smh_standardize_rows_f32")
        return Y

    def extract_patches(self, FV, W, shift, time_major=False):
        FV = _f32c(FV, "FV")
        B, F, T = FV.shape
        nP = self.num_patches(T, W, shift)
        shape = (B * nP, W, F) if time_major else (B * nP, F, W)
        out = torch.empty(shape, dtype=torch.float32, device=FV.device)
        got = _lib.check(self.lib.smh_extract_patches_f32(self._h, _ptr(FV), B, F, T, W, shift, 1 if time_major else 0,
                                                          _ptr(out) if nP else None, _stream()), "smh_extract_patches_f32")
        assert got == nP
        return out

    def features(self, S, harm, perc, W=None, shift=None, out=None, layout="time_major"):
        """(S, harm, perc) -> dict(fv[, patches]): masks + mel + dB, then standardise + patches: (B*nP, W, 2*rows) time-major, or
        (B*nP, 2*rows, W) with layout="image"."""
        self._need_hpss("features")
        lay = _layout(layout)
        S, harm, perc = _f32c(S, "S"), _f32c(harm, "harm"), _f32c(perc, "perc")
        B, K, T = S.shape
        dev = S.device
        fv = _out(out, "fv", (B, 2 * self.rows, T), torch.float32, dev)
        nP, patches = 0, None
        if W is not None:
            nP = self.num_patches(T, W, shift)
            patches = _out(out, "patches", _patch_shape(B * nP, W, 2 * self.rows, layout), torch.float32, dev)
        keys = _maxkeys(out, 2 * B, "2*B", dev)
        got = _lib.check(self.lib.smh_features_layout_f32(self._h, _ptr(S), _ptr(harm), _ptr(perc), 0, B, T, W or 0, shift or 0, lay,
                                                          _ptr(fv), _ptr(patches) if nP else None, _ptr(keys), _stream()),
                         "smh_features_layout_f32")
        assert got == nP
        return {"fv": fv, "patches": patches, "n_patches": nP, "maxkeys": keys}

    def features_l0(self, S, harm, perc, harm_layout, W, shift, model, out=None, patches=False):
        """`features` fused with the first layer of `model` (B3MTL): returns dict(fv, x0p (B*nP, 2, W, 32)[, patches]).
        Feed x0p to `model.forward_from_x0`.  Same logits as features -> forward_device within f32 tolerance.
        A FusionMTL whose 2 * n_feat equals the featuregram's rows works too: half 0 of x0p is then trunk H's first layer,
        half 1 trunk P's, and x0p goes to `model.forward_from_x0_halves`.  The same holds for a late_fusion.LateFusion ensemble
        (half 0 is model H's first layer, half 1 model P's)."""
        self._need_hpss("features_l0")
        S, harm, perc = _f32c(S, "S"), _f32c(harm, "harm"), _f32c(perc, "perc")
        B, K, T = S.shape
        if int(harm_layout) == 2 and harm.numel() < B * self.lib.smh_harm_buffer_floats(K, T):
            raise ValueError("harm_layout 2 needs smh_harm_buffer_floats(K, T) floats per clip")
        w0, rows_in = _l0_kernel(model)
        if rows_in != 2 * self.rows or model.patch_size != W:
            raise ValueError("model expects (W=%d, n_feat=%d), the front end produces (W=%d, n_feat=%d)"
                             % (model.patch_size, rows_in, W, 2 * self.rows))
        nP = self.num_patches(T, W, shift)
        dev = S.device
        fv = _out(out, "fv", (B, 2 * self.rows, T), torch.float32, dev)
        x0p = _out(out, "x0p", (B * nP, 2, W, 32), torch.float32, dev)
        pt = _out(out, "patches", (B * nP, W, 2 * self.rows), torch.float32, dev) if patches else None
        keys = _maxkeys(out, 2 * B, "2*B", dev)
        got = _lib.check(self.lib.smh_features_l0_f32(
            self._h, _ptr(S), _ptr(harm), _ptr(perc), int(harm_layout), B, T, W, shift, _ptr(fv), _ptr(pt),
            C.c_void_p(w0), _ptr(x0p), _ptr(keys), _stream()), "smh_features_l0_f32")
        assert got == nP
        return {"fv": fv, "x0p": x0p, "patches": pt, "n_patches": nP, "maxkeys": keys}

    def plain_features(self, S, W=None, shift=None, out=None, **options):
        """Plain configurations (hpss=False): S (B, K, T) -> dict(fv (B, rows, T)[, patches (B*nP, W, rows)]) -- Spec / LogSpec /
        MelSpec / LogMelSpec of lib/preprocessing.py:378-402 behind the STFT, then tile-if-short, StandardScaler per row and
        time-major patches (`smh_plain_features_layout_f32`).  The one option is layout="image": patches (B*nP, rows, W), the
        single-task Conv2D baselines' images.  (It is a keyword option, not a named parameter: tests/test_image_layout_abi.py pins
        this method's named parameters.)"""
        layout = options.pop("layout", "time_major")
        if options:
            raise TypeError("plain_features: unexpected keyword argument %r" % sorted(options)[0])
        lay = _layout(layout)
        if self.cfg.hpss:
            raise ValueError("plain_features needs a plain configuration (FrontendConfig(hpss=False)); this one is harmonic-percussive")
        S = _f32c(S, "S")
        if S.dim() != 3 or S.shape[1] != self.K:
            raise ValueError("plain_features: S must be (B, %d, T), got %s" % (self.K, tuple(S.shape)))
        B, K, T = S.shape
        dev = S.device
        fv = _out(out, "fv", (B, self.rows, T), torch.float32, dev)
        nP, patches = 0, None
        if W is not None:
            nP = self.num_patches(T, W, shift)
            patches = _out(out, "patches", _patch_shape(B * nP, W, self.rows, layout), torch.float32, dev)
        keys = _maxkeys(out, B, "B", dev)
        got = _lib.check(self.lib.smh_plain_features_layout_f32(self._h, _ptr(S), B, T, W or 0, shift or 0, lay, _ptr(fv),
                                                                _ptr(patches) if nP else None, _ptr(keys), _stream()),
                         "smh_plain_features_layout_f32")
        assert got == nP
        return {"fv": fv, "patches": patches, "n_patches": nP, "maxkeys": keys}

    # ---- fused fast path ----
    def _geometry(self, W, shift, layout):
        """The (W, shift, patch layout) arguments of this configuration's fused entries."""
        return (W or 0, shift or 0, _layout(layout))

    def run(self, audio, W=None, shift=None, taps=False, out=None, layout="time_major"):
        """audio (B, n_samples) -> dict(fv=(B, 2*rows, T)[, patches=(B*nP, W, 2*rows)][, S, harm, perc]).
        layout="image": patches=(B*nP, 2*rows, W), the Conv2D models' images, written by the same kernels (no transpose pass).
        `out` may carry preallocated 'fv' / 'patches' tensors (steady-state loops allocate nothing).
        A plain configuration (hpss=False) gives fv=(B, rows, T) and patches=(B*nP, W, rows) or, with layout="image",
        (B*nP, rows, W); its only tap is S."""
        fam = self._family
        geom = self._geometry(W, shift, layout)
        F, names = fam.row_mult * self.rows, fam.taps
        audio = _f32c(audio, "audio")
        B, N = audio.shape
        T = self.num_frames(N)
        if T < 1:
            raise ValueError("clip of %d samples is shorter than n_fft=%d" % (N, self.cfg.n_fft))
        dev = audio.device
        out = {} if out is None else out
        fv = out.get("fv")
        if fv is None or fv.shape != (B, F, T):
            fv = torch.empty((B, F, T), dtype=torch.float32, device=dev)
        patches, nP = None, 0
        if W is not None:
            nP = self.num_patches(T, W, shift)
            patches = out.get("patches")
            if patches is None or patches.shape != _patch_shape(B * nP, W, F, layout):
                patches = torch.empty(_patch_shape(B * nP, W, F, layout), dtype=torch.float32, device=dev)
        need = getattr(self.lib, fam.workspace)(self._h, B, N)
        if self._work is None or self._work.numel() < need or self._work.device != dev:
            self._work = torch.empty(need if self.cfg.hpss else max(need, 1), dtype=torch.uint8, device=dev)
        tap = {k: torch.empty((B, self.K, T), dtype=torch.float32, device=dev) for k in names} if taps else {}
        got = _lib.check(getattr(self.lib, fam.equal)(self._h, _ptr(audio), B, N, *geom, _ptr(fv), _ptr(patches) if nP else None,
                                                      _ptr(self._work), self._work.numel(), *(_ptr(tap.get(k)) for k in names),
                                                      _stream()), fam.equal)
        assert got == nP, (got, nP)
        res = {"fv": fv, "n_patches": nP}
        if W is not None:
            res["patches"] = patches
        res.update(tap)
        return res

    # ---- ragged batches ----
    def run_ragged(self, clips, W=None, shift=None, layout="time_major"):
        """Clips of DIFFERENT lengths in one call (`smh_frontend_ragged_layout_f32`).  clips: list of 1-D float32 arrays / tensors.
        Returns dict(fv=[(2*rows, T_b) tensors], patches=[(nP_b, W, 2*rows) tensors] (views of one buffer each; (nP_b, 2*rows, W)
        with layout="image"), n_patches=[...], T=[...]).  Every clip gets bit for bit what `run` gives it alone or in an equal-length batch:
        the clips are laid out at 16-byte aligned offsets, so each takes the same kernels as there.  (Not an equal-length
        batch of an odd number of samples: its clips start off 8-byte boundaries and take the generic STFT kernel, whose S
        differs from the specialised kernel's in the last bits.)"""
        fam, geom = self._family, self._geometry(W, shift, layout)
        B = len(clips)
        if B == 0:
            return {"fv": [], "patches": [], "n_patches": [], "T": []}
        dev = torch.device("cuda", torch.cuda.current_device())
        lens = [int(c.shape[0]) for c in clips]
        offs, o = [], 0
        for n in lens:
            offs.append(o)
            o += (n + 3) // 4 * 4  # next clip starts on a 16-byte boundary
        for c in clips:
            if c.ndim != 1:
                raise ValueError("run_ragged: every clip must be 1-D")
        if all(isinstance(c, np.ndarray) for c in clips):
            # host clips: laid out in ONE host buffer and uploaded by ONE copy (a copy per clip is a host synchronisation per clip)
            host = np.zeros(max(o, 1), dtype=np.float32)
            for c, n, of in zip(clips, lens, offs):
                host[of:of + n] = c
            audio = torch.from_numpy(host).to(device=dev)
        else:
            audio = torch.zeros(max(o, 1), dtype=torch.float32, device=dev)
            for c, n, of in zip(clips, lens, offs):
                t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32))
                audio[of:of + n] = t.to(device=dev, dtype=torch.float32)
        h_off = (C.c_longlong * B)(*offs)
        h_len = (C.c_int * B)(*lens)
        fv_off, p_off = (C.c_longlong * (B + 1))(), (C.c_longlong * (B + 1))()
        hT, hnP = (C.c_int * B)(), (C.c_int * B)()
        work = C.c_size_t()
        # a plain configuration (hpss=False) takes the plain pair of entries: same contract, (rows, T_b) and (nP_b, W, rows) or
        # (nP_b, rows, W) per clip
        _lib.check(getattr(self.lib, fam.ragged_sizes)(self._h, h_off, h_len, B, W or 0, shift or 0, fv_off, p_off, hT, hnP,
                                                       C.byref(work)), fam.ragged_sizes)
        F = fam.row_mult * self.rows
        fv = torch.empty(max(int(fv_off[B]), 1), dtype=torch.float32, device=dev)
        patches = torch.empty(_patch_shape(max(int(p_off[B]), 1), W or 1, F, layout), dtype=torch.float32, device=dev) if W else None
        if self._work is None or self._work.numel() < work.value or self._work.device != dev:
            self._work = torch.empty(max(work.value, 1), dtype=torch.uint8, device=dev)
        _lib.check(getattr(self.lib, fam.ragged)(self._h, _ptr(audio), h_off, h_len, B, *geom, _ptr(fv),
                                                 _ptr(patches) if (W and int(p_off[B]) > 0) else None, _ptr(self._work),
                                                 self._work.numel(), _stream()), fam.ragged_label)
        res = {"fv": [fv[int(fv_off[b]):int(fv_off[b + 1])].view(F, int(hT[b])) for b in range(B)],
               "T": [int(hT[b]) for b in range(B)], "n_patches": [int(hnP[b]) for b in range(B)]}
        if W:
            res["patches"] = [patches[int(p_off[b]):int(p_off[b + 1])] for b in range(B)]
        return res

    def patches_from_featuregram(self, fv, W, shift, layout="time_major"):
        """get_feature_patches on the device: featuregram (2*rows, T) [rows 0..F/2-1 harmonic] -> standardised patches
        (tile-if-short, StandardScaler per half, extract_patches): time-major (nP, W, 2*rows) for the TCN models (the transpose
        included), or layout="image": (nP, 2*rows, W) as get_feature_patches returns them, for the Conv2D models."""
        _layout(layout)
        fv = _f32c(fv, "fv")
        if fv.dim() != 2:
            raise ValueError("FV should be of the shape (nFeatures, nFrames)")
        x = self.standardize_rows(fv)  # per row over the frames: the per-half scaler is row-wise, so halves need no split
        return self.extract_patches(x[None], W, shift, time_major=layout == "time_major")

    # ---- frame-level scaling (PARAMS['frame_level_scaling']): featuregrams that are already on the device ----
    @staticmethod
    def _fv_table(fvs, who):
        """(kept tensors, device-pointer array, frame-count array, rows) of a list of (rows, T_b) float32 device featuregrams."""
        if len(fvs) == 0:
            raise ValueError("%s: no featuregrams" % who)
        keep = [_f32c(t, "%s: fvs[%d]" % (who, i)) for i, t in enumerate(fvs)]
        rows = int(keep[0].shape[0]) if keep[0].dim() == 2 else -1
        for i, t in enumerate(keep):
            if t.dim() != 2 or int(t.shape[0]) != rows or int(t.shape[1]) < 1:
                raise ValueError("%s: fvs[%d] has shape %s; every featuregram must be (rows = %d, T >= 1)" % (who, i, tuple(t.shape), rows))
        B = len(keep)
        return keep, (C.c_void_p * B)(*[t.data_ptr() for t in keep]), (C.c_int * B)(*[int(t.shape[1]) for t in keep]), rows

    def row_moments(self, fvs):
        """`smh_row_moments_f64`: fvs, a list of (rows, T_b) float32 device featuregrams (the HPSS pair's 2 * rows or the plain rows:
        whatever the tensors have) -> (sum (B, rows) float64, m2 (B, rows) float64 = sum((x - sum / T_b)^2), nonfinite (B, rows) int32).
        A clip's values are bit for bit the same alone and in any batch."""
        keep, h_fv, h_T, rows = self._fv_table(fvs, "row_moments")
        B, dev = len(keep), keep[0].device
        mom = torch.empty((B, rows, 2), dtype=torch.float64, device=dev)
        bad = torch.empty((B, rows), dtype=torch.int32, device=dev)
        _lib.check(self.lib.smh_row_moments_f64(self._h, h_fv, h_T, B, rows, _ptr(mom), _ptr(bad), _stream()), "smh_row_moments_f64")
        return mom[..., 0], mom[..., 1], bad

    def scaled_patches(self, fvs, mean, stdev, W, shift, layout="time_major"):
        """`smh_scaled_patches_f32`: scale_data + extract_patches of every featuregram in ONE launch.  fvs as for `row_moments`;
        mean, stdev: one value per featuregram row (arrays or tensors; read as float64).  Every element is
        float32((float64(x) - mean[r]) / (stdev[r] + 1e-10)).  Returns a list of per-clip views of one patch buffer, shaped as
        `run_ragged`'s: (nP_b, W, rows) time-major, (nP_b, rows, W) with layout="image"."""
        lay = _layout(layout)
        keep, h_fv, h_T, rows = self._fv_table(fvs, "scaled_patches")
        B, dev = len(keep), keep[0].device
        stats = []
        for name, v in (("mean", mean), ("stdev", stdev)):
            t = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v), dtype=np.float64))
            t = t.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
            if t.numel() != rows:
                raise ValueError("scaled_patches: %s has %d values, the featuregrams have %d rows" % (name, t.numel(), rows))
            stats.append(t)
        p_off = (C.c_longlong * (B + 1))()
        total = _lib.check(self.lib.smh_scaled_patches_count(h_T, B, int(W), int(shift), p_off), "smh_scaled_patches_count")
        patches = torch.empty(_patch_shape(max(int(total), 1), int(W), rows, layout), dtype=torch.float32, device=dev)
        _lib.check(self.lib.smh_scaled_patches_f32(self._h, h_fv, h_T, B, rows, _ptr(stats[0]), _ptr(stats[1]), int(W), int(shift), lay,
                                                   _ptr(patches), _stream()), "smh_scaled_patches_f32")
        return [patches[int(p_off[b]):int(p_off[b + 1])] for b in range(B)]

    # ---- the skewness-vector feed (PARAMS['skewness_vector']): statistics of every patch, no patch written ----
    _STATS = {"mean": 0, "variance": 1, "skew": 2, "kurtosis": 3}

    def patch_statistics(self, fvs, W, shift, axis, stat="skew", mean=None, stdev=None, dtype=torch.float32):
        """`smh_patch_statistics`: tools.get_data_statistics(patches, stat, axis) of every patch of every featuregram in ONE call,
        straight from the featuregrams.  fvs as for `row_moments`.  The value under the statistic is the patch element
        `patches_from_featuregram` writes (per-file StandardScaler) or, with mean / stdev (one value per row, read as float64),
        `scaled_patches`'.  axis=1: over a patch's W frames -> (nP_b, rows); axis=0: over its rows -> (nP_b, W).  The statistic is
        float64; dtype=torch.float32 rounds it once.  Returns a list of per-clip views of one buffer.  Argument errors are
        ValueErrors raised before anything is launched."""
        if axis not in (0, 1):
            raise ValueError("patch_statistics: axis must be 0 (over the rows) or 1 (over the frames), got %r" % (axis,))
        if stat not in self._STATS:
            raise ValueError("patch_statistics: stat must be one of %s, got %r" % (sorted(self._STATS), stat))
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("patch_statistics: dtype must be torch.float32 or torch.float64, got %r" % (dtype,))
        W, shift = int(W), int(shift)
        if W < 1 or shift < 1:
            raise ValueError("patch_statistics: bad patch geometry W=%d shift=%d" % (W, shift))
        if (mean is None) != (stdev is None):
            raise ValueError("patch_statistics: mean and stdev come together or not at all")
        keep, h_fv, h_T, rows = self._fv_table(fvs, "patch_statistics")
        B, dev = len(keep), keep[0].device
        stats = [None, None]
        if mean is not None:
            for k, (name, v) in enumerate((("mean", mean), ("stdev", stdev))):
                t = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v), dtype=np.float64))
                t = t.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
                if t.numel() != rows:
                    raise ValueError("patch_statistics: %s has %d values, the featuregrams have %d rows" % (name, t.numel(), rows))
                stats[k] = t
        p_off = (C.c_longlong * (B + 1))()
        total = _lib.check(self.lib.smh_scaled_patches_count(h_T, B, W, shift, p_off), "smh_scaled_patches_count")
        out = torch.empty((max(int(total), 1), rows if axis == 1 else W), dtype=dtype, device=dev)
        need = int(self.lib.smh_patch_statistics_workspace_bytes(B, rows, axis, int(mean is not None)))
        work = torch.empty(need // 8, dtype=torch.float64, device=dev) if need else None
        _lib.check(self.lib.smh_patch_statistics(self._h, h_fv, h_T, B, rows, _ptr(stats[0]), _ptr(stats[1]), W, shift,
                                                 self._STATS[stat], axis, int(dtype == torch.float32), _ptr(out), _ptr(work), need,
                                                 _stream()),
                   "smh_patch_statistics")
        return [out[int(p_off[b]):int(p_off[b + 1])] for b in range(B)]
