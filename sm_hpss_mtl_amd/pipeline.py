"""The hot path as ONE object with preallocated device buffers: audio (B, n_samples) -> logits (B*nP, out_dim).

    STFT -> HPSS medians (l_harm x l_perc) -> soft masks -> mel -> dB -> standardise -> patches -> B3_MTL forward

= `get_featuregram` (lib/preprocessing.py:414-424) + `get_feature_patches` (:137-142, 208-234) + `model.predict`
(Proposed_Work_Results.py:459-496, 520) for a batch of equal-length clips that is already resident in HBM.  Four
launches per step through the C ABI (include/smh.h), no allocation, no host synchronisation.

`bench.py` times exactly `HotPath.step`; `tests/test_bench_path_gpu.py` compares exactly `HotPath.step` with the
oracle -- the timed configuration and the tested configuration are the same code.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .model import HEADS_FUSION

STAGES = ("stft", "median", "features", "model")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class HotPath:
    def __init__(self, fe, model, batch, n_samples, patch=68, shift=None, fuse_l0=True, two_kernel_features=False,
                 model_dtype="f32", keep_patches=False, keep_trunk=False, device=None):
        """fe: Frontend, model: B3MTL, or None for the front end alone (BASELINE config 2, "HPSS-only": three launches, the step
        ends with the featuregram; no patches, no logits).  fuse_l0: the network's first 1x1 convolution runs inside the feature kernel
        (smh_features_l0_f32 + smh_model_forward_x0_f32) instead of patches -> smh_model_forward_f32.  A model of the keras-tcn 2.8
        block (tcn_block="2.8") has no such convolution: fuse_l0 falls back to the patch path (`self.fuse_l0` is False) and
        model_dtype="bf16" is refused here.
        keep_patches / keep_trunk: also write the standardised time-major patches / the TCN output (N, W, 32) -- parity taps
        that `model.predict` does not return; never set by bench.py.
        model may be a FusionMTL whose 2 * n_feat equals the featuregram's rows (f32, no trunk tap).  fuse_l0=True: the feature
        kernel applies both trunks' first layers (smh_fusion_w0_ptr) and the model starts from the per-half partials
        (forward_from_x0_halves); nothing of the patches is built.  fuse_l0=False: patches -> their two halves -> forward_device;
        the halves of a (N, W, 2 * n_feat) patch tensor are strided views, so this path COPIES them into two contiguous tensors
        every step (preallocated; the model's C ABI takes contiguous inputs).
        model may also be a late_fusion.LateFusion ensemble (f32, no trunk tap), fed exactly like the FusionMTL: fuse_l0=True -- the
        feature kernel applies both models' first layers (`w0_ptr()`) and forward_from_x0_halves starts from the per-half partials;
        fuse_l0=False -- the two contiguous halves of the patches go to forward_device.  `logits` is then the blended '3C'
        (B * nP, n_classes)."""
        if not fe.cfg.hpss:
            # Spec / LogSpec / MelSpec / LogMelSpec: no medians and no layer-0 fusion to schedule; audio -> logits on that path is
            # fe.run(...)["patches"] -> model.forward_device
            raise ValueError("HotPath drives the harmonic-percussive front end; a plain Frontend (hpss=False) goes "
                             "fe.run(audio, W, shift)['patches'] -> model.forward_device")
        self.fe, self.model, self.lib, self._h = fe, model, fe.lib, fe._h
        self.B, self.n_samples, self.W = int(batch), int(n_samples), int(patch)
        self.shift = int(patch if shift is None else shift)
        self.model_dtype = model_dtype
        if model_dtype not in ("f32", "bf16"):
            raise ValueError("model_dtype must be 'f32' or 'bf16'")
        self.fuse_l0 = bool(fuse_l0) and model is not None  # both network dtypes start from the layer-0 partials
        if model is not None and getattr(model, "block_variant", 0) != 0:
            # the keras-tcn 2.8 block has no initial 1x1 convolution to fuse and no split-bf16 forward: decided here, not by a
            # refusal in the middle of step()
            if model_dtype != "f32":
                raise ValueError("the keras-tcn 2.8 block (tcn_block=%r) has the f32 forward only, got model_dtype=%r"
                                 % (model.tcn_block, model_dtype))
            self.fuse_l0 = False  # patches -> forward_device
        self.late = model is not None and getattr(model, "LATE_FUSION", False)
        if self.late and model_dtype != "f32":
            raise ValueError("the late-fusion ensemble has the f32 forward only, got model_dtype=%r" % (model_dtype,))
        if self.late and keep_trunk:
            raise ValueError("the late-fusion ensemble has no trunk tap (keep_trunk)")
        # (two per-half inputs: the ensemble takes the FusionMTL's route through the step)
        self.fusion = model is not None and (getattr(model, "HEADS", None) == HEADS_FUSION or self.late)
        if self.fusion and model_dtype != "f32":
            raise ValueError("the intermediate-fusion model has the f32 forward only, got model_dtype=%r" % (model_dtype,))
        if self.fusion and keep_trunk:
            raise ValueError("the intermediate-fusion model has no trunk tap (keep_trunk)")
        rows_in = (2 if self.fusion else 1) * model.n_feat if model is not None else 0
        self.T = fe.num_frames(self.n_samples)
        if self.T < 1:
            raise ValueError("clip of %d samples is shorter than n_fft=%d" % (n_samples, fe.cfg.n_fft))
        if model is not None and (rows_in != 2 * fe.rows or model.patch_size != self.W):
            raise ValueError("model expects (W=%d, n_feat=%d), the front end produces (W=%d, n_feat=%d)"
                             % (model.patch_size, rows_in, self.W, 2 * fe.rows))
        self.nP = fe.num_patches(self.T, self.W, self.shift) if model is not None else 0
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        B, K, T, F = self.B, fe.K, self.T, 2 * fe.rows
        f32 = dict(dtype=torch.float32, device=dev)
        self.S = torch.empty((B, K, T), **f32)
        self.perc = torch.empty_like(self.S)
        self.harm = torch.empty((B, self.lib.smh_harm_buffer_floats(K, T)), **f32)  # room for every harm layout
        self.fv = torch.empty((B, F, T), **f32)
        self.maxkeys = torch.empty(2 * max(B, 1), dtype=torch.int32, device=dev)
        need_patches = (keep_patches or not self.fuse_l0) and model is not None
        self.patches = torch.empty((B * self.nP, self.W, F), **f32) if need_patches else None
        self.x0p = torch.empty((B * self.nP, 2, self.W, 32), **f32) if self.fuse_l0 else None
        # fusion model on patches: the contiguous copies of the two halves
        self.halves = ([torch.empty((B * self.nP, self.W, F // 2), **f32) for _ in range(2)]
                       if self.fusion and not self.fuse_l0 else None)
        self.logits = torch.empty((B * self.nP, model.out_dim), **f32) if model is not None else None
        self.trunk = torch.empty((B * self.nP, self.W, 32), **f32) if (keep_trunk and model_dtype == "f32" and model is not None) else None
        # harmonic median layout: 16-frame blocks when the single feature kernel takes the clip, else time-major
        blocked = self.lib.smh_features_blocked_ok(self._h, T, 1 if self.fuse_l0 else 0) and not two_kernel_features
        self.want_layout = 2 if blocked else 1
        self.layout = None  # what the median launch actually wrote (set by step)

    def step(self, audio, record=None):
        """One pass over one batch.  `record`: five torch.cuda.Event (timing) recorded on the launch stream around
        the four stages, or None.  Returns the logits tensor (B*nP, out_dim) = [S | M | (N) | R | 3C]."""
        if audio.shape != (self.B, self.n_samples) or audio.dtype != torch.float32 or not audio.is_cuda:
            raise ValueError("audio must be a float32 device tensor of shape (%d, %d)" % (self.B, self.n_samples))
        lib, h, fe, m = self.lib, self._h, self.fe, self.model
        st = _lib.current_stream()
        if m is not None:
            m._sync_weights()
        if record is not None:
            record[0].record()
        _lib.check(lib.smh_stft_mag_f32(h, _p(audio), self.B, self.n_samples, _p(self.S), st), "smh_stft_mag_f32")
        if record is not None:
            record[1].record()
        lay = _lib.check(lib.smh_hpss_median_ex_f32(h, _p(self.S), self.B, fe.K, self.T, fe.cfg.l_harm, fe.cfg.l_perc,
                                                    _p(self.harm), _p(self.perc), self.want_layout, st),
                         "smh_hpss_median_ex_f32")
        self.layout = lay
        if record is not None:
            record[2].record()
        if self.fuse_l0:
            w0 = m.w0_ptr() if self.late else (lib.smh_fusion_w0_ptr(m._h) if self.fusion else lib.smh_model_w0_ptr(m._h))
            got = _lib.check(lib.smh_features_l0_f32(h, _p(self.S), _p(self.harm), _p(self.perc), lay, self.B, self.T,
                                                     self.W, self.shift, _p(self.fv), _p(self.patches),
                                                     C.c_void_p(w0), _p(self.x0p),
                                                     _p(self.maxkeys), st), "smh_features_l0_f32")
        else:
            got = _lib.check(lib.smh_features_ex_f32(h, _p(self.S), _p(self.harm), _p(self.perc), lay, self.B, self.T,
                                                     self.W if m is not None else 0, self.shift if m is not None else 0,
                                                     _p(self.fv), _p(self.patches), _p(self.maxkeys), st), "smh_features_ex_f32")
        if got != self.nP:
            raise RuntimeError("feature stage produced %d patches per clip, expected %d" % (got, self.nP))
        if record is not None:
            record[3].record()
        if m is None:
            if record is not None:
                record[4].record()
            return self.fv
        if self.fusion:
            if self.fuse_l0:
                m.forward_from_x0_halves(self.x0p, out=self.logits)
            else:
                R = self.patches.shape[2] // 2
                self.halves[0].copy_(self.patches[:, :, :R])
                self.halves[1].copy_(self.patches[:, :, R:])
                m.forward_device(self.halves, out=self.logits)
        elif self.fuse_l0:
            m.forward_from_x0(self.x0p, out=self.logits, trunk=self.trunk, dtype=self.model_dtype)
        else:
            m.forward_device(self.patches, out=self.logits, trunk=self.trunk, dtype=self.model_dtype)
        if record is not None:
            record[4].record()
        return self.logits

    def harm_bkt(self):
        """The harmonic medians of the last step decoded to the reference's (B, K, T) layout (parity tap)."""
        B, K, T = self.B, self.fe.K, self.T
        if self.layout == 2:
            G = (T + 15) // 16
            return self.harm[:, :G * K * 16].view(B, G, K, 16).permute(0, 2, 1, 3).reshape(B, K, G * 16)[:, :, :T]
        if self.layout == 1:
            return self.harm[:, :K * T].view(B, T, K).transpose(1, 2)
        return self.harm[:, :K * T].view(B, K, T)
