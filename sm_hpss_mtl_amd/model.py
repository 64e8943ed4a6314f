"""B3_MTL host object: a Keras-style facade (`predict`, `get_weights`, `save_weights`, `to_json`, ...) over
the `smh_model` C ABI.  Mirrors what the reference's drivers call on the object returned by
`get_Lemaire_MTL_model` (lib/proposed_architectures.py:85-170; Proposed_Work_Results.py:345-374,520,586).

Weights are kept on the host as float32 numpy arrays in CANONICAL order (Keras array layouts):
  tcn/initial_conv kernel (1,F,32), bias (32)
  per (stack s, dilation d): conv kernel (3,32,32), bias, conv1x1 kernel (1,32,32), bias
  3C kernel (T*32, n_classes), bias
  per head (S, M, [N,] R): dense kernel (T*32,16), bias, BN gamma, beta, moving_mean, moving_variance,
                           out kernel (16, odim), out bias
  (CascadedMTL: heads S, M, R; S and M carry cat_bn gamma, beta, moving_mean, moving_variance (18 each) between their
   moving_variance and an out kernel of shape (18, 1))
  (FusionMTL: two trunks 'tcn_H/...' and 'tcn_P/...' in place of 'tcn/...', then the fused BatchNorm 'fusion_bn' gamma, beta,
   moving_mean, moving_variance (2*T*32 each); '3C' and the heads read the 2*T*32 fused features)
  (SingleTaskTCN: the trunk, then 'dense' kernel (T*32, n_classes), bias -- Keras' name for the baseline's only Dense layer)
and uploaded (re-packed into MFMA operand order by libsmh) whenever they change: the weight store, the Keras weight surface,
`predict` and the call helpers are host.HostModel's, shared with cnn_models.CnnMTL; the training surface is
training.TcnTrainingMixin's.
"""
from __future__ import annotations

import ctypes as C
import json
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .host import HEADS_CASCADED, HEADS_FUSION, HEADS_MTL, HEADS_SINGLE, HostModel, SingleOutputMixin, f32_cuda, head_spec, ptr, to_f32_cuda, workspace
from .training import TRAIN_ALL, TcnTrainingMixin

CAT = 18  # cascaded heads: width of concat[Dropout(16) of S or M, R's two outputs]


def weight_spec(n_feat, patch_size, n_classes, nb_filters=32, kernel_size=3, nb_stacks=3, n_dil=8, block_variant=0,
                heads=HEADS_MTL):
    """Ordered (name, shape, fan_in, fan_out|None) in canonical order; fan_out None -> not glorot.
    block_variant 0: the keras-tcn 2.3.x block; 1: the two-convolution block of keras-tcn >= 2.8 (include/smh.h).
    heads HEADS_CASCADED: S and M carry the concatenation BatchNorm 'cat_bn' (18) and an out kernel (18, 1).
    heads HEADS_FUSION: two trunks 'tcn_H' / 'tcn_P' (n_feat = the per-branch width), the fused BatchNorm 'fusion_bn' over
    D = 2 * patch_size * nb_filters features, then '3C' and the MTL heads on D inputs.
    heads HEADS_SINGLE: the trunk, then 'dense' (D, n_classes) in the place of '3C'; no heads."""
    Cf, D = nb_filters, patch_size * nb_filters
    if heads == HEADS_FUSION:
        if block_variant != 0:
            raise ValueError("the intermediate-fusion model is built for the keras-tcn 2.3.x block only")
        spec = []
        for t in ("tcn_H", "tcn_P"):
            spec += [(t + n[3:], shp, fi, fo) for n, shp, fi, fo in
                     weight_spec(n_feat, patch_size, n_classes, nb_filters, kernel_size, nb_stacks, n_dil) if n.startswith("tcn/")]
        D = 2 * D
        spec += [("fusion_bn/gamma", (D,), 1, None), ("fusion_bn/beta", (D,), 0, None),
                 ("fusion_bn/moving_mean", (D,), 0, None), ("fusion_bn/moving_variance", (D,), 1, None)]
        spec += [(n, shp if n != "3C/kernel" and not n.endswith("/dense/kernel") else (D,) + tuple(shp[1:]),
                  D if (n == "3C/kernel" or n.endswith("/dense/kernel")) else fi, fo)
                 for n, shp, fi, fo in weight_spec(n_feat, patch_size, n_classes, nb_filters, kernel_size, nb_stacks, n_dil)
                 if not n.startswith("tcn/")]
        return spec
    spec = []
    if block_variant == 0:
        spec = [("tcn/initial_conv/kernel", (1, n_feat, Cf), n_feat, Cf), ("tcn/initial_conv/bias", (Cf,), 0, None)]
    cin = n_feat
    for s in range(nb_stacks):
        for i in range(n_dil):
            p = "tcn/s%d_d%d" % (s, 2 ** i)
            if block_variant == 0:
                spec += [(p + "/conv/kernel", (kernel_size, Cf, Cf), kernel_size * Cf, kernel_size * Cf),
                         (p + "/conv/bias", (Cf,), 0, None),
                         (p + "/conv1x1/kernel", (1, Cf, Cf), Cf, Cf), (p + "/conv1x1/bias", (Cf,), 0, None)]
            else:
                spec += [(p + "/conv0/kernel", (kernel_size, cin, Cf), kernel_size * cin, kernel_size * Cf), (p + "/conv0/bias", (Cf,), 0, None),
                         (p + "/conv1/kernel", (kernel_size, Cf, Cf), kernel_size * Cf, kernel_size * Cf), (p + "/conv1/bias", (Cf,), 0, None)]
                if cin != Cf:
                    spec += [(p + "/matching/kernel", (1, cin, Cf), cin, Cf), (p + "/matching/bias", (Cf,), 0, None)]
                cin = Cf
    out = "dense" if heads == HEADS_SINGLE else "3C"
    spec += [(out + "/kernel", (D, n_classes), D, n_classes), (out + "/bias", (n_classes,), 0, None)]
    for name, odim, _ in head_spec(n_classes, heads):
        spec += [(name + "/dense/kernel", (D, 16), D, 16), (name + "/dense/bias", (16,), 0, None),
                 (name + "/bn/gamma", (16,), 1, None), (name + "/bn/beta", (16,), 0, None),
                 (name + "/bn/moving_mean", (16,), 0, None), (name + "/bn/moving_variance", (16,), 1, None)]
        hin = 16
        if heads == HEADS_CASCADED and name != "R":
            hin = CAT
            spec += [(name + "/cat_bn/gamma", (CAT,), 1, None), (name + "/cat_bn/beta", (CAT,), 0, None),
                     (name + "/cat_bn/moving_mean", (CAT,), 0, None), (name + "/cat_bn/moving_variance", (CAT,), 1, None)]
        spec += [(name + "/out/kernel", (hin, odim), hin, odim), (name + "/out/bias", (odim,), 0, None)]
    return spec


def initial_weights(n_feat=240, patch_size=68, n_classes=3, seed=None, nb_filters=32, kernel_size=3, nb_stacks=3,
                    n_dilations=8, block_variant=0, heads=HEADS_MTL):
    """(dropout_rate, OrderedDict name -> float32 array) of a freshly built model: Keras defaults (glorot_uniform
    kernels, zero biases, BatchNormalization gamma = moving_variance = 1) and the build-time draw of the spatial
    dropout rate (proposed_architectures.py:136).  Host-only (numpy): `B3MTL.__init__` and the generator of
    tests/golden/bench_golden.npz both call it, so `B3MTL(seed=s)` is reproducible without a GPU."""
    rng = np.random.default_rng(seed)
    dropout_rate = float(rng.uniform(0.05, 0.5))
    weights = OrderedDict()
    for name, shape, fan_in, fan_out in weight_spec(n_feat, patch_size, n_classes, nb_filters, kernel_size, nb_stacks,
                                                    n_dilations, block_variant, heads):
        if fan_out is not None:
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            weights[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        else:
            weights[name] = np.full(shape, float(fan_in), np.float32)
    return dropout_rate, weights


class B3MTL(TcnTrainingMixin, HostModel):
    """`model` object of get_Lemaire_MTL_model.  Inference runs entirely in libsmh (HIP)."""

    CLASS_NAME = "B3_MTL"
    _DENSE_ENTRY, _DENSE_WORKSPACE = "smh_model_forward_dense_f32", "smh_model_dense_workspace_bytes"
    _DENSE_ENTRY_BF16 = "smh_model_forward_dense_bf16"  # B3_MTL alone: every other model refuses dtype="bf16" (`_dense_entry`)

    def __init__(self, n_feat=240, patch_size=68, n_classes=3, TR_STEPS=1, loss_weights=None, seed=None,
                 nb_filters=32, kernel_size=3, nb_stacks=3, n_dilations=8, tcn_block="2.3"):
        """tcn_block: residual block of the third-party `tcn.TCN` the model was built with -- "2.3" (keras-tcn 2.3.x, what the
        reference's call binds under; default) or "2.8" (the two-convolution block of later releases; inference only)."""
        if str(tcn_block) not in ("2.3", "2.8"):
            raise ValueError("tcn_block must be '2.3' or '2.8', got %r" % (tcn_block,))
        self.tcn_block = str(tcn_block)
        self.block_variant = 0 if self.tcn_block == "2.3" else 1
        self.lib = _lib.require_gpu()
        self.n_feat, self.patch_size, self.n_classes = int(n_feat), int(patch_size), int(n_classes)
        self.nb_filters, self.kernel_size, self.nb_stacks, self.n_dilations = nb_filters, kernel_size, nb_stacks, n_dilations
        self.TR_STEPS, self.loss_weights = TR_STEPS, loss_weights
        # proposed_architectures.py:136 draws the (training-only) spatial dropout rate at build time
        self.dropout_rate, self.weights = initial_weights(self.n_feat, self.patch_size, self.n_classes, seed, nb_filters,
                                                          kernel_size, nb_stacks, n_dilations, self.block_variant, self.HEADS)
        self.initial_learning_rate = 0.002
        cfg = _lib.ModelCfg(self.n_feat, self.patch_size, self.n_classes, nb_filters, kernel_size, nb_stacks, n_dilations,
                            self.block_variant)
        h = C.c_void_p()
        if self.HEADS == HEADS_MTL:
            _lib.check(self.lib.smh_model_create(C.byref(cfg), C.byref(h)), "smh_model_create")
        else:
            _lib.check(self.lib.smh_model_create_heads(C.byref(cfg), self.HEADS, C.byref(h)), "smh_model_create_heads")
        self._h = h
        self.out_dim = self.lib.smh_model_out_dim(self._h)
        self._spec = weight_spec(self.n_feat, self.patch_size, self.n_classes, nb_filters, kernel_size, nb_stacks, n_dilations,
                                 self.block_variant, self.HEADS)
        self._init_store()
        self._init_training_state()

    def to_json(self):
        return json.dumps({"class_name": self.CLASS_NAME, "config": {
            "n_feat": self.n_feat, "patch_size": self.patch_size, "n_classes": self.n_classes,
            "nb_filters": self.nb_filters, "kernel_size": self.kernel_size, "nb_stacks": self.nb_stacks,
            "n_dilations": self.n_dilations, "dropout_rate": self.dropout_rate, "outputs": self.output_names,
            "tcn_block": self.tcn_block}})

    def summary(self, print_fn=print):
        kind = {HEADS_CASCADED: "cascaded MTL", HEADS_FUSION: "intermediate-fusion MTL", HEADS_SINGLE: "no"}.get(self.HEADS, "MTL")
        inputs = "2 x " if self.HEADS == HEADS_FUSION else ""
        self._summary("Model: %s (Lemaire et al. TCN + %s heads), input %s(None, %d, %d)"
                      % (self.CLASS_NAME, kind, inputs, self.patch_size, self.n_feat), print_fn)

    # ---- inference -----------------------------------------------------------------------------
    def _check_patches(self, x, what="input"):
        if x.dim() != 3 or x.shape[1] != self.patch_size or x.shape[2] != self.n_feat:
            raise ValueError("expected %s (N, %d, %d), got %s" % (what, self.patch_size, self.n_feat, tuple(x.shape)))
        return x

    def _check_x0p(self, x0p):
        if x0p.dim() != 4 or tuple(x0p.shape[1:]) != (2, self.patch_size, 32):
            raise ValueError("expected (N, 2, %d, 32), got %s" % (self.patch_size, tuple(x0p.shape)))
        return x0p

    def _train_inputs(self, x):
        """A training step's input -> [x] as a contiguous float32 CUDA tensor (N, W, n_feat) (TcnTrainingMixin.train_on_batch)."""
        x = self._check_patches(to_f32_cuda(x))
        if self.block_variant != 0:
            raise NotImplementedError("training is built for the keras-tcn 2.3.x block (tcn_block='2.3'); the 2.8 block is inference only")
        return [x]

    def _forward(self, f32_entry, bf16_entry, x, out, trunk, dtype):
        """The f32 entry point (with the trunk tap) or its split-bf16 twin on x -> out (N, out_dim), allocated unless given and
        not validated (HotPath and bench.py pass preallocated buffers).  Once per step in their timed loops: `_out`, `ptr` and
        `_call` are written out here (measured: 1.2 us of 5.6 per call through them)."""
        self._sync_weights()
        N = x.shape[0]
        if out is None:
            out = torch.empty((N, self.out_dim), dtype=torch.float32, device=x.device)
        if dtype == "f32":
            _lib.check(getattr(self.lib, f32_entry)(self._h, C.c_void_p(x.data_ptr()), N, C.c_void_p(out.data_ptr()),
                                                    None if trunk is None else C.c_void_p(trunk.data_ptr()),
                                                    _lib.current_stream()), f32_entry)
        elif dtype == "bf16":
            # "bf16" = SPLIT bf16 operands: every f32 operand travels as hi + lo (two bf16 values) and every product is three
            # bf16 MFMA (hi*hi + hi*lo + lo*hi) accumulated in f32 -- f32-grade arithmetic on the bf16 matrix pipe (7e-5 from the
            # f32 kernel), not an 8-bit-mantissa network.  Operands rounded to ONE bf16 land 3.5-5e-2 from f32, outside SURVEY
            # 8(d')'s 2e-2, and are not offered here (C ABI: smh_model_forward_bf16_ex(split = 0), measurement only).
            if trunk is not None:
                raise ValueError("the trunk tap is only available on the f32 path")
            self._call(bf16_entry, self._h, ptr(x), N, ptr(out), 1)
        else:
            raise ValueError("dtype must be 'f32' or 'bf16' (split bf16 operands), got %r" % (dtype,))
        return out

    def forward_device(self, x, out=None, trunk=None, dtype="f32"):
        """x: float32 CUDA tensor (N, W, n_feat) -> (N, out_dim) tensor [S|M|(N)|R|3C] on the device.
        dtype="bf16" selects the mixed-precision kernel (bf16 matrix-core operands, f32 everything else): faster,
        not the parity path."""
        x = self._check_patches(f32_cuda(x, "forward_device"))
        return self._forward("smh_model_forward_f32", "smh_model_forward_bf16_ex", x, out, trunk, dtype)

    def forward_from_x0(self, x0p, out=None, trunk=None, dtype="f32"):
        """Forward that starts from the per-half layer-0 partials (N, 2, W, 32) written by `Frontend.features_l0`.
        dtype as for `forward_device`; with "bf16" layer 0 stays exact f32 (it was computed by the feature kernel)."""
        x0p = f32_cuda(x0p, "forward_from_x0")
        if self.block_variant != 0:
            raise ValueError("the layer-0 fusion exists for the keras-tcn 2.3.x block only")
        return self._forward("smh_model_forward_x0_f32", "smh_model_forward_x0_bf16", self._check_x0p(x0p), out, trunk, dtype)

    def _dense_rows(self):
        """(rows of forward_dense's featuregram, what they are called in its shape error)."""
        return self.n_feat, ""

    def _dense_workspace_args(self, Tc, shift):
        return (Tc,)

    def _dense_entry(self, dtype):
        """The C entry of forward_dense for `dtype`; the refusals that need no launch: an unknown dtype (`_forward`'s wording), and
        "bf16" on anything but a B3_MTL with the keras-tcn 2.3.x block."""
        if dtype == "f32":
            return self._DENSE_ENTRY
        if dtype != "bf16":
            raise ValueError("dtype must be 'f32' or 'bf16' (split bf16 operands), got %r" % (dtype,))
        if self.HEADS != HEADS_MTL or self.block_variant != 0:
            raise ValueError("dtype='bf16': B3_MTL with the keras-tcn 2.3.x block is the only model with a bf16 path; %s%s has the f32 "
                             "forward only" % (self.CLASS_NAME, "" if self.block_variant == 0 else " with the 2.8 block"))
        return self._DENSE_ENTRY_BF16

    def forward_dense(self, fv, shift=1, out=None, dtype="f32"):
        """Every hop-`shift` patch of a standardised featuregram batch fv (n_feat, Tc) through the network (dense file-level
        inference, DAFx12_Speech_Music_Detection_B3_MTL_v2.py:634-665) WITHOUT building the (nP, W, n_feat) patches: layer 0 once
        per frame, every patch a window of it (`smh_model_forward_dense_f32`).  Returns (nP, out_dim); nP = tools.extract_patches'
        count for Tc frames.  Needs Tc >= patch_size; shorter batches are tiled by get_feature_patches and go through forward_device.
        dtype="bf16" (B3_MTL only): the network on split bf16 operands as in `forward_device` (`smh_model_forward_dense_bf16`);
        layer 0 stays the exact-f32 per-frame pass."""
        entry = self._dense_entry(dtype)
        fv = f32_cuda(fv, "forward_dense")
        rows, what = self._dense_rows()
        if fv.dim() != 2 or fv.shape[0] != rows:
            raise ValueError("expected %s(%d, Tc), got %s" % (what, rows, tuple(fv.shape)))
        if self.block_variant != 0:
            raise ValueError("the layer-0 fusion exists for the keras-tcn 2.3.x block only")
        Tc, shift = int(fv.shape[1]), int(shift)
        self._sync_weights()
        nP = self.lib.smh_num_patches(Tc, self.patch_size, shift) if Tc >= self.patch_size else -1
        if nP < 0:
            raise ValueError("forward_dense needs shift >= 1 and at least patch_size=%d frames, got Tc=%d shift=%d" % (self.patch_size, Tc, shift))
        out = self._out(out, nP, fv.device, validate=True)
        if nP == 0:
            return out
        nbytes = getattr(self.lib, self._DENSE_WORKSPACE)(self._h, *self._dense_workspace_args(Tc, shift))
        work = workspace(nbytes, fv.device)
        got = self._call(entry, self._h, ptr(fv), Tc, shift, ptr(work), nbytes, ptr(out))
        if got != nP:
            raise RuntimeError("%s produced %d patches, expected %d" % (entry, got, nP))
        return out

    def check_status(self):
        """Wait for the current stream and raise RuntimeError if a forward kernel recorded in the model's device error word
        that its outputs are not results (include/smh.h: smh_model_status).  `forward_device` / `forward_from_x0` only enqueue
        work; callers that keep results on the device call this before trusting them (`predict` and bench.py do)."""
        self._call("smh_model_status", self._h)


class CascadedMTL(B3MTL):
    """`model` object of get_Lemaire_Cascaded_MTL_model (lib/proposed_architectures.py:175-323): the B3_MTL trunk, '3C' and
    Dense(16) layers, with cascaded heads -- R = Dense(2)(Dropout(relu(BN(Dense16)))), S and M =
    sigmoid(Dense(1)(BN(concat[Dropout(relu(BN(Dense16))), R]))).  Outputs [S, M, R, 3C] like B3_MTL; n_classes widens '3C'
    only.  The same surface as B3MTL (predict / compile / fit / evaluate / persistence); the bf16 paths (forward dtype "bf16",
    train_dtype "bf16") and the single-head sub-model are B3_MTL only."""

    HEADS = HEADS_CASCADED
    CLASS_NAME = "B3_MTL_Cascaded"


class FusionMTL(B3MTL):
    """`model` object of get_Lemaire_MTL_intermediate_fusion_model (lib/proposed_architectures.py:327-420): two inputs
    'harm_input' / 'perc_input', each (N, W, n_feat) time-major, two independent keras-tcn 2.3 trunks ('tcn_initial_conv_H' /
    '_P', one build-time spatial dropout rate, independent masks), x = BatchNormalization(concat[Flatten(trunk H), Flatten(trunk
    P)]), then B3_MTL's '3C' and heads on x.  Outputs [S, M, (N,) R, 3C] like B3_MTL.  `x` is [x_H, x_P] or {'harm_input': x_H,
    'perc_input': x_P}.  The same surface as B3MTL.  Inference without materialised halves: `forward_from_x0_halves` on the per-half
    layer-0 partials of `Frontend.features_l0(..., model=self)` (what `pipeline.HotPath` runs), and `forward_dense` on a whole H||P
    featuregram (2 * n_feat, Tc) (what `inference.patch_probabilities` runs).  `forward_from_x0` (which adds the two partials up),
    the bf16 paths, the trunk tap, the keras-tcn 2.8 block and the single-head sub-model are B3_MTL only."""

    HEADS = HEADS_FUSION
    CLASS_NAME = "B3_MTL_Intermediate_Fusion"
    INPUT_NAMES = ("harm_input", "perc_input")
    _DENSE_ENTRY, _DENSE_WORKSPACE = "smh_fusion_forward_dense_f32", "smh_fusion_dense_workspace_bytes"

    def __init__(self, n_feat=120, patch_size=68, n_classes=3, TR_STEPS=1, loss_weights=None, seed=None, nb_filters=32,
                 kernel_size=3, nb_stacks=3, n_dilations=8, tcn_block="2.3"):
        if str(tcn_block) != "2.3":
            raise ValueError("the intermediate-fusion model is built for the keras-tcn 2.3.x block (tcn_block='2.3') only")
        super().__init__(n_feat=n_feat, patch_size=patch_size, n_classes=n_classes, TR_STEPS=TR_STEPS, loss_weights=loss_weights,
                         seed=seed, nb_filters=nb_filters, kernel_size=kernel_size, nb_stacks=nb_stacks, n_dilations=n_dilations,
                         tcn_block=tcn_block)

    # ---- the two inputs ----
    def _pair(self, x):
        """[x_H, x_P] or {'harm_input': x_H, 'perc_input': x_P} -> two float32 CUDA tensors (N, W, n_feat); anything else raises."""
        if isinstance(x, dict):
            if set(x) != set(self.INPUT_NAMES):
                raise ValueError("the intermediate-fusion model takes the inputs %s, got %s" % (list(self.INPUT_NAMES), sorted(x)))
            x = [x[k] for k in self.INPUT_NAMES]
        if not isinstance(x, (list, tuple)) or len(x) != 2:
            raise TypeError("the intermediate-fusion model takes two inputs: [x_H, x_P] or {'harm_input': x_H, 'perc_input': x_P}")
        for a in x:
            if not isinstance(a, (np.ndarray, torch.Tensor)):
                raise TypeError("inputs must be numpy arrays or torch tensors, got %s" % type(a).__name__)
        xh, xp = (self._check_patches(to_f32_cuda(a), "each input") for a in x)
        if xh.shape[0] != xp.shape[0]:
            raise ValueError("harm_input has %d patches, perc_input %d" % (xh.shape[0], xp.shape[0]))
        return [xh, xp]

    _device_input = _train_inputs = _pair

    def forward_device(self, x, out=None, trunk=None, dtype="f32"):
        """x: [x_H, x_P] (or the dict) -> (N, out_dim) tensor [S|M|(N)|R|3C] on the device (smh_fusion_forward_f32)."""
        if dtype != "f32":
            raise ValueError("the intermediate-fusion model has the f32 forward only, got dtype=%r" % (dtype,))
        if trunk is not None:
            raise ValueError("the intermediate-fusion model has no trunk tap")
        xh, xp = self._pair(x)
        self._sync_weights()
        N = xh.shape[0]
        out = self._out(out, N, xh.device)
        if N == 0:
            return out
        nbytes = self.lib.smh_fusion_workspace_bytes(self._h, N)
        work = workspace(nbytes, xh.device)
        self._call("smh_fusion_forward_f32", self._h, ptr(xh), ptr(xp), N, ptr(out), ptr(work), nbytes)
        return out

    def forward_from_x0(self, *args, **kwargs):
        raise ValueError("the intermediate-fusion model does not add the two layer-0 partials up (its trunks take one half each): "
                         "use forward_from_x0_halves, or forward_device on the two inputs")

    def w0_ptr(self):
        """Device address of the (2 * n_feat, 32) layer-0 kernels, trunk H's then trunk P's (smh_fusion_w0_ptr): the `w0` of
        Frontend.features_l0 for this model.  Follows the weights."""
        self._sync_weights()
        return self.lib.smh_fusion_w0_ptr(self._h)

    def forward_from_x0_halves(self, x0p, out=None):
        """x0p (N, 2, W, 32) as Frontend.features_l0(..., model=self) wrote it -- half 0 is trunk H's complete first layer, half 1
        trunk P's -- -> (N, out_dim) on the device (smh_fusion_forward_x0_f32).  The same logits as forward_device on the two halves
        of the patches within f32 tolerance."""
        x0p = self._check_x0p(f32_cuda(x0p, "forward_from_x0_halves"))
        self._sync_weights()
        N = x0p.shape[0]
        out = self._out(out, N, x0p.device, validate=True)
        if N == 0:
            return out
        nbytes = self.lib.smh_fusion_x0_workspace_bytes(self._h, N)
        work = workspace(nbytes, x0p.device)
        self._call("smh_fusion_forward_x0_f32", self._h, ptr(x0p), N, ptr(work), nbytes, ptr(out))
        return out

    def _dense_rows(self):
        return 2 * self.n_feat, "the H||P featuregram "

    def _dense_workspace_args(self, Tc, shift):
        return (Tc, shift)

    def forward_dense(self, fv, shift=1, out=None, dtype="f32"):
        """Every hop-`shift` patch of a standardised featuregram batch fv (2 * n_feat, Tc) -- the H||P featuregram exactly as
        B3MTL.forward_dense takes it: H rows, then P rows -- through the network without building the patches or their halves
        (smh_fusion_forward_dense_f32): layer 0 of both trunks once per frame, every patch a window of it.  Returns (nP, out_dim), nP
        = tools.extract_patches' count for Tc frames.  Needs Tc >= patch_size and n_feat % 4 == 0.  dtype: "f32" only (B3_MTL is the
        only model with a bf16 path)."""
        return super().forward_dense(fv, shift, out, dtype)

    def fit(self, x=None, y=None, batch_size=None, epochs=1, verbose=1, callbacks=None, validation_data=None,
            steps_per_epoch=None, validation_steps=None, initial_epoch=0, **kwargs):
        """fit(generator of ({'harm_input', 'perc_input'} | [x_H, x_P], y), steps_per_epoch=, ...) as for B3MTL, or arrays:
        x = [x_H, x_P] / the dict, y, batch_size (consecutive slices of the arrays, as B3MTL.fit takes them)."""
        if y is not None:
            if isinstance(x, dict):
                x = [x[k] for k in self.INPUT_NAMES]
            xh, xp = (np.asarray(a, np.float32) for a in x)
            yl = y if isinstance(y, (list, tuple)) else ([y] if isinstance(y, np.ndarray) else [y[k] for k in self.output_names])
            bs = batch_size or 32
            steps_per_epoch = steps_per_epoch or int(np.ceil(len(xh) / bs))

            def batches():
                s = 0
                while True:
                    a = (s * bs) % len(xh)
                    yield [xh[a:a + bs], xp[a:a + bs]], [np.asarray(t)[a:a + bs] for t in yl]
                    s += 1
            x, y = batches(), None
        return super().fit(x, y, batch_size=batch_size, epochs=epochs, verbose=verbose, callbacks=callbacks,
                           validation_data=validation_data, steps_per_epoch=steps_per_epoch, validation_steps=validation_steps,
                           initial_epoch=initial_epoch, **kwargs)


class SingleTaskTCN(SingleOutputMixin, B3MTL):
    """`model` object of get_Lemaire_model (lib/baseline_architectures.py:196-300; 5-class twin: 5_class_classification.py:54-145),
    baseline 3 of Baseline_Results.py: B3_MTL's trunk, then Flatten -> Dense(n_classes) -> softmax -- no Dense(16), no BatchNorm, no
    head dropout, no l2 term.  One input (N, W, n_feat) time-major (the reference feeds LogMelSpec patches), ONE output 'dense':
    `predict` returns one (N, n_classes) array, `y` is one one-hot (N, n_classes) array.  n_classes == 2 is compiled with
    binary_crossentropy on the two softmax outputs (so Keras' 'accuracy' is BINARY accuracy over the N x 2 outputs), 3 / 5 with
    categorical_crossentropy and categorical accuracy; metrics_names = ['loss', 'accuracy'].  f32 and the keras-tcn 2.3.x block only:
    the bf16 paths, `forward_from_x0` (the plain front end writes no layer-0 partials) and the single-head sub-model are B3_MTL's."""

    HEADS = HEADS_SINGLE
    CLASS_NAME = "B3_SingleTask"

    def __init__(self, n_feat=80, patch_size=68, n_classes=2, TR_STEPS=1, loss_weights=None, seed=None, nb_filters=32,
                 kernel_size=3, nb_stacks=3, n_dilations=8, tcn_block="2.3"):
        if str(tcn_block) != "2.3":
            raise ValueError("the single-task model is built for the keras-tcn 2.3.x block (tcn_block='2.3') only")
        if n_classes not in (2, 3, 5):
            raise ValueError("n_classes must be 2, 3 or 5, got %r" % (n_classes,))
        super().__init__(n_feat=n_feat, patch_size=patch_size, n_classes=n_classes, TR_STEPS=TR_STEPS, loss_weights=loss_weights,
                         seed=seed, nb_filters=nb_filters, kernel_size=kernel_size, nb_stacks=nb_stacks, n_dilations=n_dilations,
                         tcn_block=tcn_block)

    def forward_device(self, x, out=None, trunk=None, dtype="f32"):
        """x: float32 CUDA tensor (N, W, n_feat) -> (N, n_classes) softmax on the device."""
        if dtype != "f32":
            raise ValueError("the single-task model has the f32 forward only, got dtype=%r" % (dtype,))
        return super().forward_device(x, out, trunk, dtype)

    def forward_from_x0(self, *args, **kwargs):
        raise ValueError("the single-task model reads one plain featuregram: there are no per-half layer-0 partials to start from; "
                         "use forward_device or forward_dense")

    # ---- training surface ----
    def train_on_batch(self, x, y, drop_tcn="auto", drop_heads=None, apply=True, sync=True, _only=None, _mask=TRAIN_ALL):
        """One optimiser step -> [loss, accuracy].  There is no head dropout: drop_heads is accepted for the shared signature only."""
        if _only is not None:
            raise ValueError("single-output sub-models are built for the B3_MTL heads only")
        return super().train_on_batch(x, y, drop_tcn=drop_tcn, drop_heads=None, apply=apply, sync=sync, _mask=_mask)

    def _l2_penalty(self):
        return 0.0

    def _device_evaluate_ok(self):
        return True  # smh_model_eval_losses_f32 holds the two-output bce and the binary accuracy; there is no host restatement

    def _evaluate_device(self, x, y, steps, weight):
        tot, cnt = super()._evaluate_device(x, y, steps, weight)  # [total | loss | accuracy]
        return tot[[0, 2]], cnt
