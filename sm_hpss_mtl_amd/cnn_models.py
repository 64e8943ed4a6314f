"""Conv2D MTL baselines: host wrapper over `smh_cnn_*` (include/smh.h).

  get_Doukhan_MTL_model      lib/proposed_architectures.py:425-511
  get_Papakostas_MTL_model   lib/proposed_architectures.py:516-588
  get_Jang_MTL_model         lib/proposed_architectures.py:650-764

The layer graph, the parameter table (names, Keras shapes, order) and all arithmetic live in libsmh.so
(csrc/smh_cnn.hip); this class initialises the weights the way the reference's initialisers do and moves tensors; the
weight store, the Keras weight surface and `predict` are host.HostModel's, shared with model.B3MTL.  Training (`fit` / `train_on_batch` / `evaluate`, cnn_training.py over
`smh_cnn_train_step_f32`) is built for all three.  `CnnSingleTask` is the single-task twin of each (lib/baseline_architectures.py).
"""
from __future__ import annotations

import ctypes as C
import json
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .cnn_training import CnnTrainingMixin
from .host import HostModel, SingleOutputMixin, f32_cuda, ptr

KINDS = {"Doukhan": 0, "Papakostas": 1, "Jang": 2}
SINGLE_KIND_OFFSET = 3  # include/smh.h: SMH_CNN_DOUKHAN_SINGLE / _PAPAKOSTAS_SINGLE / _JANG_SINGLE follow the MTL kinds
# initial learning rates returned next to the model (proposed_architectures.py:499, 574, 751)
LEARNING_RATE = {"Doukhan": 0.0001, "Papakostas": 0.001, "Jang": 0.001}


class CnnMTL(CnnTrainingMixin, HostModel):
    """`model` object of get_{Doukhan,Papakostas,Jang}_MTL_model."""

    _C_PREFIX = "smh_cnn"
    _TRAINER_PREFIX = "smh_cnn_trainer"
    _KIND_OFFSET = 0
    CLASS_SUFFIX = "_MTL"

    def __init__(self, kind, input_shape, n_classes=3, seed=None, n_mels=120, n_fft=512, fs=16000, fc_width=0,
                 loss_weights=None):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s" % sorted(KINDS))
        self.lib = _lib.require_gpu()
        self.kind, self.n_classes = kind, int(n_classes)
        self.in_h, self.in_w = int(input_shape[0]), int(input_shape[1])
        if len(input_shape) > 2 and int(input_shape[2]) != 1:
            raise ValueError("input_shape must be (H, W, 1), got %s" % (tuple(input_shape),))
        self.n_mels, self.n_fft, self.fs, self.fc_width = int(n_mels), int(n_fft), float(fs), int(fc_width)
        cfg = _lib.CnnCfg(KINDS[kind] + self._KIND_OFFSET, self.in_h, self.in_w, self.n_classes, self.n_mels, self.n_fft, int(fc_width),
                          self.fs)
        h = C.c_void_p()
        _lib.check(self.lib.smh_cnn_create(C.byref(cfg), C.byref(h)), "smh_cnn_create")
        self._h = h
        self.out_dim = self.lib.smh_cnn_out_dim(self._h)
        self.feat_dim = self.lib.smh_cnn_feat_dim(self._h)
        self.initial_learning_rate = LEARNING_RATE[kind]
        self._spec = []  # (name, shape, offset)
        name = C.create_string_buffer(96)
        shape, nd, off = (C.c_int * 4)(), C.c_int(), C.c_size_t()
        for i in range(self.lib.smh_cnn_num_tensors(self._h)):
            _lib.check(self.lib.smh_cnn_tensor_info(self._h, i, name, 96, shape, C.byref(nd), C.byref(off)),
                       "smh_cnn_tensor_info")
            assert int(off.value) == self.count_params()  # offsets are the running sum of the sizes: the store slices by it
            self._spec.append((name.value.decode(), tuple(shape[:nd.value]), int(off.value)))
        self.weights = OrderedDict()
        self._init_weights(np.random.default_rng(seed))
        self._init_store()
        self.loss_weights = loss_weights
        self._init_training_state()

    # ---- initialisers of the reference ---------------------------------------------------------------------------
    def _init_weights(self, rng):
        mel = None
        for name, shape, _ in self._spec:
            leaf = name.rsplit("/", 1)[1]
            if leaf == "kernel":
                if "melCl" in name:  # Constant(get_kernel_initializer(...)): mel weights over time and 3 channels
                    if mel is None:
                        mel = self._mel_basis()
                    i = int(name.split("melCl")[1].split("/")[0])
                    nz = np.where(mel[i] > 0)[0]
                    k = np.repeat(mel[i, nz[0]:nz[-1] + 1][:, None], shape[1], axis=1)[:, :, None, None]
                    w = np.repeat(k, shape[3], axis=3).astype(np.float32)
                    assert w.shape == shape, (name, w.shape, shape)
                elif self.kind == "Papakostas" and not self._is_head(name):  # RandomNormal(stddev=0.01)
                    w = rng.normal(0.0, 0.01, size=shape).astype(np.float32)
                else:  # glorot_uniform == VarianceScaling(1, 'fan_avg', 'uniform')
                    rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
                    fan_in, fan_out = rf * shape[-2], rf * shape[-1]
                    lim = np.sqrt(6.0 / (fan_in + fan_out))
                    w = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            elif leaf == "bias":
                fill = 0.1 if (self.kind == "Papakostas" and not self._is_head(name)) else 0.0  # Constant(0.1)
                w = np.full(shape, fill, np.float32)
            elif leaf in ("gamma", "moving_variance"):
                w = np.ones(shape, np.float32)
            else:  # beta, moving_mean
                w = np.zeros(shape, np.float32)
            self.weights[name] = w

    @staticmethod
    def _is_head(name):
        return name.split("/")[0] in ("S", "M", "N", "R")

    def _mel_basis(self):
        from .frontend import Frontend, FrontendConfig
        fe = Frontend(FrontendConfig(n_fft=self.n_fft, win_length=min(400, self.n_fft), n_mels=self.n_mels,
                                     mel_sr=self.fs))
        return fe.mel_basis()

    # ---- Keras-style surface -------------------------------------------------------------------------------------
    @property
    def input_shape(self):
        return (None, self.in_h, self.in_w, 1)

    def to_json(self):
        return json.dumps({"class_name": self.kind + self.CLASS_SUFFIX, "config": {
            "input_shape": [self.in_h, self.in_w, 1], "n_classes": self.n_classes, "n_mels": self.n_mels,
            "n_fft": self.n_fft, "fs": self.fs, "fc_width": self.fc_width, "outputs": self.output_names}})

    def summary(self, print_fn=print):
        self._summary("Model: %s%s, input (None, %d, %d, 1)" % (self.kind, self.CLASS_SUFFIX, self.in_h, self.in_w), print_fn, width=22)

    # ---- inference -----------------------------------------------------------------------------------------------
    def _check_images(self, x):
        """(N, H, W) or (N, H, W, 1) -> contiguous (N, H, W)."""
        if x.dim() == 4 and x.shape[3] == 1:
            x = x[..., 0]
        if x.dim() != 3 or x.shape[1] != self.in_h or x.shape[2] != self.in_w:
            raise ValueError("expected input (N, %d, %d[, 1]), got %s" % (self.in_h, self.in_w, tuple(x.shape)))
        return x.contiguous()

    def forward_device(self, x, out=None, features=None, dtype="f32"):
        """x: float32 CUDA tensor (N, H, W) or (N, H, W, 1) -> (N, out_dim) [S|M|(N)|R|3C] on the device.
        dtype="bf16": bf16 GEMM operands with f32 accumulation (smh_cnn_forward_bf16) -- faster, not the parity path."""
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        x = self._check_images(f32_cuda(x, "forward_device"))
        self._sync_weights()
        N = x.shape[0]
        out = self._out(out, N, x.device)
        nbytes = self.lib.smh_cnn_workspace_bytes(self._h, N)
        work = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=x.device)
        self._call("smh_cnn_forward_" + dtype, self._h, ptr(x), N, ptr(out), ptr(features), ptr(work), work.numel())
        return out


class CnnSingleTask(SingleOutputMixin, CnnMTL):
    """`model` object of get_{Doukhan,Papakostas,Jang}_model (lib/baseline_architectures.py:62-108, :147-175, :358-442), baselines 1, 2
    and 4 of Baseline_Results.py: the Conv2D trunk, then Dense(n_classes) + softmax -- no S / M / R heads.  ONE output 'dense':
    `predict` returns one (N, n_classes) array, `y` is one one-hot (N, n_classes) array.  n_classes == 2 is compiled with
    binary_crossentropy on the two softmax outputs (Keras' 'accuracy' is then BINARY accuracy over the N x 2 outputs), 3 with
    categorical_crossentropy and categorical accuracy (:114-117); metrics_names = ['loss', 'accuracy'] (host.SingleOutputMixin).

    Doukhan and Papakostas are their MTL siblings' trunks; Jang is a graph of its own (ONE mel-scale layer over the whole
    (n_fft/2 + 1, W) image, 64 mel kernels by default, 'valid' pooling, no FC layers, l1_l2() on the mel kernels alone).
    Initialisers as the reference's: Doukhan VarianceScaling(1, fan_avg, uniform) and zeros, Papakostas RandomNormal(0.01) and
    Constant(0.1) on every layer -- the last Dense included (:175) --, Jang the mel Constant kernels and Keras' defaults elsewhere."""

    _KIND_OFFSET = SINGLE_KIND_OFFSET
    CLASS_SUFFIX = "_SingleTask"

    def __init__(self, kind, input_shape, n_classes=2, seed=None, n_mels=64, n_fft=512, fs=16000, fc_width=0):
        if n_classes not in (2, 3):
            raise ValueError("n_classes must be 2 or 3 (the two cases the reference compiles), got %r" % (n_classes,))
        super().__init__(kind, input_shape, n_classes=n_classes, seed=seed, n_mels=n_mels, n_fft=n_fft, fs=fs, fc_width=fc_width)

    # ---- training surface ----
    def train_on_batch(self, x, y, drop="auto", apply=True, sync=True):
        """One optimiser step -> [loss, accuracy].  drop as for CnnMTL.train_on_batch; there are no heads, so no head dropout."""
        return super().train_on_batch(x, y, drop=drop, drop_heads=None, apply=apply, sync=sync)

    def _l2_penalty(self):
        """The kernel-regulariser penalty: l1_l2() (Keras defaults l1 = l2 = 0.01) on Jang's mel kernels, nothing else anywhere."""
        if self.kind != "Jang":
            return 0.0
        w = self.get_weights_dict()
        return float(sum(0.01 * (np.sum(v.astype(np.float64) ** 2) + np.sum(np.abs(v.astype(np.float64))))
                         for k, v in w.items() if k.startswith("melCl")))
