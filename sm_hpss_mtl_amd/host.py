"""Host side shared by every model object (model.B3MTL / CascadedMTL / FusionMTL over `smh_model_*`, cnn_models.CnnMTL over
`smh_cnn_*`): the weight store, the Keras weight and output surface, and the few helpers every call into libsmh goes through.

Weight store.  `self.weights` holds float32 numpy arrays in the canonical order of `self._spec`; libsmh holds the device master
(re-packed into MFMA operand order).  Two flags say which of the two is newer:
  _dirty         the host copy changed (construction, set_weights): `_sync_weights` uploads it before the next launch;
  _device_newer  an optimiser step changed the device master (TrainingMixin.apply_gradients): `_pull_weights` downloads it before
                 the host copy is read.  set_weights on top of that drops the device copy: the host is the master again.
A class names its C family with `_C_PREFIX` (<prefix>_get_weights / _set_weights / _destroy) and `_TRAINER_PREFIX`."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .persistence import ModelSurfaceMixin, load_weights_file, save_weights_file

HEADS_MTL, HEADS_CASCADED, HEADS_FUSION = 0, 1, 2  # include/smh.h: SMH_HEADS_MTL / SMH_HEADS_CASCADED / SMH_HEADS_FUSION
HEADS_SINGLE = 3  # SMH_HEADS_SINGLE: the single-task baseline, Flatten -> Dense(n_classes) -> softmax, no auxiliary heads


def head_spec(n_classes: int, heads: int = HEADS_MTL):
    """(name, out_dim, activation) of the auxiliary heads in Keras output order
    (proposed_architectures.py:25-80,154; 5_class_classification.py:150-215,286).  The cascaded model
    (cascade_MTL_modifications, :175-234) has S, M, R[2] whatever n_classes is."""
    if heads == HEADS_SINGLE:
        return []
    if n_classes == 5 and heads != HEADS_CASCADED:  # (the intermediate-fusion model has MTL_modifications' heads)
        return [("S", 1, "sigmoid"), ("M", 1, "sigmoid"), ("N", 1, "sigmoid"), ("R", 3, "linear")]
    return [("S", 1, "sigmoid"), ("M", 1, "sigmoid"), ("R", 2, "linear")]


def f32_cuda(x, what):
    """x as a contiguous tensor; anything but a float32 CUDA tensor is a TypeError naming the entry point `what`."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError("%s expects a float32 CUDA tensor" % what)
    return x.contiguous()


def to_f32_cuda(x):
    """numpy array or tensor (any device, any dtype) -> contiguous float32 CUDA tensor."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(device="cuda", dtype=torch.float32).contiguous()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def workspace(nbytes, device):
    return torch.empty((nbytes // 4,), dtype=torch.float32, device=device)


class HostModel(ModelSurfaceMixin):
    _C_PREFIX = "smh_model"
    _TRAINER_PREFIX = "smh_trainer"
    HEADS = HEADS_MTL

    def __del__(self):
        for attr, prefix in (("_trainer", self._TRAINER_PREFIX), ("_h", self._C_PREFIX)):
            h = getattr(self, attr, None)
            if h:
                getattr(self.lib, prefix + "_destroy")(h)
                setattr(self, attr, None)

    def _call(self, entry, *args):
        """libsmh's `entry`(*args, current stream); a negative status raises under the entry's own name."""
        return _lib.check(getattr(self.lib, entry)(*args, _lib.current_stream()), entry)

    def _out(self, out, n, device, validate=False):
        if out is None:
            return torch.empty((n, self.out_dim), dtype=torch.float32, device=device)
        if validate and tuple(out.shape) != (n, self.out_dim):
            raise ValueError("out must be (%d, %d)" % (n, self.out_dim))
        return out

    # ---- weight store ----------------------------------------------------------------------------
    def _tensors(self):
        """[(name, shape)] in canonical order; `_spec` itself carries a third and fourth column per family."""
        return [(t[0], tuple(t[1])) for t in self._spec]

    def _init_store(self):
        n_host, n_lib = self.count_params(), getattr(self.lib, self._C_PREFIX + "_num_params")(self._h)
        if n_host != n_lib:
            raise RuntimeError("%s: the host weight spec has %d parameters, libsmh's %s object has %d -- the two canonical layouts "
                               "disagree" % (type(self).__name__, n_host, self._C_PREFIX, n_lib))
        self._dirty = True          # host copy newer than the device master
        self._device_newer = False  # device master newer than the host copy (after optimiser steps)

    def count_params(self):
        return int(sum(int(np.prod(s)) for _, s in self._tensors()))

    def weight_names(self):
        return [n for n, _ in self._tensors()]

    def _flat_to_dict(self, flat):
        """Flat vector in canonical order (weights, or a gradient) -> {name: array of the tensor's shape}."""
        res, o = {}, 0
        for name, shape in self._tensors():
            n = int(np.prod(shape))
            res[name] = flat[o:o + n].reshape(shape).copy()
            o += n
        return res

    def _pull_weights(self):
        if self._device_newer:
            flat = np.empty(self.count_params(), np.float32)
            self._call(self._C_PREFIX + "_get_weights", self._h, flat.ctypes.data_as(C.c_void_p), flat.size)
            self.weights.update(self._flat_to_dict(flat))
            self._device_newer = False

    def _sync_weights(self):
        if self._dirty:
            flat = np.concatenate([self.weights[n].ravel() for n in self.weight_names()]).astype(np.float32)
            self._call(self._C_PREFIX + "_set_weights", self._h, flat.ctypes.data_as(C.c_void_p), flat.size)
            self._dirty = False

    def get_weights(self):
        self._pull_weights()
        return [self.weights[n].copy() for n in self.weight_names()]

    def get_weights_dict(self):
        self._pull_weights()
        return self.weights

    def set_weights(self, arrays):
        arrays, spec = list(arrays), self._tensors()
        if len(arrays) != len(spec):
            raise ValueError("set_weights: expected %d arrays, got %d" % (len(spec), len(arrays)))
        new = {}
        for (name, shape), a in zip(spec, arrays):
            a = np.asarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError("set_weights: %s expects shape %s, got %s" % (name, shape, a.shape))
            new[name] = a.copy()
        self.weights.update(new)
        self._dirty = True
        self._device_newer = False

    def set_weights_dict(self, d):
        self.set_weights([d[n] for n in self.weight_names()])

    def save_weights(self, path):
        """`.h5` / `.hdf5`: HDF5 in Keras' weight-file layout (persistence.py); otherwise `<path>.npz`."""
        return save_weights_file(path, self.get_weights_dict())

    def load_weights(self, path, arch_json=None):
        """Weights written by `save_weights` (.h5 / .npz), or an .h5 file written by Keras itself for this architecture:
        its auto-generated layer names are mapped through the architecture JSON (`arch_json`: path or text; default
        `<path without .h5>.json`, the file the reference writes next to the weights)."""
        self.set_weights_dict(load_weights_file(path, arch_json=arch_json))

    def _summary(self, header, print_fn, width=18):
        print_fn(header)
        for name, shape in self._tensors():
            print_fn("  %-40s %-*s %d" % (name, width, str(shape), int(np.prod(shape))))
        print_fn("Total params: %d" % self.count_params())

    # ---- outputs -----------------------------------------------------------------------------------
    def _head_spec(self):
        return head_spec(self.n_classes, self.HEADS)

    @property
    def output_names(self):
        return [n for n, _, _ in self._head_spec()] + ["3C"]

    @property
    def metrics_names(self):
        """Proposed_Work_Results.py:887 expects ['loss','S_loss','M_loss','R_loss','3C_loss','3C_accuracy']."""
        return ["loss"] + [n + "_loss" for n in self.output_names] + ["3C_accuracy"]

    def split_outputs(self, out):
        """(N, out_dim) -> list in Keras output order [S, M, (N,) R, 3C]."""
        res, col = [], 0
        for _, odim, _ in self._head_spec() + [("3C", self.n_classes, None)]:
            res.append(out[:, col:col + odim])
            col += odim
        return res

    def _device_input(self, x):
        """A batch's input as forward_device takes it (the fusion model: two inputs)."""
        return to_f32_cuda(x)

    def predict(self, x, batch_size=None, verbose=0, dtype="f32"):
        """model.predict(x=batchData) -> [S, M, (N,) R, 3C] numpy arrays (Proposed_Work_Results.py:520,586)."""
        out = self.forward_device(self._device_input(x), dtype=dtype)
        self._check_device_status()  # (TrainingMixin) the forward is stream-ordered: a device-side give-up must become an exception, not a result
        host = out.cpu().numpy()  # ONE copy for all outputs (a copy per output is a host synchronisation per output)
        return [np.ascontiguousarray(o) for o in self.split_outputs(host)]


class SingleOutputMixin:
    """The Keras surface of a single-task model in front of its MTL class (model.SingleTaskTCN, cnn_models.CnnSingleTask): ONE
    output 'dense' -- `predict` returns one (N, n_classes) array, `y` is one one-hot (N, n_classes) array -- compiled with
    binary_crossentropy on the two softmax outputs for n_classes == 2 (Keras' 'accuracy' is then BINARY accuracy over the N x 2
    outputs), else categorical_crossentropy and categorical accuracy; metrics_names = ['loss', 'accuracy']."""

    @property
    def loss_name(self):
        return "binary_crossentropy" if self.n_classes == 2 else "categorical_crossentropy"

    @property
    def output_names(self):
        return ["dense"]

    @property
    def metrics_names(self):
        return ["loss", "accuracy"]

    def split_outputs(self, out):
        return [out]

    def predict(self, x, batch_size=None, verbose=0, dtype="f32"):
        """model.predict(x=batchData) -> ONE (N, n_classes) array, as a single-output Keras model returns it."""
        return super().predict(x, batch_size, verbose, dtype)[0]

    def compile(self, loss=None, optimizer=None, metrics=None, loss_weights=None, **kwargs):
        """`model.compile(loss=..., metrics='accuracy', optimizer=...)` (baseline_architectures.py:114-117, :292-295).  The loss is
        fixed by n_classes (`loss_name`): anything else is an error, not a silent change."""
        if isinstance(loss, dict):
            loss = loss.get("dense") if set(loss) == {"dense"} else loss
        if loss is not None and loss != self.loss_name:
            raise ValueError("compile: the %d-class single-task model is built with %s, not %r" % (self.n_classes, self.loss_name, loss))
        if metrics is not None:
            mm = [metrics] if isinstance(metrics, str) else list(metrics.values() if isinstance(metrics, dict) else metrics)
            if any(v not in ("accuracy", "acc") for v in mm):
                raise ValueError("compile: the only metric of the single-task model is 'accuracy', got %r" % (metrics,))
        super().compile(optimizer=optimizer, loss_weights=loss_weights, **kwargs)

    def pack_targets(self, y):
        """One one-hot (N, n_classes) array (or [array] / {'dense': array}) -> float32 CUDA tensor."""
        if isinstance(y, dict):
            y = y["dense"]
        if isinstance(y, (list, tuple)) and len(y) == 1:
            y = y[0]
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        t = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32))
        if t.dim() != 2 or t.shape[1] != self.out_dim:
            raise ValueError("targets must be one-hot (N, %d), got %s" % (self.out_dim, tuple(t.shape)))
        return t.cuda().contiguous()

    def losses_to_list(self, raw):
        """Raw device losses [loss, weighted loss, accuracy, penalty] of one step (or their mean over steps) -> [loss, accuracy]."""
        lv = raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
        return [float(lv[1] + lv[3]), float(lv[2])]

    def _losses_inference(self, x, y):
        """[loss + penalty, accuracy] of one batch in inference mode (the host route of `evaluate`), by the rule of `loss_name`, in
        float64 from the device's softmax: two classes -- Keras binary_crossentropy on both outputs (clip to [1e-7, 1 - 1e-7],
        + 1e-7 inside the logs) and binary accuracy over the N x 2 outputs; else categorical cross-entropy (the probabilities
        renormalised, then clipped, as Keras does) and categorical accuracy."""
        p = self.predict(x).astype(np.float64)
        if isinstance(y, dict):
            y = y["dense"]
        if isinstance(y, (list, tuple)):
            y = y[0]
        t = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y, np.float64).reshape(p.shape)
        eps = 1e-7
        if self.n_classes == 2:
            pc = np.clip(p, eps, 1 - eps)
            loss = float(np.mean(-(t * np.log(pc + eps) + (1 - t) * np.log(1 - pc + eps))))
            acc = float(np.mean((p > 0.5) == (t > 0.5)))
        else:
            pc = np.clip(p / p.sum(1, keepdims=True), eps, 1 - eps)
            loss = float(np.mean(-np.sum(t * np.log(pc), axis=1)))
            acc = float(np.mean(p.argmax(1) == t.argmax(1)))
        return [loss + self._eval_penalty(), acc]
