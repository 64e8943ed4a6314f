"""Counterpart of lib/baseline_architectures.py: `get_Lemaire_model`, baseline 3 of Baseline_Results.py -- the Lemaire et al. TCN
without the MTL heads, the network B3_MTL is compared against.  Same signature and return value as the reference (:196-300): a model
object with the Keras-style surface the drivers use (`sm_hpss_mtl_amd.model.SingleTaskTCN`) and the initial learning rate 0.002;
n_classes=5 selects the twin of 5_class_classification.py:54-145.

`get_Doukhan_model`, `get_Papakostas_model` and `get_Jang_model` (:62-108, :147-175, :358-442), baselines 1, 2 and 4, return a
`sm_hpss_mtl_amd.cnn_models.CnnSingleTask` and the initial learning rate, with the reference's signatures.  Each reads
PARAMS['input_shape'][PARAMS['Model']]; a PARAMS without those keys gives the builder nothing to build and is answered with
NotImplementedError (the wording an earlier test of this package pins).
"""
from __future__ import annotations

from ..cnn_models import CnnSingleTask
from ..model import SingleTaskTCN


def get_Lemaire_model(TR_STEPS, kernel_size=3, Nd=8, nb_stacks=3, n_layers=1, n_filters=32, use_skip_connections=False,
                      activation='norm_relu', bidirectional=True, N_MELS=80, n_classes=2, patch_size=68, seed=None):
    """baseline_architectures.py:196-300 -> (model, 0.002): keras-tcn 2.3 TCN(32 filters, kernel 3, nb_stacks stacks of dilations
    1 .. 2^(Nd-1), 'norm_relu', 'same' padding, no skip connections, one build-time spatial dropout rate), Flatten, Dense(n_classes),
    softmax; SGD(momentum 0.9, clipnorm 1) on ExponentialDecay(0.002, 3 * TR_STEPS, 0.1); binary_crossentropy for two classes,
    categorical_crossentropy for 3 (and 5), metrics 'accuracy'.  The reference overrides `bidirectional` with True ('same' padding),
    so its value changes nothing here either.  A value the kernels do not serve raises ValueError naming the argument."""
    if n_layers != 1:
        raise ValueError("n_layers=%r: the kernels serve one TCN layer (n_layers=1)" % (n_layers,))
    if n_filters != 32:
        raise ValueError("n_filters=%r: the kernels are tiled for n_filters=32" % (n_filters,))
    if kernel_size != 3:
        raise ValueError("kernel_size=%r: the kernels serve kernel_size=3" % (kernel_size,))
    if use_skip_connections:
        raise ValueError("use_skip_connections=%r: the kernels serve the TCN without skip connections" % (use_skip_connections,))
    if activation != 'norm_relu':
        raise ValueError("activation=%r: the kernels serve activation='norm_relu'" % (activation,))
    if n_classes not in (2, 3, 5):
        raise ValueError("n_classes=%r: the single-task model has 2, 3 or 5 classes" % (n_classes,))
    model = SingleTaskTCN(n_feat=N_MELS, patch_size=patch_size, n_classes=n_classes, TR_STEPS=TR_STEPS, seed=seed,
                          nb_filters=n_filters, kernel_size=kernel_size, nb_stacks=nb_stacks, n_dilations=Nd)
    model.compile(loss=model.loss_name, metrics='accuracy')
    return model, model.initial_learning_rate


def _input_shape(who, PARAMS):
    if not isinstance(PARAMS, dict) or "Model" not in PARAMS or "input_shape" not in PARAMS:
        raise NotImplementedError("%s: the single-task Conv2D baselines are not built from a PARAMS without 'Model' and 'input_shape'"
                                  % who)
    return PARAMS["input_shape"][PARAMS["Model"]]


def _compiled(model):
    model.compile(loss=model.loss_name, metrics=['accuracy'])
    return model, model.initial_learning_rate


def get_Doukhan_model(PARAMS, n_classes=2, seed=None):
    """baseline_architectures.py:62-108 -> (model, 0.0001): Doukhan's Conv2D trunk on PARAMS['input_shape'][Model] (the driver's
    (21, 68, 1) MelSpec patches), Dense(n_classes) softmax; Adam(1e-4)."""
    return _compiled(CnnSingleTask("Doukhan", _input_shape("get_Doukhan_model", PARAMS), n_classes=n_classes, seed=seed))


def get_Papakostas_model(PARAMS, n_classes=2, seed=None):
    """baseline_architectures.py:147-175 -> (model, 0.001): Papakostas' trunk on (201, 68, 1) Spec patches, Dense(n_classes) softmax;
    SGD on ExponentialDecay(1e-3, 700, 0.1)."""
    return _compiled(CnnSingleTask("Papakostas", _input_shape("get_Papakostas_model", PARAMS), n_classes=n_classes, seed=seed))


def get_Jang_model(PARAMS, fs=16000, Tw=25, n_mels=64, t_dim=5, n_classes=2, seed=None):
    """baseline_architectures.py:358-442 -> (model, 0.001): one mel-scale layer of n_mels kernels (started from the Slaney mel weights
    of librosa.filters.mel(fs, n_fft=PARAMS['n_fft'][Model], n_mels)) on (n_fft/2 + 1, W, 1) LogSpec patches, three Conv2D blocks,
    Dense(n_classes) softmax; Adam(1e-3).  Tw is the reference's unused argument."""
    shape = _input_shape("get_Jang_model", PARAMS)
    if t_dim != 5:
        raise ValueError("t_dim=%r: the mel-scale layer is built for t_dim=5 (the reference's only value)" % (t_dim,))
    return _compiled(CnnSingleTask("Jang", shape, n_classes=n_classes, seed=seed, n_mels=n_mels,
                                   n_fft=PARAMS["n_fft"][PARAMS["Model"]], fs=fs))
