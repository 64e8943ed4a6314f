"""float64 CPU reference of the late-fusion ensemble (Late_Fusion_Results.py:388-513) -- test infrastructure, like tests/fusion_ref.py:
two complete models (oracle.b3_mtl.forward, or tests.cascaded_ref.forward for the cascaded heads), model H on the harmonic input and
model P on the percussive one, and the numpy blend of their '3C' outputs,

    pred = np.add(alpha * pred_H, (1 - alpha) * pred_P),    pred_lab = np.argmax(pred, axis=1)            (:422-423)

PARITY_CASES are the cases the GPU parity test runs; tests/test_late_fusion_ref.py checks on the CPU that the reference alone leaves
at most 1 % of each case's patches inside the 2e-4 top-two margin that excludes a patch from the label comparison."""
from __future__ import annotations

import numpy as np

from oracle import b3_mtl
from tests import cascaded_ref

MARGIN = 2e-4      # labels are compared where the reference's top two blended probabilities differ by more than this
MAX_LEFT_OUT = 0.01  # share of a case's patches that may fall inside the margin

# (kind, W, n_classes, n_feat per model, N, alpha, seed)
PARITY_CASES = [
    ("mtl", 68, 3, 120, 48, 0.5, 1),
    ("mtl", 99, 5, 120, 17, 0.3, 2),
    ("mtl", 249, 3, 40, 5, 0.0, 3),
    ("cascaded", 68, 3, 120, 33, 0.5, 4),
    ("cascaded", 99, 3, 40, 16, 1.0, 5),
    ("cascaded", 249, 5, 120, 3, 0.3, 6),
    ("mtl", 68, 5, 120, 257, 0.3, 7),
    ("cascaded", 68, 3, 120, 1024, 0.5, 8),
]


def init_weights(kind, seed, n_feat, patch_size, n_classes):
    """(weights of model H, weights of model P): two independent draws of one architecture, canonical order."""
    fn = {"mtl": b3_mtl.init_weights, "cascaded": cascaded_ref.init_weights}[kind]
    return tuple(fn(seed=s, n_feat=n_feat, patch_size=patch_size, n_classes=n_classes, randomize_bn=True) for s in (seed, seed + 7))


def inputs(N, W, n_feat, seed):
    """(x_H, x_P): float32 (N, W, n_feat) each, standard normal like standardised patches."""
    rng = np.random.default_rng(1000 + seed)
    return tuple(rng.standard_normal((N, W, n_feat)).astype(np.float32) for _ in range(2))


def model_forward(kind, x, w, n_classes):
    """One model's own output list [S, M, (N,) R, 3C] in float64."""
    return (b3_mtl.forward if kind == "mtl" else cascaded_ref.forward)(x, w, n_classes)


def blend(pred_H, pred_P, alpha):
    """The driver's blend in the precision of its operands."""
    return np.add(alpha * pred_H, (1 - alpha) * pred_P)


def forward(kind, xH, xP, wH, wP, alpha, n_classes):
    """dict(heads_H, heads_P: each model's (N, out_dim) float64 [S|M|(N)|R|3C]; pred (N, n_classes); labels; margin: the top-two gap)."""
    hH = np.concatenate(model_forward(kind, xH, wH, n_classes), axis=1)
    hP = np.concatenate(model_forward(kind, xP, wP, n_classes), axis=1)
    pred = blend(hH[:, -n_classes:], hP[:, -n_classes:], alpha)
    top = np.sort(pred, axis=1)
    return dict(heads_H=hH, heads_P=hP, pred=pred, labels=np.argmax(pred, axis=1), margin=top[:, -1] - top[:, -2])


def case_reference(case):
    """(xH, xP, wH, wP, reference dict) of one PARITY_CASES entry."""
    kind, W, ncls, F, N, alpha, seed = case
    wH, wP = init_weights(kind, seed, F, W, ncls)
    xH, xP = inputs(N, W, F, seed)
    return xH, xP, wH, wP, forward(kind, xH, xP, wH, wP, alpha, ncls)
