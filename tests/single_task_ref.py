"""float64 CPU reference of the single-task Lemaire TCN baseline (get_Lemaire_model, lib/baseline_architectures.py:196-300) -- test
infrastructure, like oracle/, kept here because the pinned oracle has no single-task model.

  trunk: oracle.b3_mtl's restatement of the keras-tcn 2.3 block (the same trunk as B3_MTL)
  tail:  softmax(Dense(n_classes)(Flatten(trunk)))

`forward`: inference, numpy.  `torch_forward_backward`: one training step as a float64 torch autograd graph whose loss is the Keras
expression written out -- n_classes == 2: binary_crossentropy on both softmax outputs (clip to [1e-7, 1 - 1e-7], + 1e-7 inside the
logs, mean over the two outputs, then the batch) with binary accuracy; else categorical_crossentropy with categorical accuracy.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle import b3_mtl

NORM_EPS, KERAS_EPS = b3_mtl.NORM_EPS, 1e-7


def init_weights(seed=0, n_feat=80, patch_size=68, n_classes=2, nb_stacks=3, n_dil=8):
    """Canonical-order weights (sm_hpss_mtl_amd.model.weight_spec(heads=3)): oracle.b3_mtl's trunk draw, then 'dense'."""
    base = b3_mtl.init_weights(seed=seed, n_feat=n_feat, patch_size=patch_size, n_classes=3, nb_stacks=nb_stacks, n_dil=n_dil,
                               randomize_bn=True)
    rng = np.random.default_rng(seed + 2000)
    D = patch_size * 32
    w = OrderedDict((k, v) for k, v in base.items() if k.startswith("tcn/"))
    # a tenth of the Glorot range: the trunk's outputs are O(1) over D = 2176 .. 7968 inputs, and the tests want logits of O(1) --
    # probabilities away from the 1e-7 clip and from a tie -- not saturated ones
    lim = 0.1 * np.sqrt(6.0 / (D + n_classes))
    w["dense/kernel"] = rng.uniform(-lim, lim, (D, n_classes)).astype(np.float32)
    w["dense/bias"] = rng.normal(0, 0.1, n_classes).astype(np.float32)
    return w


def forward(x, w, n_classes, nb_stacks=3, n_dil=8):
    """Inference forward: x (N, W, n_feat) -> (N, n_classes) softmax, float64."""
    trunk = b3_mtl.tcn_forward(np.asarray(x, np.float32), w, nb_stacks, n_dil)
    flat = np.asarray(trunk, np.float64).reshape(trunk.shape[0], -1)
    logits = flat @ np.asarray(w["dense/kernel"], np.float64) + np.asarray(w["dense/bias"], np.float64)
    assert logits.shape[1] == n_classes
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def keras_loss_and_accuracy(p, t, n_classes):
    """(loss, accuracy) of probabilities p against one-hot t, torch tensors, as Keras computes them for this model's compile."""
    import torch
    pc = torch.clamp(p, KERAS_EPS, 1 - KERAS_EPS)
    if n_classes == 2:
        loss = torch.mean(torch.mean(-(t * torch.log(pc + KERAS_EPS) + (1 - t) * torch.log(1 - pc + KERAS_EPS)), dim=1))
        acc = float(torch.mean(((p > 0.5) == (t > 0.5)).double()))
    else:
        loss = torch.mean(-torch.sum(t * torch.log(pc), dim=1))
        acc = float(torch.mean((p.argmax(1) == t.argmax(1)).double()))
    return loss, acc


def torch_forward_backward(x, y, w, n_classes, drop_tcn=None, nb_stacks=3, n_dil=8, dtype=np.float64):
    """One training step in float64 torch autograd.  y: one-hot (N, n_classes); drop_tcn (N, n_blocks, 32) or None.
    Returns dict(loss, acc, grads{name}, probs).  dtype: the precision of the whole graph (np.float32: the same graph at the
    kernels' precision, which says how well conditioned a case is)."""
    import torch
    import torch.nn.functional as F
    T = {k: torch.tensor(np.asarray(v, dtype), requires_grad=True) for k, v in w.items()}
    xt = torch.tensor(np.asarray(x, dtype))
    N = xt.shape[0]

    def conv(h, k, b, d):  # h (N, T, Cin), k (taps, Cin, Cout): y[t] = sum_j h[t + (j - taps // 2) d] k[j] + b
        taps = k.shape[0]
        return F.conv1d(h.transpose(1, 2), k.permute(2, 1, 0), b, padding=(taps // 2) * d, dilation=d).transpose(1, 2)

    h = conv(xt, T["tcn/initial_conv/kernel"], T["tcn/initial_conv/bias"], 1)
    bi = 0
    for s in range(nb_stacks):
        for i in range(n_dil):
            d, p = 2 ** i, "tcn/s%d_d%d" % (s, 2 ** i)
            r = torch.relu(conv(h, T[p + "/conv/kernel"], T[p + "/conv/bias"], d))
            yn = r / (torch.amax(r, dim=2, keepdim=True) + NORM_EPS)
            if drop_tcn is not None:
                yn = yn * torch.tensor(np.asarray(drop_tcn, dtype)[:, bi][:, None, :])
            h = h + conv(yn, T[p + "/conv1x1/kernel"], T[p + "/conv1x1/bias"], 1)
            bi += 1
    flat = torch.relu(h).reshape(N, -1)
    p = torch.softmax(flat @ T["dense/kernel"] + T["dense/bias"], dim=1)
    t = torch.tensor(np.asarray(y, dtype).reshape(N, n_classes))
    loss, acc = keras_loss_and_accuracy(p, t, n_classes)
    loss.backward()
    grads = {k: (v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(v.shape)) for k, v in T.items()}
    return dict(loss=float(loss.detach()), acc=acc, grads=grads, probs=p.detach().numpy().astype(np.float64))
