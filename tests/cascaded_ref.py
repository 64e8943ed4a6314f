"""float64 CPU reference of the cascaded-MTL model (get_Lemaire_Cascaded_MTL_model, lib/proposed_architectures.py:175-323) --
test infrastructure, like oracle/, but kept here because the pinned oracle has no cascaded heads.

  R:  r = Dense(2)(Dropout(relu(BN16(Dense16(x)))))
  S:  s = sigmoid(Dense(1)(BN18(concat[Dropout(relu(BN16(Dense16(x)))), r])))      (M likewise, own weights)
  3C: softmax(Dense(n_classes)(x))                                                    x = the flattened TCN trunk

`forward`: inference (moving statistics), numpy on top of oracle.b3_mtl's trunk.
`torch_forward_backward`: one training step (batch statistics, Dropout masks as inputs, Keras losses, l2(0.01) on the Dense(16)
kernels) as a float64 torch autograd graph.  With heads="mtl" it builds the B3_MTL heads instead, so that
tests/test_cascaded_ref.py can pin the trunk and the loss conventions of this build against oracle.b3_mtl_train.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle import b3_mtl

BN_EPS, NORM_EPS, KERAS_EPS, L2 = b3_mtl.BN_EPS, b3_mtl.NORM_EPS, 1e-7, 0.01
CAT = 18
HEADS = [("S", 1, "sigmoid"), ("M", 1, "sigmoid"), ("R", 2, "linear")]


def init_weights(seed=0, n_feat=240, patch_size=68, n_classes=3, randomize_bn=True):
    """Canonical-order weights of the cascaded model (the order of sm_hpss_mtl_amd.model.weight_spec(heads=1)): the trunk and
    Dense(16) layers drawn like oracle.b3_mtl.init_weights, a '3C' of n_classes outputs, S / M with 'cat_bn' and an (18, 1)
    out kernel."""
    rng = np.random.default_rng(seed + 1000)
    base = b3_mtl.init_weights(seed=seed, n_feat=n_feat, patch_size=patch_size, n_classes=3, randomize_bn=randomize_bn)
    D = patch_size * 32
    w = OrderedDict((k, v) for k, v in base.items() if k.startswith("tcn/"))
    lim = np.sqrt(6.0 / (D + n_classes))
    w["3C/kernel"] = base["3C/kernel"] if n_classes == 3 else rng.uniform(-lim, lim, (D, n_classes)).astype(np.float32)
    w["3C/bias"] = base["3C/bias"] if n_classes == 3 else rng.normal(0, 0.1, n_classes).astype(np.float32)
    for name, odim, _ in HEADS:
        for t in ("dense/kernel", "dense/bias", "bn/gamma", "bn/beta", "bn/moving_mean", "bn/moving_variance"):
            w[name + "/" + t] = base[name + "/" + t]
        if name == "R":
            w["R/out/kernel"], w["R/out/bias"] = base["R/out/kernel"], base["R/out/bias"]
            continue
        if randomize_bn:
            w[name + "/cat_bn/gamma"] = rng.uniform(0.5, 1.5, CAT).astype(np.float32)
            w[name + "/cat_bn/beta"] = rng.normal(0, 0.1, CAT).astype(np.float32)
            w[name + "/cat_bn/moving_mean"] = rng.normal(0, 0.1, CAT).astype(np.float32)
            w[name + "/cat_bn/moving_variance"] = rng.uniform(0.5, 1.5, CAT).astype(np.float32)
        else:
            w[name + "/cat_bn/gamma"], w[name + "/cat_bn/beta"] = np.ones(CAT, np.float32), np.zeros(CAT, np.float32)
            w[name + "/cat_bn/moving_mean"], w[name + "/cat_bn/moving_variance"] = np.zeros(CAT, np.float32), np.ones(CAT, np.float32)
        lim = np.sqrt(6.0 / (CAT + 1))
        w[name + "/out/kernel"] = rng.uniform(-lim, lim, (CAT, 1)).astype(np.float32)
        w[name + "/out/bias"] = base[name + "/out/bias"]
    return w


def heads_forward(flat, w, n_classes=3):
    """Inference heads on the flattened trunk (float64): [S, M, R, 3C]."""
    f = np.asarray(flat, np.float64)
    g = {k: np.asarray(v, np.float64) for k, v in w.items()}

    def hidden(name):
        h = f @ g[name + "/dense/kernel"] + g[name + "/dense/bias"]
        h = (h - g[name + "/bn/moving_mean"]) / np.sqrt(g[name + "/bn/moving_variance"] + BN_EPS)
        return np.maximum(h * g[name + "/bn/gamma"] + g[name + "/bn/beta"], 0.0)

    r = hidden("R") @ g["R/out/kernel"] + g["R/out/bias"]
    outs = []
    for name in ("S", "M"):
        z = np.concatenate([hidden(name), r], axis=1)
        z = (z - g[name + "/cat_bn/moving_mean"]) / np.sqrt(g[name + "/cat_bn/moving_variance"] + BN_EPS)
        z = z * g[name + "/cat_bn/gamma"] + g[name + "/cat_bn/beta"]
        with np.errstate(over="ignore"):  # saturated logits (the 2.8 block's unnormalised trunk): exp -> inf, sigmoid -> 0
            outs.append(1.0 / (1.0 + np.exp(-(z @ g[name + "/out/kernel"] + g[name + "/out/bias"]))))
    outs.append(r)
    logits = f @ g["3C/kernel"] + g["3C/bias"]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    outs.append(e / e.sum(axis=1, keepdims=True))
    return outs


def forward(x, w, n_classes=3):
    """Inference forward: x (N, W, n_feat) -> [S, M, R, 3C] (float64).  Trunk: oracle.b3_mtl (either residual block)."""
    x = np.asarray(x, np.float32)
    trunk = b3_mtl.tcn_forward_v2(x, w) if "tcn/s0_d1/conv0/kernel" in w else b3_mtl.tcn_forward(x, w)
    return heads_forward(trunk.reshape(trunk.shape[0], -1), w, n_classes)


def torch_forward_backward(x, y, w, n_classes=3, drop_tcn=None, drop_heads=None, loss_weights=None, heads="cascaded",
                           nb_stacks=3, n_dil=8, dtype=np.float64):
    """One training step in float64 torch autograd.  y: dict output -> targets; drop_tcn (N, n_blocks, 32); drop_heads: dict
    head -> (N, 16).  Returns dict(loss (with the l2 term), losses{name}, acc, grads{name} (incl. the l2 term, like the oracle),
    bn_batch{'<head>/bn' | '<head>/cat_bn': (mean, population var)}, outputs{name}).  dtype: the precision of the whole graph
    (np.float32: the same graph at the kernels' precision, for a measured rounding floor)."""
    import torch
    import torch.nn.functional as F
    T = {k: torch.tensor(np.asarray(v, dtype), requires_grad=True) for k, v in w.items()}
    xt = torch.tensor(np.asarray(x, dtype))
    N = xt.shape[0]
    spec = b3_mtl.head_spec(n_classes) if heads == "mtl" else HEADS
    lw = {n: 1.0 for n, _, _ in spec}
    lw["3C"] = 1.0
    lw.update(loss_weights or {})

    def conv(h, k, b, d):  # h (N, T, Cin), k (taps, Cin, Cout): y[t] = sum_j h[t + (j - taps // 2) d] k[j] + b
        taps = k.shape[0]
        out = F.conv1d(h.transpose(1, 2), k.permute(2, 1, 0), b, padding=(taps // 2) * d, dilation=d)
        return out.transpose(1, 2)

    h = conv(xt, T["tcn/initial_conv/kernel"], T["tcn/initial_conv/bias"], 1)
    bi = 0
    for s in range(nb_stacks):
        for i in range(n_dil):
            d, p = 2 ** i, "tcn/s%d_d%d" % (s, 2 ** i)
            r = torch.relu(conv(h, T[p + "/conv/kernel"], T[p + "/conv/bias"], d))
            yn = r / (torch.amax(r, dim=2, keepdim=True) + NORM_EPS)  # amax shares the gradient among tied maxima
            if drop_tcn is not None:
                yn = yn * torch.tensor(np.asarray(drop_tcn, dtype)[:, bi][:, None, :])
            h = h + conv(yn, T[p + "/conv1x1/kernel"], T[p + "/conv1x1/bias"], 1)
            bi += 1
    flat = torch.relu(h).reshape(N, -1)
    bn_batch = {}

    def bn_train(v, key, gamma, beta):
        mean, var = v.mean(0), v.var(0, unbiased=False)
        bn_batch[key] = (mean.detach().numpy(), var.detach().numpy())
        return (v - mean) / torch.sqrt(var + BN_EPS) * gamma + beta

    def hidden(name):
        v = flat @ T[name + "/dense/kernel"] + T[name + "/dense/bias"]
        a = torch.relu(bn_train(v, name + "/bn", T[name + "/bn/gamma"], T[name + "/bn/beta"]))
        if drop_heads is not None and name in drop_heads:
            a = a * torch.tensor(np.asarray(drop_heads[name], dtype))
        return a

    out = {}
    if heads == "mtl":
        for name, _, act in spec:
            zo = hidden(name) @ T[name + "/out/kernel"] + T[name + "/out/bias"]
            out[name] = torch.sigmoid(zo) if act == "sigmoid" else zo
    else:
        out["R"] = hidden("R") @ T["R/out/kernel"] + T["R/out/bias"]
        for name in ("S", "M"):
            z = torch.cat([hidden(name), out["R"]], dim=1)
            z = bn_train(z, name + "/cat_bn", T[name + "/cat_bn/gamma"], T[name + "/cat_bn/beta"])
            out[name] = torch.sigmoid(z @ T[name + "/out/kernel"] + T[name + "/out/bias"])
    losses = {}
    for name, odim, act in spec:
        t = torch.tensor(np.asarray(y[name], dtype).reshape(N, odim))
        o = out[name]
        if act == "sigmoid":
            oc = torch.clamp(o, KERAS_EPS, 1 - KERAS_EPS)
            losses[name] = torch.mean(-(t * torch.log(oc + KERAS_EPS) + (1 - t) * torch.log(1 - oc + KERAS_EPS)))
        else:
            losses[name] = torch.mean((o - t) ** 2)
    logits = flat @ T["3C/kernel"] + T["3C/bias"]
    p = torch.softmax(logits, dim=1)
    t3 = torch.tensor(np.asarray(y["3C"], dtype).reshape(N, n_classes))
    losses["3C"] = torch.mean(-torch.sum(t3 * torch.log(torch.clamp(p, KERAS_EPS, 1 - KERAS_EPS)), dim=1))
    out["3C"] = p
    reg = sum(L2 * torch.sum(T[n + "/dense/kernel"] ** 2) for n, _, _ in spec)
    total = sum(lw[k] * v for k, v in losses.items()) + reg
    total.backward()
    grads = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(v.shape)) for k, v in T.items()}
    acc = float(np.mean(p.detach().numpy().argmax(1) == t3.numpy().argmax(1)))
    return dict(loss=float(total.detach()), losses={k: float(v.detach()) for k, v in losses.items()}, acc=acc, grads=grads, bn_batch=bn_batch,
                outputs={k: v.detach().numpy() for k, v in out.items()})
