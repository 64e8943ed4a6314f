"""float64 CPU reference of the intermediate-fusion MTL model (get_Lemaire_MTL_intermediate_fusion_model,
lib/proposed_architectures.py:327-420) -- test infrastructure, like tests/cascaded_ref.py, built from oracle.b3_mtl primitives.

  x = BN(concat[Flatten(trunk_H(x_H)), Flatten(trunk_P(x_P))]),   '3C' = softmax(Dense(x)),   heads = MTL_modifications(x)

`forward`: inference (moving statistics), numpy on top of oracle.b3_mtl's trunk and heads.
`torch_forward_backward`: one training step (batch statistics, Dropout masks as inputs, Keras losses, l2(0.01) on the Dense(16)
kernels) as a float64 torch autograd graph.  fuse=False drops trunk P and the fused BatchNorm: the graph is then B3_MTL on x_H,
which tests/test_fusion_ref.py pins against oracle.b3_mtl_train.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle import b3_mtl

BN_EPS, NORM_EPS, KERAS_EPS, L2 = b3_mtl.BN_EPS, b3_mtl.NORM_EPS, 1e-7, 0.01


def init_weights(seed=0, n_feat=120, patch_size=68, n_classes=3, randomize_bn=True, nb_stacks=3, n_dil=8):
    """Canonical-order weights (sm_hpss_mtl_amd.model.weight_spec(heads=HEADS_FUSION)): trunks H and P drawn like
    oracle.b3_mtl.init_weights (different seeds), the fused BatchNorm (randomised statistics and affine by default), '3C' and heads
    on D = 2 * patch_size * 32 inputs."""
    rng = np.random.default_rng(seed + 2000)
    D = 2 * patch_size * 32
    w = OrderedDict()
    for t, sd in (("tcn_H", seed), ("tcn_P", seed + 7)):
        base = b3_mtl.init_weights(seed=sd, n_feat=n_feat, patch_size=patch_size, n_classes=3, nb_stacks=nb_stacks, n_dil=n_dil,
                                   randomize_bn=randomize_bn)
        for k, v in base.items():
            if k.startswith("tcn/"):
                w[t + k[3:]] = v
    if randomize_bn:
        w["fusion_bn/gamma"] = rng.uniform(0.5, 1.5, D).astype(np.float32)
        w["fusion_bn/beta"] = rng.normal(0, 0.1, D).astype(np.float32)
        w["fusion_bn/moving_mean"] = rng.uniform(0.0, 0.5, D).astype(np.float32)
        w["fusion_bn/moving_variance"] = rng.uniform(0.2, 1.5, D).astype(np.float32)
    else:
        w["fusion_bn/gamma"], w["fusion_bn/beta"] = np.ones(D, np.float32), np.zeros(D, np.float32)
        w["fusion_bn/moving_mean"], w["fusion_bn/moving_variance"] = np.zeros(D, np.float32), np.ones(D, np.float32)
    heads = OrderedDict()
    b3_mtl.init_head_weights(heads, rng, D, n_classes)
    if randomize_bn:
        for k in list(heads):
            if k.endswith("/bias"):
                heads[k] = rng.normal(0, 0.1, heads[k].shape).astype(np.float32)
            elif k.endswith("bn/gamma") or k.endswith("bn/moving_variance"):
                heads[k] = rng.uniform(0.5, 1.5, heads[k].shape).astype(np.float32)
            elif k.endswith("bn/beta") or k.endswith("bn/moving_mean"):
                heads[k] = rng.normal(0, 0.2, heads[k].shape).astype(np.float32)
    w.update(heads)
    return w


def trunk_weights(w, t):
    """The weights of trunk t ('tcn_H' / 'tcn_P') under oracle.b3_mtl's names ('tcn/...')."""
    return {"tcn" + k[len(t):]: v for k, v in w.items() if k.startswith(t + "/")}


def forward(xH, xP, w, n_classes=3, nb_stacks=3, n_dil=8):
    """Inference forward -> [S, M, (N,) R, 3C] (float64 arithmetic behind the trunks)."""
    th = b3_mtl.tcn_forward(np.asarray(xH, np.float32), trunk_weights(w, "tcn_H"), nb_stacks, n_dil)
    tp = b3_mtl.tcn_forward(np.asarray(xP, np.float32), trunk_weights(w, "tcn_P"), nb_stacks, n_dil)
    f = np.concatenate([th.reshape(len(th), -1), tp.reshape(len(tp), -1)], axis=1).astype(np.float64)
    g = {k: np.asarray(v, np.float64) for k, v in w.items()}
    f = (f - g["fusion_bn/moving_mean"]) / np.sqrt(g["fusion_bn/moving_variance"] + BN_EPS) * g["fusion_bn/gamma"] + g["fusion_bn/beta"]
    outs = []
    for name, _, act in b3_mtl.head_spec(n_classes):
        h = f @ g[name + "/dense/kernel"] + g[name + "/dense/bias"]
        h = (h - g[name + "/bn/moving_mean"]) / np.sqrt(g[name + "/bn/moving_variance"] + BN_EPS)
        h = np.maximum(h * g[name + "/bn/gamma"] + g[name + "/bn/beta"], 0.0)
        o = h @ g[name + "/out/kernel"] + g[name + "/out/bias"]
        outs.append(1.0 / (1.0 + np.exp(-o)) if act == "sigmoid" else o)
    logits = f @ g["3C/kernel"] + g["3C/bias"]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    outs.append(e / e.sum(axis=1, keepdims=True))
    return outs


def torch_forward_backward(xH, xP, y, w, n_classes=3, drop_tcn=None, drop_heads=None, loss_weights=None, fuse=True, nb_stacks=3,
                           n_dil=8, dtype=np.float64):
    """One training step in float64 torch autograd.  drop_tcn: (2, N, n_blocks, 32) masks of trunks H and P, or None; drop_heads:
    dict head -> (N, 16).  Returns dict(loss (with the l2 term), losses{name}, acc, grads{name} (incl. the l2 term), bn_batch{'<head>'
    | 'fusion_bn': (mean, population var)}, outputs{name}).  dtype: the precision of the whole graph (np.float32: the same graph at
    the kernels' precision, for a measured rounding floor)."""
    import torch
    import torch.nn.functional as F
    T = {k: torch.tensor(np.asarray(v, dtype), requires_grad=True) for k, v in w.items()}
    spec = b3_mtl.head_spec(n_classes)
    lw = {n: 1.0 for n, _, _ in spec}
    lw["3C"] = 1.0
    lw.update(loss_weights or {})

    def conv(h, k, b, d):
        taps = k.shape[0]
        return F.conv1d(h.transpose(1, 2), k.permute(2, 1, 0), b, padding=(taps // 2) * d, dilation=d).transpose(1, 2)

    def trunk(x, t, drop):
        h = conv(torch.tensor(np.asarray(x, dtype)), T[t + "/initial_conv/kernel"], T[t + "/initial_conv/bias"], 1)
        bi = 0
        for s in range(nb_stacks):
            for i in range(n_dil):
                d, p = 2 ** i, "%s/s%d_d%d" % (t, s, 2 ** i)
                r = torch.relu(conv(h, T[p + "/conv/kernel"], T[p + "/conv/bias"], d))
                yn = r / (torch.amax(r, dim=2, keepdim=True) + NORM_EPS)
                if drop is not None:
                    yn = yn * torch.tensor(np.asarray(drop, dtype)[:, bi][:, None, :])
                h = h + conv(yn, T[p + "/conv1x1/kernel"], T[p + "/conv1x1/bias"], 1)
                bi += 1
        return torch.relu(h).reshape(h.shape[0], -1)

    N = len(xH)
    bn_batch = {}

    def bn_train(v, key, gamma, beta):
        mean, var = v.mean(0), v.var(0, unbiased=False)
        bn_batch[key] = (mean.detach().numpy(), var.detach().numpy())
        return (v - mean) / torch.sqrt(var + BN_EPS) * gamma + beta

    flat = trunk(xH, "tcn_H", None if drop_tcn is None else drop_tcn[0])
    if fuse:
        flat = torch.cat([flat, trunk(xP, "tcn_P", None if drop_tcn is None else drop_tcn[1])], dim=1)
        flat = bn_train(flat, "fusion_bn", T["fusion_bn/gamma"], T["fusion_bn/beta"])
    out = {}
    for name, _, act in spec:
        v = flat @ T[name + "/dense/kernel"] + T[name + "/dense/bias"]
        a = torch.relu(bn_train(v, name, T[name + "/bn/gamma"], T[name + "/bn/beta"]))
        if drop_heads is not None and name in drop_heads:
            a = a * torch.tensor(np.asarray(drop_heads[name], dtype))
        zo = a @ T[name + "/out/kernel"] + T[name + "/out/bias"]
        out[name] = torch.sigmoid(zo) if act == "sigmoid" else zo
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
    return dict(loss=float(total.detach()), losses={k: float(v.detach()) for k, v in losses.items()}, acc=acc, grads=grads,
                bn_batch=bn_batch, outputs={k: v.detach().numpy() for k, v in out.items()})
