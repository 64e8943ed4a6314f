"""The case table and the helpers of the heads-plan and optimiser GPU tests -- TEST INFRASTRUCTURE, a plain module like
tests/heads_plans.py: tests/test_heads_plans.py (no GPU), tests/test_heads_plans_gpu.py and tests/test_optimisers_gpu.py import
it, and none of them imports another test module.

It holds: the cases (named for the plan of tests/heads_plans.py they are there for), the problems (weights, inputs, targets,
dropout masks; host only), the float64 references and the same graphs in float32, the distances the tests hold, the measured
float32 floor of those distances, and the gate margins of a draw."""
from __future__ import annotations

import numpy as np

from oracle import b3_mtl, b3_mtl_train as tr
from tests import cascaded_ref as cref, fusion_ref as fref

SHALLOW = dict(F=20, nb=1, nd=2, W=20)   # two residual blocks, D = 640
FULL = dict(F=240, nb=3, nd=8, W=68)     # the reference's network, D = 2176


def case(kind, ncls, N, plan, seed, full=False, heads_global=False, drop_heads=True, lw=None):
    return dict(kind=kind, ncls=ncls, N=N, plan=plan, full=full, heads_global=heads_global, drop_heads=drop_heads, lw=lw, seed=seed)


# `seed`: the draw of inputs, targets and masks.  On the shallow trunk it is the first draw whose float64 trunk has no gate inside
# float32 rounding (`gate_margins` >= GAP_MIN / GATE_MIN / GATE_MIN; tests/test_heads_plans.py asserts it for every shallow case).
CASES = [
    # B3_MTL, 3 classes: staged up to N = 538, 1024 threads from N = 513
    case("B3_MTL", 3, 513, "staged1024", 0), case("B3_MTL", 3, 538, "staged1024", 4), case("B3_MTL", 3, 539, "global1024", 0),
    case("B3_MTL", 3, 1030, "global1024", 10), case("B3_MTL", 3, 512, "global512", 0, heads_global=True),
    case("B3_MTL", 3, 538, "staged1024", 0, full=True), case("B3_MTL", 3, 600, "global1024", 0, full=True),
    case("B3_MTL", 3, 539, "global1024", 0, drop_heads=False),
    # B3_MTL, 5 classes: staged up to N = 390
    case("B3_MTL", 5, 390, "staged512", 1), case("B3_MTL", 5, 391, "global512", 0), case("B3_MTL", 5, 513, "global1024", 3),
    # intermediate fusion: the same launch code behind the fused BatchNorm
    case("fusion", 3, 513, "staged1024", 1), case("fusion", 3, 538, "staged1024", 5), case("fusion", 3, 539, "global1024", 4),
    case("fusion", 5, 391, "global512", 1), case("fusion", 5, 513, "global1024", 3),
    case("fusion", 3, 539, "global1024", 4, drop_heads=False),
    # cascaded: the S / M / 3C kernel turns global at N = 904, the R kernel at N = 1617
    case("cascaded", 3, 903, "sm_staged+r_staged", 0), case("cascaded", 5, 904, "sm_global+r_staged", 0),
    case("cascaded", 3, 1616, "sm_global+r_staged", 4), case("cascaded", 3, 1617, "sm_global+r_global", 12),
    # the weighted total is assembled in the R kernel from losses the S / M / 3C launch left in memory
    case("cascaded", 3, 1617, "sm_global+r_global", 12, lw={"S": 0.7, "M": 1.5, "R": 1.3, "3C": 0.5}),
    case("cascaded", 3, 904, "sm_global+r_staged", 2, drop_heads=False),
]
# the cross-plan check toggles SMH_HEADS_GLOBAL at batches that are staged by default, one per thread count
CROSS_PLAN_N = [510, 530]
# bit-reproducibility cases added next to the existing ones: tests/test_training_gpu.py (B3_MTL) and tests/test_cascaded_gpu.py
DETERMINISM_CASES = [("B3_MTL", 3, 530, "staged1024"), ("cascaded", 3, 904, "sm_global+r_staged"),
                     ("cascaded", 3, 1617, "sm_global+r_global")]


def case_id(c):
    return "%s-%dc-N%d-%s%s%s%s%s" % (c["kind"], c["ncls"], c["N"], c["plan"], "-full" if c["full"] else "",
                                      "-forced" if c["heads_global"] else "", "" if c["drop_heads"] else "-nodrop",
                                      "-lw" if c["lw"] else "")


# ---- problems -----------------------------------------------------------------------------------------------------
def problem(kind, ncls, N, full=False, seed=0):
    """(weights in the model's canonical order, inputs, targets, drop_tcn, drop_heads, head names, trunk shape); host only."""
    s = FULL if full else SHALLOW
    F, nb, nd, W = s["F"], s["nb"], s["nd"], s["W"]
    rng = np.random.default_rng(1000 * seed + N)
    spec = b3_mtl.head_spec(ncls) if kind != "cascaded" else cref.HEADS
    heads = [n for n, _, _ in spec]
    y = {n: ((rng.random((N, od)) > 0.5).astype(np.float32) if act == "sigmoid" else rng.random((N, od)).astype(np.float32))
         for n, od, act in spec}
    y["3C"] = np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, N)]
    drop_heads = ((rng.random((N, len(heads), 16)) > 0.4) / 0.6).astype(np.float32)
    if kind == "fusion":
        w = fref.init_weights(seed=5, n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dil=nd)
        x = [rng.standard_normal((N, W, F)).astype(np.float32) for _ in range(2)]
        drop_tcn = ((rng.random((2, N, nb * nd, 32)) > 0.2) / 0.8).astype(np.float32)
    else:
        w = b3_mtl.init_weights(seed=3, n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dil=nd, randomize_bn=True)
        if kind == "cascaded":  # the cascaded heads on this trunk (tests/test_model_shapes_gpu.py)
            trunk = [(k, v) for k, v in w.items() if k.startswith("tcn/")]
            casc = cref.init_weights(seed=5, n_feat=F, patch_size=W, n_classes=ncls)
            w = dict(trunk + [(k, v) for k, v in casc.items() if not k.startswith("tcn/")])
        x = rng.standard_normal((N, W, F)).astype(np.float32)
        drop_tcn = ((rng.random((N, nb * nd, 32)) > 0.2) / 0.8).astype(np.float32)
    return w, x, y, drop_tcn, drop_heads, heads, s


def build(kind, ncls, N, full=False, lw=None, seed=0):
    """(model holding the problem's weights,) + problem(...).  Needs the GPU."""
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL, FusionMTL
    w, x, y, drop_tcn, drop_heads, heads, s = problem(kind, ncls, N, full, seed)
    cls = {"B3_MTL": B3MTL, "cascaded": CascadedMTL, "fusion": FusionMTL}[kind]
    m = cls(n_feat=s["F"], patch_size=s["W"], n_classes=ncls, nb_stacks=s["nb"], n_dilations=s["nd"], loss_weights=lw, TR_STEPS=10)
    assert [n for n, _, _, _ in m._spec] == list(w)
    m.set_weights_dict(w)
    return m, w, x, y, drop_tcn, drop_heads, heads, s


def flat_to_dict(m, flat):
    out, o = {}, 0
    for name, shape, _, _ in m._spec:
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    return out


def batch_statistics(kind, st, heads, D):
    """The statistics part of the bucket -> {key: (mean, var)} (smh_train.hip: bnstat; cascaded 'cat_bn' and the fused BatchNorm
    sit behind the 4 x 32 floats of the heads' BatchNorm(16)).  Keys: '<head>' (B3_MTL, fusion), '<head>/bn' and '<head>/cat_bn'
    (cascaded), 'fusion_bn' -- the keys of the references' `bn_batch`."""
    out = {}
    for h, name in enumerate(heads):
        out[name + "/bn" if kind == "cascaded" else name] = (st[h * 32:h * 32 + 16], st[h * 32 + 16:h * 32 + 32])
    if kind == "cascaded":
        for h, name in enumerate(("S", "M")):
            c = 128 + h * 36
            out[name + "/cat_bn"] = (st[c:c + 18], st[c + 18:c + 36])
    if kind == "fusion":
        out["fusion_bn"] = (st[128:128 + D], st[128 + D:128 + 2 * D])
    return out


def step(m, x, y, drop_tcn, drop_heads):
    """One training step without the update -> (losses, {name: gradient}, statistics part of the bucket).  Needs the GPU."""
    import torch
    dt = torch.from_numpy(drop_tcn).cuda()
    dh = None if drop_heads is None else torch.from_numpy(drop_heads).cuda()
    got = m.train_on_batch(x, y, drop_tcn=dt, drop_heads=dh, apply=False)
    torch.cuda.synchronize()
    bucket = m._bucket_tensor().cpu().numpy().copy()
    n = m.count_params()
    return got, flat_to_dict(m, bucket[:n]), bucket[n:]


# ---- references ---------------------------------------------------------------------------------------------------
def reference(kind, x, y, w, ncls, drop_tcn, drop_heads, heads, lw, s, dtype=np.float64, order=None):
    """The training step of the model kind as dict(loss, losses, acc, grads, bn_batch) with `bn_batch` under the keys of
    `batch_statistics`.  float64: oracle.b3_mtl_train.forward_backward (B3_MTL), tests/cascaded_ref.py, tests/fusion_ref.py.
    float32: the same graphs in torch at the kernels' precision (B3_MTL: the heads="mtl" build of tests/cascaded_ref.py, which
    tests/test_cascaded_ref.py pins against the oracle); `order` takes the batch in another order, i.e. other roundings of
    the same sums."""
    if order is not None:
        x = [a[order] for a in x] if kind == "fusion" else x[order]
        y = {k: v[order] for k, v in y.items()}
        drop_tcn = drop_tcn[:, order] if kind == "fusion" else drop_tcn[order]
        drop_heads = None if drop_heads is None else drop_heads[order]
    dh = None if drop_heads is None else {h: drop_heads[:, i] for i, h in enumerate(heads)}
    kw = dict(nb_stacks=s["nb"], n_dil=s["nd"])
    if kind == "fusion":
        return fref.torch_forward_backward(x[0], x[1], y, w, ncls, drop_tcn, dh, lw, dtype=dtype, **kw)
    if kind == "cascaded":
        return cref.torch_forward_backward(x, y, w, ncls, drop_tcn, dh, lw, dtype=dtype, **kw)
    if dtype == np.float64:
        return tr.forward_backward(x, y, w, ncls, drop_tcn, dh, lw, **kw)
    r = cref.torch_forward_backward(x, y, w, ncls, drop_tcn, dh, lw, heads="mtl", dtype=dtype, **kw)
    r["bn_batch"] = {k[:-3]: v for k, v in r["bn_batch"].items()}  # '<head>/bn' -> '<head>'
    return r


def distances(kind, losses, grads, stats, ref, names):
    """{quantity: distance of a candidate step from the float64 reference `ref`}, the quantities the tests bound:
      'loss'            worst of total and per-output losses, |a - b| / max(1, |b|)
      'accuracy'        |a - b|
      'l2 <tensor>'     relative L2 of a gradient tensor (not for the Dense(16) biases: analytically zero)
      'el <tensor>'     worst element, relative to max |ref| of the tensor; ABSOLUTE for the Dense(16) biases
      'trunk <prefix>'  relative L2 over a whole trunk of the fusion model
      'stats'           worst batch statistic, |a - b| / max(1, max |b|) per vector
    losses: [total, per-output in `names` order ..., accuracy]; grads: {name: array} INCLUDING the l2 term of the Dense(16)
    kernels; stats: {key of batch_statistics: (mean, var)}."""
    d = {"loss": max([abs(losses[0] - ref["loss"]) / max(1.0, abs(ref["loss"]))] +
                     [abs(losses[1 + i] - ref["losses"][n]) / max(1.0, abs(ref["losses"][n])) for i, n in enumerate(names)]),
         "accuracy": abs(losses[-1] - ref["acc"])}
    terr, tref = {}, {}
    for name, gref in ref["grads"].items():
        if name.endswith(tr.TRAINABLE_SKIP):
            continue
        gref = np.asarray(gref, np.float64)
        e = np.asarray(grads[name], np.float64) - gref
        if name.endswith("/dense/bias"):
            d["el " + name] = float(np.abs(e).max())
            continue
        d["l2 " + name] = float(np.linalg.norm(e) / max(np.linalg.norm(gref), 1e-12))
        d["el " + name] = float(np.abs(e).max() / max(np.abs(gref).max(), 1e-6))
        if kind == "fusion" and name.startswith("tcn_"):
            terr.setdefault(name[:5], []).append(e.ravel())
            tref.setdefault(name[:5], []).append(gref.ravel())
    for t in terr:
        d["trunk " + t] = float(np.linalg.norm(np.concatenate(terr[t])) / np.linalg.norm(np.concatenate(tref[t])))
    worst = 0.0
    for key, (rmean, rvar) in ref["bn_batch"].items():
        for a, b in zip(stats[key], (rmean, rvar)):
            worst = max(worst, float(np.abs(np.asarray(a, np.float64) - b).max() / max(1.0, np.abs(b).max())))
    d["stats"] = worst
    return d


def reference_distances(kind, cand, ref, names):
    """`distances` of a reference-shaped candidate (the float32 graph)."""
    losses = [cand["loss"]] + [cand["losses"][n] for n in names] + [cand["acc"]]
    return distances(kind, losses, cand["grads"], cand["bn_batch"], ref, names)


N_FLOOR_EVALS = 4
FLOAT32_ROUNDING = 2.0 ** -24


def float32_floor(kind, x, y, w, ncls, drop_tcn, drop_heads, heads, lw, s, ref, seed):
    """{quantity: the largest distance from the float64 reference `ref` that the SAME graph evaluated in float32 on the CPU shows},
    over N_FLOOR_EVALS evaluations: the batch as it stands and in N_FLOOR_EVALS - 1 permuted orders (other roundings of the same
    sums; one evaluation alone is one sample of a rounding error, and a bound of four times ONE sample of a scalar -- a loss, a
    two-element bias -- is exceeded by an equally good evaluation about one time in six).  A RELATIVE figure is never taken below
    one rounding of the format, FLOAT32_ROUNDING = 2^-24: a one-element tensor such as S/out/bias can land within a fraction of its
    last bit of the float64 value in four evaluations out of four (measured: 8e-9 .. 2e-8), which says nothing about how near
    another correct float32 evaluation must come -- a result stored in float32 is up to 2^-24 from the real number it rounds.  The
    Dense(16) biases, absolute figures of an analytically zero sum, keep their measured floor."""
    rng = np.random.default_rng(seed)
    N = len(y["3C"])
    names = heads + ["3C"]
    floor = {}
    for i in range(N_FLOOR_EVALS):
        order = None if i == 0 else rng.permutation(N)
        c32 = reference(kind, x, y, w, ncls, drop_tcn, drop_heads, heads, lw, s, dtype=np.float32, order=order)
        for q, v in reference_distances(kind, c32, ref, names).items():
            floor[q] = max(floor.get(q, 0.0), v)
    return {q: (v if q.endswith("/dense/bias") or q == "accuracy" else max(v, FLOAT32_ROUNDING)) for q, v in floor.items()}


# ---- gates of the trunk ------------------------------------------------------------------------------------------
GAP_MIN = 1e-6    # two largest channels of a row, relative to the larger: 16 float32 roundings
GATE_MIN = 1e-7   # a relu input (the blocks', the trunk output's, the heads' behind BatchNorm(16)), relative to the largest of its tensor


def gate_margins(kind, w, x, drop_tcn, s):
    """(gap, gate, head_gate) of a draw, from its float64 training forward: the smallest relative distance between the two largest
    channels of a row in any block (a tie of the channel maximum), the smallest |relu input| / max |relu input| over the blocks' relus
    and the trunk's output relu, and the same over the heads' relus behind BatchNorm(16) (batch statistics; the head dropout comes
    after the relu).  A draw whose margins are inside float32 rounding has a gradient that a float32
    forward is free to evaluate on the other branch: it cannot be held to a rounding-sized bound."""
    gap, gate, flats = np.inf, np.inf, []
    trunks = [("tcn_H", x[0], drop_tcn[0]), ("tcn_P", x[1], drop_tcn[1])] if kind == "fusion" else [("tcn", x, drop_tcn)]
    for prefix, xx, drop in trunks:
        g = {k: np.asarray(v, np.float64) for k, v in w.items() if k.startswith(prefix + "/")}
        h = tr._conv_same(np.asarray(xx, np.float64), g[prefix + "/initial_conv/kernel"], g[prefix + "/initial_conv/bias"], 1)
        for bi, (p, d) in enumerate(tr.block_names(s["nb"], s["nd"])):
            p = prefix + p[3:]
            u = tr._conv_same(h, g[p + "/conv/kernel"], g[p + "/conv/bias"], d)
            r = np.maximum(u, 0.0)
            top = np.sort(r, axis=2)[..., -2:]
            assert (top[..., 1] > 0).all()
            gap = min(gap, float(((top[..., 1] - top[..., 0]) / top[..., 1]).min()))
            gate = min(gate, float(np.abs(u).min() / np.abs(u).max()))
            yn = r / (top[..., 1:] + b3_mtl.NORM_EPS) * np.asarray(drop, np.float64)[:, bi][:, None, :]
            h = h + tr._conv_same(yn, g[p + "/conv1x1/kernel"], g[p + "/conv1x1/bias"], 1)
        gate = min(gate, float(np.abs(h).min() / np.abs(h).max()))
        flats.append(np.maximum(h, 0.0).reshape(len(h), -1))
    flat = np.concatenate(flats, axis=1)
    g = {k: np.asarray(v, np.float64) for k, v in w.items() if not k.startswith("tcn")}
    if kind == "fusion":
        flat = (flat - flat.mean(0)) / np.sqrt(flat.var(0) + b3_mtl.BN_EPS) * g["fusion_bn/gamma"] + g["fusion_bn/beta"]
    head_gate = np.inf
    for name in [k[:-len("/dense/kernel")] for k in g if k.endswith("/dense/kernel")]:
        hd = flat @ g[name + "/dense/kernel"] + g[name + "/dense/bias"]
        bn = (hd - hd.mean(0)) / np.sqrt(hd.var(0) + b3_mtl.BN_EPS) * g[name + "/bn/gamma"] + g[name + "/bn/beta"]
        head_gate = min(head_gate, float(np.abs(bn).min() / np.abs(bn).max()))
    return gap, gate, head_gate


# ---- the heads alone, in float32, in any batch order (the cross-plan check's measured bound) -------------------------------
def heads_f32(flat, y, w, ncls, drop_heads, order):
    """The heads of oracle.b3_mtl_train.forward_backward (forward, losses, backward to the flattened trunk) in FLOAT32 numpy, with
    the batch taken in `order`: the same function as the float64 reference, its sums in another order at the kernels' precision.
    Returns {quantity: array}: the head and '3C' gradients (the Dense(16) bias, analytically zero, among them), 'dflat' (d loss / d trunk output, back in the original order), the
    losses and the batch statistics."""
    f = np.float32
    fl = np.ascontiguousarray(flat[order], f)
    N = len(fl)
    eps, bn_eps = f(tr.KERAS_EPS), f(b3_mtl.BN_EPS)
    out, losses, stats = {}, [], []
    dflat = np.zeros_like(fl)
    for hi, (name, odim, act) in enumerate(b3_mtl.head_spec(ncls)):
        p = {k: np.asarray(w[name + "/" + k], f) for k in ("dense/kernel", "dense/bias", "bn/gamma", "bn/beta", "out/kernel", "out/bias")}
        hd = fl @ p["dense/kernel"] + p["dense/bias"]
        mean = hd.mean(axis=0, dtype=f)
        var = np.mean((hd - mean) ** 2, axis=0, dtype=f)
        inv = f(1.0) / np.sqrt(var + bn_eps)
        xhat = (hd - mean) * inv
        bn = xhat * p["bn/gamma"] + p["bn/beta"]
        dm = np.asarray(drop_heads[order][:, hi], f)
        ad = np.maximum(bn, f(0.0)) * dm
        zo = ad @ p["out/kernel"] + p["out/bias"]
        t = np.asarray(y[name], f).reshape(-1, odim)[order]
        if act == "sigmoid":
            o = f(1.0) / (f(1.0) + np.exp(-zo))
            oc = np.clip(o, eps, f(1.0) - eps)
            losses.append(np.mean(-(t * np.log(oc + eps) + (f(1.0) - t) * np.log(f(1.0) - oc + eps)), dtype=f))
            inside = (o > eps) & (o < f(1.0) - eps)
            dzo = -(t / (oc + eps) - (f(1.0) - t) / (f(1.0) - oc + eps)) / f(N * odim) * inside * o * (f(1.0) - o)
        else:
            losses.append(np.mean((zo - t) ** 2, dtype=f))
            dzo = f(2.0) * (zo - t) / f(N * odim)
        out[name + "/out/kernel"], out[name + "/out/bias"] = ad.T @ dzo, dzo.sum(axis=0, dtype=f)
        dbn = (dzo @ p["out/kernel"].T) * dm * (bn > 0)
        out[name + "/bn/gamma"], out[name + "/bn/beta"] = (dbn * xhat).sum(axis=0, dtype=f), dbn.sum(axis=0, dtype=f)
        dxhat = dbn * p["bn/gamma"]
        dhd = inv / f(N) * (f(N) * dxhat - dxhat.sum(axis=0, dtype=f) - xhat * (dxhat * xhat).sum(axis=0, dtype=f))
        out[name + "/dense/kernel"], out[name + "/dense/bias"] = fl.T @ dhd, dhd.sum(axis=0, dtype=f)
        dflat += dhd @ p["dense/kernel"].T
        stats += [mean, var]
    k3, b3 = np.asarray(w["3C/kernel"], f), np.asarray(w["3C/bias"], f)
    logits = fl @ k3 + b3
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True, dtype=f)
    t3 = np.asarray(y["3C"], f)[order]
    losses.append(np.mean(-np.sum(t3 * np.log(np.clip(p, eps, f(1.0) - eps)), axis=1, dtype=f), dtype=f))
    dlog = (p - t3) / f(N)
    out["3C/kernel"], out["3C/bias"] = fl.T @ dlog, dlog.sum(axis=0, dtype=f)
    dflat += dlog @ k3.T
    back = np.empty_like(dflat)
    back[order] = dflat
    out["dflat"] = back
    assert all(v.dtype == f for v in out.values())
    out["losses"], out["stats"] = np.array(losses, np.float64), np.concatenate(stats).astype(np.float64)
    return out


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def cpu_reorder_figures(N, w, x, y, drop_heads, ncls, s, n_perm=8):
    """{quantity: the worst distance of `heads_f32` on a permuted batch from `heads_f32` on the batch as it stands}, over n_perm
    permutations (relative L2 per tensor, ABSOLUTE for the analytically zero Dense(16) biases; losses relative to max(1, |loss|),
    statistics to max(1, max |statistic|)); the heads' input is the oracle's inference trunk output (any fixed trunk output serves: the trunk's own dropout
    does not enter a statement about the heads' summation order)."""
    flat = np.asarray(b3_mtl.tcn_forward(x, w, s["nb"], s["nd"]), np.float32).reshape(N, -1)
    base = heads_f32(flat, y, w, ncls, drop_heads, np.arange(N))
    rng = np.random.default_rng(N)
    cpu = {}
    for _ in range(n_perm):
        other = heads_f32(flat, y, w, ncls, drop_heads, rng.permutation(N))
        for k in base:
            if k == "losses":
                d = float(np.max(np.abs(other[k] - base[k]) / np.maximum(1.0, np.abs(base[k]))))
            elif k.endswith("/dense/bias"):  # analytically zero: an absolute figure
                d = float(np.abs(other[k] - base[k]).max())
            elif k == "stats":
                d = float(np.abs(other[k] - base[k]).max() / max(1.0, np.abs(base[k]).max()))
            else:
                d = float(rel_l2(other[k], base[k]))
            cpu[k] = max(cpu.get(k, 0.0), d)
    return cpu
