"""GPU: the heads-training kernels of the three TCN models at EVERY launch plan, against the float64 references.

The training step picks its heads kernel from the batch size (tests/heads_plans.py restates the launch code):
  B3_MTL / fusion  heads_train_kernel<STAGED, THREADS>   staged 512 | global 512 | staged 1024 | global 1024
  cascaded         cascade_sm_kernel<STAGED>, cascade_r_kernel<STAGED>   each staged | global
Each case (tests/heads_cases.py) is named for the plan it is there for and sits next to a threshold; tests/test_heads_plans.py (no
GPU) proves that it lands there.  Per case: train_on_batch(apply=False) with fixed dropout masks, then losses, accuracy, every
gradient tensor and the BatchNorm batch statistics behind the gradient in the bucket, against oracle.b3_mtl_train.forward_backward
(B3_MTL), tests/cascaded_ref.py and tests/fusion_ref.py (float64 torch autograd).

Trunk.  The heads kernels see the trunk only as D = 32 W inputs, and a gradient's distance from a float64 reference is dominated
by relu / channel-maximum gates of the trunk that float32 rounding flips.  Most cases therefore run a shallow, narrow trunk
(n_feat 20, one stack of two dilations, W = 20), which keeps the float64 reference to a second at N = 1617; B3_MTL keeps one
full-size case (n_feat 240, 3 x 8 blocks, W = 68) for staged 1024 and for global 1024, because dwh_mfma_kernel and the trunk
backward read the `dpre` these plans write in their own layout.

Bounds.
* The two full-size cases: the project's (tests/test_training_gpu.py: test_gradients_and_losses_at_the_config4_batch): losses
  2e-4 max(1, |ref|), accuracy 1e-6, batch statistics 1e-4 max(1, max |ref|), gradients 2e-3 relative L2 per tensor and 1e-2
  max |ref| per element (a Dense(16) bias, analytically zero in front of its BatchNorm: 2e-5 absolute).
* The shallow cases: those bounds are three orders of magnitude slack there, so every quantity (tests.heads_cases.distances: the
  losses, each tensor's relative L2 and worst element, each fusion trunk, the statistics) is held to FOUR TIMES the distance that
  the same graph evaluated in float32 on the CPU shows to the float64 reference (tests.heads_cases.float32_floor: the worst of
  four evaluations, the batch in four orders; the rule of tests/test_cnn_train_gpu.py), and never to more than the project's
  bound; accuracy stays at 1e-6.  The floors are measured at run time and printed with the device's figures (-s).  CPU floors
  measured for the 21 cases: losses 6e-8 .. 1.1e-7, statistics 9e-8 .. 3e-7, a tensor's relative L2 from 6e-8 (2^-24) to 2.5e-6
  for B3_MTL and fusion (a trunk bias, fusion_bn/beta) and to 1.3e-5 for the cascaded model (S or M bn/gamma) -- one exception,
  M/out/bias at B3_MTL N = 539 with head dropout, a one-element sum that nearly cancels: 1.6e-4 --, a Dense(16) bias 3e-9 .. 1.5e-7 absolute.  A relative floor is never taken below one float32 rounding, 2^-24
  (tests.heads_cases.float32_floor says why).
* The shallow cases run with deterministic_gradients: by default the N workgroups' weight-gradient contributions meet in float
  atomics, whose order -- and with it the last bits of every trunk tensor -- changes from run to run; a bound of a few roundings
  needs a device figure that is a function of the inputs.  The two full-size cases keep the default float atomics.
* Device figures with these bounds, measured on an MI355X, the same to the last printed digit in two runs (deterministic mode:
  six steps of a case give `array_equal` buckets).  Per case "worst relative L2 of a tensor (which) | worst device / bound (of
  which quantity)"; over all 21 shallow cases the losses are 4.1e-8 .. 1.4e-7, the statistics 9.7e-8 .. 3.1e-7, the Dense(16)
  biases 1.2e-8 .. 1.4e-7 absolute.
    B3_MTL 3c  N 513  8.0e-7 tcn/s0_d1/conv1x1/bias | 0.40 l2 S/out/bias      N 538  6.2e-7 tcn/initial_conv/bias | 0.58 l2 M/out/bias
               N 539  1.5e-4 M/out/bias | 0.65 el M/bn/gamma                  N 539 nodrop  6.7e-6 M/out/bias | 0.60 l2 M/out/bias
               N 1030 1.2e-6 R/dense/kernel | 0.46 el R/dense/bias            N 512 forced  6.1e-7 M/out/bias | 0.50 el S/dense/bias
    B3_MTL 5c  N 390  6.5e-7 R/dense/kernel | 0.46 el N/dense/bias            N 391  5.7e-7 tcn/s0_d1/conv/bias | 0.54 el S/bn/beta
               N 513  6.9e-7 tcn/s0_d1/conv/bias | 0.63 l2 M/out/bias
    fusion 3c  N 513  8.9e-7 fusion_bn/beta | 0.35 loss                       N 538  1.3e-6 fusion_bn/beta | 0.33 l2 S/bn/beta
               N 539  9.4e-7 fusion_bn/beta | 0.67 l2 S/out/bias              N 539 nodrop  8.0e-7 tcn_P/s0_d2/conv/bias | 0.33 el M/dense/kernel
    fusion 5c  N 391  5.7e-7 M/out/bias | 0.65 el N/bn/gamma                  N 513  7.5e-7 tcn_H/s0_d1/conv1x1/bias | 0.53 l2 R/out/bias
    cascaded   N 903  4.4e-6 M/bn/gamma | 0.29 el tcn/initial_conv/kernel     N 904 5c  1.5e-5 M/bn/gamma | 0.66 l2 S/out/bias
               N 904 nodrop  1.0e-5 S/bn/gamma | 0.40 stats                   N 1616  6.9e-6 M/bn/gamma | 0.61 l2 S/out/bias
               N 1617  7.5e-6 S/bn/gamma | 0.44 l2 S/out/bias                 N 1617 lw  8.0e-6 S/bn/gamma | 0.40 l2 S/out/bias
  The full-size cases (float atomics, the project's bounds): 6.1e-4 tcn/s2_d128/conv/kernel | 0.31 at N = 538, 5.3e-5
  tcn/s2_d64/conv/kernel | 0.03 at N = 600.
* Why deterministic, measured: with float atomics six steps of one case differ in exactly the 14 tensors the backward kernels
  sum over the workgroups (the trunk's kernels and biases, the Dense(16) kernels, 3C/kernel); losses, statistics and every small
  head tensor are bit-identical from step to step on every plan, the cascaded global forms included.  The worst device / bound
  then wanders: 0.69 .. 0.93 at cascaded N = 1616 and 0.47 .. 0.88 at N = 903 (el tcn/initial_conv/kernel: 1616 contributions
  per element in arrival order, against a blocked float32 sum on the CPU), 0.56 .. 0.87 at B3_MTL N = 1030 -- near enough to 1
  to cross it one run in a few.  On the fixed-point grid the same quantity sits at 0.29 (N = 903).

Draws.  With two blocks and 20 frames one row is 1 / sqrt(N W) ~ 1e-2 of a trunk tensor's norm, so ONE gate that float32 takes on
the other branch moves the trunk tensors in front of it by 3e-3 .. 2e-2 (measured on first draws: B3_MTL N = 1030, where the two
largest channels of block s0_d2 at patch 13, frame 7 are 8.0e-9 apart; fusion N = 539 and cascaded N = 1616, whose trunk output
relu has an input of 3.2e-8 and 7.2e-9 of the largest) while heads, losses and statistics stay at 1e-6.  Every shallow case
therefore uses the first draw whose float64 forward has no such gate (tests.heads_cases.gate_margins: channel maxima at least 1e-6
apart, relu inputs at least 1e-7 of the largest; asserted without a GPU in tests/test_heads_plans.py).  The screen covers the
heads' own relus behind BatchNorm(16) too: at cascaded N = 1617 a draw whose S head has a relu input of 2.2e-8 of the largest let
one of the four float32 CPU evaluations take the other branch, which raised the floors of S/bn/gamma (8e-3), S/dense/kernel and,
through d loss / d trunk, of every trunk tensor (1e-3) -- the bound of the head tensors most exposed to a wrong batch sum fell back
to the project's.  With the screened draws no floor of a tensor is above 2e-6 except the one named above."""
import numpy as np
import pytest

from oracle import b3_mtl_train as tr
from tests import heads_cases as H
from tests.heads_cases import CASES, CROSS_PLAN_N, case_id

pytestmark = pytest.mark.gpu


def project_bound(q):
    """The project's bound of a quantity of tests.heads_cases.distances (see the module docstring)."""
    if q == "loss":
        return 2e-4
    if q == "accuracy":
        return 1e-6
    if q == "stats":
        return 1e-4
    kind, name = q.split(" ", 1)
    if kind == "trunk":                      # tests/test_fusion_gpu.py: each whole trunk
        return 2e-3
    if name.endswith("/dense/bias"):
        return 2e-5                          # absolute
    if name.startswith("tcn_"):              # tests/test_fusion_gpu.py: a trunk tensor of the fusion model, relative L2 only
        return 1e-2 if kind == "l2" else np.inf
    return 2e-3 if kind == "l2" else 1e-2 + 1e-6


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_heads_plan_vs_float64_reference(c, monkeypatch):
    kind, ncls, N = c["kind"], c["ncls"], c["N"]
    if c["heads_global"]:
        monkeypatch.setenv("SMH_HEADS_GLOBAL", "1")
    else:
        monkeypatch.delenv("SMH_HEADS_GLOBAL", raising=False)
    m, w, x, y, drop_tcn, drop_heads, heads, s = H.build(kind, ncls, N, c["full"], c["lw"], c["seed"])
    if not c["drop_heads"]:
        drop_heads = None   # no head dropout: the kernels' `dm = 1` branch instead of the mask load
    # The shallow cases are held to a few float32 roundings, so their weight gradients are summed on the 2^-36 fixed-point grid:
    # by default the contributions of the N workgroups meet in float atomics, whose order changes from run to run.
    m.deterministic_gradients = not c["full"]
    got, g, st = H.step(m, x, y, drop_tcn, drop_heads)
    ref = H.reference(kind, x, y, w, ncls, drop_tcn, drop_heads, heads, c["lw"], s)
    D = 32 * s["W"] * (2 if kind == "fusion" else 1)
    assert st.size == 128 + (72 if kind == "cascaded" else 0) + (2 * D if kind == "fusion" else 0)
    assert set(g) == set(ref["grads"])
    # the l2 term of the Dense(16) kernels is added at apply time on the device
    grads = {k: v.astype(np.float64) + (2 * tr.L2 * w[k] if k.endswith("/dense/kernel") else 0.0) for k, v in g.items()}
    dev = H.distances(kind, got, grads, H.batch_statistics(kind, st, heads, D), ref, heads + ["3C"])
    bound = {q: project_bound(q) for q in dev}
    floor = None
    if not c["full"]:
        floor = H.float32_floor(kind, x, y, w, ncls, drop_tcn, drop_heads, heads, c["lw"], s, ref, seed=N)
        assert set(floor) == set(dev)
        bound = {q: (b if q == "accuracy" else min(b, 4 * floor[q])) for q, b in bound.items()}
    l2 = {q: v for q, v in dev.items() if q.startswith(("l2 ", "trunk "))}
    bias = {q: v for q, v in dev.items() if q.endswith("/dense/bias")}
    el = {q: v for q, v in dev.items() if q.startswith("el ") and q not in bias}
    ratio = {q: dev[q] / bound[q] for q in dev if bound[q] > 0}
    print("\n%s: loss %.1e, statistics %.1e, relative L2 %.1e (%s), element %.1e (%s), Dense(16) bias %.1e; worst device / bound %.2f (%s)"
          % (case_id(c), dev["loss"], dev["stats"], max(l2.values()), max(l2, key=l2.get)[3:], max(el.values()), max(el, key=el.get)[3:],
             max(bias.values()), max(ratio.values()), max(ratio, key=ratio.get)))
    if floor is not None:
        print("  float32 floor: loss %.1e, statistics %.1e, relative L2 %.1e .. %.1e, Dense(16) bias %.1e"
              % (floor["loss"], floor["stats"], min(floor[q] for q in l2), max(floor[q] for q in l2), max(floor[q] for q in bias)))
    failures = [(q, dev[q], bound[q]) for q in dev if not dev[q] <= bound[q]]
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------
# the two plans of one batch against each other
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", CROSS_PLAN_N)
def test_staged_and_global_plan_of_one_batch_agree(N, monkeypatch):
    """SMH_HEADS_GLOBAL toggled at a batch that is staged by default (3 classes; N = 510: 512 threads, N = 530: 1024 threads).  The
    trunk forward is bit-identical, so the two heads plans compute the same function and may differ by summation order only: this
    comparison is free of the gate noise of a float64 reference.  deterministic_gradients is on, so that the weight gradients behind
    `dpre` are a fixed function of it and not of the order of float atomics.

    Bound, measured and not chosen: the heads of the float64 reference re-evaluated in float32 with the batch in a permuted order
    (tests.heads_cases.heads_f32, eight permutations against the identity, reference against reference, on the CPU), the worst
    figure per quantity; the device may differ by four times that.  Quantities: the losses (relative to max(1, |loss|)), every
    head tensor and '3C' (relative L2), the trunk tensors (relative L2, held against the CPU figure of d loss / d trunk output, of
    which they are a linear function on fixed gates), the batch statistics (relative to max(1, max |statistic|)), and the
    Dense(16) biases -- analytically zero, and the one quantity the two plans sum by different means (per-wave float sums /
    2^-36 fixed-point atomics) -- as absolute differences, each head against its own CPU figure.

    CPU figures (N = 510 / 530): losses 4.2e-07 / 1.8e-07, head tensors between 3.5e-07 and 8.6e-06 / 2.2e-07 and 4.0e-06 (worst:
    M/out/bias / R/dense/kernel), d loss / d trunk output 7.3e-07 / 6.3e-07, statistics 1.0e-06 / 9.5e-07, Dense(16) biases
    S 1.3e-07 / 8.6e-08, M 6.9e-08 / 5.5e-08, R 9.3e-07 / 7.1e-07 absolute.
    Device figures, measured on an MI355X at both N: losses, statistics, every head tensor and every trunk tensor 0 (the two
    forms run phases A, B and D in the same order, so they are bit-identical there); the Dense(16) biases 6.1e-09 / 8.0e-09
    absolute at worst, against bounds of 2.2e-07 and more."""
    kind, ncls = "B3_MTL", 3
    m, w, x, y, drop_tcn, drop_heads, heads, s = H.build(kind, ncls, N)
    m.deterministic_gradients = True
    runs = {}
    for form in ("staged", "global"):
        if form == "global":
            monkeypatch.setenv("SMH_HEADS_GLOBAL", "1")
        else:
            monkeypatch.delenv("SMH_HEADS_GLOBAL", raising=False)
        runs[form] = H.step(m, x, y, drop_tcn, drop_heads)
    cpu = H.cpu_reorder_figures(N, w, x, y, drop_heads, ncls, s)
    print("\nN = %d CPU figures: losses %.2e, statistics %.2e, dflat %.2e, head tensors %s"
          % (N, cpu["losses"], cpu["stats"], cpu["dflat"], {k: "%.1e" % v for k, v in cpu.items() if "/" in k}))
    assert max(cpu.values()) > 0  # the permutation did reorder the sums
    (la, ga, sa), (lb, gb, sb) = runs["staged"], runs["global"]
    failures = []
    dev_loss = max(abs(a - b) / max(1.0, abs(a)) for a, b in zip(la[:-1], lb[:-1]))
    if dev_loss > 4 * cpu["losses"]:
        failures.append(("losses", dev_loss, cpu["losses"]))
    assert abs(la[-1] - lb[-1]) < 1e-6
    dev_stat = float(np.abs(sa - sb).max() / max(1.0, np.abs(sa).max()))
    if dev_stat > 4 * cpu["stats"]:
        failures.append(("statistics", dev_stat, cpu["stats"]))
    dev_head, dev_trunk, dev_bias = 0.0, 0.0, {}
    for name in ga:
        if name.endswith(tr.TRAINABLE_SKIP):
            continue
        if name.endswith("/dense/bias"):
            d = dev_bias[name] = float(np.abs(ga[name].astype(np.float64) - gb[name]).max())
            bound = 4 * cpu[name]
        else:
            d = float(H.rel_l2(gb[name], ga[name]))
            if name.startswith("tcn/"):
                dev_trunk, bound = max(dev_trunk, d), 4 * cpu["dflat"]
            else:
                dev_head, bound = max(dev_head, d), 4 * cpu[name]
        if d > bound:
            failures.append((name, d, bound))
    print("DEVICE FIGURES N = %d: losses %.2e, statistics %.2e, head tensors %.2e, trunk tensors %.2e, Dense(16) biases %s absolute"
          % (N, dev_loss, dev_stat, dev_head, dev_trunk, {k: "%.1e" % v for k, v in dev_bias.items()}))
    assert not failures, failures
