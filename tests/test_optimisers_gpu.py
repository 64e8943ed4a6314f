"""GPU: the optimiser pass of the TCN training step (seg_sumsq_kernel / seg_opt_kernel / smh_trainer_apply_f32) against
oracle.b3_mtl_train's sgd_step / adam_step / nadam_step (pinned against torch.optim on the CPU: tests/test_oracle_train.py), for
the three optimisers on B3_MTL and for SGD and Adam on the cascaded and the intermediate-fusion model, four steps each.

What is compared.  Each step runs train_on_batch(apply=False), reads the bucket [gradient | BatchNorm batch statistics], then
apply_gradients().  The oracle's optimiser is fed the DEVICE gradient of that step (as test_single_head_sub_model_nadam_fine_tuning
does): this is a check of the update arithmetic -- the l2 term 2 * 0.01 * w of the Dense(16) kernels, the per-tensor clipnorm with
the norm of a tensor longer than kSegChunk = 4096 added up from several workgroups' partial sums, momentum / the moments, Adam's
alpha(t), Nadam's momentum schedule and its running product, the 0.99 / 0.01 moving statistics -- and the gradient itself is held
against the float64 references elsewhere (tests/test_heads_plans_gpu.py, test_training_gpu.py).  The weights live in float32 on the
device, so each oracle step starts from the device's stored weights (again as that test does), while velocity, moments, step
count and m_schedule stay the oracle's own float64 state for all four steps: a wrong bias correction or a lost moment shows from
the step it happens.

Bound per tensor and step, the one of test_sgd_step_matches_oracle: |got - want| <= 2e-3 * (how far the oracle moved the tensor in
this step) + 1e-7."""
import numpy as np
import pytest

from oracle import b3_mtl_train as tr
from tests.heads_cases import batch_statistics, build, step

pytestmark = pytest.mark.gpu

K_SEG_CHUNK = 4096  # smh_train.hip: kSegChunk
# clipnorm of the clipped runs: the reference's own (lib/proposed_architectures.py:156-158).  On these problems (fresh weights, random
# inputs) about half of the gradient tensors are longer than that -- the Dense(16) kernels with their l2 term at 5 to 36, the
# convolution kernels of the trunk -- and half are shorter (biases, most BatchNorm tensors); every step asserts that both occur
CLIP = 1.0


def make_optimizer(opt, clipnorm):
    from sm_hpss_mtl_amd import optimizers
    if opt == "sgd":  # lib/proposed_architectures.py:156-158 with TR_STEPS = 10: a rate that decays from step to step
        return optimizers.SGD(learning_rate=optimizers.ExponentialDecay(0.002, 30, 0.1), momentum=0.9, clipnorm=clipnorm)
    return (optimizers.Adam if opt == "adam" else optimizers.Nadam)(learning_rate=1e-3, clipnorm=clipnorm)


def oracle_learning_rate(opt, t):
    return tr.exponential_decay(t, 0.002, 30, 0.1) if opt == "sgd" else 1e-3


def moving_name(key):
    """Key of tests.heads_cases.batch_statistics -> prefix of the moving statistics it feeds."""
    return key if ("/" in key or key == "fusion_bn") else key + "/bn"


def run_steps(kind, opt, clipnorm, sizes):
    """len(sizes) optimiser steps, step t on the first sizes[t] rows of one problem -> the trainer capacities seen."""
    N = max(sizes)
    m, w, x, y, drop_tcn, drop_heads, heads, s = build(kind, 3, N, full=True)
    m.compile(optimizer=make_optimizer(opt, clipnorm))
    assert (m.optimizer.kind, m.optimizer.clipnorm) == (opt, clipnorm)
    D = 32 * s["W"] * (2 if kind == "fusion" else 1)
    trainable = [k for k in w if not k.endswith(tr.TRAINABLE_SKIP)]
    state, caps, worst = {}, [], (0.0, None)
    for t, n in enumerate(sizes):
        now = m.get_weights_dict()
        wd = {k: now[k].astype(np.float64) for k in w}   # the device's stored float32 weights
        xs = [a[:n] for a in x] if kind == "fusion" else x[:n]
        dts = drop_tcn[:, :n] if kind == "fusion" else drop_tcn[:n]
        lr = m.learning_rate()
        assert abs(lr - oracle_learning_rate(opt, t)) < 1e-12
        _, g, st = step(m, xs, {k: v[:n] for k, v in y.items()}, np.ascontiguousarray(dts), drop_heads[:n])
        caps.append(m._trainer_cap)
        grads, clipped, kept = {}, [], []
        for k in trainable:
            gk = g[k].astype(np.float64)
            if k.endswith("/dense/kernel"):
                gk = gk + 2 * tr.L2 * wd[k]   # kernel_regularizer=l2(0.01): added at apply time on the device
            nrm = np.sqrt(np.sum(gk * gk))
            if clipnorm is not None and nrm > clipnorm:
                gk = gk * (clipnorm / nrm)
                clipped.append(k)
            else:
                kept.append(k)
            grads[k] = gk
        if clipnorm is not None:
            # the step does exercise clipnorm, on both sides -- and on a tensor whose norm is the sum of several workgroups' partials
            assert len(clipped) >= 1 and len([k for k in kept if not k.endswith("/dense/bias")]) >= 1, (t, clipped, kept)
            assert any(w[k].size > K_SEG_CHUNK for k in clipped), (t, clipped)
        else:
            assert any(np.sqrt(np.sum(grads[k] ** 2)) > CLIP for k in trainable)  # ... and its absence is a different update
        m.apply_gradients()
        own = {k: wd[k] for k in trainable}
        if opt == "sgd":
            new, vel = tr.sgd_step(own, grads, state.get("vel", {}), {}, lr, momentum=0.9, clipnorm=None)
            state = {"vel": vel}
        elif opt == "adam":
            new, state = tr.adam_step(own, grads, state, lr, names=trainable)
        else:
            new, state = tr.nadam_step(own, grads, state, lr, names=trainable)
        want = dict(new)
        for key, (mean, var) in batch_statistics(kind, st.astype(np.float64), heads, D).items():
            p = moving_name(key)
            want[p + "/moving_mean"] = tr.BN_MOMENTUM * wd[p + "/moving_mean"] + (1 - tr.BN_MOMENTUM) * mean
            want[p + "/moving_variance"] = tr.BN_MOMENTUM * wd[p + "/moving_variance"] + (1 - tr.BN_MOMENTUM) * var
        assert set(want) == set(w)
        got = m.get_weights_dict()
        failures = []
        for k in w:
            delta = np.abs(want[k] - wd[k]).max()   # how far the oracle moved this tensor in this step
            err = np.abs(got[k] - want[k]).max()
            bound = 2e-3 * delta + 1e-7
            worst = max(worst, (err / bound, "step %d %s" % (t, k)))
            if err > bound:
                failures.append((t, k, err, delta))
            if not k.endswith("/dense/bias"):
                assert delta > 0, (t, k)   # every tensor is trained (a Dense(16) bias in front of BatchNorm has no gradient)
        assert not failures, failures
    print("\n%s %s clipnorm %s: worst error / bound %.3f (%s)" % (kind, opt, clipnorm, worst[0], worst[1]))
    assert m.iterations == len(sizes)
    return caps


@pytest.mark.parametrize("clipnorm", [None, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("opt", ["sgd", "adam", "nadam"])
def test_b3mtl_four_steps_of_every_optimiser_match_the_oracle(opt, clipnorm):
    """B3_MTL, all groups active, W = 68 (the Dense(16) kernels are 34 816 elements: nine kSegChunk pieces each, clipped in the
    clipped runs).  SGD with clipnorm is the optimiser exactly as the reference builds it: momentum 0.9, clipnorm 1, a rate that
    decays from step to step.  Four steps: Adam's alpha(t) and Nadam's m_schedule product are past their first values."""
    run_steps("B3_MTL", opt, clipnorm, [12] * 4)


@pytest.mark.parametrize("clipnorm", [None, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("kind", ["cascaded", "fusion"])
def test_cascaded_and_fusion_four_steps_match_the_oracle(kind, opt, clipnorm):
    """The same four steps, unclipped and clipped, for the models with more tensors: '*/cat_bn/*' (affine and moving statistics of the cascaded
    concatenation BatchNorm), 'fusion_bn/*' (4 352 wide: two kSegChunk pieces) and both trunks of the fusion model."""
    run_steps(kind, opt, clipnorm, [12] * 4)


def test_growing_the_trainer_keeps_nadam_state():
    """A larger batch at step 3 re-creates the native trainer (capacity 64 -> 96): the moments, `step` and Nadam's `m_schedule`
    travel in smh_trainer_copy_state.  The oracle's state knows nothing of the growth: the trajectory must stay on it
    (test_growing_the_trainer_keeps_the_optimiser_state covers SGD's momentum only)."""
    caps = run_steps("B3_MTL", "nadam", None, [48, 48, 96, 96])
    assert caps == [64, 64, 96, 96]
