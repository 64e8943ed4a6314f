"""CPU: the float64 reference of the single-task Lemaire TCN baseline (tests/single_task_ref.py) against an independent torch.nn
build, the loss conventions it states, the parameter count of the weight spec, and the conditions the GPU tests put on their own
reference inputs (tests/test_single_task_gpu.py asserts them again where it uses them)."""
import numpy as np
import pytest
import torch

from tests import single_task_plans as plans
from tests import single_task_ref as sref


class _Net(torch.nn.Module):
    """The network from torch.nn layers: Conv1d modules and a Linear, nothing shared with the reference's functions."""

    def __init__(self, w, F, W, ncls, nb_stacks=3, n_dil=8):
        super().__init__()
        nn = torch.nn

        def conv(k, b, d):
            taps, cin, cout = k.shape
            c = nn.Conv1d(cin, cout, taps, padding=(taps // 2) * d, dilation=d).double()
            c.weight.data = torch.tensor(np.asarray(k, np.float64)).permute(2, 1, 0).contiguous()
            c.bias.data = torch.tensor(np.asarray(b, np.float64))
            return c
        self.first = conv(w["tcn/initial_conv/kernel"], w["tcn/initial_conv/bias"], 1)
        self.blocks = nn.ModuleList()
        for s in range(nb_stacks):
            for i in range(n_dil):
                p = "tcn/s%d_d%d" % (s, 2 ** i)
                self.blocks.append(nn.ModuleList([conv(w[p + "/conv/kernel"], w[p + "/conv/bias"], 2 ** i),
                                                  conv(w[p + "/conv1x1/kernel"], w[p + "/conv1x1/bias"], 1)]))
        self.dense = nn.Linear(W * 32, ncls).double()
        self.dense.weight.data = torch.tensor(np.asarray(w["dense/kernel"], np.float64)).t().contiguous()
        self.dense.bias.data = torch.tensor(np.asarray(w["dense/bias"], np.float64))

    def forward(self, x):  # x (N, W, F) float32
        """oracle.b3_mtl's trunk keeps float32 storage between layers (float64 products, every layer's output rounded to float32,
        the normalisation and the residual sum in float32); the layers here round at the same points, so that what is compared is
        the arithmetic of two implementations and not 49 float32 roundings (3e-7 at the outputs)."""
        h = self.first(x.double().transpose(1, 2)).float()
        for dil, one in self.blocks:
            r = torch.relu(dil(h.double()).float())
            yn = r / (r.amax(dim=1, keepdim=True) + torch.tensor(sref.NORM_EPS, dtype=torch.float32))
            h = h + one(yn.double()).float()
        flat = torch.relu(h).double().transpose(1, 2).reshape(x.shape[0], -1)  # Keras Flatten of (W, 32): time-major
        return torch.softmax(self.dense(flat), dim=1)


@pytest.mark.parametrize("W,F,ncls,N", [(68, 80, 2, 5), (99, 21, 3, 4), (68, 100, 5, 3)])
def test_numpy_forward_equals_torch_nn_build(W, F, ncls, N):
    w = sref.init_weights(seed=3, n_feat=F, patch_size=W, n_classes=ncls)
    x = np.random.default_rng(W + N).standard_normal((N, W, F)).astype(np.float32)
    ref = sref.forward(x, w, ncls)
    with torch.no_grad():
        got = _Net(w, F, W, ncls)(torch.tensor(x)).numpy()
    assert ref.shape == (N, ncls) and np.abs(got - ref).max() <= 1e-10, np.abs(got - ref).max()
    # the autograd graph is the same network in float64 throughout: apart from the trunk's 49 float32 roundings (2^-24 each on O(1)
    # activations, 3e-6 if they all lined up) its forward is the same function
    y = np.eye(ncls)[np.arange(N) % ncls]
    assert np.abs(sref.torch_forward_backward(x, y, w, ncls)["probs"] - ref).max() <= 1e-5


def train_problem(N, ncls, W=68, F=80, n_blocks=24):
    """The inputs of the GPU training-step cases (seeded by N alone)."""
    rng = np.random.default_rng(plans.TRAIN_SEED + N)
    x = rng.standard_normal((N, W, F)).astype(np.float32)
    y = np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, N)]
    drop = ((rng.random((N, n_blocks, 32)) > 0.2) / 0.8).astype(np.float32)
    return x, y, drop


@pytest.mark.parametrize("N", [5, 65])
def test_two_class_bce_is_minus_log_p_true_and_binary_accuracy_is_categorical(N):
    """With two softmax outputs 1 - p_1 = p_0, so Keras' bce averaged over the two outputs is -log(p_true + 1e-7), and an output is
    above 0.5 exactly when it is the argmax: the two accuracies agree."""
    w = sref.init_weights(seed=5, n_classes=2)
    x, y, drop = train_problem(N, 2)
    r = sref.torch_forward_backward(x, y, w, 2, drop)
    p_true = (r["probs"] * y).sum(1)
    assert abs(r["loss"] - float(np.mean(-np.log(p_true)))) <= 1e-6
    assert r["acc"] == float(np.mean(r["probs"].argmax(1) == y.argmax(1)))


@pytest.mark.parametrize("W,F,ncls", [(68, 80, 2), (68, 100, 3), (249, 80, 5), (99, 21, 2)])
def test_weight_spec_parameter_count(W, F, ncls):
    from sm_hpss_mtl_amd.host import HEADS_SINGLE
    from sm_hpss_mtl_amd.model import initial_weights, weight_spec
    spec = weight_spec(F, W, ncls, heads=HEADS_SINGLE)
    trunk = F * 32 + 32 + 24 * (3 * 32 * 32 + 32 + 32 * 32 + 32)
    assert sum(int(np.prod(s)) for _, s, _, _ in spec) == trunk + W * 32 * ncls + ncls
    assert [n for n, _, _, _ in spec][-2:] == ["dense/kernel", "dense/bias"]
    assert [n for n, _, _, _ in spec] == list(sref.init_weights(n_feat=F, patch_size=W, n_classes=ncls))
    _, w = initial_weights(F, W, ncls, seed=0, heads=HEADS_SINGLE)
    lim = np.sqrt(6.0 / (W * 32 + ncls))  # Keras Dense: glorot_uniform kernel, zero bias
    assert np.abs(w["dense/kernel"]).max() <= lim and not w["dense/bias"].any()


def test_head_plan_change_points_are_among_the_train_cases():
    assert plans.plan(1) == plans.plan(512) == (512, 1) and plans.plan(513) == (512, 2)
    assert plans.change_points(600) == [512, 513]
    ns = [c[0] for c in plans.TRAIN_CASES]
    assert set(plans.change_points(max(ns))) <= set(ns)
    assert {1, 2, 3, 4, 5, 63, 64, 65, 510} <= set(ns) and {c[1] for c in plans.TRAIN_CASES} == {2, 3, 5}


@pytest.mark.parametrize("N,ncls,nb,nd,W", plans.TRAIN_CASES)
def test_train_cases_are_well_conditioned(N, ncls, nb, nd, W):
    """What the GPU cases ask of their own inputs, on the reference alone.  Every reference probability lies in [1e-6, 1 - 1e-6]:
    the unclipped branch is the one compared.  And the same graph evaluated in float32 gives every gradient tensor within a TENTH
    of the GPU test's bound, 2e-4 max|ref| + 1e-7: no relu gate or channel-maximum tie of the case sits within float32 rounding
    (tests/single_task_plans.py; the 24-block trunk at 510 patches misses this at 7e-3 of a tensor's maximum)."""
    w = sref.init_weights(seed=5, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dil=nd)
    x, y, drop = train_problem(N, ncls, W=W, n_blocks=nb * nd)
    r64 = sref.torch_forward_backward(x, y, w, ncls, drop, nb, nd)
    p = r64["probs"]
    assert p.min() >= 1e-6 and p.max() <= 1 - 1e-6, (N, ncls, p.min(), p.max())
    r32 = sref.torch_forward_backward(x, y, w, ncls, drop, nb, nd, dtype=np.float32)
    for name, gref in r64["grads"].items():
        err, scale = np.abs(r32["grads"][name] - gref).max(), np.abs(gref).max()
        assert err <= 2e-4 * scale + 1e-7, (name, err, scale)


def test_builder_argument_checks_need_no_gpu():
    from sm_hpss_mtl_amd.lib import baseline_architectures as ba
    for kw, word in [(dict(n_layers=2), "n_layers"), (dict(n_filters=16), "n_filters"), (dict(kernel_size=5), "kernel_size"),
                     (dict(use_skip_connections=True), "use_skip_connections"), (dict(activation="relu"), "activation"),
                     (dict(n_classes=4), "n_classes")]:
        with pytest.raises(ValueError, match=word):
            ba.get_Lemaire_model(10, **kw)
    for fn in (ba.get_Doukhan_model, ba.get_Papakostas_model, ba.get_Jang_model):
        with pytest.raises(NotImplementedError, match="single-task Conv2D baselines are not built"):
            fn({})
    import lib.baseline_architectures as shim
    assert shim.get_Lemaire_model is ba.get_Lemaire_model
