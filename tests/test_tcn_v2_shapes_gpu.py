"""GPU: the forward of the keras-tcn >= 2.8 residual block (smh_tcn_v2.hip, `tcn_block="2.8"`) at every kind of shape the library
accepts, against the numpy oracle (oracle.b3_mtl.tcn_forward_v2, itself cross-checked against a float64 torch build in
tests/test_oracle_pins.py), and the two serving paths a 2.8 model goes through.

The kernel has its own layer 0 (streamed from the patches in HBM, k padded to 4 * ceil(n_feat / 4) with masked tails), its own
offset table into the canonical weight tensor and its own two-barrier block schedule.  The other GPU tests of this block run
n_feat = 240 (one cascaded case: 120), 3 x 8 blocks and W in {68, 99, 249}; why each shape below is here:

- (20, 1, 1): one block -- the later-blocks loop never runs.  From block 1 on the block input and the branch are both >= 0, so
  relu(x + y) never clips there: ONLY block 0, whose shortcut reads the raw (signed) input, exercises the outer relu, and only a
  one-block model shows its result undiluted.  The (., 1, 1, .) cases therefore also demand that a good share of the oracle's
  trunk is exactly zero and a good share positive.
- n_feat = 32 = nb_filters: Keras builds no 'matching' 1x1 convolution when the channel counts agree; block 0 has the identity
  shortcut on the raw input (no matching tensors in the canonical order).  Alone (1 x 1), at depth with a batch, and cascaded.
- 31 and 33, the neighbours of 32, and 61, 75: n_feat % 4 != 0, so FQ * 4 > n_feat and the masked k tail of both block-0 phases
  runs; 402 (FQ * 4 = 404) is the widest layer-0 stream.
- (61, 10, 16): 160 blocks, dilations up to 32768 >> T: both side taps are skipped and `row + offset` is far outside the buffer
  unless guarded.
- (75, 10, 8, W = 25, N = 307): two patches per workgroup, 50 rows -- not a multiple of the 16-row tile --, one patch in the last
  workgroup: dilated taps must stop at the patch boundary inside a tile.  (40, 3, 8, 25, 769): four patches per workgroup, one in
  the last.  Cascaded (61, 3, 3, 50, 307): two per workgroup.
- W = 5: shorter than one tile and than the larger dilations.  W = 512: the longest patch the library takes (x and y buffers
  147.7 kB of the 156 kB gate), 32 column tiles on 8 waves.
- (240, 1, 1, 100, 1, 5): one patch, one block, five classes.

Inputs lie in the middle of a NaN-filled buffer: the clamped t - 1 row of the first patch and t + 1 row of the last are where a
block-0 load could leave the batch, and a load on either side turns outputs into NaN (in-bounds memory: no fault).  The trunk
tensor starts as NaN, so an unwritten row shows.

Weights: init_weights_v2(randomize_bn=True) with the dilated-convolution kernels scaled by 0.5 as tests/test_parity_gpu.py scales
them (no channel normalisation in this block: the trunk grows with depth), by 0.4 at 80 blocks and 0.3 at 160.  Every case asserts
on the ORACLE alone that its trunk is alive and bounded (maximum in [0.1, 200], at most 90 % zeros), so a dead or exploded trunk
cannot pass silently.

Tolerances are those of the existing test of this block (tests/test_parity_gpu.py): trunk within 2e-4 * max(1, max |ref trunk|),
outputs within 2e-4, '3C' argmax equal on the checked rows, at every depth: a float32-accumulating numpy restatement of the same
trunk with another summation order lies 0.6-4.2e-7 of the trunk's scale from the float64 oracle on these cases (outputs: at most
4.5e-6, at 160 blocks), so the rounding floor of a float32 evaluation is two orders below the bounds."""
import numpy as np
import pytest
import torch

from oracle import b3_mtl
from oracle import frontend as ofe
from oracle import inference as oinf
from tests import cascaded_ref as cref

pytestmark = pytest.mark.gpu

TOL = 2e-4  # tests/test_parity_gpu.py::test_b3mtl_two_conv_block_variant_vs_oracle


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def inside_nan(x, pad=64):
    """x as a contiguous device tensor with NaN in the `pad` floats before its first element and behind its last: a kernel that
    reads a row before the first patch or past the last turns outputs into NaN (in-bounds memory: no fault)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.full((x.size + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[pad:pad + x.size] = torch.from_numpy(x.ravel()).cuda()
    return buf[pad:pad + x.size].view(x.shape)


def rows_to_check(N, n=8):
    return np.unique(np.r_[0:min(n // 2, N), max(0, N - n // 2):N])


def kernel_scale(nb, nd):
    return 0.5 if nb * nd <= 24 else (0.4 if nb * nd <= 80 else 0.3)


def weights(F, W, ncls, nb, nd, seed=9):
    w = b3_mtl.init_weights_v2(seed=seed, n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dil=nd, randomize_bn=True)
    for k in w:
        if "/conv" in k and k.endswith("kernel"):
            w[k] = (w[k] * kernel_scale(nb, nd)).astype(np.float32)
    return w


def check_oracle_trunk(ref_trunk, one_block):
    """Conditions on the oracle alone: the comparison below means something only on a live, bounded trunk."""
    zeros = float(np.mean(ref_trunk == 0))
    assert 0.1 <= float(ref_trunk.max()) <= 200.0, float(ref_trunk.max())
    assert zeros <= 0.9, zeros
    if one_block:  # the outer relu of block 0 both clips and passes
        assert zeros >= 0.2 and float(np.mean(ref_trunk > 0)) >= 0.2, zeros


def compare(m, x, sel, ref, ref_trunk, tol_t, tol_o, ncls):
    """forward_device with the trunk tap on the NaN-guarded input against the oracle's rows `sel`."""
    N, W = x.shape[:2]
    trunk = torch.full((N, W, 32), float("nan"), device="cuda")
    out = host(m.forward_device(inside_nan(x), trunk=trunk))
    m.check_status()
    trunk = host(trunk)
    assert np.isfinite(out).all() and np.isfinite(trunk).all()
    err_t, err_o = float(np.abs(trunk[sel] - ref_trunk).max()), float(np.abs(out[sel] - ref).max())
    print("trunk max %.4g, zeros %.3f; |trunk - ref| %.3g (bound %.3g); |out - ref| %.3g (bound %.3g)"
          % (ref_trunk.max(), np.mean(ref_trunk == 0), err_t, tol_t, err_o, tol_o))
    assert err_t <= tol_t
    assert err_o <= tol_o
    assert np.array_equal(out[sel][:, -ncls:].argmax(1), ref[:, -ncls:].argmax(1))
    return out


FORWARD_SHAPES = [  # (n_feat, nb_stacks, n_dilations, W, N, n_classes)
    (20, 1, 1, 25, 3, 3), (32, 1, 1, 68, 3, 3), (32, 3, 8, 68, 307, 5), (31, 3, 3, 50, 3, 3), (33, 3, 3, 50, 3, 5),
    (61, 10, 16, 50, 3, 3), (75, 10, 8, 25, 307, 5), (40, 3, 8, 25, 769, 5), (402, 3, 8, 68, 3, 3), (60, 3, 3, 5, 3, 3),
    (240, 3, 8, 512, 2, 3), (240, 1, 1, 100, 1, 5),
]


@pytest.mark.parametrize("F,nb,nd,W,N,ncls", FORWARD_SHAPES)
def test_v2_forward_and_trunk_vs_oracle(F, nb, nd, W, N, ncls):
    from sm_hpss_mtl_amd.model import B3MTL
    w = weights(F, W, ncls, nb, nd)
    m = B3MTL(n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dilations=nd, tcn_block="2.8")
    assert [n for n, _, _, _ in m._spec] == list(w) and m.count_params() == sum(v.size for v in w.values())
    m.set_weights_dict(w)
    x = np.random.default_rng(F * 7 + W + N).standard_normal((N, W, F)).astype(np.float32)
    sel = rows_to_check(N)

    def heads(trunk):
        return np.concatenate(b3_mtl.mtl_heads(trunk.reshape(trunk.shape[0], -1), w, ncls), axis=1)

    ref_trunk = b3_mtl.tcn_forward_v2(x[sel], w, nb, nd)
    check_oracle_trunk(ref_trunk, nb * nd == 1)
    compare(m, x, sel, heads(ref_trunk), ref_trunk, TOL * max(1.0, float(np.abs(ref_trunk).max())), TOL, ncls)


@pytest.mark.parametrize("F,nb,nd,W,N,ncls", [(32, 3, 8, 68, 7, 3), (61, 3, 3, 50, 307, 5)])
def test_v2_cascaded_forward_vs_reference(F, nb, nd, W, N, ncls):
    from sm_hpss_mtl_amd.model import CascadedMTL
    m = CascadedMTL(n_feat=F, patch_size=W, n_classes=ncls, nb_stacks=nb, n_dilations=nd, seed=0, tcn_block="2.8")
    w = cref.init_weights(seed=3, n_feat=F, patch_size=W, n_classes=ncls)
    w.update((k, v) for k, v in weights(F, W, 3, nb, nd, seed=3).items() if k.startswith("tcn/"))
    w = {name: w[name] for name, _, _, _ in m._spec}  # the model's canonical order; drops the 2.3 trunk of cref.init_weights
    m.set_weights_dict(w)
    x = np.random.default_rng(W + N).standard_normal((N, W, F)).astype(np.float32)
    sel = rows_to_check(N)
    ref_trunk = b3_mtl.tcn_forward_v2(x[sel], w, nb, nd)
    check_oracle_trunk(ref_trunk, False)
    ref = np.concatenate(cref.heads_forward(ref_trunk.reshape(len(sel), -1), w, ncls), axis=1)
    compare(m, x, sel, ref, ref_trunk, TOL * max(1.0, float(np.abs(ref_trunk).max())), TOL, ncls)


# ---------------------------------------------------------------------------------------------------
# serving paths of a 2.8 model
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def m28():
    from sm_hpss_mtl_amd.model import B3MTL
    w = weights(240, 68, 3, 3, 8, seed=2)
    m = B3MTL(n_feat=240, patch_size=68, n_classes=3, seed=0, tcn_block="2.8")
    m.set_weights_dict(w)
    return m, w


def test_hot_path_takes_the_patch_route_for_a_v2_model(m28):
    """HotPath's default fuses the network's first 1x1 convolution into the feature kernel; the 2.8 block has none.  Decided at
    construction: fuse_l0 falls back to patches -> forward_device, the split-bf16 network is refused before anything is launched."""
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.pipeline import HotPath
    from sm_hpss_mtl_amd.synth import synth_clips
    m, w = m28
    fe = Frontend(FrontendConfig())
    hp = HotPath(fe, m, 4, 16000, keep_patches=True)
    assert hp.fuse_l0 is False and hp.x0p is None and hp.patches is not None
    logits = hp.step(torch.from_numpy(synth_clips(4, seed=0)).cuda())
    m.check_status()
    assert logits.shape == (4 * hp.nP, m.out_dim) and hp.nP >= 1
    assert torch.equal(logits, m.forward_device(hp.patches))
    sel = np.arange(min(8, logits.shape[0]))
    ref = np.concatenate(b3_mtl.forward(host(hp.patches)[sel], w), axis=1)
    err = float(np.abs(host(logits)[sel] - ref).max())
    print("|HotPath logits - oracle| %.3g" % err)
    assert err <= TOL
    with pytest.raises(ValueError, match="f32 forward only"):
        HotPath(fe, m, 4, 16000, model_dtype="bf16")


def test_patch_probabilities_of_a_v2_model_vs_oracle(m28, monkeypatch):
    """The inputs of test_inference_gpu.py::test_patch_probabilities_vs_oracle -- a 298-frame featuregram walked in batches of
    120 frames, the short last one tiled -- with a 2.8 model: the dense entry (layer 0 once per frame) does not exist for this
    block, every batch goes through built patches."""
    from sm_hpss_mtl_amd import inference as inf
    from sm_hpss_mtl_amd.synth import synth_clips
    m, w = m28
    fv = ofe.featuregram(synth_clips(1, seed=3, n_samples=48000)[0], "LogMelHarmPercSpec")
    assert fv.shape == (240, 298)
    with pytest.raises(ValueError, match="2.3.x block only"):
        m.forward_dense(torch.zeros((240, 120), device="cuda"), 1)

    def not_taken(*args, **kwargs):
        raise AssertionError("patch_probabilities took the dense entry with a 2.8 model")
    monkeypatch.setattr(m, "forward_dense", not_taken)
    got = inf.patch_probabilities(fv, m, 68, 1, output="M", batch_frames=120)
    ref = oinf.patch_probabilities(fv, w, 68, 1, output="M", batch_frames=120)
    assert got.shape == ref.shape and got.shape[0] == 2 * (120 - 68) + len(ofe.patch_starts(116, 68, 1))
    err = float(np.abs(got - ref).max())
    print("|track - oracle| %.3g" % err)
    assert err <= TOL
