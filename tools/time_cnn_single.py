"""GPU timing of the single-task Conv2D baselines (get_Doukhan_model / get_Papakostas_model / get_Jang_model) and of their feed, one run:

  1. forward (smh_cnn_forward_f32) at 48 and 256 patches and one training step (train_on_batch, masks drawn, update applied) at the
     drivers' batch -- 3 x 16 patches for Doukhan / Jang, 3 x 64 for Papakostas (Baseline_Results.py:545) -- of each single-task
     model AND of its MTL sibling, ALTERNATING in rounds.  Doukhan and Papakostas run at the single-task input ((30, 68) for Doukhan:
     the MTL kind refuses fewer than 24 rows, the reference's 21 are timed for the single-task model alone) so that the pair runs the
     same trunk; Jang's two graphs differ, its numbers are recorded only.
  2. the plain front end's ragged call on 256 files of 1-10 s (tools/time_ragged.py's workload, W = 68, shift 68) writing IMAGE
     patches (smh_plain_frontend_ragged_layout_f32, patch_layout 0) against the time-major call and the time-major call +
     permute(0, 2, 1).contiguous(), for MelSpec (21 rows), Spec (201) and LogSpec (257, n_fft 512).

Protocol of tools/time_cnn_feed.py: warm-up calls, a host clock around K calls that ends in a device synchronise, the variants
alternating over several rounds; the median round and the spread (min, max) are printed.

    python tools/time_cnn_single.py [B=256] [max seconds=10]"""
import os, sys, time
import ctypes as C
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import _lib
from sm_hpss_mtl_amd.cnn_models import CnnMTL, CnnSingleTask
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig, _ptr, _stream

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
MAXS = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
W = SHIFT = 68
ROUNDS = 5


def rounds(variants, K):
    """variants: [(label, callable)] -> {label: sorted ms per call over ROUNDS rounds}, the variants alternating."""
    for _ in range(2):
        for _, f in variants:
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in variants}
    for _ in range(ROUNDS):
        for k, f in variants:
            t0 = time.perf_counter()
            for _ in range(K):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / K * 1e3)
    return {k: sorted(v) for k, v in ms.items()}


def report(what, ms):
    for k, v in ms.items():
        print("    %-34s %-16s median %8.3f ms (min %8.3f, max %8.3f)" % (what, k, v[ROUNDS // 2], v[0], v[-1]), flush=True)
    if len(ms) == 2:
        (a, va), (b, vb) = ms.items()
        print("    %-34s %s / %s = %.3f; spread of %s: %.3f" % (what, a, b, va[ROUNDS // 2] / vb[ROUNDS // 2], b, vb[-1] / vb[0]), flush=True)


def y_single(n, nc=3):
    return np.eye(nc, dtype=np.float32)[np.arange(n) % nc]


def y_mtl(n):
    c = np.arange(n) % 3
    return {"S": (c == 1).astype(np.float32)[:, None], "M": (c == 0).astype(np.float32)[:, None],
            "R": np.full((n, 2), 0.5, np.float32), "3C": np.eye(3, dtype=np.float32)[c]}


print("single-task Conv2D baselines against their MTL siblings: median of %d alternating rounds" % ROUNDS, flush=True)
# (kind, single-task input, MTL input or None = the same, training batch, calls per round)
MODELS = [("Doukhan", (21, 68), None, 48, 10), ("Doukhan", (30, 68), (30, 68), 48, 10), ("Papakostas", (201, 68), (201, 68), 192, 3),
          ("Jang", (257, 68), (514, 68), 48, 3)]
for kind, shape, mtl_shape, batch, K in MODELS:
    single = CnnSingleTask(kind, shape + (1,), n_classes=3, seed=0)
    models = [("single-task", single, shape)]
    if mtl_shape is not None:
        models.append(("MTL", CnnMTL(kind, mtl_shape + (1,), n_classes=3, seed=0), mtl_shape))
    print("%s %s (MTL %s): %s" % (kind, shape, mtl_shape, ", ".join("%s %d weights" % (k, m.count_params()) for k, m, _ in models)), flush=True)
    for N in (48, 256):
        xs = {k: torch.randn((N,) + s, device="cuda") for k, _, s in models}
        report("forward N = %d" % N, rounds([(k, (lambda m=m, k=k: m.forward_device(xs[k]))) for k, m, _ in models], K))
    xs = {k: torch.randn((batch,) + s, device="cuda") for k, _, s in models}
    ys = {"single-task": single.pack_targets(y_single(batch))}
    if mtl_shape is not None:
        ys["MTL"] = models[1][1].pack_targets(y_mtl(batch))
    report("training step N = %d" % batch, rounds([(k, (lambda m=m, k=k: m.train_on_batch(xs[k], ys[k], sync=False))) for k, m, _ in models], K))
    del models, single, xs, ys
    torch.cuda.empty_cache()

rng = np.random.default_rng(0)
lens = [int(rng.uniform(1.0, MAXS) * 16000) // 2 * 2 for _ in range(B)]  # tools/time_ragged.py's files
offs, o = [], 0
for n in lens:
    offs.append(o)
    o += (n + 3) // 4 * 4
audio = torch.rand(o, device="cuda") - 0.5
h_off, h_len = (C.c_longlong * B)(*offs), (C.c_int * B)(*lens)
print("plain front end, %d files of 1-%.0f s (%.0f s of audio), W = %d, shift = %d" % (B, MAXS, sum(lens) / 16000.0, W, SHIFT), flush=True)
CONFIGS = [("Doukhan_et_al    MelSpec, 21 mels  ", FrontendConfig(n_fft=400, n_mels=21, log_db=False, mel_sr=16000.0, hpss=False)),
           ("Papakostas_et_al Spec, n_fft 400   ", FrontendConfig(n_fft=400, n_mels=0, log_db=False, mel_sr=16000.0, hpss=False)),
           ("Jang_et_al       LogSpec, n_fft 512", FrontendConfig(n_fft=512, n_mels=0, log_db=True, mel_sr=16000.0, hpss=False))]
for name, cfg in CONFIGS:
    fe = Frontend(cfg)
    F = fe.rows
    fv_off, p_off = (C.c_longlong * (B + 1))(), (C.c_longlong * (B + 1))()
    hT, hnP, work = (C.c_int * B)(), (C.c_int * B)(), C.c_size_t()
    _lib.check(fe.lib.smh_plain_frontend_ragged_sizes(fe._h, h_off, h_len, B, W, SHIFT, fv_off, p_off, hT, hnP, C.byref(work)))
    nP = int(p_off[B])
    fv = torch.empty(int(fv_off[B]), device="cuda")
    p_img = torch.empty((nP, F, W), device="cuda")
    p_tm = torch.empty((nP, W, F), device="cuda")
    wk = torch.empty(work.value, dtype=torch.uint8, device="cuda")

    def ragged(layout, patches):
        _lib.check(fe.lib.smh_plain_frontend_ragged_layout_f32(fe._h, _ptr(audio), h_off, h_len, B, W, SHIFT, layout, _ptr(fv),
                                                               _ptr(patches), _ptr(wk), wk.numel(), _stream()))

    def tm_permute():
        ragged(1, p_tm)
        return p_tm.permute(0, 2, 1).contiguous()

    ragged(0, p_img)
    assert torch.equal(p_img, tm_permute())  # the three variants time the same result
    ms = rounds([("image", lambda: ragged(0, p_img)), ("time-major", lambda: ragged(1, p_tm)), ("tm + permute", tm_permute)], 10)
    print("%s  %d rows, %d frames, %d patches (%.0f MB)" % (name, F, sum(hT), nP, nP * F * W * 4 / 1e6), flush=True)
    report("ragged call", ms)
    med = {k: v[ROUNDS // 2] for k, v in ms.items()}
    print("    image / time-major = %.3f; image / (tm + permute) = %.3f" % (med["image"] / med["time-major"], med["image"] / med["tm + permute"]),
          flush=True)
    del fe, fv, p_img, p_tm, wk
