"""GPU timing of dense file-level inference (DAFx12_Speech_Music_Detection_B3_MTL_v2.py:594-706): one file's
featuregram (240, T), hop-1 patches of W frames, the 'M' head's probability per patch, then the 501-wide median.  Prints ms per
10 000-frame batch and patches per second, by parts, and -- in the same run, the two dtypes alternating call by call --
`forward_dense` alone and the whole `patch_probabilities` call for dtype "f32" and "bf16" (split bf16 operands,
smh_model_forward_dense_bf16), with the maximum difference of the two tracks.

    python tools/time_dense_inference.py [T = 10000] [W = 68] [reps = 30]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import inference
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
from sm_hpss_mtl_amd.model import B3MTL

T = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
W = int(sys.argv[2]) if len(sys.argv) > 2 else 68
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 30
rng = np.random.default_rng(0)
fv = torch.from_numpy(rng.standard_normal((240, T)).astype(np.float32) * 12 - 40).cuda()
model = B3MTL(n_feat=240, patch_size=W, n_classes=3, seed=0)
fe = Frontend(FrontendConfig())


def timed(fn, reps=10):
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def alternating(fns, reps=REPS):
    """fns: {label: call}; every call warmed, then timed one at a time (host clock around a device synchronise), the labels taking
    turns -> {label: (median ms, min ms, max ms)}, {label: last result}."""
    outs = {}
    for _ in range(3):
        for k, fn in fns.items():
            outs[k] = fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            outs[k] = fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ms.items()}, outs


ms, track = timed(lambda: inference.patch_probabilities(fv, model, W, 1, "M"))
n = len(track)
print("patch_probabilities (layer 0 once per frame, patches as windows): T = %d frames, W = %d -> %d patches: %.3f ms = %.2f M patches/s" % (T, W, n, ms, n / ms / 1e3), flush=True)
os.environ["SMH_DENSE_PATCHES"] = "1"
ms_b, track_b = timed(lambda: inference.patch_probabilities(fv, model, W, 1, "M"))
del os.environ["SMH_DENSE_PATCHES"]
print("patch_probabilities (patches built, SMH_DENSE_PATCHES=1): %.3f ms = %.2f M patches/s; max |difference| of the two tracks %.2e" % (
    ms_b, n / ms_b / 1e3, float(np.max(np.abs(track - track_b)))), flush=True)
std = torch.cat([fe.standardize_rows(fv[:120]), fe.standardize_rows(fv[120:])], dim=0)
ms_d, _ = timed(lambda: model.forward_dense(std, 1))
print("  forward_dense alone (l0_frames_kernel + the forward from windows): %.3f ms" % ms_d, flush=True)
R = 120
d = torch.cat([fe.standardize_rows(fv[:R]), fe.standardize_rows(fv[R:])], dim=0)


def gather():
    h = fe.extract_patches(fe.standardize_rows(d[:R])[None], W, 1, time_major=True)
    p = fe.extract_patches(fe.standardize_rows(d[R:])[None], W, 1, time_major=True)
    return torch.cat([h, p], dim=2)


ms_g, x = timed(gather)
ms_f, _ = timed(lambda: model.forward_device(x))
print("  parts: standardise + hop-1 patch gather + concat %.3f ms (%.0f MB of patches), forward from patches %.3f ms" % (ms_g, x.numel() * 4 / 1e6, ms_f), flush=True)
tr = torch.from_numpy(track).cuda()
ms_m, _ = timed(lambda: inference.medfilt(tr, 501))
print("  medfilt(501) over the %d-value track: %.3f ms" % (n, ms_m), flush=True)
# ---- f32 against split bf16 operands, alternating in this process ----
DTYPES = ("f32", "bf16")
res, outs = alternating({dt: (lambda dt=dt: model.forward_dense(std, 1, dtype=dt)) for dt in DTYPES})
for dt in DTYPES:
    med, lo, hi = res[dt]
    print("forward_dense dtype=%s: median %.3f ms (min %.3f, max %.3f) per %d-frame chunk = %.2f M patches/s" % (
        dt, med, lo, hi, T, outs[dt].shape[0] / med / 1e3), flush=True)
print("forward_dense f32 / bf16 time: %.2f; max |difference| of the outputs %.2e" % (
    res["f32"][0] / res["bf16"][0], float((outs["f32"] - outs["bf16"]).abs().max())), flush=True)
res, outs = alternating({dt: (lambda dt=dt: inference.patch_probabilities(fv, model, W, 1, "M", dtype=dt)) for dt in DTYPES})
for dt in DTYPES:
    med, lo, hi = res[dt]
    print("patch_probabilities dtype=%s: median %.3f ms (min %.3f, max %.3f) = %.2f M patches/s" % (
        dt, med, lo, hi, len(outs[dt]) / med / 1e3), flush=True)
print("patch_probabilities f32 / bf16 time: %.2f; max |difference| of the two tracks %.2e" % (
    res["f32"][0] / res["bf16"][0], float(np.max(np.abs(outs["f32"] - outs["bf16"])))), flush=True)
