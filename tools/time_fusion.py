"""GPU timing of the intermediate-fusion model next to B3_MTL at the same shapes: the f32 forward at 1024 patches and the f32
training step (forward-train, fused BN, heads, backward of both trunks, SGD) at 48 and 510 patches, W = 68 and 249.  B3_MTL reads the
240-wide H||P patches, the fusion model the two 120-wide halves.  The two models are timed in alternating rounds on the same warm
device; each line reports the median and range over the rounds.

With --inference: the fusion model's inference without materialised input halves, each row against the only way to the same
result without it (materialised halves -> forward_device), on the same inputs, alternating rounds:
  * forward from the front end's outputs (S, medians), 1024 patches, W = 68: features (patches) + the two halves copied out +
    forward_device, against features_l0 + forward_from_x0_halves;
  * file-level, one 10 000-frame chunk at hop 1, W = 68: extract_patches per half + forward_device, against forward_dense;
  * the trunks in two launches (SMH_FUSION_TWO_LAUNCH=1) against one, on forward_from_x0_halves at 48 and 1024 patches.

    python tools/time_fusion.py [--rounds 5] [--reps 30] [--inference]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inference", action="store_true", help="the x0-halves / dense / one-launch rows instead of the B3_MTL comparison")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sm_hpss_mtl_amd.model import B3MTL, FusionMTL

    def timed(fn, reps):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def report(what, models, fns, reps):
        res = {k: [] for k in models}
        for _ in range(args.rounds):
            for k in models:
                res[k].append(timed(fns[k], reps))
        for k in models:
            v = np.array(res[k])
            print(json.dumps({"what": what, "model": k, "ms_median": round(float(np.median(v)), 4),
                              "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4)}), flush=True)

    if args.inference:
        return inference_rows(args, torch, FusionMTL, report)

    for W in (68, 249):
        models = {"B3_MTL": B3MTL(n_feat=240, patch_size=W, n_classes=3, TR_STEPS=100, seed=0),
                  "fusion": FusionMTL(n_feat=120, patch_size=W, n_classes=3, TR_STEPS=100, seed=0)}
        N = 1024
        x = torch.randn((N, W, 240), device="cuda")
        xs = [x[:, :, :120].contiguous(), x[:, :, 120:].contiguous()]
        out = {k: torch.empty((N, m.out_dim), device="cuda") for k, m in models.items()}
        inp = {"B3_MTL": x, "fusion": xs}
        report("forward f32, %d patches, W=%d" % (N, W), models,
               {k: (lambda m=m, o=out[k], i=inp[k]: m.forward_device(i, out=o)) for k, m in models.items()}, args.reps)
        for N in (48, 510):
            rng = np.random.default_rng(0)
            cls = rng.integers(0, 3, N)
            y = {"S": (cls == 1).astype(np.float32)[:, None], "M": (cls == 0).astype(np.float32)[:, None],
                 "R": rng.random((N, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[cls]}
            xt = {"B3_MTL": x[:N].contiguous(), "fusion": [a[:N].contiguous() for a in xs]}
            yt = {k: m.pack_targets(y) for k, m in models.items()}
            report("train step f32, %d patches, W=%d" % (N, W), models,
                   {k: (lambda m=m, t=yt[k], i=xt[k]: m.train_on_batch(i, t, sync=False)) for k, m in models.items()},
                   max(args.reps // 2, 10))
        for m in models.values():
            m.check_status()


def inference_rows(args, torch, FusionMTL, report):
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.synth import bench_clips
    W = 68
    m = FusionMTL(n_feat=120, patch_size=W, n_classes=3, TR_STEPS=100, seed=0)
    fe = Frontend(FrontendConfig())
    # 1024 one-second clips, one patch each: the front end's outputs, then the two ways to the logits
    B = 1024
    taps = fe.run(torch.from_numpy(bench_clips(B)).cuda(), taps=True)
    S, harm, perc = taps["S"], taps["harm"], taps["perc"]
    bufs = {}
    halves = [torch.empty((B, W, 120), device="cuda") for _ in range(2)]
    out = torch.empty((B, m.out_dim), device="cuda")

    def via_patches():
        r = bufs["p"] = fe.features(S, harm, perc, W, W, out=bufs.get("p"))
        halves[0].copy_(r["patches"][:, :, :120])
        halves[1].copy_(r["patches"][:, :, 120:])
        return m.forward_device(halves, out=out)

    def via_x0():
        r = bufs["x"] = fe.features_l0(S, harm, perc, 0, W, W, m, out=bufs.get("x"))
        return m.forward_from_x0_halves(r["x0p"], out=out)

    a, b = via_patches().clone(), via_x0().clone()
    print(json.dumps({"what": "x0 halves against patches, max |diff|", "value": float((a - b).abs().max())}), flush=True)
    report("features + forward, %d patches, W=%d" % (B, W), ["patches -> halves -> forward_device", "features_l0 -> forward_from_x0_halves"],
           {"patches -> halves -> forward_device": via_patches, "features_l0 -> forward_from_x0_halves": via_x0}, args.reps)

    # one 10 000-frame chunk at hop 1
    fv = torch.randn((240, 10000), device="cuda")

    def dense_patches():
        xs = [fe.extract_patches(fv[h * 120:(h + 1) * 120][None], W, 1, time_major=True) for h in range(2)]
        return m.forward_device(xs)

    a, b = dense_patches().clone(), m.forward_dense(fv, 1).clone()
    print(json.dumps({"what": "dense against patches, max |diff|", "value": float((a - b).abs().max()), "patches": int(a.shape[0])}), flush=True)
    report("file-level, 10000 frames, hop 1, W=%d" % W, ["extract_patches -> forward_device", "forward_dense"],
           {"extract_patches -> forward_device": dense_patches, "forward_dense": lambda: m.forward_dense(fv, 1)}, max(args.reps // 5, 5))

    # the trunks in one launch or two (the switch is read per call)
    for N in (48, 1024):
        x0p = torch.randn((N, 2, W, 32), device="cuda")
        o = torch.empty((N, m.out_dim), device="cuda")

        def run(two, x0p=x0p, o=o):
            if two:
                os.environ["SMH_FUSION_TWO_LAUNCH"] = "1"
            else:
                os.environ.pop("SMH_FUSION_TWO_LAUNCH", None)
            return m.forward_from_x0_halves(x0p, out=o)

        report("forward_from_x0_halves, %d patches, W=%d" % (N, W), ["two launches", "one launch"],
               {"two launches": lambda: run(True), "one launch": lambda: run(False)}, args.reps)
    os.environ.pop("SMH_FUSION_TWO_LAUNCH", None)
    m.check_status()


if __name__ == "__main__":
    main()
