"""GPU timing of the intermediate-fusion model next to B3_MTL at the same shapes: the f32 forward at 1024 patches and the f32
training step (forward-train, fused BN, heads, backward of both trunks, SGD) at 48 and 510 patches, W = 68 and 249.  B3_MTL reads the
240-wide H||P patches, the fusion model the two 120-wide halves.  The two models are timed in alternating rounds on the same warm
device; each line reports the median and range over the rounds.

    python tools/time_fusion.py [--rounds 5] [--reps 30]
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


if __name__ == "__main__":
    main()
