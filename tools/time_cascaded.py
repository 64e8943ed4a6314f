"""GPU timing of the cascaded-MTL model next to B3_MTL at the same shapes: the f32 forward (1024 patches, W = 68, n_feat 240 and
120) and the f32 training step (510 patches: forward-train, heads, backward, SGD).  The two models are timed in alternating rounds
on the same warm device; each line reports the median and range over the rounds.

    python tools/time_cascaded.py [--rounds 7] [--reps 50]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sm_hpss_mtl_amd.model import B3MTL, CascadedMTL

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

    for F in (240, 120):
        models = {"B3_MTL": B3MTL(n_feat=F, patch_size=68, n_classes=3, seed=0),
                  "cascaded": CascadedMTL(n_feat=F, patch_size=68, n_classes=3, seed=0)}
        x = torch.randn((1024, 68, F), device="cuda")
        out = {k: torch.empty((1024, m.out_dim), device="cuda") for k, m in models.items()}
        report("forward f32, 1024 patches, W=68, n_feat=%d" % F, models,
               {k: (lambda m=m, o=out[k]: m.forward_device(x, out=o)) for k, m in models.items()}, args.reps)
        for m in models.values():
            m.check_status()
    N = 510
    models = {"B3_MTL": B3MTL(n_feat=240, patch_size=68, n_classes=3, TR_STEPS=100, seed=0),
              "cascaded": CascadedMTL(n_feat=240, patch_size=68, n_classes=3, TR_STEPS=100, seed=0)}
    x = torch.randn((N, 68, 240), device="cuda")
    rng = np.random.default_rng(0)
    cls = rng.integers(0, 3, N)
    y = {"S": (cls == 1).astype(np.float32)[:, None], "M": (cls == 0).astype(np.float32)[:, None],
         "R": rng.random((N, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[cls]}
    yt = {k: m.pack_targets(y) for k, m in models.items()}
    report("train step f32, 510 patches, W=68, n_feat=240", models,
           {k: (lambda m=m, t=yt[k]: m.train_on_batch(x, t, sync=False)) for k, m in models.items()}, max(args.reps // 2, 10))
    for m in models.values():
        m.check_status()


if __name__ == "__main__":
    main()
