"""GPU timing of the single-task Lemaire TCN baseline (get_Lemaire_model) next to B3_MTL at the same shapes in the same run:

  * the f32 forward at 48 / 256 / 1024 patches, W = 68, F = 80;
  * the f32 training step at 510 patches (forward-train, head, backward, SGD);
  * LogMelSpec front end + patches + forward for 1024 one-second clips (the single-task model alone: B3_MTL does not read LogMelSpec).

The two models are timed in alternating rounds on the same warm device; each line reports the median and range over the rounds.  The
yardstick is B3_MTL's own line: the single-task model does strictly less work behind the trunk, so a forward or step slower than
B3_MTL's by more than the spread of B3_MTL's rounds is a defect.

    python tools/time_single_task.py [--rounds 7] [--reps 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, F = 68, 80


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.model import B3MTL, SingleTaskTCN

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

    def report(what, fns, reps):
        res = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k in fns:
                res[k].append(timed(fns[k], reps))
        for k in fns:
            v = np.array(res[k])
            print(json.dumps({"what": what, "model": k, "ms_median": round(float(np.median(v)), 4),
                              "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4)}), flush=True)

    models = {"B3_MTL": B3MTL(n_feat=F, patch_size=W, n_classes=3, TR_STEPS=100, seed=0),
              "single_task": SingleTaskTCN(n_feat=F, patch_size=W, n_classes=2, TR_STEPS=100, seed=0)}
    for N in (48, 256, 1024):
        x = torch.randn((N, W, F), device="cuda")
        out = {k: torch.empty((N, m.out_dim), device="cuda") for k, m in models.items()}
        report("forward f32, %d patches, W=%d, n_feat=%d" % (N, W, F),
               {k: (lambda m=m, o=out[k]: m.forward_device(x, out=o)) for k, m in models.items()}, args.reps)
    N = 510
    x = torch.randn((N, W, F), device="cuda")
    rng = np.random.default_rng(0)
    cls = rng.integers(0, 3, N)
    y = {"B3_MTL": {"S": (cls == 1).astype(np.float32)[:, None], "M": (cls == 0).astype(np.float32)[:, None],
                    "R": rng.random((N, 2)).astype(np.float32), "3C": np.eye(3, dtype=np.float32)[cls]},
         "single_task": np.eye(2, dtype=np.float32)[cls % 2]}
    yt = {k: m.pack_targets(y[k]) for k, m in models.items()}
    report("train step f32, %d patches, W=%d, n_feat=%d" % (N, W, F),
           {k: (lambda m=m, t=yt[k]: m.train_on_batch(x, t, sync=False)) for k, m in models.items()}, max(args.reps // 2, 10))
    fe = Frontend(FrontendConfig.from_params({"Model": "Lemaire_et_al", "Tw": 25, "Ts": 10}, 400, F, "LogMelSpec"))
    audio = torch.randn((1024, 16000), device="cuda") * 0.1
    m = models["single_task"]

    def end_to_end():
        patches = fe.run(audio, W=W, shift=W)["patches"]
        return m.forward_device(patches)
    report("LogMelSpec front end + patches + forward, 1024 one-second clips", {"single_task": end_to_end}, max(args.reps // 5, 5))
    for mm in models.values():
        mm.check_status()


if __name__ == "__main__":
    main()
