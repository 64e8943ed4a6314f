"""GPU timing of the late-fusion ensemble (late_fusion.LateFusion) on one device, W = 68, two B3_MTL models of n_feat = 120.

  * forward on patches at N = 48, 256, 1024:
      (a) paired      LateFusion.forward_device, both models in one launch + the blend kernel
      (b) two-launch  the same under SMH_LATE_FUSION_TWO_LAUNCH=1
      (c) baseline    what a user has without the ensemble: two forward_device calls, then the blend and argmax in torch on the device
  * features + forward from the layer-0 partials against two separate HotPath steps (one per model, the emulation: the front end
    runs once per model), 1024 one-second clips;
  * file-level: one 10 000-frame chunk at hop 1, forward_dense against extract_patches per half + forward_device.
The variants of a row are timed in alternating rounds on the same warm device; each line reports the median and the range over the
rounds.  Variant (b)'s environment switch is set once per round, outside the timed calls (the library reads it per call), so the
three variants carry the same host work.  A timing tool: it asserts nothing.

    python tools/time_late_fusion.py [--rounds 7] [--reps 300]
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
    ap.add_argument("--reps", type=int, default=300)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    from sm_hpss_mtl_amd.late_fusion import LateFusion
    from sm_hpss_mtl_amd.model import B3MTL
    from sm_hpss_mtl_amd.pipeline import HotPath
    from sm_hpss_mtl_amd.synth import bench_clips

    def timed(fn, reps, env=None):
        os.environ.update(env or {})
        try:
            return timed_calls(fn, reps)
        finally:
            for k in env or {}:
                os.environ.pop(k, None)

    def timed_calls(fn, reps):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def report(what, fns, reps, env=None):
        """fns: variant name -> callable; env: variant name -> environment of that variant's rounds."""
        res = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k in fns:
                res[k].append(timed(fns[k], reps, (env or {}).get(k)))
        for k in fns:
            v = np.array(res[k]) * 1000.0
            print(json.dumps({"what": what, "variant": k, "us_median": round(float(np.median(v)), 1),
                              "us_min": round(float(v.min()), 1), "us_max": round(float(v.max()), 1)}), flush=True)

    W, F = 68, 120
    mH, mP = (B3MTL(n_feat=F, patch_size=W, n_classes=3, TR_STEPS=100, seed=s) for s in (0, 1))
    ens = LateFusion(mH, mP, alpha=0.5)

    for N in (48, 256, 1024):
        xH, xP = (torch.randn((N, W, F), device="cuda") for _ in range(2))
        pred = torch.empty((N, 3), device="cuda")
        labels = torch.empty((N,), dtype=torch.int32, device="cuda")
        oH, oP = (torch.empty((N, mH.out_dim), device="cuda") for _ in range(2))

        def paired(xH=xH, xP=xP, pred=pred, labels=labels):
            return ens.forward_device([xH, xP], out=pred, labels=labels)

        def baseline(xH=xH, xP=xP, oH=oH, oP=oP):
            mH.forward_device(xH, out=oH)
            mP.forward_device(xP, out=oP)
            p = 0.5 * oH[:, -3:] + 0.5 * oP[:, -3:]
            return p, p.argmax(1)

        a, b = paired().clone(), baseline()[0]
        print(json.dumps({"what": "paired against baseline, N=%d, max |diff|" % N, "value": float((a - b).abs().max())}), flush=True)
        report("forward on patches, N=%d, W=%d" % (N, W),
               {"(a) paired": paired, "(b) two-launch": paired, "(c) two forward_device + torch blend": baseline}, args.reps,
               env={"(b) two-launch": {"SMH_LATE_FUSION_TWO_LAUNCH": "1"}})

    # features + forward: the ensemble from the layer-0 partials against one HotPath step per model
    B = 1024
    fe = Frontend(FrontendConfig())
    audio = torch.from_numpy(bench_clips(B)).cuda()
    hp_ens = HotPath(fe, ens, batch=B, n_samples=audio.shape[1], patch=W)
    # the emulation: each model alone reads ITS half, so a user runs the front end once per model, cuts the half out of the
    # featuregram and builds its patches (standardised per clip, as get_feature_patches does)
    hp_plain = HotPath(fe, None, batch=B, n_samples=audio.shape[1], patch=W)
    nP = fe.num_patches(hp_plain.T, W, W)

    def emulation():
        outs = []
        for i, m in enumerate((mH, mP)):
            fv = hp_plain.step(audio)  # STFT, medians, featuregram (B, 2F, T): once per model
            half = fe.standardize_rows(fv[:, i * F:(i + 1) * F].contiguous())
            outs.append(m.forward_device(fe.extract_patches(half, W, W, time_major=True)))
        p = 0.5 * outs[0][:, -3:] + 0.5 * outs[1][:, -3:]
        return p, p.argmax(1)

    a, b = hp_ens.step(audio).clone(), emulation()[0]
    print(json.dumps({"what": "HotPath(ensemble) against the per-model emulation, max |diff|", "value": float((a - b).abs().max()),
                      "patches": int(B * nP)}), flush=True)
    report("audio -> blended 3C, %d clips, W=%d" % (B, W),
           {"HotPath(ensemble, fuse_l0)": lambda: hp_ens.step(audio), "front end + forward_device per model + torch blend": emulation},
           max(args.reps // 5, 5))

    # one 10 000-frame chunk at hop 1
    fv = torch.randn((2 * F, 10000), device="cuda")

    def dense_patches():
        xs = [fe.extract_patches(fv[h * F:(h + 1) * F][None], W, 1, time_major=True) for h in range(2)]
        return ens.forward_device(xs)

    a, b = dense_patches().clone(), ens.forward_dense(fv, 1).clone()
    print(json.dumps({"what": "dense against patches, max |diff|", "value": float((a - b).abs().max()), "patches": int(a.shape[0])}), flush=True)
    report("file-level, 10000 frames, hop 1, W=%d" % W,
           {"extract_patches -> forward_device": dense_patches, "forward_dense": lambda: ens.forward_dense(fv, 1)}, max(args.reps // 5, 5))
    ens.check_status()


if __name__ == "__main__":
    main()
