"""GPU timing of the plain front end (smh_plain_frontend_f32: Spec / LogSpec / MelSpec / LogMelSpec of lib/preprocessing.py:378-402)
against the harmonic-percussive one (smh_frontend_f32, whose code this feature does not touch) on the same machine, in the same run:
B one-second clips through `Frontend.run(W=68, shift=68)` -- featuregram + standardised time-major patches.  Protocol of
tools/time_ragged.py (warm-up calls, a host clock around K calls that ends in a device synchronise), with the two front ends
ALTERNATING over several rounds so that a drift of the machine hits both; the median round and the spread are printed.

    python tools/time_plain.py [B=1024] [featName=LogMelSpec] [stft_precision=f32]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
from sm_hpss_mtl_amd.synth import bench_clips

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
NAME = sys.argv[2] if len(sys.argv) > 2 else "LogMelSpec"
PREC = sys.argv[3] if len(sys.argv) > 3 else "f32"
PARAMS = {"Model": "m", "Tw": 25, "Ts": 10, "stft_precision": PREC, "l_harm": {"m": 21}, "l_perc": {"m": 11}}
plain = Frontend(FrontendConfig.from_params(PARAMS, 400, 120, NAME))
hpss = Frontend(FrontendConfig.from_params(PARAMS, 400, 120, "LogMelHarmPercSpec"))
audio = torch.from_numpy(bench_clips(B)).cuda()  # the benchmark's batch: B distinct clips
outs = {"plain": {}, "hpss": {}}
fes = {"plain": plain, "hpss": hpss}


def call(which):
    res = fes[which].run(audio, W=68, shift=68, out=outs[which])
    outs[which].update(fv=res["fv"], patches=res["patches"])


for _ in range(3):
    call("plain"), call("hpss")
torch.cuda.synchronize()
K, ROUNDS = 50, 7
ms = {"plain": [], "hpss": []}
for _ in range(ROUNDS):
    for which in ("plain", "hpss"):
        t0 = time.perf_counter()
        for _ in range(K):
            call(which)
        torch.cuda.synchronize()
        ms[which].append((time.perf_counter() - t0) / K * 1e3)
T = plain.num_frames(16000)
for which in ("plain", "hpss"):
    v = sorted(ms[which])
    print("%-5s %s (%s STFT): %d clips of 1 s, %d frames: median %.3f ms per call (min %.3f, max %.3f over %d rounds of %d calls) = "
          "%.0f clips/s" % (which, NAME if which == "plain" else "LogMelHarmPercSpec", PREC, B, T, v[len(v) // 2], v[0], v[-1], ROUNDS, K,
                            B / v[len(v) // 2] * 1e3), flush=True)
mp, mh = sorted(ms["plain"])[ROUNDS // 2], sorted(ms["hpss"])[ROUNDS // 2]
# the bytes the plain path's two kernels and the STFT must move per clip (f32): audio in, S out + in, fv out, fv in twice + out
# (dB features), patches out
K_, rows, nP = plain.K, plain.rows, plain.num_patches(T, 68, 68)
byts = 4 * (16000 + 2 * K_ * T + rows * T * (4 if plain.cfg.log_db else 3) + nP * 68 * rows)
print("plain / hpss = %.3f; plain path moves %.0f KB per clip -> %.0f GB/s end to end" % (mp / mh, byts / 1e3, byts * B / mp / 1e6), flush=True)
