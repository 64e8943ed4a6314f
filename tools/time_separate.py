"""GPU timing of HPSS audio separation (`Frontend.separate` = smh_hpss_audio_f32: STFT -> medians -> the resynthesis kernel) on B
one-second clips against its first two stages alone (`stft_mag` + `hpss_median`, whose code this feature does not touch) on the same
machine, in the same run.  Protocol of tools/time_plain.py (warm-up calls, a host clock around K calls that ends in a device
synchronise), the two ALTERNATING over several rounds so that a drift of the machine hits both; the median round and the spread are
printed, and from their difference the resynthesis kernel's share and the HBM bandwidth its traffic model implies.

    python tools/time_separate.py [B=1024] [stft_precision=f32] [n_fft=400]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import _lib
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig, _ptr, _stream
from sm_hpss_mtl_amd.synth import bench_clips

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
PREC = sys.argv[2] if len(sys.argv) > 2 else "f32"
NFFT = int(sys.argv[3]) if len(sys.argv) > 3 else 400
fe = Frontend(FrontendConfig(n_fft=NFFT, stft_precision=PREC))
audio = torch.from_numpy(bench_clips(B)).cuda()  # the benchmark's batch: B distinct clips
N = audio.shape[1]
T = fe.num_frames(N)
out = {"harmonic": torch.empty_like(audio), "percussive": torch.empty_like(audio)}
S, harm, perc = (torch.empty((B, fe.K, T), dtype=torch.float32, device=audio.device) for _ in range(3))


def separate():
    fe.separate(audio, out=out)


def stages():  # the same two launches into preallocated tensors, as smh_hpss_audio_f32 issues them into its workspace
    _lib.check(fe.lib.smh_stft_mag_f32(fe._h, _ptr(audio), B, N, _ptr(S), _stream()), "smh_stft_mag_f32")
    _lib.check(fe.lib.smh_hpss_median_f32(fe._h, _ptr(S), B, fe.K, T, fe.cfg.l_harm, fe.cfg.l_perc, _ptr(harm), _ptr(perc), _stream()),
               "smh_hpss_median_f32")


calls = {"separate": separate, "stft+median": stages}
for _ in range(3):
    separate(), stages()
torch.cuda.synchronize()
K, ROUNDS = 50, 7
ms = {k: [] for k in calls}
for _ in range(ROUNDS):
    for which, fn in calls.items():
        t0 = time.perf_counter()
        for _ in range(K):
            fn()
        torch.cuda.synchronize()
        ms[which].append((time.perf_counter() - t0) / K * 1e3)
for which in calls:
    v = sorted(ms[which])
    print("%-11s (%s STFT, n_fft %d): %d clips of %d samples, %d frames: median %.3f ms per call (min %.3f, max %.3f over %d rounds of "
          "%d calls) = %.0f clips/s" % (which, PREC, NFFT, B, N, T, v[len(v) // 2], v[0], v[-1], ROUNDS, K, B / v[len(v) // 2] * 1e3),
          flush=True)
full, part = sorted(ms["separate"])[ROUNDS // 2], sorted(ms["stft+median"])[ROUNDS // 2]
kern = full - part
# the bytes the resynthesis kernel must move per clip (f32): audio in, harm and perc in, y_harm and y_perc out
byts = 4 * (N + 2 * fe.K * T + 2 * N)
print("resynthesis kernel (difference of the medians): %.3f ms = %.1f %% of separate; traffic model %.0f KB per clip -> %.0f GB/s "
      "= %.1f %% of 8 TB/s" % (kern, 100 * kern / full, byts / 1e3, byts * B / kern / 1e6, 100 * byts * B / kern / 1e6 / 8000), flush=True)
