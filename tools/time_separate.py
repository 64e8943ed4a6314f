"""GPU timing of HPSS audio separation (`Frontend.separate` = smh_hpss_audio_f32: STFT -> medians -> the resynthesis kernel) on B
one-second clips against its first two stages alone (`stft_mag` + `hpss_median`, whose code this feature does not touch) on the same
machine, in the same run.  Protocol of tools/time_plain.py (warm-up calls, a host clock around K calls that ends in a device
synchronise), the two ALTERNATING over several rounds so that a drift of the machine hits both; the median round and the spread are
printed, and from their difference the resynthesis kernel's share and the HBM bandwidth its traffic model implies.

    python tools/time_separate.py [B=1024] [stft_precision=f32] [n_fft=400]

Ragged mode: `Frontend.separate_ragged` (smh_hpss_audio_ragged_f32: one launch per stage for all files) against `separate(list)` (one
call of three launches per distinct length) on the project's standard ragged workload, B files of 1-10 s drawn as tools/time_ragged.py
draws them (seed 0), resident on the device.  Same process, warm, ALTERNATING, the median of the rounds and the spread; the outputs of
both are compared bit for bit first.  Then the C entry alone on the packed buffer (no packing copies), and the three kernels' share of
the device time from torch's profiler.

    python tools/time_separate.py ragged [B=256] [stft_precision=f32] [n_fft=400]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import _lib
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig, _ptr, _stream
from sm_hpss_mtl_amd.synth import bench_clips



def ragged_mode(argv):
    import ctypes as C
    B = int(argv[0]) if len(argv) > 0 else 256
    prec = argv[1] if len(argv) > 1 else "f32"
    nfft = int(argv[2]) if len(argv) > 2 else 400
    fe = Frontend(FrontendConfig(n_fft=nfft, stft_precision=prec))
    rng = np.random.default_rng(0)
    lens = [int(rng.uniform(1.0, 10.0) * 16000) // 2 * 2 for _ in range(B)]
    offs, o = [], 0
    for n in lens:
        offs.append(o)
        o += (n + 3) // 4 * 4
    torch.manual_seed(0)
    audio = torch.rand(o, device="cuda") - 0.5
    sigs = [audio[of:of + n] for of, n in zip(offs, lens)]
    out = {"harmonic": torch.empty(o, device="cuda"), "percussive": torch.empty(o, device="cuda")}
    h_off, h_len = (C.c_longlong * B)(*offs), (C.c_int * B)(*lens)
    work, route = C.c_size_t(), (C.c_int * B)()
    _lib.check(fe.lib.smh_hpss_audio_ragged_sizes(fe._h, h_off, h_len, B, None, C.byref(work)), "smh_hpss_audio_ragged_sizes")
    _lib.check(fe.lib.smh_internal_hpss_audio_ragged_route(fe._h, _ptr(audio), h_off, h_len, B, route), "route")
    wk = torch.empty(work.value, dtype=torch.uint8, device="cuda")

    def entry():  # the C entry on the packed buffer
        _lib.check(fe.lib.smh_hpss_audio_ragged_f32(fe._h, _ptr(audio), h_off, h_len, B, _ptr(out["harmonic"]), _ptr(out["percussive"]),
                                                    _ptr(wk), wk.numel(), _stream()), "smh_hpss_audio_ragged_f32")

    calls = {"separate_ragged": lambda: fe.separate_ragged(sigs, out=out), "separate(list)": lambda: fe.separate(sigs),
             "C entry": entry}
    a, b = fe.separate_ragged(sigs), fe.separate(sigs)
    same = all(torch.equal(a[c][i], b[c][i]) for c in ("harmonic", "percussive") for i in range(B))
    secs = sum(lens) / 16000.0
    print("ragged workload (%s STFT, n_fft %d): %d files of 1-10 s, %.0f s of audio, %d distinct lengths, %d files on the ragged kernels, "
          "workspace %.1f MB; separate_ragged == separate(list) bit for bit: %s" % (
              prec, nfft, B, secs, len(set(lens)), sum(1 for r in route if r == 0), work.value / 1e6, same), flush=True)
    for fn in calls.values():
        fn(), fn()
    torch.cuda.synchronize()
    K, ROUNDS = 5, 7
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for which, fn in calls.items():
            t0 = time.perf_counter()
            for _ in range(K):
                fn()
            torch.cuda.synchronize()
            ms[which].append((time.perf_counter() - t0) / K * 1e3)
    med = {}
    for which in calls:
        v = sorted(ms[which])
        med[which] = v[len(v) // 2]
        print("%-15s: median %.3f ms per call (min %.3f, max %.3f over %d rounds of %d calls) = %.0f files/s = %.0f s of audio per second"
              % (which, med[which], v[0], v[-1], ROUNDS, K, B / med[which] * 1e3, secs / med[which] * 1e3), flush=True)
    print("separate_ragged / separate(list) = %.3f (%.1f times faster)" % (med["separate_ragged"] / med["separate(list)"],
                                                                            med["separate(list)"] / med["separate_ragged"]), flush=True)
    try:  # the three kernels' share of the C entry's device time
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                entry()
            torch.cuda.synchronize()
        us = {"stft": 0.0, "median": 0.0, "resynth": 0.0, "other": 0.0}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            t = getattr(e, "cuda_time_total", 0.0) if t is None else t
            us[next((k for k in ("stft", "median", "resynth") if k in e.key), "other")] += t / 3
        tot = sum(us.values())
        if tot <= 0:
            raise RuntimeError("no device times")
        print("kernels of one C entry call (profiler, mean of 3): " + ", ".join(
            "%s %.1f us = %.1f %%" % (k, v, 100 * v / tot) for k, v in us.items()), flush=True)
    except Exception as e:  # no kernel tracing here: named as not measured
        print("kernels' share: not measured (%s: %s)" % (type(e).__name__, e), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "ragged":
    ragged_mode(sys.argv[2:])
    sys.exit(0)
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
