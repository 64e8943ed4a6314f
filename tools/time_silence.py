"""GPU timing of the signal-conditioning stage (normalise -> rms -> removeSilence -> normalise) on the bench batch.
Prints one JSON line: ms per pass, clips/s, algorithmic GB/s (read x + write out = 8 bytes per sample) for
  preprocess_signal            the route the library takes at (B, N): the clip-in-LDS kernel at the default N = 16000
  preprocess_signal_multipass  the same batch with SMH_SILENCE_MULTIPASS set: the multi-pass kernels
  preprocess_signal_long       N_LONG = 48000 samples, beyond the LDS route: the multi-pass kernels as callers reach them
  normalize, rms, mix_signals  the stand-alone entries (mix_signals: music of N // 3 + 1 samples, looped)
Environment: B, N, N_LONG, K (timed calls per row).  SMH_LIBSMH_PATH chooses the library, so two builds can be timed alternately."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import silence as sil

B, N = int(os.environ.get("B", 1024)), int(os.environ.get("N", 16000))
N_LONG, K = int(os.environ.get("N_LONG", 48000)), int(os.environ.get("K", 20))


def batch(n):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((B, n)).astype(np.float32)
    x[0::2, n // 8: n // 8 + 3000] *= 1e-4
    x[0::2, n // 2: n // 2 + 3000] *= 1e-4
    return torch.from_numpy(x).cuda()


def multipass(fn):
    def run():
        os.environ["SMH_SILENCE_MULTIPASS"] = "1"  # read by the library on every call
        try:
            return fn()
        finally:
            del os.environ["SMH_SILENCE_MULTIPASS"]
    return run


os.environ.pop("SMH_SILENCE_MULTIPASS", None)
d, d_long = batch(N), batch(N_LONG)
music = d[:, :N // 3 + 1].contiguous()
res = {}
for name, n, fn in (("preprocess_signal", N, lambda: sil.preprocess_signal(d, 16000, 25, 10)),
                    ("preprocess_signal_multipass", N, multipass(lambda: sil.preprocess_signal(d, 16000, 25, 10))),
                    ("preprocess_signal_long", N_LONG, lambda: sil.preprocess_signal(d_long, 16000, 25, 10)),
                    ("normalize", N, lambda: sil.normalize(d)),
                    ("rms", N, lambda: sil.rms(d, 400, 160)),
                    ("mix_signals", N, lambda: sil.mix_signals(d, music, 5.0))):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / K
    res[name] = {"N": n, "ms": round(ms, 4), "clips_per_s": round(B / ms * 1e3), "algo_GBps": round(8.0 * B * n / ms / 1e6, 1)}
print(json.dumps({"B": B, "N": N, **res}), flush=True)
