"""GPU timing of frame-level scaling (PARAMS['frame_level_scaling']) on tools/time_ragged.py's workload -- B = 256 files of 1..10 s,
W = 68, the driver's shift 68 -- two questions in one run:

1.  the scaled ragged feed against the standardised one, per feature configuration:
        standardised   the ragged front-end call writing StandardScaler patches (what the generators run with the switch off)
        scaled         the same call WITHOUT patches + smh_scaled_patches_f32 over its featuregrams (the switch on): no per-clip row
                       statistics, one more read of the featuregram
        scaled, cached fv   smh_scaled_patches_f32 alone: a later epoch, the featuregrams served from the device cache
2.  smh_row_moments_f64 over the same featuregrams (get_data_stats' device work, per file) against two plain reads of the
    featuregram buffer (torch.sum twice): the floor of any two-pass statistic.

Configurations: LogMelSpec at 21 mels (21 rows), LogSpec at n_fft = 400 (201 rows; the baselines' other plain shape) and
LogMelHarmPercSpec at 120 mels (240 rows).  Protocol of tools/time_cnn_feed.py: warm-up calls, a host clock around K calls that ends in
a device synchronise, the variants ALTERNATING over several rounds; the median round and the spread are printed.

    python tools/time_frame_scaling.py [B=256] [max seconds=10]"""
import os, sys, time
import ctypes as C
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import _lib
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig, _FAMILIES, _ptr, _stream

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
MAXS = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
W = SHIFT = 68
K, ROUNDS = 10, 7
CONFIGS = [("LogMelSpec, 21 mels             ", FrontendConfig(n_fft=400, n_mels=21, log_db=True, mel_sr=16000.0, hpss=False)),
           ("LogSpec, n_fft 400              ", FrontendConfig(n_fft=400, n_mels=0, log_db=True, mel_sr=16000.0, hpss=False)),
           ("LogMelHarmPercSpec, 120 mels    ", FrontendConfig(n_fft=400, n_mels=120, log_db=True))]
rng = np.random.default_rng(0)
lens = [int(rng.uniform(1.0, MAXS) * 16000) // 2 * 2 for _ in range(B)]  # tools/time_ragged.py's files
offs, o = [], 0
for n in lens:
    offs.append(o)
    o += (n + 3) // 4 * 4
audio = torch.rand(o, device="cuda") - 0.5
h_off, h_len = (C.c_longlong * B)(*offs), (C.c_int * B)(*lens)
print("%d files of 1-%.0f s (%.0f s of audio), W = %d, shift = %d; median of %d rounds of %d calls, the variants alternating"
      % (B, MAXS, sum(lens) / 16000.0, W, SHIFT, ROUNDS, K), flush=True)


def timed(variants):
    for _ in range(3):
        for _, f in variants:
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in variants}
    for _ in range(ROUNDS):
        for k, f in variants:
            t0 = time.perf_counter()
            for _ in range(K):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / K * 1e3)
    for k, _ in variants:
        v = sorted(ms[k])
        print("    %-22s median %.3f ms per call (min %.3f, max %.3f) = %.2f us per file" % (k, v[ROUNDS // 2], v[0], v[-1], v[ROUNDS // 2] / B * 1e3),
              flush=True)
    return {k: sorted(v)[ROUNDS // 2] for k, v in ms.items()}


for name, cfg in CONFIGS:
    fe = Frontend(cfg)
    fam = _FAMILIES[bool(cfg.hpss)]
    F = fam.row_mult * fe.rows
    fv_off, p_off = (C.c_longlong * (B + 1))(), (C.c_longlong * (B + 1))()
    hT, hnP, work = (C.c_int * B)(), (C.c_int * B)(), C.c_size_t()
    _lib.check(getattr(fe.lib, fam.ragged_sizes)(fe._h, h_off, h_len, B, W, SHIFT, fv_off, p_off, hT, hnP, C.byref(work)))
    nP = int(p_off[B])
    fv = torch.empty(int(fv_off[B]), device="cuda")
    p_std, p_scl = torch.empty((nP, W, F), device="cuda"), torch.empty((nP, W, F), device="cuda")
    wk = torch.empty(work.value, dtype=torch.uint8, device="cuda")
    h_fv = (C.c_void_p * B)(*[fv.data_ptr() + 4 * int(fv_off[b]) for b in range(B)])
    assert fe.lib.smh_scaled_patches_count(hT, B, W, SHIFT, None) == nP
    mom = torch.empty((B, F, 2), dtype=torch.float64, device="cuda")
    bad = torch.empty((B, F), dtype=torch.int32, device="cuda")

    def ragged(patches):
        _lib.check(getattr(fe.lib, fam.ragged)(fe._h, _ptr(audio), h_off, h_len, B, W if patches is not None else 0,
                                               SHIFT if patches is not None else 0, 1, _ptr(fv), _ptr(patches), _ptr(wk), wk.numel(), _stream()))

    def moments():
        _lib.check(fe.lib.smh_row_moments_f64(fe._h, h_fv, hT, B, F, _ptr(mom), _ptr(bad), _stream()))

    ragged(None)
    moments()
    torch.cuda.synchronize()
    # plausible statistics of the fold: the pooled row means and deviations of these files
    T_all = torch.tensor([int(t) for t in hT], dtype=torch.float64, device="cuda")
    mean = (mom[..., 0].sum(0) / T_all.sum()).contiguous()
    stdev = torch.sqrt((mom[..., 1] + T_all[:, None] * (mom[..., 0] / T_all[:, None] - mean) ** 2).sum(0) / (T_all.sum() - 1)).contiguous()
    assert int(bad.sum()) == 0 and bool(torch.isfinite(stdev).all())

    def scaled():
        _lib.check(fe.lib.smh_scaled_patches_f32(fe._h, h_fv, hT, B, F, _ptr(mean), _ptr(stdev), W, SHIFT, 1, _ptr(p_scl), _stream()))

    def scaled_feed():
        ragged(None)
        scaled()

    def two_reads():
        return fv.sum(), fv.sum()

    print("%s %d rows, %d frames, %d patches (%.0f MB), featuregrams %.0f MB" % (name, F, sum(hT), nP, nP * F * W * 4 / 1e6, fv.numel() * 4 / 1e6),
          flush=True)
    m = timed((("standardised feed", lambda: ragged(p_std)), ("scaled feed", scaled_feed), ("scaled, cached fv", scaled)))
    print("    scaled feed / standardised feed = %.3f" % (m["scaled feed"] / m["standardised feed"]), flush=True)
    m = timed((("row moments", moments), ("two reads (torch.sum)", two_reads)))
    print("    row moments / two reads = %.3f" % (m["row moments"] / m["two reads (torch.sum)"]), flush=True)
    del fe, fv, p_std, p_scl, wk, mom, bad
