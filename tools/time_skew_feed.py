"""GPU timing of the skewness-vector feed (PARAMS['skewness_vector'] = 'Row' / 'Col') on tools/time_ragged.py's workload -- B = 256
files of 1..10 s, LogMelHarmPercSpec at 120 mels (240 rows) -- at (W, shift) = (68, 68), the driver's test geometry, and (249, 24), its
training geometry, both modes:

    fused, resident fv   ONE smh_patch_statistics call over featuregrams that are on the device (a later epoch, served from the cache)
    fused feed           the ragged front-end call WITHOUT patches + that call (what the generators run)
    composition          what it replaces: the ragged call writing time-major standardised patches, .double(), smh_data_statistics_f64
                         (the patches (nP, W, 2F) read as (N, f = W, t = 2F): 'Row' is its axis 0, 'Col' its axis 1)

Float32 skewness vectors from the fused call, float64 from the composition (as lib.cython_impl.tools returns them).  Protocol of
tools/time_frame_scaling.py: warm-up calls, a host clock around K calls that ends in a device synchronise, the variants ALTERNATING over
several rounds; the median round and the spread are printed.

    python tools/time_skew_feed.py [B=256] [max seconds=10]"""
import os, sys, time
import ctypes as C
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import _lib
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig, _FAMILIES, _ptr, _stream

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
MAXS = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
K, ROUNDS = 10, 7
GEOMETRIES = [(68, 68), (249, 24)]
SKEW = 2
rng = np.random.default_rng(0)
lens = [int(rng.uniform(1.0, MAXS) * 16000) // 2 * 2 for _ in range(B)]  # tools/time_ragged.py's files
offs, o = [], 0
for n in lens:
    offs.append(o)
    o += (n + 3) // 4 * 4
audio = torch.rand(o, device="cuda") - 0.5
h_off, h_len = (C.c_longlong * B)(*offs), (C.c_int * B)(*lens)
print("%d files of 1-%.0f s (%.0f s of audio), LogMelHarmPercSpec, 120 mels; median of %d rounds of %d calls, the variants alternating"
      % (B, MAXS, sum(lens) / 16000.0, ROUNDS, K), flush=True)


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


fe = Frontend(FrontendConfig(n_fft=400, n_mels=120, log_db=True))
fam = _FAMILIES[True]
F = fam.row_mult * fe.rows
for W, SHIFT in GEOMETRIES:
    fv_off, p_off = (C.c_longlong * (B + 1))(), (C.c_longlong * (B + 1))()
    hT, hnP, work = (C.c_int * B)(), (C.c_int * B)(), C.c_size_t()
    _lib.check(getattr(fe.lib, fam.ragged_sizes)(fe._h, h_off, h_len, B, W, SHIFT, fv_off, p_off, hT, hnP, C.byref(work)))
    nP = int(p_off[B])
    fv = torch.empty(int(fv_off[B]), device="cuda")
    patches = torch.empty((nP, W, F), device="cuda")
    wk = torch.empty(work.value, dtype=torch.uint8, device="cuda")
    h_fv = (C.c_void_p * B)(*[fv.data_ptr() + 4 * int(fv_off[b]) for b in range(B)])
    assert fe.lib.smh_scaled_patches_count(hT, B, W, SHIFT, None) == nP
    print("W = %d, shift = %d: %d rows, %d frames, %d patches (%.0f MB as float32, %.0f MB as float64), featuregrams %.0f MB"
          % (W, SHIFT, F, sum(hT), nP, nP * F * W * 4 / 1e6, nP * F * W * 8 / 1e6, fv.numel() * 4 / 1e6), flush=True)

    def ragged(p):
        _lib.check(getattr(fe.lib, fam.ragged)(fe._h, _ptr(audio), h_off, h_len, B, W if p is not None else 0,
                                               SHIFT if p is not None else 0, 1, _ptr(fv), _ptr(p), _ptr(wk), wk.numel(), _stream()))

    ragged(None)
    torch.cuda.synchronize()
    for mode, axis in (("Row", 1), ("Col", 0)):
        width = F if axis == 1 else W
        out32 = torch.empty((nP, width), device="cuda")
        out64 = torch.empty((nP, width), dtype=torch.float64, device="cuda")
        need = int(fe.lib.smh_patch_statistics_workspace_bytes(B, F, axis, 0))
        ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device="cuda")

        def fused():
            _lib.check(fe.lib.smh_patch_statistics(fe._h, h_fv, hT, B, F, None, None, W, SHIFT, SKEW, axis, 1, _ptr(out32), _ptr(ws), need,
                                                   _stream()))

        def fused_feed():
            ragged(None)
            fused()

        def composition():
            ragged(patches)
            p64 = patches.double()
            _lib.check(fe.lib.smh_data_statistics_f64(_ptr(p64), nP, W, F, SKEW, 1 - axis, _ptr(out64), _stream()))

        fused()
        composition()
        torch.cuda.synchronize()
        d = float((out32.double() - out64).abs().max())
        # (the same statistic up to the float32 rounding of the result and the last bits of the ragged call's own standardisation)
        print("  %s (axis %d), (%d, %d) vectors; max |fused - composition| = %.2e" % (mode, axis, nP, width, d), flush=True)
        m = timed((("fused, resident fv", fused), ("fused feed", fused_feed), ("composition", composition)))
        print("    fused feed / composition = %.3f" % (m["fused feed"] / m["composition"]), flush=True)
        del out32, out64, ws
    del fv, patches, wk
