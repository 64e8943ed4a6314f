"""GPU timing of the Conv2D models' feed: the ragged front end writing IMAGE patches (smh_frontend_ragged_layout_f32, patch_layout 0:
(nP, 2*rows, W), what Doukhan_et_al_MTL / Papakostas_et_al_MTL / Jang_et_al_MTL read) against the two alternatives on the same
machine, in the same run:

    image          the ragged call with patch_layout 0
    time-major     the ragged call with patch_layout 1 (the TCN's layout; what smh_frontend_ragged_f32 runs)
    tm + permute   the time-major call followed by patches.permute(0, 2, 1).contiguous(): the only device-side way to the image
                   layout without patch_layout 0

The workload of tools/time_ragged.py -- B = 256 files of 1..10 s, W = 68, the driver's shift 68 -- for the three feature
configurations of Proposed_Work_Results.py:754-756, 794-796: MelHarmPercSpec at 120 mels (240 rows), HarmPercSpec at n_fft = 400
(402 rows), LogHarmPercSpec at n_fft = 512 (514 rows).  Protocol of tools/time_plain.py: warm-up calls, a host clock around K calls
that ends in a device synchronise, the three variants ALTERNATING over several rounds; the median round and the spread are printed.

    python tools/time_cnn_feed.py [B=256] [max seconds=10]"""
import os, sys, time
import ctypes as C
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import _lib
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig, _ptr, _stream

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
MAXS = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
W = SHIFT = 68
K, ROUNDS = 10, 7
CONFIGS = [("Doukhan_et_al_MTL    MelHarmPercSpec, 120 mels", FrontendConfig(n_fft=400, n_mels=120, log_db=False)),
           ("Papakostas_et_al_MTL HarmPercSpec, n_fft 400  ", FrontendConfig(n_fft=400, n_mels=0, log_db=False)),
           ("Jang_et_al_MTL       LogHarmPercSpec, n_fft 512", FrontendConfig(n_fft=512, n_mels=0, log_db=True))]
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
for name, cfg in CONFIGS:
    fe = Frontend(cfg)
    F = 2 * fe.rows
    fv_off, p_off = (C.c_longlong * (B + 1))(), (C.c_longlong * (B + 1))()
    hT, hnP, work = (C.c_int * B)(), (C.c_int * B)(), C.c_size_t()
    _lib.check(fe.lib.smh_frontend_ragged_sizes(fe._h, h_off, h_len, B, W, SHIFT, fv_off, p_off, hT, hnP, C.byref(work)))
    nP = int(p_off[B])
    fv = torch.empty(int(fv_off[B]), device="cuda")
    p_img = torch.empty((nP, F, W), device="cuda")
    p_tm = torch.empty((nP, W, F), device="cuda")
    wk = torch.empty(work.value, dtype=torch.uint8, device="cuda")

    def ragged(layout, patches):
        _lib.check(fe.lib.smh_frontend_ragged_layout_f32(fe._h, _ptr(audio), h_off, h_len, B, W, SHIFT, layout, _ptr(fv), _ptr(patches),
                                                         _ptr(wk), wk.numel(), _stream()))

    def tm_permute():
        ragged(1, p_tm)
        return p_tm.permute(0, 2, 1).contiguous()

    variants = (("image", lambda: ragged(0, p_img)), ("time-major", lambda: ragged(1, p_tm)), ("tm + permute", tm_permute))
    for _ in range(3):
        for _, f in variants:
            f()
    torch.cuda.synchronize()
    assert torch.equal(p_img, tm_permute())  # the three variants time the same result
    ms = {k: [] for k, _ in variants}
    for _ in range(ROUNDS):
        for k, f in variants:
            t0 = time.perf_counter()
            for _ in range(K):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / K * 1e3)
    med = {k: sorted(v)[ROUNDS // 2] for k, v in ms.items()}
    print("%s  %d rows, %d frames, %d patches (%.0f MB)" % (name, F, sum(hT), nP, nP * F * W * 4 / 1e6), flush=True)
    for k, _ in variants:
        v = sorted(ms[k])
        print("    %-13s median %.3f ms per call (min %.3f, max %.3f) = %.0f s of audio per second"
              % (k, med[k], v[0], v[-1], sum(lens) / 16000.0 / med[k] * 1e3), flush=True)
    print("    image / time-major = %.3f; image / (tm + permute) = %.3f" % (med["image"] / med["time-major"], med["image"] / med["tm + permute"]),
          flush=True)
    del fe, fv, p_img, p_tm, wk
