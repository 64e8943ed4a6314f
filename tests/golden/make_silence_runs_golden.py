"""Generate tests/golden/silence_runs_golden.npz (run in the BUILD container: python tests/golden/make_silence_runs_golden.py).

The crafted-energy cases of tests/silence_cases.py through the reference's own lib/cython_impl/tools.pyx compiled unmodified
(oracle/_ref/tools*.so, `tools.medfilt` rebound as in make_silence_golden.py).  Signals and energies are re-creatable from the
case table; only checksums of them are stored.  Per case: the frame marker (int8), the packed sample marker, the sha256 of the
output and [N, kept, untouched, totalSilDuration].  oracle/silence.py must agree with the compiled module on every case.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

import scipy.signal as ss  # noqa: E402

import tools as ref_tools  # noqa: E402  (compiled reference module)
from oracle import silence as osil  # noqa: E402
from tests import silence_cases as sc  # noqa: E402

ref_tools.medfilt = lambda v, k: ss.medfilt(np.asarray(v, float), k)
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    g = {}
    for c in sc.CRAFTED:
        x = sc.crafted_signal(c)
        e = c.energy
        assert x.dtype == np.float32 and e.dtype == np.float32
        # the reference takes alpha and beta as keywords with the defaults 0.025 / 0.075
        out, sm, fm, tot = ref_tools.removeSilence(x, len(x), e, len(e), c.fs, c.Tw, c.Ts, alpha=c.alpha, beta=c.beta)
        o2, s2, f2, t2 = osil.remove_silence(x, e, c.fs, c.Tw, c.Ts, c.alpha, c.beta)
        assert np.array_equal(out, o2) and np.array_equal(sm, s2) and np.array_equal(fm, f2) and tot == t2, c.name
        assert (out is x) == (o2 is x), c.name
        g[c.name + "_x_sha"] = sc.sha(x)
        g[c.name + "_energy_sha"] = sc.sha(e)
        g[c.name + "_frame_marker"] = fm.astype(np.int8)
        g[c.name + "_sample_marker"] = np.packbits(sm.astype(np.uint8))
        g[c.name + "_out_sha"] = sc.sha(out)
        g[c.name + "_meta"] = np.array([len(x), int(sm.sum()), int(out is x), tot], np.int64)
    path = os.path.join(OUT, "silence_runs_golden.npz")
    np.savez_compressed(path, **g)
    print("silence_runs_golden.npz", os.path.getsize(path) // 1024, "KiB,", len(sc.CRAFTED), "cases")


if __name__ == "__main__":
    main()
