"""Generate tests/golden/ref_tools_golden.npz (run in the BUILD container: python tests/golden/make_ref_tools_golden.py).

The outputs of the reference's own lib/cython_impl/tools.pyx compiled unmodified (oracle/_ref/tools*.so) on the inputs of
the `*_vs_compiled_reference*` tests of tests/test_oracle_pins.py, so that those tests run wherever the repository is
checked out, without the reference source.  Inputs are re-created from the same seeds; only SHA-256 digests of them are
stored (the tests check them first, so a changed input fails loudly instead of comparing against another case).  Outputs
the tests compare bit for bit are stored as digests + shape, the float statistics (compared with a tolerance) as arrays.
`tools.medfilt` is rebound to a float64-returning scipy.signal.medfilt as in the tests (modern scipy keeps the integer
dtype the 2021 one promoted).
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

import scipy.signal as ss  # noqa: E402

import tools as ref_tools  # noqa: E402  (compiled reference module)
from oracle import frontend as ofe  # noqa: E402
from oracle import silence as osil  # noqa: E402
from sm_hpss_mtl_amd.synth import SILENCE_CASES, gappy_clip  # noqa: E402

ref_tools.medfilt = lambda v, k: ss.medfilt(np.asarray(v, float), k)
OUT = os.path.dirname(os.path.abspath(__file__))

# the cases of tests/test_oracle_pins.py
PATCH_T = (69, 98, 137, 300)
PATCH_W_SHIFT = ((68, 68), (68, 34), (99, 34), (249, 24))
STATS = ("mean", "variance", "skew", "kurtosis")


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def main():
    g = {}
    rng = np.random.default_rng(5)
    for T in PATCH_T:
        FV = rng.standard_normal((9, T)).astype(np.float32)
        g["patches_T%d_in_sha" % T] = sha(FV)
        for W, shift in PATCH_W_SHIFT:
            FVt = ofe.tile_if_short(FV, W)
            ref = ref_tools.extract_patches(FVt, FVt.shape, W, shift)
            assert ref.dtype == np.float64 and np.array_equal(ref, ofe.extract_patches(FVt, W, shift))
            g["patches_T%d_W%d_s%d_sha" % (T, W, shift)] = sha(ref)
            g["patches_T%d_W%d_s%d_shape" % (T, W, shift)] = np.array(ref.shape, np.int64)

    rng = np.random.default_rng(3)
    for dt in (np.float32, np.float64):
        FV = rng.normal(size=(42, 68)).astype(dt) * 7 - 3
        ref = ref_tools.scale_data(FV, FV.mean(axis=1), FV.std(axis=1))
        assert ref.dtype == np.float64
        g["scale_%s_in_sha" % np.dtype(dt).name] = sha(FV)
        g["scale_%s_sha" % np.dtype(dt).name] = sha(ref)
        g["scale_%s_shape" % np.dtype(dt).name] = np.array(ref.shape, np.int64)

    rng = np.random.default_rng(11)
    FV = rng.gamma(2.0, size=(5, 21, 34)) - rng.normal(size=(5, 21, 34)) ** 2
    g["stats_in_sha"] = sha(FV)
    for stat in STATS:
        for axis in (0, 1):
            g["stats_%s_%d" % (stat, axis)] = np.asarray(ref_tools.get_data_statistics(FV, stat_type=stat, axis=axis))

    for c in range(len(SILENCE_CASES)):
        x = osil.normalize_signal(gappy_clip(c))
        e = osil.rms(x, 400, 160)
        out, sm, fm, tot = ref_tools.removeSilence(x, len(x), e, len(e), 16000, 25, 10)
        g["silence_c%d_in_sha" % c] = sha(np.concatenate([x, e]))
        g["silence_c%d_out_sha" % c] = sha(out)
        g["silence_c%d_out_dtype" % c] = np.array(out.dtype.str)
        g["silence_c%d_meta" % c] = np.array([len(out), int(out is x), len(sm), int(tot)], np.int64)
        g["silence_c%d_sample_marker" % c] = np.packbits(np.asarray(sm).astype(np.uint8))
        g["silence_c%d_frame_marker" % c] = np.asarray(fm).astype(np.int8)
        assert set(np.unique(sm)) <= {0, 1} and set(np.unique(fm)) <= {0, 1}

    np.savez_compressed(os.path.join(OUT, "ref_tools_golden.npz"), **g)
    print("ref_tools_golden.npz", os.path.getsize(os.path.join(OUT, "ref_tools_golden.npz")) // 1024, "KiB")


if __name__ == "__main__":
    main()
