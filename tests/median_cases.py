"""The case table and the inputs of tests/test_median_layouts_gpu.py -- TEST INFRASTRUCTURE, a plain module like
tests/median_plans.py: tests/test_median_plans.py (no GPU) shows that every row reaches the kernel family and the harm layout it
is named for and that the table covers every (family, requested layout, entry point) that exists; the GPU test runs the rows.

A row names the entry point, the shape, the windows, the batch (a number, or '2cu-1' / '2cu' / '2cu+3' in units of the device's
compute units: the persistent kernel starts at two clips per CU), the requested harm layout, the value of SMH_MEDIAN_PERSIST
(None: unset), and what it is there for: `family` and `wrote`, the layout the entry point must return.  `why` is the condition the
shape was chosen for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import median_plans as P

N_CU_MI355X = 256  # the CPU test resolves '2cu' with the MI355X's count; the GPU test with the device's own

CASES = []


def case(entry, K, T, lh, lp, B, lay, family, wrote, why, persist=None):
    CASES.append(dict(entry=entry, K=K, T=T, lh=lh, lp=lp, B=B, lay=lay, family=family, wrote=wrote, why=why, persist=persist))


def batch(B, n_cu):
    return B if isinstance(B, int) else {"2cu-1": 2 * n_cu - 1, "2cu": 2 * n_cu, "2cu+3": 2 * n_cu + 3}[B]


def case_id(c):
    return "%s-K%dT%d-w%d_%d-B%s-lay%d-%s%d%s" % (c["entry"], c["K"], c["T"], c["lh"], c["lp"], c["B"], c["lay"], c["family"],
                                                  c["wrote"], "" if c["persist"] is None else "-persist" + c["persist"])


# ---- partial 16-frame blocks, float4 or scalar stores: the block-split kernel, every layout, both entry points -----------------
for T in (16, 17, 31, 33, 47, 98):
    for lay in (0, 1, 2):
        for lh, lp in ((11, 11), (17, 17), (21, 11)):
            case("hpss_ex", 24, T, lh, lp, 3, lay, "split", lay, "partial blocks")
        for lh in (3, 11, 21):
            case("time_ex", 24, T, lh, 0, 3, lay, "split", lay, "partial blocks")
# ---- segments: nsh = 1 .. 4 comes with the shapes above; segment lengths of 23 (67 / 3) and of 32 (64 / 2) frames ------------------
for lay in (1, 2):
    case("hpss_ex", 24, 67, 11, 11, 3, lay, "split", lay, "segments")
    case("hpss_ex", 24, 64, 11, 11, 3, lay, "split", lay, "segments")
    case("time_ex", 40, 67, 11, 0, 2, lay, "split", lay, "segments")
# ---- clips of more than one frame tile (tile starts at multiples of TT: 79, 83, 57 frames) -------------------------------------------
for B in (1, 3):
    for lay in (1, 2):
        case("hpss_ex", 201, 101, 21, 11, B, lay, "split", lay, "tiles")  # two tiles, the second 22 frames
        case("hpss_ex", 201, 180, 21, 11, B, lay, "split", lay, "tiles")  # three tiles: 0, 79, 158
        case("hpss_ex", 201, 333, 17, 17, B, lay, "split", lay, "tiles")  # five tiles of 83, the last one frame
        case("hpss_ex", 257, 130, 21, 11, B, lay, "split", lay, "tiles")  # three tiles of 57
case("time_ex", 201, 180, 21, 0, 3, 2, "split", 2, "tiles")
case("time_ex", 201, 180, 21, 0, 1, 1, "split", 1, "tiles")
case("time_ex", 257, 130, 17, 0, 3, 2, "split", 2, "tiles")
# ---- the persistent kernel: two clips per CU, one tile, conflict-free T ---------------------------------------------------------------
for lay in (0, 1, 2):
    for lh, lp, persist in ((21, 11, None), (21, 21, None), (17, 17, "1"), (11, 11, "1")):
        case("hpss_ex", 25, 33, lh, lp, "2cu+3", lay, "persist", lay, "persist", persist)  # 3300-byte clips: every 16-byte phase
        case("hpss_ex", 24, 34, lh, lp, "2cu", lay, "persist", lay, "persist", persist)
for lay in (1, 2):
    case("hpss_ex", 25, 45, 11, 11, "2cu+3", lay, "persist", lay, "persist", "1")  # two harmonic segments of 23 frames
    case("hpss_ex", 24, 36, 21, 11, "2cu", lay, "split", lay, "persist")       # T = 36 is not conflict-free
    case("hpss_ex", 25, 33, 21, 11, "2cu-1", lay, "split", lay, "persist")     # one clip short of two per CU
    case("hpss_ex", 25, 33, 17, 17, "2cu", lay, "split", lay, "persist")       # windows up to 17 ask for it only when forced
    case("hpss_ex", 25, 33, 21, 11, "2cu", lay, "split", lay, "persist", "0")  # and the switch turns it off
# ---- demotion 2 -> 1: the delete/insert kernel has no blocked store ---------------------------------------------------------------------
for lay in (0, 1, 2):
    wrote = 1 if lay == 2 else lay
    case("hpss_ex", 40, 33, 31, 31, 3, lay, "delete_insert", wrote, "demotion")
    case("hpss_ex", 40, 33, 11, 51, 3, lay, "delete_insert", wrote, "demotion")
    case("time_ex", 24, 33, 23, 0, 3, lay, "delete_insert", wrote, "demotion")
    case("time_ex", 24, 47, 63, 0, 3, lay, "delete_insert", wrote, "demotion")
case("hpss_ex", 201, 180, 31, 31, 2, 2, "delete_insert", 1, "demotion")  # over tiles
# ---- fallback to layout 0 ------------------------------------------------------------------------------------------------------------------
for lay in (0, 1, 2):
    case("hpss_ex", 40, 33, 5, 31, 3, lay, "two_singles", 0, "fallback")   # pairs outside kPairs
    case("hpss_ex", 40, 33, 13, 7, 3, lay, "two_singles", 0, "fallback")
    case("hpss_ex", 24, 14, 21, 11, 3, lay, "two_singles", 0, "fallback")  # T <= l_harm / 2 + 4
    case("hpss_ex", 9, 33, 21, 11, 3, lay, "two_singles", 0, "fallback")   # K <= l_perc / 2 + 4
    case("hpss_ex", 24, 33, 1, 11, 3, lay, "two_singles", 0, "fallback")   # l_harm == 1
    case("time_ex", 24, 14, 21, 0, 3, lay, "small", 0, "fallback")
    case("time_ex", 24, 5, 11, 0, 3, lay, "small", 0, "fallback")          # several reflections
    case("time_ex", 24, 33, 1, 0, 3, lay, "copy", 0, "fallback")
for lay in (1, 2):
    case("hpss_ex", 24, 33, 21, 11, 0, lay, None, lay, "fallback")         # B == 0: the requested layout, nothing touched
    case("time_ex", 24, 33, 21, 0, 0, lay, None, lay, "fallback")
# ---- tall spectrograms: the whole LDS to one workgroup from K = 698 (l_harm = 21), tiles of 37 / 21 / 19 frames ---------------------------
for lay in (1, 2):
    case("hpss_ex", 698, 77, 21, 11, 2, lay, "delete_insert", 1, "tall")
    case("time_ex", 698, 77, 21, 0, 1, lay, "delete_insert", 1, "tall")
case("hpss_ex", 960, 45, 21, 11, 1, 2, "delete_insert", 1, "tall")   # the last K whose 16 waves fit: 15 harmonic + 1 percussive
case("time_ex", 1024, 41, 21, 0, 1, 2, "delete_insert", 1, "tall")   # 16 harmonic waves
# ---- the entry points without a layout argument take the same routes -----------------------------------------------------------------------
case("hpss", 24, 33, 21, 11, 3, 0, "split", 0, "plain entries")
case("hpss", 201, 180, 21, 11, 2, 0, "split", 0, "plain entries")
case("hpss", 25, 33, 21, 11, "2cu+3", 0, "persist", 0, "plain entries")
case("hpss", 40, 33, 31, 31, 3, 0, "delete_insert", 0, "plain entries")
case("hpss", 40, 33, 13, 7, 3, 0, "two_singles", 0, "plain entries")
case("time", 24, 33, 21, 0, 3, 0, "split", 0, "plain entries")
case("time", 24, 47, 63, 0, 3, 0, "delete_insert", 0, "plain entries")
case("time", 24, 14, 21, 0, 3, 0, "small", 0, "plain entries")
case("time", 24, 33, 1, 0, 3, 0, "copy", 0, "plain entries")

# Refused shapes: (entry, K, T, l_harm, l_perc, requested layout, the text of smh_last_error()).  More than 16 waves per workgroup
# is what make_plan meets first on the way up in K (l_harm = 21, two tiles and a little: 961 for a pair, 1025 for a single filter);
# the LDS refusal behind the tall branch starts at K = 1939, and K = 1938 (a one-frame tile) fails on its waves.
REFUSED = [
    ("hpss_ex", 961, 45, 21, 11, 2, "tile 961x21 needs more than 16 waves per workgroup"),
    ("time_ex", 1025, 41, 21, 0, 2, "tile 1025x19 needs more than 16 waves per workgroup"),
    ("hpss_ex", 1938, 15, 21, 11, 1, "tile 1938x1 needs more than 16 waves per workgroup"),
    ("hpss_ex", 1939, 15, 21, 11, 2, "K=1939 too large for an LDS tile with l_harm=21"),
    ("time_ex", 1939, 15, 21, 0, 1, "K=1939 too large for an LDS tile with l_harm=21"),
]

# the harm of smh_median_time_ex_f32 equals the harm of smh_hpss_median_ex_f32 in the same layout: (K, T, l_harm, l_perc, B, requested
# layout, layout both write)
CROSS_ENTRY = [(24, 47, 11, 11, 3, 2, 2), (201, 180, 21, 11, 2, 2, 2), (40, 33, 31, 31, 3, 2, 1)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def clips(K, T):
    """(3, K, T) float32 >= 0, finite, no -0.0: |Gaussian| noise; the same quantised to multiples of 1/4 (many ties); a clip whose
    first third of rows is zero and whose other values are, a quarter each, f32 subnormals (1e-41 .. 1e-39), values near 1e30, and
    noise."""
    rng = np.random.default_rng(K * 1000 + T)
    S = np.abs(rng.standard_normal((3, K, T))).astype(np.float32)
    S[1] = np.round(S[1] * 4) / 4
    kind = rng.integers(0, 4, (K, T))
    sub = (rng.integers(8, 714, (K, T)).astype(np.float64) * 1.4e-42).astype(np.float32)  # 1.1e-41 .. 1.0e-39, steps of a few ulp
    S[2] = np.where(kind == 0, sub, np.where(kind == 1, (1e30 * (1.0 + S[2])).astype(np.float32), S[2]))
    S[2, : max(1, K // 3)] = 0.0
    assert np.isfinite(S).all() and not np.signbit(S).any()
    return S


def clip_index(B):
    """Clip b of a batch is clips(K, T)[clip_index(B)[b]]."""
    return np.arange(B) % 3


# ---- the library's own decision ------------------------------------------------------------------------------------------------------------
FAMILY_CODE = {None: -1, "copy": 0, "small": 1, "split": 2, "persist": 3, "delete_insert": 4, "two_singles": 5}


def library_route(lib, entry, K, T, lh, lp, B, lay, n_cu=0, align=16):
    """smh_internal_median_plan (test-only export, not in include/smh.h) as the dict of median_plans.route; raises
    median_plans.Refused with the text of smh_last_error() where the entry point would return SMH_E_INVALID.  n_cu = 0: the library
    asks the device; align: the input clip's alignment class.  The switches are the process's environment."""
    from sm_hpss_mtl_amd import _lib
    out = (C.c_int * len(P.FIELDS))()
    rc = lib.smh_internal_median_plan(P.ALL_ENTRIES.index(entry), K, T, lh, lp, B, lay, n_cu, align, out)
    if rc == _lib.SMH_E_INVALID:
        raise P.Refused(_lib.last_error())
    assert rc == 0, _lib.last_error()
    r = dict(zip(P.FIELDS, out))
    r["family"] = {v: k for k, v in FAMILY_CODE.items()}[r["family"]]
    return r
