"""Python restatement of the routing of the HPSS median filters (sm_hpss_mtl_amd/csrc/smh_median.hip, smh_median_split.h,
smh_median_split.hip, smh_median_singles.hip) -- TEST INFRASTRUCTURE.

It computes no medians: `route` only says which kernel family a call of one of the median entry points takes, which harm layout
that kernel writes and how it tiles and segments the clip, so that tests/test_median_plans.py can show that every case of
tests/test_median_layouts_gpu.py reaches the route it is named for, and the GPU test can hold the library's own decision
(smh_internal_median_route) against it.  Each function cites the C++ it copies; a change of a threshold there must be mirrored
here, and the hand-computed pins of tests/test_median_plans.py then say which cases have moved off the path they were chosen for.

The tuning switches SMH_MEDIAN_NOSPLIT, SMH_MEDIAN_SEG and SMH_MEDIAN_PTHREADS are not modelled (the tests skip when one is set);
SMH_MEDIAN_PERSIST is the `persist` argument of `route`.

The module also holds the numpy decoders (and encoders) of harm layouts 1 and 2 that the GPU test reads its buffers with.
"""
from __future__ import annotations

from itertools import product

import numpy as np

LDS_BYTES_PER_CU = 160 * 1024  # smh_common.h: kLdsBytesPerCU
MAX_MEDIAN = 63                # include/smh.h: SMH_MAX_MEDIAN
MAX_BATCH = 65535              # smh_median.hip check_args: `B <= 65535`
SPLIT_MAX_WINDOW = 21          # smh_median_split.h: kSplitMaxWindow

_SWEEP = (11, 21, 31, 41, 51)
# smh_median.hip: kPairs -- both filters in one launch
PAIRS = frozenset({(21, 11), (17, 17)} | set(product(_SWEEP, _SWEEP)))
# smh_median_singles.hip: kSingles -- SMH_MEDIAN_SINGLE(w) = (w, 0) and (0, w), every odd window 3 .. 63
SINGLES = frozenset({(w, 0) for w in range(3, 64, 2)} | {(0, w) for w in range(3, 64, 2)})
# smh_median_split.hip: kSplit -- five pairs, SMH_SPLIT_SINGLE(w) for every odd window 3 .. 21
SPLIT = frozenset({(21, 11), (17, 17), (11, 11), (11, 21), (21, 21)}
                  | {(w, 0) for w in range(3, 22, 2)} | {(0, w) for w in range(3, 22, 2)})
# smh_median_split.hip: kPersist -- (l_harm, l_perc, threads)
PERSIST = frozenset({(lh, lp, t) for (lh, lp) in ((21, 11), (17, 17), (11, 11), (11, 21), (21, 21)) for t in (512, 768)}
                    | {(17, 17, 1024)})
PERSIST_THREADS = 512          # smh_median.hip launch_route: `int pthreads = 512`

FAMILIES = ("copy", "small", "split", "persist", "delete_insert", "two_singles")
ENTRIES = ("hpss_ex", "time_ex", "hpss", "time")  # smh_hpss_median_ex_f32, smh_median_time_ex_f32, smh_hpss_median_f32, smh_median_time_f32

assert all(max(e) <= SPLIT_MAX_WINDOW for e in SPLIT)


class Refused(ValueError):
    """The call returns SMH_E_INVALID; str(e) is the text of smh_last_error()."""


def fast_ok(n, w):
    """smh_median.hip fast_ok: the register-window kernels fold once per side."""
    return w >= 3 and w // 2 + 4 < n


def split_threads(lh, lp):
    """smh_median_split.h SplitCfg<LH, LP>::kThreads."""
    return 512 if max(lh, lp) <= 17 else 384


def _waves(n, seg):
    return (n * seg + 63) // 64 if seg else 0


def make_plan(K, T, lh, lp):
    """smh_median.hip make_plan: {TT, ntiles, stride, lds, tall, nsh, nsp, nwh, nwp} -- the frame tile, and the segments of the
    delete/insert kernel.  Raises Refused with the library's message."""
    hh = lh // 2
    budget_words = (LDS_BYTES_PER_CU // 2 - 1024) // 4
    tall = False
    if K * (T | 1) <= budget_words:
        TT, stride = T, T | 1
    else:
        maxcols = budget_words // K
        if maxcols % 2 == 0:
            maxcols -= 1
        TT = maxcols - 2 * hh
        if TT < 8:  # very tall spectrograms: one workgroup gets the whole 160 KiB
            tall = True
            maxcols = ((LDS_BYTES_PER_CU - 1024) // 4) // K
            if maxcols % 2 == 0:
                maxcols -= 1
            TT = maxcols - 2 * hh
            if TT < 1:
                raise Refused("K=%d too large for an LDS tile with l_harm=%d" % (K, lh))
        TT = min(TT, T)
        stride = (TT + 2 * hh) | 1
    nt = TT
    nsh, nsp = (2 if lh else 0), (3 if lp else 0)
    if lh and nt < 2 * lh:
        nsh = 1
    if lp and K < 6 * lp:
        nsp = 1
    nwh, nwp = _waves(K, nsh), _waves(nt, nsp)
    while nwh + nwp > 16:
        if nsh > 1 and nwh >= nwp:
            nsh -= 1
        elif nsp > 1:
            nsp -= 1
        elif nsh > 1:
            nsh -= 1
        else:
            break
        nwh, nwp = _waves(K, nsh), _waves(nt, nsp)
    if nwh + nwp > 16:
        raise Refused("tile %dx%d needs more than 16 waves per workgroup" % (K, nt))
    return dict(TT=TT, ntiles=(T + TT - 1) // TT, stride=stride, lds=K * stride * 4, tall=tall, nsh=nsh, nsp=nsp, nwh=nwh, nwp=nwp)


def make_split_roles(K, nt, lh, lp, maxwaves):
    """smh_median.hip make_split_roles: (nsh, nsp, nwh, nwp) of the block-split and persistent kernels, or None when no pair of
    segment counts fits `maxwaves` waves."""
    best, bh, bp = -1, 0, 0
    for nsh in range(1 if lh else 0, (4 if lh else 0) + 1):
        if lh and nsh > 1 and nt < 2 * lh * nsh:
            break
        for nsp in range(1 if lp else 0, (6 if lp else 0) + 1):
            if lp and nsp > 1 and K < 2 * lp * nsp:
                break
            if _waves(K, nsh) + _waves(nt, nsp) > maxwaves:
                continue
            ch = ((nt + nsh - 1) // nsh + lh) * (lh + 6) if lh else 0
            cp = ((K + nsp - 1) // nsp + lp) * (lp + 6) if lp else 0
            c = max(ch, cp)
            if best < 0 or c < best:
                best, bh, bp = c, nsh, nsp
    if best < 0:
        return None
    return bh, bp, _waves(K, bh), _waves(nt, bp)


def persist_tile_bytes(K, T):
    """smh_median_split.h persist_tile_bytes."""
    return ((K * T * 4 + 16) + 1023) & ~1023


def conflict_free(T):
    """smh_median.hip launch_route: gcd(T, 64) <= 2."""
    return bool(T & 1) or (T & 63) % 4 == 2


def _result(family, layout, ntiles=0, TT=0, nsh=0, nsp=0):
    return dict(family=family, layout=layout, ntiles=ntiles, TT=TT, nsh=nsh, nsp=nsp)


def launch_route(K, T, lh, lp, B, harm_layout, n_cu, persist=None):
    """smh_median.hip launch_route, the decision of launch(): persistent kernel, block-split kernel, else the delete/insert kernel,
    which has no blocked store (2 -> 1).  persist: the value of SMH_MEDIAN_PERSIST (None unset, else 0 / 1)."""
    if ((lh, lp) not in PAIRS) if (lh and lp) else ((lh, lp) not in SINGLES):
        raise Refused("no median kernel for (l_harm,l_perc)=(%d,%d)" % (lh, lp))
    p = make_plan(K, T, lh, lp)
    want_persist = (lh > 17 or lp > 17) if persist is None else bool(int(persist))
    if want_persist and lh and lp and (lh, lp, PERSIST_THREADS) in PERSIST:
        if (p["ntiles"] == 1 and conflict_free(T) and 2 * persist_tile_bytes(K, T) <= LDS_BYTES_PER_CU and B >= 2 * n_cu):
            q = make_split_roles(K, T, lh, lp, PERSIST_THREADS // 64)
            if q:
                return _result("persist", harm_layout, 1, p["TT"], q[0], q[1])
    if (lh, lp) in SPLIT:
        q = make_split_roles(K, p["TT"], lh, lp, split_threads(lh, lp) // 64)
        if q:
            return _result("split", harm_layout, p["ntiles"], p["TT"], q[0], q[1])
    return _result("delete_insert", 1 if harm_layout == 2 else harm_layout, p["ntiles"], p["TT"], p["nsh"], p["nsp"])


def check_args(name, B, K, T, w):
    """smh_median.hip check_args (the null-pointer requirement apart)."""
    if not (B >= 0 and K >= 1 and T >= 1):
        raise Refused("%s: bad shape B=%d K=%d T=%d" % (name, B, K, T))
    if not (1 <= w <= MAX_MEDIAN and w & 1):
        raise Refused("%s: window must be odd in [1,%d], got %d" % (name, MAX_MEDIAN, w))
    if B > MAX_BATCH:
        raise Refused("%s: B=%d exceeds the grid limit; split the batch" % (name, B))


def time_route(K, T, lh, B, n_cu, persist=None):
    """smh_median.hip time_route, the decision of smh_median_time_f32."""
    if lh == 1:
        return _result("copy", 0)
    if not fast_ok(T, lh):
        return _result("small", 0)
    return launch_route(K, T, lh, 0, B, 0, n_cu, persist)


def pair_fused(K, T, lh, lp):
    """smh_median.hip pair_fused: both filters in one launch."""
    return fast_ok(T, lh) and fast_ok(K, lp) and (lh, lp) in PAIRS


def route(entry, K, T, lh, lp, B, harm_layout, n_cu, persist=None):
    """{family, layout, ntiles, TT, nsh, nsp} of one call.  entry: one of ENTRIES; `lp` and `harm_layout` are ignored where the
    entry has no such argument.  family 'two_singles' (one launch per filter, layout 0), 'copy' and 'small' carry no tiling.  B == 0
    launches nothing: family None, the requested layout.  Raises Refused where the call returns SMH_E_INVALID."""
    name = {"hpss_ex": "smh_hpss_median_ex_f32", "time_ex": "smh_median_time_ex_f32", "hpss": "smh_hpss_median_f32",
            "time": "smh_median_time_f32"}[entry]
    pair = entry in ("hpss_ex", "hpss")
    if not pair:
        lp = 0
    if entry in ("hpss", "time"):
        harm_layout = 0
    check_args(name, B, K, T, lh)
    if pair:
        check_args(name, B, K, T, lp)
    if harm_layout not in (0, 1, 2):
        raise Refused("%s: harm_layout must be 0, 1 or 2" % name)
    if B == 0:
        return _result(None, harm_layout)
    if pair:  # smh_median::launch_hpss and smh_hpss_median_f32 (hpss_route)
        if pair_fused(K, T, lh, lp):
            return launch_route(K, T, lh, lp, B, harm_layout, n_cu, persist)
        # one launch per filter: either may still be refused
        time_route(K, T, lh, B, n_cu, persist)
        if lp != 1 and fast_ok(K, lp):
            launch_route(K, T, 0, lp, B, 0, n_cu, persist)
        return _result("two_singles", 0)
    if entry == "time_ex" and not (lh == 1 or not fast_ok(T, lh) or harm_layout == 0):  # time_ex_route
        return launch_route(K, T, lh, 0, B, harm_layout, n_cu, persist)
    return time_route(K, T, lh, B, n_cu, persist)


def segment_starts(T, TT, nsh):
    """Frame at which each (tile, segment) harmonic task starts: hpss_median_split_kernel, `ts = t0 + sg * seglen` with
    seglen = ceil(nt / nsh) of the tile's own nt frames."""
    out = []
    for t0 in range(0, T, TT):
        nt = min(T, t0 + TT) - t0
        seglen = (nt + nsh - 1) // nsh
        out += [t0 + sg * seglen for sg in range(nsh) if sg * seglen < nt]
    return out


# ---- harm layouts (include/smh.h: "Layouts of the harmonic median") ----------------------------------------------------------------
def harm_buffer_floats(K, T):
    """smh_frontend.hip smh_harm_buffer_floats."""
    return (T + 15) // 16 * 16 * K


def owned_floats(layout, B, K, T):
    """Floats of the harm buffer a call may write: layouts 0 and 1 the (B, K, T) image, layout 2 whole 16-frame blocks."""
    return B * (harm_buffer_floats(K, T) if layout == 2 else K * T)


def encode_harm(h, layout, pad=0.0, shift=0):
    """(B, K, T) -> the flat buffer of `layout`.  shift != 0 stores frame t in the slot of frame t + shift (wrapping): what a
    store one slot off would leave; for the decoders' own test."""
    h = np.asarray(h)
    B, K, T = h.shape
    if shift:
        h = np.roll(h, shift, axis=2)
    if layout == 0:
        return np.ascontiguousarray(h).reshape(-1)
    if layout == 1:
        return np.ascontiguousarray(h.transpose(0, 2, 1)).reshape(-1)
    nb = (T + 15) // 16
    buf = np.full((B, nb, K, 16), pad, h.dtype)
    for t in range(T):
        buf[:, t // 16, :, t % 16] = h[:, :, t]
    return buf.reshape(-1)


def decode_harm(buf, layout, B, K, T):
    """The flat buffer of `layout` -> (B, K, T); layout 2 drops the padding frames t >= T of the last block."""
    buf = np.asarray(buf).reshape(-1)
    if layout == 0:
        return buf[:B * K * T].reshape(B, K, T)
    if layout == 1:
        return buf[:B * K * T].reshape(B, T, K).transpose(0, 2, 1)
    nb = (T + 15) // 16
    img = buf[:B * nb * K * 16].reshape(B, nb, K, 16)
    return img.transpose(0, 2, 1, 3).reshape(B, K, nb * 16)[:, :, :T]
