"""Python restatement of the launch plan of the HPSS median filters (sm_hpss_mtl_amd/csrc/smh_median_plan.h; launchers in
smh_median.hip) -- TEST INFRASTRUCTURE.

It computes no medians: `route` says which kernel family a call of one of the median entry points (or the ragged launch) takes, which
harm layout that kernel writes, how it tiles and segments the clip, with how many waves, threads and LDS bytes on which grid, and
whether the block-split kernel stages the clip by LDS-DMA, so that tests/test_median_plans.py can show that every case of
tests/test_median_layouts_gpu.py reaches the route it is named for and hold the library's own plan (smh_internal_median_plan)
against it without a GPU.  Each function cites the C++ it restates; a change of a threshold there must be mirrored here, and the
hand-computed pins of tests/test_median_plans.py then say which cases have moved off the path they were chosen for.  Nothing here
calls the library.

The switches are the `env` argument, a dict of the SMH_MEDIAN_* variables that are set (`switches`); `persist` of `route` is
shorthand for SMH_MEDIAN_PERSIST.  The probe SMH_MEDIAN_PROBE_NOLOAD is not modelled.

The module also holds the numpy decoders (and encoders) of harm layouts 1 and 2 that the GPU test reads its buffers with.
"""
from __future__ import annotations

import re
from itertools import product

import numpy as np

LDS_BYTES_PER_CU = 160 * 1024  # smh_common.h: kLdsBytesPerCU
MAX_MEDIAN = 63                # include/smh.h: SMH_MAX_MEDIAN
MAX_BATCH = 65535              # smh_median.hip check_args: `B <= 65535`
SPLIT_MAX_WINDOW = 21          # smh_median_plan.h: kSplitMaxWindow

_SWEEP = (11, 21, 31, 41, 51)
# SMH_MEDIAN_PAIRS -- both filters in one launch
PAIRS = frozenset({(21, 11), (17, 17)} | set(product(_SWEEP, _SWEEP)))
# SMH_MEDIAN_SINGLES -- (w, 0) and (0, w), every odd window 3 .. 63
SINGLES = frozenset({(w, 0) for w in range(3, 64, 2)} | {(0, w) for w in range(3, 64, 2)})
# SMH_MEDIAN_SPLIT_PAIRS, SMH_MEDIAN_SPLIT_SINGLES -- five pairs, every odd window 3 .. 21
SPLIT = frozenset({(21, 11), (17, 17), (11, 11), (11, 21), (21, 21)}
                  | {(w, 0) for w in range(3, 22, 2)} | {(0, w) for w in range(3, 22, 2)})
# SMH_MEDIAN_PERSIST_BUILDS -- (l_harm, l_perc, threads)
PERSIST = frozenset({(lh, lp, t) for (lh, lp) in ((21, 11), (17, 17), (11, 11), (11, 21), (21, 21)) for t in (512, 768)}
                    | {(17, 17, 1024)})
PERSIST_THREADS = 512          # MedianSwitches::pthreads
DELETE_INSERT_THREADS = 1024   # smh_median_kernel.h: __launch_bounds__(1024)

FAMILIES = ("copy", "small", "split", "persist", "delete_insert", "two_singles")
ENTRIES = ("hpss_ex", "time_ex", "hpss", "time")  # smh_hpss_median_ex_f32, smh_median_time_ex_f32, smh_hpss_median_f32, smh_median_time_f32
ALL_ENTRIES = ENTRIES + ("freq", "rag")           # smh_internal_median_plan's numbers: 4 smh_median_freq_f32, 5 the ragged launch
SWITCHES = ("SMH_MEDIAN_NOSPLIT", "SMH_MEDIAN_PERSIST", "SMH_MEDIAN_PTHREADS", "SMH_MEDIAN_SEG", "SMH_MEDIAN_DMA_STAGE")
# the order of smh_internal_median_plan's ints (median_plan_ints)
FIELDS = ("family", "layout", "ntiles", "TT", "nsh", "nsp", "stride", "nwh", "nwp", "threads", "lds", "grid_x", "grid_y", "dma")

assert all(max(e) <= SPLIT_MAX_WINDOW for e in SPLIT)


class Refused(ValueError):
    """The call returns SMH_E_INVALID; str(e) is the text of smh_last_error()."""


def _atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def switches(env=None):
    """read_median_switches: {nosplit, persist (None unset, else 0 / 1), pthreads, seg (None, or (nsh, nsp) as given), dma}."""
    env = env or {}
    m = re.match(r"\s*([+-]?\d+),\s*([+-]?\d+)", env.get("SMH_MEDIAN_SEG", ""))  # sscanf("%d,%d") == 2
    return dict(nosplit="SMH_MEDIAN_NOSPLIT" in env,
                persist=int(_atoi(env["SMH_MEDIAN_PERSIST"]) != 0) if "SMH_MEDIAN_PERSIST" in env else None,
                pthreads=_atoi(env["SMH_MEDIAN_PTHREADS"]) if "SMH_MEDIAN_PTHREADS" in env else PERSIST_THREADS,
                seg=(int(m.group(1)), int(m.group(2))) if m else None,
                dma=not ("SMH_MEDIAN_DMA_STAGE" in env and _atoi(env["SMH_MEDIAN_DMA_STAGE"]) == 0))


def fast_ok(n, w):
    """fast_ok: the register-window kernels fold once per side."""
    return w >= 3 and w // 2 + 4 < n


def split_threads(lh, lp):
    """split_threads of a listed (lh, lp) -- SplitCfg<LH, LP>::kThreads; 0: no block-split build."""
    return 0 if (lh, lp) not in SPLIT else 512 if max(lh, lp) <= 17 else 384


def _waves(n, seg):
    return (n * seg + 63) // 64 if seg else 0


def _odd_cols(budget_words, K):
    """The columns of K rows in the budget, made odd."""
    c = budget_words // K
    return c - 1 if c % 2 == 0 else c


def make_plan(K, T, lh, lp, env=None):
    """plan_tile and delete_insert_roles: {TT, ntiles, stride, lds, tall, nsh, nsp, nwh, nwp} -- the frame tile, and the segments of
    the delete/insert kernel.  Raises Refused with the library's message."""
    hh = lh // 2
    budget_words = (LDS_BYTES_PER_CU // 2 - 1024) // 4
    tall = False
    if K * (T | 1) <= budget_words:
        TT, stride = T, T | 1
    else:
        TT = _odd_cols(budget_words, K) - 2 * hh
        if TT < 8:  # very tall spectrograms: one workgroup gets the whole 160 KiB
            tall = True
            TT = _odd_cols((LDS_BYTES_PER_CU - 1024) // 4, K) - 2 * hh
            if TT < 1:
                raise Refused("K=%d too large for an LDS tile with l_harm=%d" % (K, lh))
        TT = min(TT, T)
        stride = (TT + 2 * hh) | 1
    nt = TT
    nsh, nsp = (2 if lh else 0), (3 if lp else 0)
    seg = switches(env)["seg"]
    if seg:
        if lh and seg[0] >= 1:
            nsh = seg[0]
        if lp and seg[1] >= 1:
            nsp = seg[1]
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


def make_split_roles(K, nt, lh, lp, maxwaves, env=None):
    """split_roles: (nsh, nsp, nwh, nwp) of the block-split and persistent kernels, or None when no pair of segment counts fits
    `maxwaves` waves.  SMH_MEDIAN_SEG replaces the counts when its own fit."""
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
    seg = switches(env)["seg"]
    if seg and (not lh or seg[0] >= 1) and (not lp or seg[1] >= 1):
        a, b = (seg[0] if lh else 0), (seg[1] if lp else 0)
        if _waves(K, a) + _waves(nt, b) <= maxwaves:
            bh, bp = a, b
    return bh, bp, _waves(K, bh), _waves(nt, bp)


def persist_tile_bytes(K, T):
    """persist_tile_bytes."""
    return ((K * T * 4 + 16) + 1023) & ~1023


def conflict_free(T):
    """conflict_free: gcd(T, 64) <= 2."""
    return bool(T & 1) or (T & 63) % 4 == 2


def dma_stage_bytes(nbytes, align):
    """dma_stage_bytes: the copy runs from the 16-byte boundary below the clip to the one above it; a start known only to `align`
    bytes can lie 16 - align bytes behind a boundary."""
    return (nbytes + (16 - align) + 15) & ~15


def dma_staged(K, T, ntiles, lds, align, env=None):
    """dma_staged: the block-split kernel stages a whole clip by LDS-DMA.  align: 16 / 8 / 4, the largest of them that divides both
    the input pointer and K T 4; 0: the pointer is not 4-byte aligned."""
    return (switches(env)["dma"] and ntiles == 1 and align != 0 and conflict_free(T)
            and dma_stage_bytes(K * T * 4, align) <= lds)


def _result(family, layout, ntiles=0, TT=0, nsh=0, nsp=0, stride=0, nwh=0, nwp=0, threads=0, lds=0, grid_x=0, grid_y=0, dma=0):
    return dict(family=family, layout=layout, ntiles=ntiles, TT=TT, nsh=nsh, nsp=nsp, stride=stride, nwh=nwh, nwp=nwp,
                threads=threads, lds=lds, grid_x=grid_x, grid_y=grid_y, dma=dma)


def _env_of(persist, env):
    env = dict(env or {})
    if persist is not None:
        env["SMH_MEDIAN_PERSIST"] = str(persist)
    return env


def launch_route(K, T, lh, lp, B, harm_layout, n_cu, persist=None, env=None, align=16):
    """plan_launch: persistent kernel, block-split kernel, else the delete/insert kernel, which has no blocked store (2 -> 1).
    `stride` is the row stride the kernel is given: T for the persistent kernel and a clip staged by DMA, else the tile's odd one."""
    env = _env_of(persist, env)
    sw = switches(env)
    if ((lh, lp) not in PAIRS) if (lh and lp) else ((lh, lp) not in SINGLES):
        raise Refused("no median kernel for (l_harm,l_perc)=(%d,%d)" % (lh, lp))
    p = make_plan(K, T, lh, lp, env)
    want_persist = (lh > 17 or lp > 17) if sw["persist"] is None else bool(sw["persist"])
    if not sw["nosplit"] and want_persist and lh and lp and (lh, lp, sw["pthreads"]) in PERSIST:
        if (p["ntiles"] == 1 and conflict_free(T) and 2 * persist_tile_bytes(K, T) <= LDS_BYTES_PER_CU and B >= 2 * n_cu):
            q = make_split_roles(K, T, lh, lp, sw["pthreads"] // 64, env)
            if q:
                return _result("persist", harm_layout, 1, p["TT"], q[0], q[1], T, q[2], q[3], sw["pthreads"],
                               2 * persist_tile_bytes(K, T), n_cu, 1)
    if not sw["nosplit"] and split_threads(lh, lp):
        q = make_split_roles(K, p["TT"], lh, lp, split_threads(lh, lp) // 64, env)
        if q:
            dma = int(dma_staged(K, T, p["ntiles"], p["lds"], align, env))
            return _result("split", harm_layout, p["ntiles"], p["TT"], q[0], q[1], T if dma else p["stride"], q[2], q[3],
                           split_threads(lh, lp), p["lds"], p["ntiles"], B, dma)
    return _result("delete_insert", 1 if harm_layout == 2 else harm_layout, p["ntiles"], p["TT"], p["nsh"], p["nsp"], p["stride"],
                   p["nwh"], p["nwp"], DELETE_INSERT_THREADS, p["lds"], p["ntiles"], B)


def check_args(name, B, K, T, w):
    """smh_median.hip check_args (the null-pointer requirement apart)."""
    if not (B >= 0 and K >= 1 and T >= 1):
        raise Refused("%s: bad shape B=%d K=%d T=%d" % (name, B, K, T))
    if not (1 <= w <= MAX_MEDIAN and w & 1):
        raise Refused("%s: window must be odd in [1,%d], got %d" % (name, MAX_MEDIAN, w))
    if B > MAX_BATCH:
        raise Refused("%s: B=%d exceeds the grid limit; split the batch" % (name, B))


def time_route(K, T, lh, B, n_cu, persist=None, env=None, align=16):
    """plan_time, the decision of smh_median_time_f32."""
    if lh == 1:
        return _result("copy", 0)
    if not fast_ok(T, lh):
        return _result("small", 0)
    return launch_route(K, T, lh, 0, B, 0, n_cu, persist, env, align)


def freq_route(K, T, lp, B, n_cu, persist=None, env=None, align=16):
    """plan_freq, the decision of smh_median_freq_f32."""
    if lp == 1:
        return _result("copy", 0)
    if not fast_ok(K, lp):
        return _result("small", 0)
    return launch_route(K, T, 0, lp, B, 0, n_cu, persist, env, align)


def pair_fused(K, T, lh, lp):
    """pair_fused: both filters in one launch."""
    return fast_ok(T, lh) and fast_ok(K, lp) and (lh, lp) in PAIRS


def rag_tile(K, lh, lp, env=None):
    """rag_tile_frames: (frames, row stride) of the ragged launch's tile -- a multiple of 4 frames, at least 2 (l_harm // 2) + 8,
    whose halo columns fit the budget of two workgroups per CU -- or None."""
    if switches(env)["nosplit"] or not (lh and lp) or not split_threads(lh, lp):
        return None
    hh = lh // 2
    TT = (_odd_cols((LDS_BYTES_PER_CU // 2 - 1024) // 4, K) - 2 * hh) & ~3
    return (TT, (TT + 2 * hh) | 1) if TT >= 2 * hh + 8 else None


def rag_route(K, lh, lp, n_items, env=None):
    """plan_rag: the block-split kernel on (clip, tile) items, layout 2, the per-XCD grid of 8 ceil(n / 8) workgroups."""
    tile = rag_tile(K, lh, lp, env)
    q = tile and make_split_roles(K, tile[0], lh, lp, split_threads(lh, lp) // 64, env)
    if not q:
        raise Refused("ragged medians: no block-split kernel for (l_harm,l_perc)=(%d,%d), K=%d" % (lh, lp, K))
    return _result("split", 2, 0, tile[0], q[0], q[1], tile[1], q[2], q[3], split_threads(lh, lp), K * tile[1] * 4,
                   8 * ((n_items + 7) // 8), 1)


def blocked_harm_ok(K, T, lh, lp, env=None):
    """blocked_harm_ok: the pair is fused and the block-split kernel covers a tile, whatever B."""
    if switches(env)["nosplit"] or not pair_fused(K, T, lh, lp) or not split_threads(lh, lp):
        return False
    try:
        p = make_plan(K, T, lh, lp, env)
    except Refused:
        return False
    return make_split_roles(K, p["TT"], lh, lp, split_threads(lh, lp) // 64, env) is not None


def route(entry, K, T, lh, lp, B, harm_layout, n_cu, persist=None, env=None, align=16):
    """The plan of one call as a dict of FIELDS.  entry: one of ALL_ENTRIES; arguments the entry does not have are ignored ('rag':
    B is the item count).  family 'two_singles' (one launch per filter, layout 0), 'copy' and 'small' carry nothing else.  B == 0
    launches nothing: family None, the requested layout.  Raises Refused where the call returns SMH_E_INVALID."""
    if entry == "rag":
        return rag_route(K, lh, lp, B, env) if B > 0 else _result(None, 2)
    name = {"hpss_ex": "smh_hpss_median_ex_f32", "time_ex": "smh_median_time_ex_f32", "hpss": "smh_hpss_median_f32",
            "time": "smh_median_time_f32", "freq": "smh_median_freq_f32"}[entry]
    pair = entry in ("hpss_ex", "hpss")
    if entry == "freq":
        lh = 0
    elif not pair:
        lp = 0
    if entry in ("hpss", "time", "freq"):
        harm_layout = 0
    check_args(name, B, K, T, lp if entry == "freq" else lh)
    if pair:
        check_args(name, B, K, T, lp)
    if harm_layout not in (0, 1, 2):
        raise Refused("%s: harm_layout must be 0, 1 or 2" % name)
    if B == 0:
        return _result(None, harm_layout)
    if entry == "freq":
        return freq_route(K, T, lp, B, n_cu, persist, env, align)
    if pair:  # plan_hpss_ex
        if pair_fused(K, T, lh, lp):
            return launch_route(K, T, lh, lp, B, harm_layout, n_cu, persist, env, align)
        # one launch per filter: either may still be refused
        time_route(K, T, lh, B, n_cu, persist, env, align)
        freq_route(K, T, lp, B, n_cu, persist, env, align)
        return _result("two_singles", 0)
    if entry == "time_ex" and not (lh == 1 or not fast_ok(T, lh) or harm_layout == 0):  # plan_time_ex
        return launch_route(K, T, lh, 0, B, harm_layout, n_cu, persist, env, align)
    return time_route(K, T, lh, B, n_cu, persist, env, align)


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
