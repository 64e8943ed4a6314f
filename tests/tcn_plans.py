"""Python restatement of how the network forward of N patches of T frames is launched (sm_hpss_mtl_amd/csrc/smh_tcn.hip:
plan_forward behind launch_forward, smh_internal_tcn_plan and smh_internal_tcn_schedule) -- TEST INFRASTRUCTURE.

It computes no numbers: patches per workgroup, LDS rows and bytes, column tiles, waves, the kernel's schedule and the split last
tile, from the shape and the SMH_TCN_* switches alone.  tests/test_tcn_plans.py pins it against values worked out by hand (no GPU)
and shows which plan branch every case of the existing GPU tests reaches; tests/test_tcn_plan_gpu.py holds the library's own plan
against it.  Each step cites the C++ it restates: a threshold that moves there must move here, and the pins then say which cases
have left the path they were chosen for.
"""
from __future__ import annotations

import re
from collections import namedtuple

SX = 36                 # smh_model.h: LDS row stride of x in floats
MAX_G = 16              # kMaxG: patches per workgroup <= MFMA N
PS = 80                 # kPS: row stride of the Dense-on-trunk outputs
BLOCK_FLOATS = 24 * 2 * 64 + 8 * 2 * 64 + 32 + 32   # kBlockFloats: one block's packed weights
WEIGHT_RING = 4         # smh_tcn.hip: kWeightRing, LDS block slots of the 16-wave lab form
NET_LDS_LIMIT = 156 * 1024   # kNetLdsLimit
ONE_SET, PREFETCH, SKEW, SKEW16 = 0, 1, 2, 3    # smh_tcn.hip: the MODE template argument of b3mtl_forward_kernel
MODE_NAMES = {ONE_SET: "one-set", PREFETCH: "prefetch", SKEW: "skew", SKEW16: "skew16"}
SWITCHES = ("SMH_TCN_G", "SMH_TCN_SKEW", "SMH_TCN_WAVES", "SMH_TCN_PREFETCH", "SMH_TCN_SPLIT", "SMH_TCN_SKEW16")

Plan = namedtuple("Plan", "G GRP units nwaves mode wlds split_last lds")


class Refused(Exception):
    pass


def _atoi(s):
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


def _round16(n):
    return (n + 15) // 16 * 16


def group(T, F, N, env=None):
    """(G, GRP): patches and LDS rows per workgroup."""
    env = env or {}
    gmax = max(1, min(272 // T, MAX_G))            # up to 272 rows (17 column tiles), at most one MFMA tile of patches
    G = max(1, min((N + 255) // 256, gmax))        # ceil(N / 256): as few workgroups as CUs when the batch allows it
    if "SMH_TCN_G" in env and 1 <= _atoi(env["SMH_TCN_G"]) <= gmax:
        G = _atoi(env["SMH_TCN_G"])
    GRP = _round16(G * T)
    head_scratch = 8 * 4 * 128 + MAX_G * PS        # Dense partial sums + pre[kMaxG][kPS] live in one activation buffer
    if GRP * SX < head_scratch:
        GRP = -(-head_scratch // SX)
    FQ = (F + 3) // 4
    if GRP * SX < FQ * 2 * 64:                     # the layer-0 A operands are staged there
        GRP = -(-FQ * 2 * 64 // SX)
    return G, _round16(GRP)


def plan(T, F, n_blocks, N, train=False, env=None, lab=False):
    """The plan of a forward of N patches (T frames, F features, n_blocks residual blocks) as Plan(G, GRP, units, nwaves, mode,
    wlds, split_last, lds), or Refused.  env: the SMH_TCN_* switches that are set; lab: a lab build, which alone reads
    SMH_TCN_SKEW16."""
    env = env or {}
    G, GRP = group(T, F, N, env)
    lds_x = 4 * 2 * (GRP + 1) * SX                 # x and y, each with its zero row
    lds_w = 4 * 2 * BLOCK_FLOATS                   # two weight slots
    lds_xch = 4 * (2 * 64 * 4 + 4)                 # the exchange area of the split last tile
    wlds = 1 if lds_x + lds_w + lds_xch <= NET_LDS_LIMIT else 0
    lds = lds_x + (lds_w + lds_xch if wlds else 0)
    if lds > NET_LDS_LIMIT:
        raise Refused("patch_size %d too long for the LDS-resident TCN" % T)
    units = (min(G, N) * T + 15) // 16
    nwaves = 8                                     # the fewest of 8..12 waves that minimise ceil(tiles / waves), without slots only
    for w in range(9, 13):
        if not wlds and -(-units // w) < -(-units // nwaves):
            nwaves = w
    if "SMH_TCN_WAVES" in env:
        nwaves = max(4, min(12, _atoi(env["SMH_TCN_WAVES"])))
    prefetch = nwaves <= 8 and bool(wlds)
    if "SMH_TCN_PREFETCH" in env:
        prefetch = prefetch and _atoi(env["SMH_TCN_PREFETCH"]) != 0
    skew_ok = bool(wlds) and 1 <= units <= 32 and n_blocks * units < 2048 and T >= 16
    skew = skew_ok and units >= 12 and 8 * ((units + 7) // 8) - units >= 3 and units != 13
    if "SMH_TCN_SKEW" in env:
        v = _atoi(env["SMH_TCN_SKEW"])
        skew = skew_ok if v == 2 else (skew and v != 0)
    if skew and "SMH_TCN_WAVES" not in env:
        nwaves = 8
    if skew:
        nwaves = min(nwaves, 8)
    lds16 = 4 * (2 * (GRP + 1) * SX + WEIGHT_RING * BLOCK_FLOATS + 128)
    skew16 = lab and _atoi(env.get("SMH_TCN_SKEW16", "0")) != 0 and skew and not train and lds16 <= NET_LDS_LIMIT
    if skew16:
        nwaves, lds = 16, lds16
    split_last = int(not skew and prefetch and nwaves == 8 and units >= 2 and units % 8 in (1, 5))
    if "SMH_TCN_SPLIT" in env:
        split_last = int(bool(split_last) and _atoi(env["SMH_TCN_SPLIT"]) != 0)
    mode = SKEW16 if skew16 else SKEW if skew else PREFETCH if prefetch else ONE_SET
    return Plan(G, GRP, units, nwaves, mode, wlds, split_last, lds)

