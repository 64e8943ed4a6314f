"""Python restatement of the launch plan of one TCN training step (sm_hpss_mtl_amd/csrc/smh_train_plan.h: plan_train) -- TEST
INFRASTRUCTURE.  It computes no numbers: it says which forward, which heads kernels in which form, which trunk backward on which
grid with how much LDS, and which small kernels around it a step of N patches takes.

The heads part is tests/heads_plans.py and tests/single_task_plans.py, imported here; the backward part is restated below from
the kernels' LDS layouts.  tests/test_train_plans.py pins the boundaries by hand; tests/test_train_plan_gpu.py holds every value
to the library's own answer (smh_internal_train_plan), so a threshold that moves in the header without moving here fails there.
"""
from __future__ import annotations

from tests import heads_plans as H
from tests import single_task_plans as S

C, SX, PS, HIDDEN = 32, 36, 80, 16          # smh_model.h: C, SX, kPS, kHidden
LDS_PER_CU = 160 * 1024                     # smh_common.h: kLdsBytesPerCU
NET_LDS_LIMIT = LDS_PER_CU - 4 * 1024       # smh_model.h: kNetLdsLimit
KINDS = ("B3_MTL", "cascaded", "fusion", "single")
FORWARDS = ("f32", "bf16", "trunk_pair")    # TrainForward
FAMILIES = ("mtl", "cascaded", "single")    # HeadsFamily
ROUTES = ("bf16", "mfma_short", "mfma_long", "scalar")   # BwdRoute (kBwdRefused: Refused here)
DWH = ("none", "mfma", "valu")              # DwhKind
SWITCHES = ("SMH_TRAIN_VALU", "SMH_BWD_BF16", "SMH_DWH_VALU", "SMH_HEADS_GLOBAL")
MFMA_SHORT_T, MFMA_LONG_T = 128, 256        # kMfmaMaxT, kMfmaLongT
SLOT_BYTES = 21 * 1024                      # kSlotBytes: ten hi units, the bias piece, ten lo units of 1 KiB
# the order of smh_internal_train_plan's ints (TrainPlanInts)
FIELDS = ("forward", "family", "h0_staged", "h0_threads", "h0_grid", "h0_lds", "h1_staged", "h1_threads", "h1_grid", "h1_lds",
          "route", "grid", "threads", "lds", "G", "K32", "RPm", "use_wt", "acts_last_only", "dtrunk_x", "dtrunk_y", "dwh", "dwh_x",
          "dwh_y", "dwh_z", "gt_patch_floats", "pack_bytes")


class Refused(Exception):
    pass


def head_shape(kind, n_classes):
    """(n_heads, out_dim) of a model kind (smh_model_create_heads)."""
    if kind == "single":
        return 0, n_classes
    if kind == "cascaded":           # always S, M, R[2]
        return 3, 4 + n_classes
    od = H.head_odims(n_classes)
    return len(od), sum(od) + n_classes


def heads(kind, n_classes, N, env=None):
    """The two HeadsLaunch of plan_heads as (staged, threads, grid, lds) each; the second is zeros unless cascaded."""
    env = env or {}
    none = (0, 0, 0, 0)
    if kind == "single":
        return "single", (0, S.plan(N)[0], 1, 0), none
    if kind == "cascaded":
        p, (sm, r) = H.cascade_plan(N), H.cascade_lds_bytes(N)
        st_sm, st_r = p["sm"] == "staged", p["r"] == "staged"
        return "cascaded", (int(st_sm), 512, 3, sm if st_sm else 0), (int(st_r), 512, 1, r if st_r else 0)
    form, threads = H.mtl_plan(n_classes, N, heads_global="SMH_HEADS_GLOBAL" in env)
    staged = form == "staged"
    return "mtl", (int(staged), threads, head_shape(kind, n_classes)[0] + 1, H.mtl_lds_bytes(n_classes, N) if staged else 0), none


def bf16_geo(T):
    """bwd_geo: (G patches per workgroup, K32, bytes per patch) of the split-bf16 backward, or None where the patch does not fit."""
    if T < 1 or T > 128:
        return None
    units = (T + 15) // 16
    K32 = (16 * units + 31) // 32
    sxt, st = 2 * (2 * 8 + 32 * K32) + 16, 2 * 32 * K32 + 16       # xT rows with their 8-frame halos; yT / gT / duT rows
    per_patch = 2 * 32 * sxt + 3 * 2 * 32 * st + 2 * (T + 1) * 80  # x | y, g, du transposed | du, each hi and lo
    per_patch = (per_patch + 15) // 16 * 16
    if 16 * units * SX * 4 > per_patch:
        return None
    G = 2 if 2 * per_patch + SLOT_BYTES <= LDS_PER_CU else 1
    if G * per_patch + SLOT_BYTES > LDS_PER_CU:
        return None
    return (G, K32, per_patch) if (G == 2 and K32 <= 3) or (G == 1 and K32 == 4) else None


def mfma(T):
    """plan_mfma: (route, lds, RPm) or Refused."""
    RPm = (T + 15) // 16 * 16
    tail = PS + C + 3 * SX + 4                                    # pre row, a channel row, the zero words
    lds_short, lds_long = 4 * (4 * RPm * SX + 4 * C * 36 + tail), 4 * (4 * RPm * SX + tail)
    if lds_short <= NET_LDS_LIMIT and T <= MFMA_SHORT_T:
        return "mfma_short", lds_short, RPm
    if lds_long <= NET_LDS_LIMIT and T <= MFMA_LONG_T:
        return "mfma_long", lds_long, RPm
    raise Refused("patch_size %d too long for the trunk backward (at most %d frames)" % (T, MFMA_LONG_T))


def scalar(T):
    """(lds, use_wt) of tcn_backward_kernel, or Refused."""
    kernels = 3 * C * C + C * C
    lds, use_wt = 4 * (4 * T * 33 + 2 * kernels + C + 3 * T + PS), 1
    if lds > NET_LDS_LIMIT:
        lds, use_wt = lds - 4 * kernels, 0
    if lds > NET_LDS_LIMIT:
        raise Refused("patch_size %d too long for the backward kernel (at most 264 frames)" % T)
    return lds, use_wt


def backward(kind, T, n_blocks, n_classes, N, dtype=0, env=None):
    """plan_backward as a dict of the backward FIELDS."""
    env = env or {}
    p = dict.fromkeys(FIELDS[FIELDS.index("route"):], 0)
    p["use_wt"] = 1
    if kind == "fusion":                     # each trunk: MFMA, fed by the fusion layers; no switch
        p["route"], p["lds"], p["RPm"] = mfma(T)
        p["grid"], p["threads"] = N, 512
        return p
    valu = "SMH_TRAIN_VALU" in env
    bf16_on = env.get("SMH_BWD_BF16", "1").strip() not in ("0", "+0", "-0", "00")
    geo = bf16_geo(T)
    D, n_heads = T * C, head_shape(kind, n_classes)[0]
    if dtype == 1 and not valu and bf16_on and geo:
        G, K32, per_patch = geo
        p.update(route="bf16", grid=(N + G - 1) // G, threads=512 * G, lds=G * per_patch + SLOT_BYTES, G=G, K32=K32, acts_last_only=1,
                 pack_bytes=n_blocks * SLOT_BYTES + N * D * 4)
    elif T <= MFMA_LONG_T and not valu:
        p["route"], p["lds"], p["RPm"] = mfma(T)
        p.update(grid=N, threads=512, gt_patch_floats=D)
    else:
        p["lds"], p["use_wt"] = scalar(T)
        p.update(route="scalar", grid=N, threads=1024)
        return p
    p.update(dtrunk_x=D // 16, dtrunk_y=max(1, min(8, (N + 15) // 16 // 16)))
    if "SMH_DWH_VALU" in env:
        p.update(dwh="valu", dwh_x=(D * HIDDEN + 255) // 256, dwh_y=(N + 15) // 16, dwh_z=1 + n_heads)
    else:
        p.update(dwh="mfma", dwh_x=(D // 16 + 3) // 4, dwh_y=1 + n_heads, dwh_z=8)
    return p


def plan(kind, T, n_blocks, n_classes, N, dtype=0, env=None):
    """The plan of one step as a dict over FIELDS (names, not enum values), or Refused: a patch too long for every backward kernel of
    the kind, or dtype 1 on a model that has no split-bf16 step (every kind but B3_MTL).  env: the switches that are set."""
    if kind not in KINDS:
        raise ValueError(kind)
    if dtype == 1 and kind != "B3_MTL":
        raise Refused("the split-bf16 training step has the B3_MTL heads only")
    p = {"forward": "trunk_pair" if kind == "fusion" else "bf16" if dtype == 1 else "f32"}
    p["family"], h0, h1 = heads(kind, n_classes, N, env)
    for i, h in enumerate((h0, h1)):
        p.update(zip(("h%d_staged" % i, "h%d_threads" % i, "h%d_grid" % i, "h%d_lds" % i), h))
    p.update(backward(kind, T, n_blocks, n_classes, N, dtype, env))
    p["dwh"] = p["dwh"] or "none"
    return p


def ints(p):
    """A plan in the form smh_internal_train_plan answers in."""
    enums = {"forward": FORWARDS, "family": FAMILIES, "route": ROUTES, "dwh": DWH}
    return tuple(enums[f].index(p[f]) if f in enums else int(p[f]) for f in FIELDS)


def ask_library(lib, model, N, dtype):
    """The library's own plan of a step of N patches of `model` (a handle) under the switches set now, as the ints of `ints`, or None
    where the library refuses the step.  smh_internal_train_plan is a test-only export, not in include/smh.h.  Needs the GPU."""
    import ctypes as C
    q = lib.smh_internal_train_plan
    q.restype, q.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int * len(FIELDS))]
    got = (C.c_int * len(FIELDS))()
    return tuple(got) if q(model, N, dtype, C.byref(got)) == 0 else None
