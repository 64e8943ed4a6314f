"""Python restatement of the launch plans of the TCN models' heads-training kernels (sm_hpss_mtl_amd/csrc/smh_train.hip:
launch_heads_train, B3_MTL and intermediate fusion; smh_train_cascade.hip: launch_cascade_heads_train) -- TEST INFRASTRUCTURE.

It computes no numbers: it only says which instantiation of a heads kernel a batch of N patches takes, so that
tests/test_heads_plans.py can show that every case of tests/test_heads_plans_gpu.py reaches the plan it is named for.  Each
function cites the C++ it copies (today: plan_heads in smh_train_plan.h, which those launchers execute).  It is the heads part of
tests/train_plans.py, which tests/test_train_plan_gpu.py holds to the library's own answer: a threshold that moves there without
moving here fails that test, and the hand-computed boundary pins of tests/test_heads_plans.py then say which cases have moved off
the path they were chosen for.
"""
from __future__ import annotations

K_HIDDEN = 16                     # smh_model.h: kHidden, the Dense(16) of every head
MTL_STAGE_BYTES = 122 * 1024      # smh_train_plan.h: kHeadsStageBytes
CASCADE_STAGE_BYTES = 120 * 1024  # smh_train_plan.h: kCascadeStageBytes
KINDS = ("B3_MTL", "fusion", "cascaded")


def head_odims(n_classes):
    """oracle.b3_mtl.head_spec: S, M, (N,) R."""
    return [1, 1, 1, 3] if n_classes == 5 else [1, 1, 2]


def mtl_lds_bytes(n_classes, N):
    """launch_heads_train: the staged tile of `pre` (n_classes + 16 n_heads columns) and of the targets (out_dim columns), both at
    an odd row stride (`| 1`)."""
    od = head_odims(n_classes)
    nhc = n_classes + K_HIDDEN * len(od)
    out_dim = sum(od) + n_classes
    return 4 * (N * (nhc | 1) + N * (out_dim | 1))


def mtl_plan(n_classes, N, heads_global=False):
    """heads_train_kernel<STAGED, THREADS>: (\"staged\" | \"global\", 512 | 1024).  heads_global: SMH_HEADS_GLOBAL is set."""
    staged = mtl_lds_bytes(n_classes, N) <= MTL_STAGE_BYTES and not heads_global
    return ("staged" if staged else "global", 512 if N <= 512 else 1024)


def cascade_lds_bytes(N):
    """launch_cascade_heads_train: (lds_sm, lds_r) = 4 (N (2 * 16 + 1) + N), 4 (N (16 + 1) + 2 N)."""
    return 4 * (N * (2 * K_HIDDEN + 1) + N), 4 * (N * (K_HIDDEN + 1) + 2 * N)


def cascade_plan(N):
    """{\"sm\": cascade_sm_kernel<STAGED>, \"r\": cascade_r_kernel<STAGED>} as \"staged\" | \"global\"; n_classes does not enter
    (the '3C' workgroup reads global memory either way)."""
    sm, r = cascade_lds_bytes(N)
    return {"sm": "staged" if sm <= CASCADE_STAGE_BYTES else "global", "r": "staged" if r <= CASCADE_STAGE_BYTES else "global"}


def plan(kind, n_classes, N, heads_global=False):
    """The plan of every heads kernel of one training step: {\"heads\": (form, threads)} for B3_MTL and fusion (one kernel, the
    same launch code), {\"sm\": form, \"r\": form} for the cascaded model."""
    if kind not in KINDS:
        raise ValueError(kind)
    if kind == "cascaded":
        if heads_global:
            raise ValueError("the cascaded heads have no switch")
        return cascade_plan(N)
    return {"heads": mtl_plan(n_classes, N, heads_global)}


def plan_name(kind, n_classes, N, heads_global=False):
    """The name a GPU case carries: 'staged512' / 'global512' / 'staged1024' / 'global1024', cascaded 'sm_<form>+r_<form>'."""
    p = plan(kind, n_classes, N, heads_global)
    if kind == "cascaded":
        return "sm_%s+r_%s" % (p["sm"], p["r"])
    return "%s%d" % p["heads"]
