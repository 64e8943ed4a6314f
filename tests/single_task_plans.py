"""Python restatement of the launch plan of the single-task model's head kernel (sm_hpss_mtl_amd/csrc/smh_train_single.hip:
launch_single_head_train) -- TEST INFRASTRUCTURE, like tests/heads_plans.py, and like it a part of tests/train_plans.py, which
tests/test_train_plan_gpu.py holds to the library.  It computes no numbers.

The kernel has ONE instantiation: one workgroup of kTh = 512 threads, a sample per lane, no staged tile.  What a batch size changes
is the number of passes over the per-wave accumulator rows -- the first pass assigns them, every later one adds to them -- so the
plan is (threads, passes) and it moves where N crosses a multiple of 512."""
from __future__ import annotations

K_TH = 512  # smh_train_single.hip: kTh


def plan(N):
    return (K_TH, (N + K_TH - 1) // K_TH)


def change_points(n_max):
    """Every N in [2, n_max] whose plan differs from N - 1's, each together with its predecessor."""
    out = []
    for n in range(2, n_max + 1):
        if plan(n) != plan(n - 1):
            out += [n - 1, n]
    return out


# The cases of tests/test_single_task_gpu.py: (N, n_classes, nb_stacks, Nd, W), the three class counts spread over the batch sizes.
# The trunk's gradient is discontinuous at every relu gate and at every tie of the channel maximum, and a float32 forward takes the
# other branch than the float64 reference on a fraction ~ 1e-7 of them (tests/test_training_gpu.py, tests/test_model_shapes_gpu.py:
# one such gate moves single elements by up to 1e-2 of a tensor's maximum, which is why those tests widen their element bound to
# 1e-2 from 100 patches on).  Measured here: a float32 torch evaluation of the reference graph itself, 24 blocks and W = 68, misses
# the float64 one by 4e-3 .. 1.3e-2 of a tensor's maximum in 5 of 55 seeded cases -- about one gate in 5e6 -- and the device's
# float32 forward did so at N = 65 (6.6e-5 on a tensor whose maximum is 7.4e-3).  This test keeps 2e-3 at every N, so it keeps the
# number of gates, N x W x 32 x blocks, small: the reference's trunk (24 blocks, W = 68) at 1 and 5 patches, one block elsewhere,
# with W = 25 from 63 patches on -- 1.7e6 gates over all cases.  What changes with N is the head kernel, which neither the depth
# of the trunk nor W enters; the 24-block trunk backward at hundreds of patches is the subject of the two files named above.
# tests/test_single_task_ref.py holds every case to a tenth of the bound in a float32 evaluation of the reference graph itself.
TRAIN_CASES = [(1, 2, 3, 8, 68), (2, 3, 1, 1, 68), (3, 5, 1, 1, 68), (4, 2, 1, 1, 68), (5, 3, 3, 8, 68), (63, 5, 1, 1, 25),
               (64, 2, 1, 1, 25), (65, 3, 1, 1, 25), (510, 2, 1, 1, 25), (512, 5, 1, 1, 25), (513, 2, 1, 1, 25)]
TRAIN_SEED = 5000  # train_problem draws case N from default_rng(TRAIN_SEED + N)
