"""The case table of the silence-removal and signal-conditioning edge tests -- TEST INFRASTRUCTURE, a plain host-only module like
tests/cnn_plans.py and tests/heads_cases.py: tests/test_silence_cases.py (no GPU), tests/test_silence_edges_gpu.py and
tests/golden/make_silence_runs_golden.py import it, and none of them imports another test module.

It holds
  (a) CRAFTED: energies written frame by frame for `remove_silence` (which takes the energy as an input), each with the claim it
      is there for -- the branch of find_runs / compacted_index (smh_silence.hip: the rules that silence_runs_kernel,
      silence_compact_kernel and preprocess_fused_kernel call) that no audio clip reaches on purpose;
  (b) AUDIO: clips for `preprocess_signal` at the lengths where its route or its load path changes, and at other frame parameters;
  (c) MIXED_BATCH: one batch of clips with different outcomes;
  and the route arithmetic of smh_preprocess_signal_f32 restated from the source.
"""
from __future__ import annotations

import hashlib
from collections import namedtuple

import numpy as np

from oracle import silence as osil

LOUD, QUIET = np.float32(1.0), np.float32(1e-4)
KCHUNK = 8192  # samples per workgroup of the streaming kernels (smh_silence.hip: kChunk)


def frame_params(fs, Tw, Ts):
    """(frame size, frame shift) in samples: tools.pyx:88-89, int((T * fs) / 1000)."""
    return int((Tw * fs) / 1000), int((Ts * fs) / 1000)


def n_frames(N, fs, Tw, Ts):
    """Frame count of librosa.feature.rms (centre=True) for these parameters; 1 + N // hop for an even frame."""
    frame, hop = frame_params(fs, Tw, Ts)
    return 1 + (N + 2 * (frame // 2) - frame) // hop


# ---- route arithmetic of smh_preprocess_signal_f32 (restated from smh_silence.hip: plan_frames / CondPlan) ------------------
FUSED_MAX_N = 36000
LDS_BUDGET = 155 * 1024


def lds_bytes(N, frame, hop):
    """Dynamic LDS of preprocess_fused_kernel (CondPlan::lds): samples rounded up to a multiple of 4, energies (float), run table (maxrun x 3 int),
    raw and filtered frame markers (bytes)."""
    nF = 1 + (N + 2 * (frame // 2) - frame) // hop
    maxrun = nF // 2 + 2
    return ((N + 3) & ~3) * 4 + nF * 4 + maxrun * 12 + 2 * nF


def route(N, fs, Tw, Ts, multipass=False):
    """1 = the clip-in-LDS kernel, 0 = the multi-pass path."""
    frame, hop = frame_params(fs, Tw, Ts)
    return int(N <= FUSED_MAX_N and not multipass and lds_bytes(N, frame, hop) <= LDS_BUDGET)


# ---- (a) crafted energies ----------------------------------------------------------------------------------------------------------
# claim: what the case is there for, as facts that tests/test_silence_cases.py asserts with the oracle alone:
#   runs       the removed [k, l) in order (the runs that pass beta -- also when fewer than two pass and nothing is removed)
#   n_runs     len(runs), where listing 83 runs would say nothing more
#   kept       number of retained samples when the clip is compacted
#   untouched  True: fewer than two runs, the input comes back as is
#   straddles  a sample index s with k < s < l for some run
#   moves      (source sample, destination sample) of a kept sample that crosses a chunk boundary of the compaction
#   fmark      {frame: value} of the median-filtered frame marker
Crafted = namedtuple("Crafted", "name N fs Tw Ts alpha beta energy claim")


def _energy(nF, silent, loud=LOUD, quiet=QUIET):
    e = np.full(nF, loud, np.float32)
    for a, b in silent:  # frames [a, b)
        e[a:b] = quiet
    return e


def _case(name, N, silent, claim, fs=16000, Tw=25, Ts=10, alpha=0.025, beta=0.075, nF=None, edit=None):
    e = _energy(n_frames(N, fs, Tw, Ts) if nF is None else nF, silent)
    if edit is not None:
        edit(e)
    return Crafted(name, N, fs, Tw, Ts, alpha, beta, e, claim)


def _many(N, phase):
    nF = n_frames(N, 16000, 25, 10)
    return [(t, t + 1) for t in range(nF) if (t + phase) % 12 < 9]


THRESH = np.float32(0.025)  # float32(alpha * max energy) for max energy 1.0
BELOW = np.nextafter(THRESH, np.float32(0))


def _tie(e):
    e[20:35] = THRESH  # equal to the threshold: loud (>=)
    e[60:75] = BELOW   # one ulp below: silent


def _set(frames, value):
    def edit(e):
        for a, b in frames:
            e[a:b] = value
    return edit


CRAFTED = [
    # -- (32000, 25, 10): frame 400, hop 160, 201 frames; four chunks of 8192 samples
    _case("straddle_8192", 32000, [(40, 60), (110, 125)],
          dict(runs=[(6640, 9840), (17840, 20240)], kept=26400, straddles=8192, moves=(16384, 13184))),
    _case("straddle_16384_24576", 32000, [(95, 110), (148, 160)],
          dict(runs=[(15440, 17840), (23920, 25840)], kept=27680, straddles=16384, moves=(25840, 21520))),
    # frames 0, 1 and the last two alone are loud: the zero padding of medfilt(., 5) turns them silent.  Isolated single (40) and
    # double (50, 51) silent frames vanish; so does the single loud frame 95 inside silence.
    _case("medfilt_ends", 32000, [(2, 20), (40, 41), (50, 52), (80, 95), (96, 111), (181, 199)],
          dict(runs=[(240, 3440), (13040, 18000), (29200, 32000)], kept=21040,
               fmark={0: 0, 1: 0, 2: 0, 19: 0, 20: 1, 40: 1, 50: 1, 51: 1, 95: 0, 111: 1, 180: 1, 199: 0, 200: 0})),
    # -- (160000, 25, 10): 1001 frames, twenty chunks, dozens of runs
    _case("many_runs", 160000, _many(160000, 0), dict(n_runs=83, kept=40480)),
    _case("many_runs_phase5", 160000, _many(160000, 5), dict(n_runs=82, kept=41920)),
    _case("two_long_runs", 160000, [(100, 400), (600, 990)], dict(runs=[(16240, 64240), (96240, 158640)], kept=49600)),
    # -- (16000, 5, 10): frame 80 below the shift 160
    _case("k_clamped_to_1", 16000, [(0, 12), (50, 63)], dict(runs=[(1, 1840), (7920, 10000)], kept=12081), Tw=5),
    # the last frame stops the silent loop without being consumed: l = 160 * 99 + 80 = 15920 < N, the last 80 samples stay
    _case("short_frame_ends_in_silence", 16000, [(30, 45), (85, 101)], dict(runs=[(4720, 7120), (13520, 15920)], kept=11200), Tw=5),
    _case("short_frame_starts_in_sound", 16000, [(3, 14), (40, 52)], dict(runs=[(400, 2160), (6320, 8240)], kept=12320), Tw=5),
    # -- (16000, 25, 10): 101 frames
    _case("k_not_clamped", 16000, [(0, 12), (50, 63)], dict(runs=[(240, 2160), (8240, 10320)], kept=12000)),
    _case("l_clamped_to_N", 16000, [(20, 36), (90, 101)], dict(runs=[(3440, 6000), (14640, 16000)], kept=12080)),
    _case("ends_in_sound", 16000, [(30, 42), (85, 98)], dict(runs=[(5040, 6960), (13840, 15920)], kept=12000, fmark={98: 1, 100: 1})),
    _case("starts_in_sound", 16000, [(3, 15), (60, 75)], dict(runs=[(720, 2640), (9840, 12240)], kept=11680, fmark={0: 1, 2: 1, 3: 0})),
    # one stretch AT the float threshold (loud), one an ulp below (silent): one run, nothing removed
    _case("thresh_tie", 16000, [], dict(runs=[(9840, 12240)], untouched=True, fmark={20: 1, 34: 1, 60: 0, 74: 0}), edit=_tie),
    # three stretches of 5, 12 and 6 frames: only the second passes beta
    _case("one_of_many", 16000, [(10, 15), (40, 52), (80, 86)], dict(runs=[(6640, 8560)], untouched=True, fmark={12: 0, 45: 0, 83: 0})),
    _case("all_loud", 16000, [], dict(runs=[], untouched=True)),
    # threshold 0: every frame is marked, no run
    _case("all_zero_energy", 16000, [], dict(runs=[], untouched=True, fmark={0: 1, 50: 1, 100: 1}), edit=_set([(0, 101)], 0.0)),
    # -- (16000, 25, 5): hop 80, 201 frames; beta * fs = 1200 samples = 15 frames exactly
    _case("beta_exact", 16000, [(30, 45), (120, 135)], dict(runs=[], untouched=True, fmark={30: 0, 44: 0, 120: 0}), Ts=5),
    _case("beta_above", 16000, [(30, 46), (120, 136)], dict(runs=[(2720, 4000), (9920, 11200)], kept=13440), Ts=5),
    _case("beta_exact_between", 16000, [(10, 26), (60, 75), (120, 136)], dict(runs=[(1120, 2400), (9920, 11200)], kept=13440), Ts=5),
    # -- alpha = 0.1, beta = 0.2: energy 0.05 is silent here (loud at 0.025); 3200 samples = 20 frames must be exceeded
    _case("alpha_beta", 16000, [], dict(runs=[(1840, 5840), (9840, 13840)], kept=8000, fmark={10: 0, 45: 0, 60: 0}),
          alpha=0.1, beta=0.2, edit=_set([(10, 35), (40, 55), (60, 85)], 0.05)),
    _case("alpha_beta_exact", 16000, [], dict(runs=[(8240, 12240)], untouched=True), alpha=0.1, beta=0.2,
          edit=_set([(10, 30), (50, 75)], 0.05)),
    _case("alpha_beta_quiet_is_loud", 16000, [], dict(runs=[], untouched=True, fmark={20: 1}), alpha=0.1, beta=0.2,
          edit=_set([(10, 40), (50, 90)], 0.1)),
    # -- nFrames = 100, one less than 1 + N / hop (the C ABI takes any nFrames up to that)
    _case("fewer_frames", 16000, [(20, 36), (90, 100)], dict(runs=[(3440, 6000), (14640, 16000)], kept=12080), nF=100),
    _case("fewer_frames_ends_in_sound", 16000, [(30, 42), (85, 97)], dict(runs=[(5040, 6960), (13840, 15760)], kept=12160), nF=100),
    _case("fewer_frames_all_loud", 16000, [], dict(runs=[], untouched=True), nF=100),
]
CRAFTED_BY_NAME = {c.name: c for c in CRAFTED}


def crafted_signal(c: Crafted) -> np.ndarray:
    """Seeded noise, float32, |x| < 1.6: the samples carry no decision here (the energy is an input), only their positions."""
    seed = 2000 + [k.name for k in CRAFTED].index(c.name)
    return (0.3 * np.random.default_rng(seed).standard_normal(c.N)).astype(np.float32)


def shape_key(c: Crafted):
    return (c.N, len(c.energy), c.fs, c.Tw, c.Ts, c.alpha, c.beta)


def neighbours(c: Crafted):
    """The two cases that follow `c` (cyclically) among those of its shape and parameters: rows 0 and 2 of the batch of three."""
    group = [k for k in CRAFTED if shape_key(k) == shape_key(c)]
    assert len(group) >= 3, c.name
    i = group.index(c)
    return group[(i + 1) % len(group)], group[(i + 2) % len(group)]


def oracle_remove(c: Crafted, x=None):
    x = crafted_signal(c) if x is None else x
    return (x,) + tuple(osil.remove_silence(x, c.energy, c.fs, c.Tw, c.Ts, c.alpha, c.beta))


def sha(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


# ---- (b) audio ---------------------------------------------------------------------------------------------------------------------
# gaps as fractions of the clip length (the lengths run from 201 to 44101 samples)
GAPS = {
    "two_runs": ((0.10, 0.35), (0.55, 0.80)),
    "one_run": ((0.40, 0.70),),
    "both_ends": ((0.0, 0.25), (0.40, 0.60), (0.75, 1.0)),
    "ends_in_silence": ((0.20, 0.40), (0.80, 1.0)),
    "none": (),
}
Audio = namedtuple("Audio", "name fs Tw Ts lengths gaps")
AUDIO = [
    # 36000 / 36001: N <= kFusedMaxN decides; 35998 / 35999 / 36001 / 8193: the float4 load needs N % 4 == 0 (remainders 2, 3, 1, 1)
    Audio("a16k_two_runs", 16000, 25, 10, [36000, 36001, 35998, 35999, 8193, 201], "two_runs"),
    Audio("a16k_both_ends", 16000, 25, 10, [36000, 36001, 35998, 35999], "both_ends"),
    Audio("a16k_one_run", 16000, 25, 10, [36000, 35999, 8193], "one_run"),
    Audio("a16k_ends_in_silence", 16000, 25, 10, [36001, 35998, 201], "ends_in_silence"),
    # hop 16: the LDS budget decides, 33408 is the last length inside it
    Audio("hop16_two_runs", 16000, 25, 1, [33408, 33409], "two_runs"),
    Audio("hop16_ends_in_silence", 16000, 25, 1, [33408, 33409], "ends_in_silence"),
    # frame 551 (odd): 1 + (N - 1) // hop frames
    Audio("f22k_both_ends", 22050, 25, 10, [22050, 44101], "both_ends"),
    Audio("f22k_one_run", 22050, 25, 10, [22050, 44101], "one_run"),
    Audio("f8k_two_runs", 8000, 30, 15, [8000], "two_runs"),
    Audio("f8k_ends_in_silence", 8000, 30, 15, [8000], "ends_in_silence"),
    # frame 80 below the shift 160: samples between frames enter no energy
    Audio("short_frame_both_ends", 16000, 5, 10, [16000], "both_ends"),
    Audio("short_frame_one_run", 16000, 5, 10, [16000], "one_run"),
]
AUDIO_PARAMS = [(a, n) for a in AUDIO for n in a.lengths]


def audio_id(p):
    return "%s-N%d" % (p[0].name, p[1])


def make_clip(n, fs, gaps, seed):
    """Built like sm_hpss_mtl_amd.synth.gappy_clip: noise x sawtooth envelope, gaps x 1e-4, plus a DC offset of 0.01."""
    del fs
    rng = np.random.default_rng(seed)
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x *= (0.75 + 0.5 * ((np.arange(n) % 4000) / 4000.0)).astype(np.float32)
    for a, b in gaps:
        x[int(a * n):int(b * n)] *= np.float32(1e-4)
    return x + np.float32(0.01)


def audio_clip(a: Audio, n: int) -> np.ndarray:
    return make_clip(n, a.fs, GAPS[a.gaps], 3000 + 10 * AUDIO.index(a) + a.lengths.index(n))


# ---- (c) the mixed batch ------------------------------------------------------------------------------------------------------------
MIXED_N, MIXED_FS, MIXED_TW, MIXED_TS = 16000, 16000, 25, 10
MIXED_BATCH = [("removed", "two_runs"), ("untouched", "one_run"), ("none", "none"), ("removed", "ends_in_silence"),
               ("both ends", "both_ends"), ("untouched", "one_run"), ("removed", "two_runs"), ("none", "none")]
MIXED_REPEAT = 17  # 8 x 17 = 136 clips


def mixed_batch() -> np.ndarray:
    return np.stack([make_clip(MIXED_N, MIXED_FS, GAPS[g], 5000 + i) for i, (_, g) in enumerate(MIXED_BATCH)])


# ---- what the oracle says about a clip ---------------------------------------------------------------------------------------------
def audio_facts(raw, fs, Tw, Ts, alpha=0.025, beta=0.075):
    """dict(n_keep, n_runs, runs, candidates, energy_margin, beta_margin_hops) from oracle/silence.py alone.
    energy_margin: min |energy - thresh| / thresh over the frames; beta_margin_hops: min over the CANDIDATE runs (every silent
    stretch, qualifying or not) of |(l - k) - beta * fs| in frame shifts."""
    frame, hop = frame_params(fs, Tw, Ts)
    xn = osil.normalize_signal(np.asarray(raw, np.float32))
    e = osil.rms(xn, frame, hop)
    thresh = np.float32(float(alpha) * float(np.max(e)))
    out, sm, fm, _ = osil.remove_silence(xn, e, fs, Tw, Ts, alpha, beta)
    runs = osil.silence_runs(fm, len(xn), fs, Tw, Ts, beta)
    cand = osil.silence_runs(fm, len(xn), fs, Tw, Ts, -np.inf)
    return dict(n_keep=len(xn) if out is xn else int(sm.sum()), n_runs=len(runs), runs=runs, candidates=cand,
                energy_margin=float(np.min(np.abs(e.astype(np.float64) - float(thresh))) / float(thresh)),
                beta_margin_hops=min(abs((l - k) - beta * fs) / hop for k, l in cand))


ENERGY_MARGIN_MIN = 1e-2   # float32 sums of <= 720 squares in another order move an energy by < 1e-5 relative
BETA_MARGIN_MIN_HOPS = 1.0
