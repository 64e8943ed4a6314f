"""The case table of the LDS-image feature kernels' edge tests -- TEST INFRASTRUCTURE, a plain host-only module like
tests/silence_cases.py and tests/median_cases.py: tests/test_feature_cases.py (no GPU) shows that every case holds the condition it
is there for at every length it is used at, tests/test_feature_edges_gpu.py runs the cases through features_half_kernel,
features_clip_kernel and the two-kernel path (csrc/smh_feat.hip).

It holds
  (a) `blocked`: the harmonic median in the 16-frame blocked layout (harm_layout = 2) those kernels read;
  (b) `reference_from_parts`: the oracle behind the medians -- soft masks, mel, dB with the top-dB floor -- from a GIVEN (S, harm, perc).
      The kernels take the medians as inputs and do not care whether they are medians of S, so the cases write them freely;
  (c) CASES: crafted (S, harm, perc), each with a `premise`: counts computed from the inputs and the reference alone, which say that
      the case reaches the branch it was written for;
  (d) the lengths, and the LDS budget of smh_feat.h restated (`t_last`), which the GPU test holds against the library's predicate.
"""
from __future__ import annotations

import numpy as np

from oracle import frontend as ofe

TINY = np.float32(np.finfo(np.float32).tiny)
DEN_MIN = np.float32(2.0 ** -100)  # features_half_kernel: kDenMin, below it the wave takes the normalised mask
WAVE_FRAMES = 128                  # features_half_kernel: a lane is a PAIR of frames, a wave covers 128 frames of one bin
K_MIN = 201                        # the bin regions of `mixed` are written for the 201 bins of n_fft = 400

# patch geometry of the edge tests: two 16-frame layer-0 tiles, the second partial; every T below 20 is tiled
W, SHIFT = 20, 7
BASE_LENGTHS = (1, 2, 15, 16, 17, 33, 34, 98)

# ---- the LDS budget (smh_feat.h: clip_image_bytes, kClipImageLimit; smh_feat.hip: features_image_ok) ---------------------------------
CLIP_IMAGE_LIMIT = 158 * 1024


def clip_image_bytes(rows, T, with_l0):
    b = 4 * (2 * rows * (T | 1) + 3 * 2 * rows) + 128
    return b + (4 * 2 * rows * 32 if with_l0 else 0)


def t_last(rows, with_l0):
    """The last T the single-kernel path takes (None: none, layer 0 needs rows % 4 == 0 and rows <= 128).  Always odd: an even T
    pays for the odd row stride T | 1 = T + 1."""
    if with_l0 and (rows % 4 != 0 or rows > 128):
        return None
    ok = [T for T in range(1, 2049) if clip_image_bytes(rows, T, with_l0) <= CLIP_IMAGE_LIMIT]
    return ok[-1] if ok else None


def lengths(rows, with_l0):
    """BASE_LENGTHS that fit, T_last - 1 (even: features_half_kernel at a full image) and T_last (odd: features_clip_kernel)."""
    tl = t_last(rows, with_l0)
    if tl is None:
        return []
    return sorted({T for T in BASE_LENGTHS if T <= tl} | {T for T in (tl - 1, tl) if T >= 1})


# ---- (a) harm_layout = 2 ------------------------------------------------------------------------------------------------------------------
def harm_buffer_floats(K, T):
    """smh_harm_buffer_floats (smh_frontend.hip)."""
    return (T + 15) // 16 * 16 * K


def blocked(harm):
    """(B, K, T) -> (B, ceil(T / 16), K, 16), zero padded: frame t of bin k sits at [t // 16][k][t % 16]."""
    harm = np.asarray(harm, np.float32)
    B, K, T = harm.shape
    nb = (T + 15) // 16
    pad = np.zeros((B, K, nb * 16), np.float32)
    pad[:, :, :T] = harm
    out = np.ascontiguousarray(pad.reshape(B, K, nb, 16).transpose(0, 2, 1, 3))
    assert out[0].size == harm_buffer_floats(K, T)
    return out


def unblocked(hb, T):
    B, nb, K, _ = hb.shape
    return np.ascontiguousarray(hb.transpose(0, 2, 1, 3).reshape(B, K, nb * 16)[:, :, :T])


# ---- (b) the oracle behind the medians -------------------------------------------------------------------------------------------------------
def reference_from_parts(S, harm, perc, n_mels, log_db):
    """One clip, (K, T) each -> (2 * rows, T) float32: featuregram_from_S without its medians, with the functions of oracle/frontend.py
    in its order of operations."""
    S = np.asarray(S, np.float32)
    harm, perc = np.asarray(harm, np.float32), np.asarray(perc, np.float32)
    H, P = S * ofe.softmask(harm, perc), S * ofe.softmask(perc, harm)
    if n_mels:
        H, P = ofe.mel_project(H, n_mels), ofe.mel_project(P, n_mels)
    if log_db:
        H, P = ofe.power_to_db(H ** 2), ofe.power_to_db(P ** 2)
    return np.append(H, P, axis=0).astype(np.float32)


def feat_name(n_mels, log_db):
    return ("Log" if log_db else "") + ("Mel" if n_mels else "") + "HarmPercSpec"


# ---- (c) the cases ---------------------------------------------------------------------------------------------------------------------------
def _music_like(rng, K, T):
    """Log-normal magnitudes over about ten decades (1e-5 .. 1e5) with medians within a decade of them."""
    S = 10.0 ** np.clip(rng.normal(0.0, 1.7, (K, T)), -5.0, 5.0)
    harm = S * 10.0 ** rng.normal(0.0, 0.4, (K, T))
    perc = S * 10.0 ** rng.normal(0.0, 0.4, (K, T))
    return S.astype(np.float32), harm.astype(np.float32), perc.astype(np.float32)


def quiet_split(T):
    """The odd frame at which the quiet regions of `mixed` end / begin (the whole clip at T = 1)."""
    t1 = (T // 2) | 1
    return t1 if t1 < T else 1


def build_mixed(K, T, seed=0, edges=True, scale=1.0):
    """Bins (frames)          what
       10..19                  harm = perc = 0, S > 0: split_zeros
       30..39  (0 .. t1)       both medians * 1e-17: den < 2^-100 with Z >= FLT_MIN on most bins, the normalised mask with a real ratio;
                               t1 odd, so the pair (t1 - 1, t1) has .x inside and .y outside
       40..49  (t1 .. T)       the same, the pair's .y inside and .x outside
       60..69 / 70..79         harm / perc * 1e-21: own^2 underflows, den stays normal
       90..99                  both medians 1e-40 .. 1e-39 (denormal)
       100..104                harm denormal, perc normal
       110..119                harm == perc
       125..129 / 130..134     harm / perc exactly 0, the other normal: masks 0 and 1
       150..200                S, harm, perc * 1e-7: on the top-dB floor
       all (T - T // 3 .. T)   the same for the last third of the frames: a mel row gathers bins, so quiet bins alone leave wide
                               filters above the floor"""
    assert K >= K_MIN
    rng = np.random.default_rng(1000 * seed + T)
    S, harm, perc = _music_like(rng, K, T)
    if edges:
        t1 = quiet_split(T)
        harm[10:20] = perc[10:20] = 0.0
        harm[30:40, :t1] *= np.float32(1e-17)
        perc[30:40, :t1] *= np.float32(1e-17)
        harm[40:50, t1:] *= np.float32(1e-17)
        perc[40:50, t1:] *= np.float32(1e-17)
        harm[60:70] *= np.float32(1e-21)
        perc[70:80] *= np.float32(1e-21)
        harm[90:100] = (1e-40 * rng.uniform(1.0, 10.0, (10, T))).astype(np.float32)
        perc[90:100] = (1e-40 * rng.uniform(1.0, 10.0, (10, T))).astype(np.float32)
        harm[100:105] = np.float32(3e-40)
        perc[110:120] = harm[110:120]
        harm[125:130] = 0.0
        perc[130:135] = 0.0
        for a in (S, harm, perc):
            a[150:] *= np.float32(1e-7)
            a[:150, T - T // 3:] *= np.float32(1e-7)
    if scale != 1.0:
        S, harm, perc = (a * np.float32(scale) for a in (S, harm, perc))
    return S, harm, perc


def _stack(clips):
    return tuple(np.stack([c[i] for c in clips]).astype(np.float32) for i in range(3))


def case_mixed(K, T):
    return _stack([build_mixed(K, T, seed) for seed in (1, 2, 3)])


def case_int16_scale(K, T):
    """The music-like part of `mixed` at the scale of int16 samples."""
    return _stack([build_mixed(K, T, 4, edges=False, scale=32768.0)])


def case_max_last(K, T):
    """Clip 0: each half's maximum lies in the last frame only (the lone frame of odd T, the .y of the last pair); clip 1: in the
    last rows of the first frame (the last bin carries the most; bins K-3 and K-2 lie on the last mel filter's falling slope only).
    harm = 2 perc there, so the H array's maximum is 4 x the P array's; everything else is 1e-8 of it."""
    rng = np.random.default_rng(77 + T)
    out = []
    for variant in (0, 1):
        S = (0.01 * 10.0 ** rng.uniform(-0.5, 0.0, (K, T))).astype(np.float32)
        harm, perc = S.copy(), (S * np.float32(0.5)).astype(np.float32)
        if variant == 0:
            S[5::7, T - 1] = 1e6 * rng.uniform(0.5, 1.0, len(S[5::7, T - 1]))
            S[K - 1, T - 1] = 2e6
            harm[:, T - 1], perc[:, T - 1] = S[:, T - 1], S[:, T - 1] * np.float32(0.5)
        else:
            S[K - 3:, 0] = (5e5, 7.5e5, 1e6)
            harm[K - 3:, 0], perc[K - 3:, 0] = S[K - 3:, 0], S[K - 3:, 0] * np.float32(0.5)
        out.append((S, harm, perc))
    return _stack(out)


def case_all_zero(K, T):
    z = np.zeros((1, K, T), np.float32)
    return z, z.copy(), z.copy()


def case_flat(K, T):
    S = np.stack([np.full((K, T), c, np.float32) for c in (1.0, 0.37, 1234.5)])
    return S, S.copy(), S.copy()


def case_near_constant(K, T):
    """harm = perc = S (both masks exactly 0.5); every bin constant in time except one frame, which is (1 + 2^-16) times it -- the
    same frame for all bins, so every featuregram row is constant except there.  Clip 0: rows of one level; clip 1: log-normal."""
    rng = np.random.default_rng(5 + T)
    level = [np.full(K, 3.0), 10.0 ** rng.uniform(-1.0, 2.0, K)]
    S = np.stack([np.repeat(lv[:, None], T, axis=1) for lv in level]).astype(np.float32)
    S[:, :, T // 3] *= np.float32(1.0 + 2.0 ** -16)
    return S, S.copy(), S.copy()


CASES = {"mixed": case_mixed, "max_last": case_max_last, "all_zero": case_all_zero, "flat": case_flat,
         "near_constant": case_near_constant, "int16_scale": case_int16_scale}
_BUILT = {}


def build(name, K, T):
    """(S, harm, perc), each (B, K, T) float32, B <= 3.  Built once per (name, K, T) and never written to."""
    key = (name, K, T)
    if key not in _BUILT:
        arrs = CASES[name](K, T)
        for a in arrs:
            assert a.dtype == np.float32 and a.shape == arrs[0].shape and a.shape[0] <= 3 and np.isfinite(a).all() and not np.signbit(a).any()
            a.setflags(write=False)
        _BUILT[key] = arrs
    return _BUILT[key]


# ---- premises --------------------------------------------------------------------------------------------------------------------------------
def mask_kinds(harm, perc):
    """Boolean (K, T) arrays naming how the kernels meet each bin of one clip, from the medians alone and in f32 as they compute."""
    h, p = np.asarray(harm, np.float32), np.asarray(perc, np.float32)
    with np.errstate(under="ignore"):
        h2, p2 = h * h, p * p
        den = h2 + p2
    Z = np.maximum(h, p)
    fallback = den < DEN_MIN  # features_half_kernel's test
    return dict(fallback=fallback,
                split_zeros=(h == 0) & (p == 0),                # librosa's split_zeros on exact zeros
                tiny_z=(Z < TINY) & (Z > 0),                    # ... and on denormal medians
                normalised=fallback & (Z >= TINY),              # the normalised form with a real ratio
                own_underflow=~fallback & (((h2 == 0) & (h > 0)) | ((p2 == 0) & (p > 0))),
                denormal=((h > 0) & (h < TINY)) | ((p > 0) & (p < TINY)),
                equal=(h == p) & (h >= TINY),                   # masks exactly 0.5 / 0.5
                one_zero=((h == 0) & (p >= TINY)) | ((p == 0) & (h >= TINY)))  # masks exactly 0 / 1


def premise(name, S, harm, perc, n_mels):
    """Counts of one clip (K, T) that say the case is what it claims; tests/test_feature_cases.py asserts them."""
    S, harm, perc = (np.asarray(a, np.float32) for a in (S, harm, perc))
    K, T = S.shape
    kinds = mask_kinds(harm, perc)
    live = S > 0
    out = {k: int((v & live).sum()) for k, v in kinds.items()}
    fb = kinds["fallback"]
    mixed_waves = 0
    for t0 in range(0, T, WAVE_FRAMES):
        w = fb[:, t0:t0 + WAVE_FRAMES]
        mixed_waves += int((w.any(axis=1) & ~w.all(axis=1)).sum())
    out["mixed_waves"] = mixed_waves
    n2 = T // 2 * 2
    x, y = fb[:, 0:n2:2], fb[:, 1:n2:2]
    out["pairs_x_in_y_out"], out["pairs_y_in_x_out"] = int((x & ~y).sum()), int((y & ~x).sum())
    lin = reference_from_parts(S, harm, perc, n_mels, False).astype(np.float64)
    db = reference_from_parts(S, harm, perc, n_mels, True)
    rows = lin.shape[0] // 2
    out["finite"] = bool(np.isfinite(lin).all() and np.isfinite(db).all())
    out["floor_fraction"] = [float(np.mean(h <= h.max() - 80.0 + 1e-4)) for h in (db[:rows], db[rows:])]
    out["argmax"] = [tuple(int(i) for i in np.unravel_index(np.argmax(h), h.shape)) for h in (lin[:rows], lin[rows:])]
    # the largest value outside the frame that holds the maximum, relative to it, and how much of the dB array the top-dB floor
    # decides outside that frame
    rest, floored = [], []
    for h, d in ((lin[:rows], db[:rows]), (lin[rows:], db[rows:])):
        t = np.unravel_index(np.argmax(h), h.shape)[1]
        other = np.delete(h, t, axis=1)
        rest.append(float(other.max() / h.max()) if other.size and h.max() > 0 else 0.0)
        od = np.delete(d, t, axis=1)
        floored.append(float(np.mean(od == d.max() - np.float32(80.0))) if od.size else 1.0)
    out["rest_over_max"], out["rest_on_floor"] = rest, floored
    # rows of the linear featuregram: constant, or constant but for one frame
    const = near = 0
    for r in lin:
        vals, counts = np.unique(r, return_counts=True)
        const += len(vals) == 1
        near += len(vals) == 2 and T >= 3 and counts.min() == 1
    out["constant_rows"], out["near_constant_rows"], out["rows"] = int(const), int(near), int(lin.shape[0])
    return out
