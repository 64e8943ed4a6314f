"""GPU: whole-clip staging of hpss_median_split_kernel by LDS-DMA (csrc/smh_median_split.h, decided in smh_median_plan.h dma_staged).

When the tile is the whole clip, gcd(T, 64) <= 2 and the copy fits the tile the plan allocates, the block-split kernel stages the clip
as the flat K x T image by LDS-DMA (16-byte chunks from the aligned address below the clip) instead of through VGPRs into the
odd-stride tile; SMH_MEDIAN_DMA_STAGE=0 forces the register staging.  Medians are selections: every value must be the oracle's, and
the two stagings must give the same bits.

Windows (17, 17) and (21, 11), the block-split kernel forced with SMH_MEDIAN_PERSIST=0.  Shapes: K = 201 with T = 98 (the headline),
34 (gcd 2, one wave of percussive lanes per segment) and 97 (odd: the plan's tile has no room for the copy, the register staging
runs); K = 9, T = 34 (the percussive axis is too short for the pair kernel: one launch per filter, the harmonic one staged by DMA).
B = 1 and B = 5: K T 4 bytes is no multiple of 16 at any of these shapes, so clips 1 and 3 of five start 8 bytes off a 16-byte
boundary.  Harm layouts 1 and 2.  Which staging each case takes is asserted from the library's own plan (smh_internal_median_plan,
given the alignment class of the input: 8, and 4 at T = 97).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import median_cases as M
from tests import median_plans as P

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.0  # no median of a magnitude spectrogram


@functools.lru_cache(maxsize=None)
def _S(K, T):
    """Three clips of magnitudes with ties (quantised) and a silent stretch."""
    rng = np.random.default_rng(1000 * K + T)
    s = np.abs(rng.standard_normal((3, K, T))).astype(np.float32)
    s[1] = np.round(s[1] * 4) / 4
    s[2, :, T // 3:T // 3 + 5] = 0.0
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _oracle(K, T, w, along_t):
    f = ofe.median_time if along_t else ofe.median_freq
    out = np.stack([f(s, w) for s in _S(K, T)])
    out.setflags(write=False)
    return out


def _run(lib, S, B, K, T, lh, lp, lay):
    """smh_hpss_median_ex_f32 -> (layout written, harm (B, K, T), perc (B, K, T)); guards in front of and behind both outputs."""
    nh = P.owned_floats(2, B, K, T)  # the largest of the three layouts
    harm = torch.full((GUARD + nh + GUARD,), SENTINEL, device="cuda")
    perc = torch.full((GUARD + B * K * T + GUARD,), SENTINEL, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = lib.smh_hpss_median_ex_f32(None, C.c_void_p(S.data_ptr()), B, K, T, lh, lp, C.c_void_p(harm.data_ptr() + 4 * GUARD),
                                     C.c_void_p(perc.data_ptr() + 4 * GUARD), lay, st)
    torch.cuda.synchronize()
    assert got in (0, 1, 2), got
    owned = P.owned_floats(got, B, K, T)
    assert bool((harm[:GUARD] == SENTINEL).all()) and bool((harm[GUARD + owned:] == SENTINEL).all()), "harm: a guard was touched"
    assert bool((perc[:GUARD] == SENTINEL).all()) and bool((perc[GUARD + B * K * T:] == SENTINEL).all()), "perc: a guard was touched"
    h = P.decode_harm(harm[GUARD:GUARD + owned].cpu().numpy(), got, B, K, T)
    return got, h, perc[GUARD:GUARD + B * K * T].cpu().numpy().reshape(B, K, T)


@pytest.mark.parametrize("lay", [1, 2])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K,T", [(201, 98), (201, 34), (201, 97), (9, 34)])
@pytest.mark.parametrize("lh,lp", [(17, 17), (21, 11)])
def test_dma_staging_gives_the_oracles_medians_and_the_register_stagings_bits(lh, lp, K, T, B, lay, monkeypatch):
    from sm_hpss_mtl_amd import _lib
    lib = _lib.require_gpu()
    for name in ("SMH_MEDIAN_NOSPLIT", "SMH_MEDIAN_SEG", "SMH_MEDIAN_PTHREADS", "SMH_MEDIAN_DMA_STAGE", "SMH_MEDIAN_PROBE_NOLOAD"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SMH_MEDIAN_PERSIST", "0")
    idx = [i % 3 for i in range(B)]
    # the clips between sentinels, on a 16-byte boundary: clip b starts b K T 4 bytes behind it
    buf = torch.full((GUARD + B * K * T + GUARD,), SENTINEL, device="cuda")
    buf[GUARD:GUARD + B * K * T] = torch.from_numpy(_S(K, T)[idx]).cuda().reshape(-1)
    S = buf[GUARD:GUARD + B * K * T]
    assert S.data_ptr() % 16 == 0 and (K * T * 4) % 16 != 0
    align = 8 if (K * T * 4) % 8 == 0 else 4
    assert align == (4 if T == 97 else 8)

    def staging():
        """(family, dma) of the launch that computes harm, from the library's plan."""
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        plan = M.library_route(lib, "hpss_ex", K, T, lh, lp, B, lay, n_cu=n_cu, align=align)
        if K == 9:  # one launch per filter: the harmonic one is a block-split launch, the percussive axis takes rank counting
            assert plan["family"] == "two_singles"
            assert M.library_route(lib, "freq", K, T, 0, lp, B, 0, n_cu=n_cu, align=align)["family"] == "small"
            plan = M.library_route(lib, "time", K, T, lh, 0, B, 0, n_cu=n_cu, align=align)
        return plan["family"], plan["dma"]

    assert staging() == ("split", 0 if T == 97 else 1)
    got, h, p = _run(lib, S, B, K, T, lh, lp, lay)
    ref_h, ref_p = _oracle(K, T, lh, True)[idx], _oracle(K, T, lp, False)[idx]
    assert np.array_equal(h, ref_h), "harm differs at (clip, bin, frame) %s" % np.argwhere(h != ref_h)[:4].tolist()
    assert np.array_equal(p, ref_p), "perc differs at (clip, bin, frame) %s" % np.argwhere(p != ref_p)[:4].tolist()
    monkeypatch.setenv("SMH_MEDIAN_DMA_STAGE", "0")
    assert staging() == ("split", 0)
    got0, h0, p0 = _run(lib, S, B, K, T, lh, lp, lay)
    assert got0 == got and np.array_equal(h0, h) and np.array_equal(p0, p), "SMH_MEDIAN_DMA_STAGE=0 against the default"
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + B * K * T:] == SENTINEL).all()), "the input's guards were written"
