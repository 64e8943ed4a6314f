"""The median filters' harm layouts 1 = (B, T, K) and 2 = (B, ceil(T / 16), K, 16) on every kernel route, bit for bit.

Every case of tests/median_cases.py (a) holds the library's own routing decision (the test-only smh_internal_median_plan, which
calls the functions the launcher plans with) against the restatement tests/median_plans.route for this device's CU count, (b) calls
the entry point, (c) asserts that the layout it returns is the predicted one, and (d) decodes the buffer by the RETURNED layout and
compares every value of every frame t < T with oracle.frontend.median_time / median_freq (pinned to scipy in
tests/test_oracle_pins.py) with np.array_equal -- no tolerance, nothing sampled.  `perc` is compared wherever the entry writes it.

Every output sits inside a larger tensor with 64 sentinel floats before and after the floats the returned layout owns (layouts 0
and 1: B K T; layout 2: B smh_harm_buffer_floats(K, T)); all of them must be untouched afterwards.  The padding frames t >= T of the
last 16-frame block are unspecified and not compared.

Inputs (tests/median_cases.clips): |Gaussian| noise, a clip of multiples of 1/4 (ties), and a clip with zero rows, f32 subnormals and
values near 1e30.  No NaN, no infinities, no -0.0: the kernels use +-inf as sentinels and fminf / fmaxf / v_med3_f32, which order
neither NaN nor the two zeros the way a sort does, and the reference's own order of +-0 is arbitrary; |S| is none of these.

SMH_MEDIAN_PERSIST is read on every call and is set by the cases that name it.  With it, SMH_MEDIAN_NOSPLIT or a tuning switch set
from outside the cases have nothing to say."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import frontend as ofe
from tests import median_cases as M
from tests import median_plans as P
from tests.median_cases import CASES, CROSS_ENTRY, REFUSED, batch, case_id

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.0  # no median of a magnitude spectrogram


@pytest.fixture(autouse=True)
def _skip_if_forced():
    """A test that asserts WHICH kernel ran has nothing to say when an environment switch forces another one: skipped, not failed."""
    forced = [n for n in ("SMH_MEDIAN_NOSPLIT", "SMH_MEDIAN_PERSIST", "SMH_MEDIAN_SEG", "SMH_MEDIAN_PTHREADS") if os.environ.get(n)]
    if forced:
        pytest.skip("implementation forced by " + ", ".join(forced))


@pytest.fixture(scope="module")
def lib():
    from sm_hpss_mtl_amd import _lib
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _S(K, T):
    return M.clips(K, T)


@functools.lru_cache(maxsize=None)
def _oracle(K, T, w, along_t):
    """(3, K, T): the three clips' medians, computed once per shape and window."""
    f = ofe.median_time if along_t else ofe.median_freq
    out = np.stack([f(s, w) for s in _S(K, T)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _S_dev(K, T, B):
    return torch.from_numpy(_S(K, T)[M.clip_index(B)]).cuda().contiguous()


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 4 * offset)


def _guarded(n):
    return torch.full((GUARD + n + GUARD,), SENTINEL, device="cuda")


def _call(lib, entry, S, B, K, T, lh, lp, harm, perc, lay):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, p = _ptr(harm, GUARD), _ptr(perc, GUARD)
    if entry == "hpss_ex":
        rc = lib.smh_hpss_median_ex_f32(None, _ptr(S), B, K, T, lh, lp, h, p, lay, st)
    elif entry == "time_ex":
        rc = lib.smh_median_time_ex_f32(None, _ptr(S), B, K, T, lh, h, lay, st)
    elif entry == "hpss":
        rc = lib.smh_hpss_median_f32(None, _ptr(S), B, K, T, lh, lp, h, p, st)
    else:
        rc = lib.smh_median_time_f32(None, _ptr(S), B, K, T, lh, h, st)
    torch.cuda.synchronize()
    return rc


def _untouched(buf, owned):
    """Everything but the `owned` floats behind the front guard still holds the sentinel."""
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + owned:] == SENTINEL).all())


def _run(lib, n_cu, c, monkeypatch):
    """(a) .. (c) of one case -> (returned layout, harm (B, K, T) decoded by it, perc (B, K, T) or None, B)."""
    if c["persist"] is not None:
        monkeypatch.setenv("SMH_MEDIAN_PERSIST", c["persist"])
    K, T, lh, lp, lay, entry = c["K"], c["T"], c["lh"], c["lp"], c["lay"], c["entry"]
    B = batch(c["B"], n_cu)
    want = P.route(entry, K, T, lh, lp, B, lay, n_cu, c["persist"])
    assert M.library_route(lib, entry, K, T, lh, lp, B, lay) == want
    assert (want["family"], want["layout"]) == (c["family"], c["wrote"]), "the device's CU count moves this case off its route"
    assert lib.smh_harm_buffer_floats(K, T) == P.harm_buffer_floats(K, T)
    nb = max(B, 3)  # B == 0: buffers of three clips, none of which may be touched
    S = _S_dev(K, T, nb)
    harm, perc = _guarded(P.owned_floats(lay, nb, K, T)), _guarded(nb * K * T)
    got = _call(lib, entry, S, B, K, T, lh, lp, harm, perc, lay)
    assert got == c["wrote"], "returned layout %d, predicted %d" % (got, c["wrote"])
    assert _untouched(harm, P.owned_floats(got, B, K, T)), "harm: a guard or a float behind the written layout was touched"
    writes_perc = entry in ("hpss_ex", "hpss") and B > 0
    assert _untouched(perc, B * K * T if writes_perc else 0), "perc: a guard was touched"
    assert torch.equal(S, torch.from_numpy(_S(K, T)[M.clip_index(nb)]).cuda()), "the input was written"
    h = P.decode_harm(harm[GUARD:GUARD + P.owned_floats(got, B, K, T)].cpu().numpy(), got, B, K, T)
    p = perc[GUARD:GUARD + B * K * T].cpu().numpy().reshape(B, K, T) if writes_perc else None
    return got, h, p, B


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_layout_written_and_every_value(lib, n_cu, c, monkeypatch):
    got, h, p, B = _run(lib, n_cu, c, monkeypatch)
    idx = M.clip_index(B)
    ref = _oracle(c["K"], c["T"], c["lh"], True)[idx]
    bad = np.argwhere(h != ref)
    assert np.array_equal(h, ref), "harm differs at %d places, first (clip, bin, frame) %s" % (len(bad), bad[:4].tolist())
    if p is not None:
        ref = _oracle(c["K"], c["T"], c["lp"], False)[idx]
        bad = np.argwhere(p != ref)
        assert np.array_equal(p, ref), "perc differs at %d places, first (clip, bin, frame) %s" % (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("entry,K,T,lh,lp,lay,msg", REFUSED)
def test_refused_shapes_return_invalid_with_their_message_and_touch_nothing(lib, n_cu, entry, K, T, lh, lp, lay, msg):
    from sm_hpss_mtl_amd import _lib
    with pytest.raises(P.Refused) as e:
        M.library_route(lib, entry, K, T, lh, lp, 1, lay)
    assert str(e.value) == msg
    harm, perc = _guarded(P.owned_floats(lay, 1, K, T)), _guarded(K * T)
    rc = _call(lib, entry, _S_dev(K, T, 1), 1, K, T, lh, lp, harm, perc, lay)
    assert rc == _lib.SMH_E_INVALID and _lib.last_error() == msg
    assert _untouched(harm, 0) and _untouched(perc, 0)


@pytest.mark.parametrize("K,T,lh,lp,B,lay,wrote", CROSS_ENTRY)
def test_harm_of_the_single_entry_equals_harm_of_the_pair_entry(lib, n_cu, K, T, lh, lp, B, lay, wrote, monkeypatch):
    images = []
    for entry, w2 in (("hpss_ex", lp), ("time_ex", 0)):
        c = dict(entry=entry, K=K, T=T, lh=lh, lp=w2, B=B, lay=lay, persist=None, wrote=wrote,
                 family=P.route(entry, K, T, lh, w2, B, lay, n_cu)["family"])
        got, h, _, _ = _run(lib, n_cu, c, monkeypatch)
        images.append((got, h))
    assert images[0][0] == images[1][0] == wrote
    assert np.array_equal(images[0][1], images[1][1])
    assert np.array_equal(images[0][1], _oracle(K, T, lh, True)[M.clip_index(B)])
