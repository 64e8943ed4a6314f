"""The host / device master protocol of host.HostModel's weight store (`_dirty`, `_device_newer`), against a stub library that
records its `<prefix>_set_weights` / `<prefix>_get_weights` calls and copies a flat array: no GPU, no libsmh."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from sm_hpss_mtl_amd import _lib
from sm_hpss_mtl_amd.cnn_models import CnnMTL
from sm_hpss_mtl_amd.model import B3MTL

SHAPES = [("a/kernel", (2, 3)), ("a/bias", (3,)), ("b/kernel", (3, 1))]
N_PARAMS = 12


class StubLib:
    """`<prefix>_set_weights(h, host, n, stream)` keeps a copy of the n floats as the device master; `<prefix>_get_weights`
    copies the master back; `<prefix>_num_params` counts it.  Every call is recorded by name."""

    def __init__(self, prefix):
        self.device, self.calls = np.zeros(N_PARAMS, np.float32), []
        setattr(self, prefix + "_set_weights", self._set)
        setattr(self, prefix + "_get_weights", self._get)
        setattr(self, prefix + "_num_params", lambda h: N_PARAMS)

    @staticmethod
    def _view(p, n):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,))

    def _set(self, h, p, n, stream):
        self.calls.append("set")
        self.device = self._view(p, n).copy()
        return 0

    def _get(self, h, p, n, stream):
        self.calls.append("get")
        self._view(p, n)[:] = self.device
        return 0


def _arrays(base):
    return [np.full(shape, base + i, np.float32) for i, (_, shape) in enumerate(SHAPES)]


@pytest.fixture(params=[(B3MTL, "smh_model"), (CnnMTL, "smh_cnn")], ids=["smh_model", "smh_cnn"])
def store(request, monkeypatch):
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    cls, prefix = request.param
    assert cls._C_PREFIX == prefix
    m = cls.__new__(cls)  # the store alone: no device, no trainer
    m.lib, m._h = StubLib(prefix), None  # (no handle: nothing for __del__ to destroy)
    off = np.cumsum([0] + [int(np.prod(s)) for _, s in SHAPES])
    m._spec = ([(n, s, 0, None) for n, s in SHAPES] if cls is B3MTL else [(n, s, int(o)) for (n, s), o in zip(SHAPES, off)])
    m.weights = OrderedDict(zip([n for n, _ in SHAPES], _arrays(0.0)))
    m._init_store()
    return m


def test_one_upload_serves_every_forward_until_the_weights_change(store):
    store.set_weights(_arrays(1.0))
    assert store.lib.calls == []  # set_weights alone moves nothing
    store._sync_weights()
    store._sync_weights()
    assert store.lib.calls == ["set"]
    np.testing.assert_array_equal(store.lib.device, np.concatenate([a.ravel() for a in _arrays(1.0)]))


def test_one_download_after_the_device_became_newer(store):
    store._sync_weights()
    store.lib.calls.clear()
    store.lib.device = np.arange(N_PARAMS, dtype=np.float32)  # an optimiser step on the device
    store._device_newer = True  # what TrainingMixin.apply_gradients sets
    first, second = store.get_weights(), store.get_weights()
    assert store.lib.calls == ["get"]
    for got in (first, second):
        assert [a.shape for a in got] == [s for _, s in SHAPES]
        np.testing.assert_array_equal(np.concatenate([a.ravel() for a in got]), np.arange(N_PARAMS, dtype=np.float32))
    store._sync_weights()
    assert store.lib.calls == ["get"]  # a download does not make the host copy newer


def test_set_weights_drops_a_newer_device_copy(store):
    store._sync_weights()
    store.lib.calls.clear()
    store.lib.device = np.arange(N_PARAMS, dtype=np.float32)
    store._device_newer = True
    store.set_weights(_arrays(5.0))
    for got, want in zip(store.get_weights(), _arrays(5.0)):
        np.testing.assert_array_equal(got, want)
    assert store.lib.calls == []  # no download: the host copy is the master again
    store._sync_weights()
    store._sync_weights()
    assert store.lib.calls == ["set"]
    np.testing.assert_array_equal(store.lib.device, np.concatenate([a.ravel() for a in _arrays(5.0)]))


@pytest.mark.parametrize("bad", ["count", "shape"])
def test_refused_weights_leave_the_store_unchanged(store, bad):
    store._sync_weights()
    store.lib.calls.clear()
    arrays = _arrays(9.0)
    if bad == "count":
        arrays = arrays[:-1]
    else:
        arrays[-1] = arrays[-1].reshape(1, 3)  # the LAST tensor: the ones before it must not have been taken over
    with pytest.raises(ValueError):
        store.set_weights(arrays)
    assert not store._dirty and not store._device_newer
    for got, want in zip(store.get_weights(), _arrays(0.0)):
        np.testing.assert_array_equal(got, want)
    store._sync_weights()
    assert store.lib.calls == []


def test_a_parameter_count_the_library_does_not_share_is_an_error_naming_both(store):
    """The host weight spec and the library's canonical layout are two statements of one order: where they disagree (a tensor one
    side has and the other does not) construction stops with both counts, not with a bare assertion."""
    setattr(store.lib, store._C_PREFIX + "_num_params", lambda h: N_PARAMS + 1056)
    with pytest.raises(RuntimeError, match=r"\b%d\b.*\b%d\b" % (N_PARAMS, N_PARAMS + 1056)):
        store._init_store()
