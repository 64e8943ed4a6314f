"""csrc/smh_gather.hip through the C ABI: smh_gather_windows_f32 bit for bit against a numpy gather in both layouts (plain, tiled
and repeated windows; the 16-byte and the scalar store paths; one and several tiles per axis), the fused noise against
smh_noise_augment_f32 over the finished batch, offsets past 2^31 elements, and every refusal of the entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dafx_ref

pytestmark = pytest.mark.gpu

ENTRY = "smh_gather_windows_f32"
T = 700
FILL = -7.0


@pytest.fixture(scope="module")
def ctx():
    from sm_hpss_mtl_amd.inference import _frontend
    return _frontend()


@pytest.fixture(scope="module")
def fv240():
    """(240, T) host featuregram, its device copy; smaller F are its leading rows re-packed."""
    return np.random.RandomState(7).standard_normal((240, T)).astype(np.float32)


def _fv(fv240, F):
    h = np.ascontiguousarray(fv240[:F])
    return h, torch.from_numpy(h).cuda()


def _table(N, W):
    """The windows of a batch: (base, period, first).  Row 3 alone is the N = 1 case."""
    rows = [(13, W + 20, 7),            # odd base, a plain window inside a longer part
            (T - (W + 5), W + 5, 5),    # ends on the last frame: base + period == T, first + W == period
            (101, 36, 0),               # a 36-frame part: tiled (period < W) for W = 99 and 68
            (101, 36, 17),              # first > 0 inside the tiled part, odd base
            (333, 1, 0),                # a one-frame part
            (333, 1, 4),
            (13, W + 20, 7),            # the same window twice in one batch
            (0, T, T - W)]              # the whole featuregram as one part, its last window
    if N == 1:
        return np.array([rows[3]], np.int32)
    rng = np.random.RandomState(N * 1000 + W)
    while len(rows) < N:
        period = int(rng.randint(1, 3 * W))
        base = int(rng.randint(0, T - period + 1))
        rows.append((base, period, int(rng.randint(0, 2 * period))))
    return np.array(rows[:N], np.int32)


def _call(ctx, d_fv, F, frames, table, W, layout, scale=0.0, seed=0, offset=0, out=None, N=None):
    from sm_hpss_mtl_amd import _lib
    table = np.ascontiguousarray(table, np.int32)
    N = len(table) if N is None else N
    if out is None:
        out = torch.full((max(N, 0) * W * F + 8,), FILL, device="cuda")
    rc = ctx.lib.smh_gather_windows_f32(ctx._h, C.c_void_p(d_fv.data_ptr()), F, frames, table.ctypes.data_as(C.POINTER(C.c_int)), N, W,
                                        layout, scale, seed, offset, C.c_void_p(out.data_ptr()), _lib.current_stream())
    return rc, out


@pytest.mark.parametrize("layout", [0, 1], ids=["image", "time_major"])
@pytest.mark.parametrize("N", [1, 33])
@pytest.mark.parametrize("W", [99, 68, 5])
@pytest.mark.parametrize("F", [240, 7, 1])
def test_gather_equals_numpy_bit_for_bit(ctx, fv240, F, W, N, layout):
    h, d = _fv(fv240, F)
    table = _table(N, W)
    assert len(table) == N
    rc, out = _call(ctx, d, F, T, table, W, layout)
    assert rc == 0
    got = out.cpu().numpy()
    want = dafx_ref.numpy_gather(h, table, W, "time_major" if layout else "image")
    assert want.shape == ((N, W, F) if layout else (N, F, W))
    assert np.array_equal(got[:N * W * F].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.all(got[N * W * F:] == FILL)  # nothing written past the end


@pytest.mark.parametrize("layout", [0, 1], ids=["image", "time_major"])
@pytest.mark.parametrize("F, W", [(240, 99), (7, 5), (6, 68)])
def test_fused_noise_is_the_augmentation_of_the_finished_batch(ctx, fv240, F, W, layout):
    """F % 4 == 0 is the 16-byte store path (one Philox group per store), the others draw element by element; F * W * N is no
    multiple of 4 at (7, 5, 33), so the batch ends inside a group."""
    from sm_hpss_mtl_amd import _lib
    h, d = _fv(fv240, F)
    N = 33
    table = _table(N, W)
    n = N * W * F
    seed, offset, scale = (0x5A17 << 32) | 0xC0FFEE, (3 << 32) | 9, 5e-3
    rc, plain = _call(ctx, d, F, T, table, W, layout)
    assert rc == 0
    rc, noisy = _call(ctx, d, F, T, table, W, layout, scale, seed, offset)
    assert rc == 0
    _lib.check(ctx.lib.smh_noise_augment_f32(C.c_void_p(plain.data_ptr()), C.c_void_p(plain.data_ptr()), n, scale, seed, offset,
                                             _lib.current_stream()))
    got, want = noisy.cpu().numpy(), plain.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got[n:] == FILL)
    clean = dafx_ref.numpy_gather(h, table, W, "time_major" if layout else "image").reshape(-1)
    z = (got[:n].astype(np.float64) - clean) / scale
    assert abs(z.mean()) < 5 / np.sqrt(n) + 1e-3 and abs(z.std() - 1) < 5 / np.sqrt(n) + 2e-3  # it is noise, of that scale
    # another offset is another stream; noise_scale == 0 is the bit copy
    rc, other = _call(ctx, d, F, T, table, W, layout, scale, seed, offset + 1)
    assert rc == 0 and not torch.equal(other, noisy)
    rc, zero = _call(ctx, d, F, T, table, W, layout, 0.0, seed, offset)
    assert rc == 0 and np.array_equal(zero.cpu().numpy()[:n].view(np.uint32), clean.view(np.uint32))


@pytest.mark.parametrize("layout", [0, 1], ids=["image", "time_major"])
def test_offsets_past_2_31_elements(ctx, layout):
    """F = 240, T = 9 000 000: 2.16 G floats (8.6 GB, uninitialised); only the last 300 frames are filled and read -- the rows
    from 239 on start beyond 2^31 elements."""
    F, frames, W, keep = 240, 9_000_000, 99, 300
    if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
        pytest.skip("needs 12 GB of free device memory")
    small = np.random.RandomState(31).standard_normal((F, keep)).astype(np.float32)
    big = torch.empty((F, frames), dtype=torch.float32, device="cuda")
    big[:, frames - keep:] = torch.from_numpy(small).cuda()
    table = np.array([(0, keep, 0), (keep - W, W, 0), (150, 36, 17), (101, 150, 51)], np.int32)
    shifted = table.copy()
    shifted[:, 0] += frames - keep
    rc, out = _call(ctx, big, F, frames, shifted, W, layout)
    assert rc == 0
    got = out.cpu().numpy()
    del big
    want = dafx_ref.numpy_gather(small, table, W, "time_major" if layout else "image").reshape(-1)
    assert np.array_equal(got[:want.size].view(np.uint32), want.view(np.uint32))
    assert np.all(got[want.size:] == FILL)


def test_empty_batch_launches_nothing(ctx, fv240):
    _, d = _fv(fv240, 8)
    rc, out = _call(ctx, d, 8, T, np.zeros((1, 3), np.int32), 5, 1, N=0)
    assert rc == 0 and bool((out == FILL).all())


GOOD = dict(F=8, frames=T, W=5, layout=1, scale=0.0, N=3)
BAD = [
    ("null ctx", dict(null="ctx")), ("null FV", dict(null="fv")), ("null table", dict(null="desc")), ("null out", dict(null="out")),
    ("N < 0", dict(N=-1)), ("W < 1", dict(W=0)), ("F < 1", dict(F=0)), ("layout 2", dict(layout=2)), ("layout -1", dict(layout=-1)),
    ("noise_scale < 0", dict(scale=-1e-3)), ("out misaligned", dict(misalign=4)),
    ("base < 0", dict(row=(-1, 10, 0))), ("period < 1", dict(row=(5, 0, 0))), ("first < 0", dict(row=(5, 10, -1))),
    ("base + period > T", dict(row=(T - 9, 10, 0))), ("T too small", dict(frames=17)),
]


@pytest.mark.parametrize("what, change", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_refusals_leave_the_output_unwritten(ctx, fv240, what, change):
    from sm_hpss_mtl_amd import _lib
    _, d = _fv(fv240, GOOD["F"])
    table = np.array([(13, 30, 7), (17, 2, 1), (T - 10, 10, 5)], np.int32)
    out = torch.full((GOOD["N"] * GOOD["W"] * GOOD["F"] + 8,), FILL, device="cuda")

    def call(**kw):
        a = dict(GOOD, **kw)
        tab = table.copy()
        if "row" in a:
            tab[1] = a["row"]
        null = a.get("null")
        return ctx.lib.smh_gather_windows_f32(
            None if null == "ctx" else ctx._h, None if null == "fv" else C.c_void_p(d.data_ptr()), a["F"], a["frames"],
            None if null == "desc" else tab.ctypes.data_as(C.POINTER(C.c_int)), a["N"], a["W"], a["layout"], a["scale"], 1, 2,
            None if null == "out" else C.c_void_p(out.data_ptr() + a.get("misalign", 0)), _lib.current_stream())

    rc = call(**change)
    assert rc == _lib.SMH_E_INVALID, what
    assert ENTRY in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == FILL).all()), what
    # the same call with nothing wrong then runs
    assert call() == 0
    got = out.cpu().numpy()
    want = dafx_ref.numpy_gather(fv240[:GOOD["F"]], table, GOOD["W"], "time_major").reshape(-1)
    assert np.array_equal(got[:want.size], want) and np.all(got[want.size:] == FILL)


def test_capture_is_refused_before_anything_is_enqueued(ctx, fv240):
    """The table comes from a staging buffer, as the ragged entries' tables do: a capturing stream is refused."""
    from sm_hpss_mtl_amd import _lib
    _, d = _fv(fv240, 8)
    table = np.array([(13, 30, 7)], np.int32)
    out = torch.full((5 * 8 + 8,), FILL, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc, _ = _call(ctx, d, 8, T, table, 5, 1, out=out)
        err = _lib.last_error()
    torch.cuda.synchronize()
    assert rc == _lib.SMH_E_INVALID and ENTRY in err and "cannot be captured in a graph" in err
    assert bool((out == FILL).all())


def test_python_wrapper(ctx, fv240):
    """dafx.gather_windows: shapes per layout, the same bits, and the table's shape is checked."""
    from sm_hpss_mtl_amd import dafx
    h, d = _fv(fv240, 12)
    table = _table(33, 68)
    for layout in ("time_major", "image"):
        got = dafx.gather_windows(d, table, 68, layout)
        assert tuple(got.shape) == ((33, 68, 12) if layout == "time_major" else (33, 12, 68))
        assert np.array_equal(got.cpu().numpy(), dafx_ref.numpy_gather(h, table, 68, layout))
    with pytest.raises(ValueError, match="base, period, first"):
        dafx.gather_windows(d, table[:, :2], 68)
    with pytest.raises(ValueError, match="smh_gather_windows_f32"):
        dafx.gather_windows(d, np.array([(T - 5, 10, 0)], np.int32), 68)
