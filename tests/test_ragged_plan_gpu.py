"""The ragged planner that the harmonic-percussive and the plain front end share (smh_rag.h), pinned from outside through the C ABI:
one HPSS context (defaults) and one plain context (LogMelSpec, 80 mels), both n_fft = 400 / hop = 160, over ONE clip list.

The list holds a member of every class the planner knows, at the smallest length that reaches it -- the lengths come from
`smh_num_frames` and `smh_internal_frontend_route` of the HPSS context, none is written down here:

    0  LDS image, even T          1  LDS image, odd T          2  streamed: the first T beyond `smh_features_blocked_ok`
    3  T = 1: no ragged median kernel takes it                  4  shorter than W: tile-if-short
    5  a clip that starts 4 mod 8 bytes into the buffer (a hand-built offset table): both front ends send it through their
       equal-length entry alone, with the generic STFT kernel
    6-8  three more streamed clips (the next lengths, odd T among them).  Without them clip 2 is two thirds of the whole workspace
       and "a third of the workspace" could not hold it: the call would be refused, as the contract says, and nothing be compared.

Every clip alone goes through `Frontend.run` on a view of the SAME device buffer, so that clip 5 starts off the 8-byte boundary there
too and takes the same STFT kernel.

The "minimum" workspace, max_b *_frontend_workspace_bytes(1, len_b), is below what the planners' estimates ask for the longest clip alone
(plain: 136 192 bytes given, 136 788 estimated for T = 168, 137 604 for T = 169), but not below what that sub-batch truly occupies
(tables and S of the T = 169 clip end at byte 136 144): such a clip runs alone, and `Tables::upload` checks the true extent."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_FFT, HOP, W, SHIFT = 400, 160, 68, 34


def _frontends():
    from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig
    hpss = Frontend(FrontendConfig())
    plain = Frontend(FrontendConfig.from_params({"Model": "m", "Tw": 25, "Ts": 10}, N_FFT, 80, "LogMelSpec"))
    assert hpss.cfg.hpss and not plain.cfg.hpss and plain.cfg.log_db and plain.rows == 80
    return {"hpss": hpss, "plain": plain}


def _lengths(hpss):
    """Sample counts of the clip list, derived from the integer functions of the HPSS context."""
    lib, h = hpss.lib, hpss._h
    route = lambda T: lib.smh_internal_frontend_route(h, T)
    first = lambda pred: next(T for T in range(1, 4096) if pred(T))
    T_even, T_odd = first(lambda T: route(T) == 0), first(lambda T: route(T) == 1)
    T_long = first(lambda T: T > T_even and not lib.smh_features_blocked_ok(h, T, 0))
    assert T_even % 2 == 0 and T_odd % 2 == 1 and route(T_long) == 2 and route(T_long - 1) in (0, 1) and route(1) == 3
    T_short = W // 2
    assert lib.smh_tiled_frames(T_short, W) > T_short
    Ts = [T_even, T_odd, T_long, 1, T_short, T_even, T_long + 1, T_long + 2, T_long + 3]
    lens = [N_FFT + (T - 1) * HOP for T in Ts]
    assert [lib.smh_num_frames(n, N_FFT, HOP) for n in lens] == Ts
    return lens, Ts


class _Env:
    """One front end, the clip list in one device buffer, and what every clip gives alone (computed once, never changed)."""

    def __init__(self, fe, lens, Ts):
        self.fe, self.lib, self.lens, self.Ts = fe, fe.lib, lens, Ts
        self.F = (2 if fe.cfg.hpss else 1) * fe.rows
        stem = "smh_frontend_ragged" if fe.cfg.hpss else "smh_plain_frontend_ragged"
        self.sizes, self.entry = getattr(fe.lib, stem + "_sizes"), getattr(fe.lib, stem + "_f32")
        self.one_clip_bytes = fe.lib.smh_frontend_workspace_bytes if fe.cfg.hpss else fe.lib.smh_plain_frontend_workspace_bytes
        self.B = len(self.lens)
        offs, o = [], 0
        for i, n in enumerate(self.lens):  # 16-byte aligned starts, except clip 5: one float on, 4 mod 8 bytes
            offs.append(o + (i == 5))
            o += (n + (i == 5) + 3) // 4 * 4
        rng = np.random.default_rng(17)
        host = np.zeros(o, np.float32)
        for i, (n, of) in enumerate(zip(self.lens, offs)):
            host[of:of + n] = (0.3 * (1e-2, 1.0, 30.0)[i % 3] * rng.standard_normal(n)).astype(np.float32)
        assert all(offs[i] + self.lens[i] <= offs[i + 1] for i in range(self.B - 1))
        self.offs, self.audio = offs, torch.from_numpy(host).cuda()
        assert [(self.audio.data_ptr() + 4 * of) % 8 for of in offs] == [0, 0, 0, 0, 0, 4, 0, 0, 0]
        self.h_off, self.h_len = (C.c_longlong * self.B)(*offs), (C.c_int * self.B)(*self.lens)
        self.alone = [fe.run(self.audio[of:of + n][None], W=W, shift=SHIFT) for n, of in zip(self.lens, offs)]
        torch.cuda.synchronize()

    def plan(self, w, shift):
        B = self.B
        fv_off, p_off = (C.c_longlong * (B + 1))(), (C.c_longlong * (B + 1))()
        hT, hnP, work = (C.c_int * B)(), (C.c_int * B)(), C.c_size_t()
        rc = self.sizes(self.fe._h, self.h_off, self.h_len, B, w, shift, fv_off, p_off, hT, hnP, C.byref(work))
        assert rc == 0
        return list(hT), list(hnP), list(fv_off), list(p_off), work.value

    def call(self, work_bytes, fv=None, pt=None, wk=None):
        from sm_hpss_mtl_amd import _lib
        from sm_hpss_mtl_amd.frontend import _ptr
        _, _, fv_off, p_off, _ = self.plan(W, SHIFT)
        fv = torch.full((fv_off[-1],), float("nan"), device="cuda") if fv is None else fv
        pt = torch.full((p_off[-1], W, self.F), float("nan"), device="cuda") if pt is None else pt
        wk = torch.empty(max(work_bytes, 16), dtype=torch.uint8, device="cuda") if wk is None else wk
        rc = self.entry(self.fe._h, _ptr(self.audio), self.h_off, self.h_len, self.B, W, SHIFT, _ptr(fv), _ptr(pt), _ptr(wk),
                        work_bytes, _lib.current_stream())
        return rc, fv, pt

    def full(self):
        if not hasattr(self, "_full"):
            rc, fv, pt = self.call(self.plan(W, SHIFT)[4])
            torch.cuda.synchronize()
            assert rc == 0
            self._full = (fv, pt)
        return self._full


_ENVS = {}


@pytest.fixture(params=["hpss", "plain"])
def env(request):
    if not _ENVS:
        fes = _frontends()
        lens, Ts = _lengths(fes["hpss"])
        _ENVS.update((name, _Env(fe, lens, Ts)) for name, fe in fes.items())
    return _ENVS[request.param]


@pytest.mark.parametrize("w,shift", [(W, SHIFT), (0, 0)])
def test_ragged_sizes_outputs(env, w, shift):
    """T, nP, fv_off and patch_off of `*_ragged_sizes` against the integer functions and running sums."""
    lib = env.lib
    hT, hnP, fv_off, p_off, work = env.plan(w, shift)
    T = [lib.smh_num_frames(n, N_FFT, HOP) for n in env.lens]
    nP = [lib.smh_num_patches(lib.smh_tiled_frames(t, w), w, shift) if w > 0 else 0 for t in T]
    assert hT == T == env.Ts and hnP == nP
    assert fv_off == [env.F * sum(T[:b]) for b in range(env.B + 1)]
    assert p_off == [sum(nP[:b]) for b in range(env.B + 1)]
    assert work % 256 == 0 and work >= max(env.one_clip_bytes(env.fe._h, 1, n) for n in env.lens)
    if w > 0:
        assert min(nP) >= 1 and [a["n_patches"] for a in env.alone] == nP


def test_full_workspace_equals_every_clip_alone(env):
    hT, hnP, fv_off, p_off, _ = env.plan(W, SHIFT)
    fv, pt = env.full()
    for b, one in enumerate(env.alone):
        assert torch.equal(fv[fv_off[b]:fv_off[b + 1]].view(env.F, hT[b]), one["fv"][0]), ("fv", b, hT[b])
        assert torch.equal(pt[p_off[b]:p_off[b + 1]], one["patches"]), ("patches", b, hT[b])


@pytest.mark.parametrize("kind", ["third", "minimum", "4096"])
def test_sub_batch_workspaces(env, kind):
    """A third of the reported workspace and the largest single clip's minimum run in sub-batches and give the bytes of the full
    workspace; 4096 bytes are refused with SMH_E_WORKSPACE."""
    from sm_hpss_mtl_amd import _lib
    need = env.plan(W, SHIFT)[4]
    minimum = (max(env.one_clip_bytes(env.fe._h, 1, n) for n in env.lens) + 255) // 256 * 256
    work = {"third": need // 3 // 256 * 256, "minimum": minimum, "4096": 4096}[kind]
    fv0, pt0 = env.full()
    rc, fv, pt = env.call(work)
    torch.cuda.synchronize()
    print("%s: reported %d, minimum %d, given %d -> rc %d (%s)" % (kind, need, minimum, work, rc, _lib.last_error() if rc else "ok"))
    if kind == "4096":
        assert rc == _lib.SMH_E_WORKSPACE
        return
    assert minimum <= work < need
    assert rc == 0, _lib.last_error()
    assert torch.equal(fv, fv0) and torch.equal(pt, pt0)


def test_capture_is_refused_before_anything_is_enqueued(env):
    """On a capturing stream the call returns the SMH_E_INVALID capture refusal and leaves the outputs untouched."""
    from sm_hpss_mtl_amd import _lib
    _, _, fv_off, p_off, need = env.plan(W, SHIFT)
    fv = torch.full((fv_off[-1],), -7.0, device="cuda")
    pt = torch.full((p_off[-1], W, env.F), -7.0, device="cuda")
    wk = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc, _, _ = env.call(need, fv, pt, wk)
        err = _lib.last_error()
    torch.cuda.synchronize()
    assert rc == _lib.SMH_E_INVALID and "cannot be captured in a graph" in err
    assert bool((fv == -7.0).all()) and bool((pt == -7.0).all())
