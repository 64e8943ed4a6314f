"""GPU timing of the fine-tuning feed of the segmentation workflow (sm_hpss_mtl_amd.dafx.generator: descriptor queues + ONE
smh_gather_windows_f32 launch per batch, noise fused) against the same batches built from the calls the package had before it:
per refill `Frontend.extract_patches` on the part (time-major), `torch.cat` onto a materialised queue, a slice per class and
`torch.cat` for the batch, then `device_rng.add_normal_noise` -- the reference generator's own shape, on the device.

Driver's shape: W = 99, W_shift = 34, batch_size = 16 (32 patches per batch), F = 240, noise on; a synthetic standardised
featuregram of FRAMES frames, half of them positive.  Two phases, each with fresh feeds:
    parts : the first batches of a run -- every refill is a 1 088-frame part (90 + 30 patches)
    wrap  : both class cursors moved to the end of their frames, the steady state of a long run -- every refill is the whole
            range [0, n) of a class (n = FRAMES / 2): one progression for the descriptor queue, n / 11 + n / 34 materialised
            patches (95 KB each) for the composition
Protocol of tools/time_plain.py: warm-up batches, a host clock around K batches that ends in a device synchronise, the two
forms ALTERNATING over several rounds; the median round and the spread are printed.  The batches of the two forms are compared
bit for bit with noise off before anything is timed.

    python tools/time_dafx_feed.py [FRAMES=2000000] [K=100] [ROUNDS=7]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import dafx
from sm_hpss_mtl_amd.batching import NOISE_SCALES
from sm_hpss_mtl_amd.device_rng import add_normal_noise, fresh_seed
from sm_hpss_mtl_amd.inference import _frontend

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
K = int(sys.argv[2]) if len(sys.argv) > 2 else 100
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
W, W_SHIFT, BS, F = 99, 34, 16, 240
PARAMS = {"Model": "Lemaire_et_al_MTL", "signal_type": "music", "W": W, "W_shift": W_SHIFT, "data_augmentation_with_noise": True}

torch.manual_seed(0)
FV = torch.randn((F, FRAMES), device="cuda")
labels = (np.arange(FRAMES) // 5000 % 2).astype(np.int32)  # 50-second runs of either class
fe = _frontend()
REFILL_BYTES = sys.getsizeof(dafx._Refill(0, 1, 1, 1, 1, True))


class Composed:
    """The reference generator's materialised queues on the device, from the package's earlier calls.  The part cursor is
    FeedPlanner's (the same integers); only what a refill and a batch DO differs."""

    def __init__(self, noise, wrap):
        self.p = dafx.FeedPlanner(labels, W, W_SHIFT, BS, "music", n_feat=F)
        self.noise = noise
        self.q = [None, None]
        self.refills = 0
        if wrap:
            for c in self.p.classes:
                c.part_j = c.n

    def _refill(self):
        self.refills += 1
        for i, c in enumerate(self.p.classes):
            before = len(c.queue)
            self.p._refill(c)
            if len(c.queue) == before:
                continue
            r = c.queue.pop()  # the progression only says which part this refill is
            new = fe.extract_patches(FV[:, r.base:r.base + r.period].contiguous()[None], W, r.hop, time_major=True)
            assert new.shape[0] == r.count
            self.q[i] = new if self.q[i] is None else torch.cat([self.q[i], new])

    def next(self):
        p = self.p
        while min(c.balance for c in p.classes) < BS:
            self._refill()
        x = torch.cat([self.q[0][:BS], self.q[1][:BS]])
        self.q = [q[BS:] for q in self.q]
        for c in p.classes:
            c.balance -= BS
        if self.noise:
            x = add_normal_noise(x, float(np.random.choice(NOISE_SCALES)), out=x)
        return x


class Device:
    def __init__(self, noise, wrap):
        self.p = dafx.FeedPlanner(labels, W, W_SHIFT, BS, "music", n_feat=F)
        self.noise = noise
        if wrap:
            for c in self.p.classes:
                c.part_j = c.n

    @property
    def refills(self):
        return self.p.classes[0].refills

    def next(self):
        scale, seed = (float(np.random.choice(NOISE_SCALES)), fresh_seed()) if self.noise else (0.0, 0)
        return dafx.gather_windows(FV, self.p.next_batch(), W, "time_major", scale, seed, 0, ctx=fe)


# the generator itself is the Device form (same planner, same call): one batch of it against the class above, then the two forms
g = dafx.generator(dict(PARAMS, data_augmentation_with_noise=False), FV, labels, labels, BS)
assert torch.equal(next(g)[0], Device(False, False).next())
for wrap in (False, True):
    a, b = Device(False, wrap), Composed(False, wrap)
    for i in range(8):
        assert torch.equal(a.next(), b.next()), (wrap, i)
    del a, b
torch.cuda.empty_cache()
print("one-launch feed and composition agree bit for bit (noise off, 8 batches per phase)", flush=True)
print("FV (%d, %d) f32 = %.2f GB resident; %d patches of (%d, %d) per batch; %d rounds of %d batches"
      % (F, FRAMES, F * FRAMES * 4 / 2 ** 30, 2 * BS, W, F, ROUNDS, K), flush=True)

for wrap in (False, True):
    feeds = {"gather": Device(True, wrap), "composed": Composed(True, wrap)}
    for k, f in feeds.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.next()
        torch.cuda.synchronize()
        print("%-5s %-8s first batch, with the phase's first refill: %.3f ms" % ("wrap" if wrap else "parts", k,
                                                                               (time.perf_counter() - t0) * 1e3), flush=True)
        for _ in range(5):
            f.next()
    torch.cuda.synchronize()
    ms = {k: [] for k in feeds}
    for _ in range(ROUNDS):
        for k, f in feeds.items():
            t0 = time.perf_counter()
            for _ in range(K):
                f.next()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / K * 1e3)
    for k, f in feeds.items():
        v = sorted(ms[k])
        queued = sum(c.balance for c in f.p.classes)
        if k == "composed":
            held = "%.2f GB of patches" % (queued * W * F * 4 / 2 ** 30)
        else:  # the progressions themselves (sys.getsizeof of a slotted object: header + 7 references)
            held = "%d bytes in %d progressions of %d bytes" % (sum(sys.getsizeof(r) for c in f.p.classes for r in c.queue),
                                                                sum(len(c.queue) for c in f.p.classes), REFILL_BYTES)
        print("%-5s %-8s median %.4f ms per batch (min %.4f, max %.4f); %d refills so far, %d patches queued, the queues hold %s"
              % ("wrap" if wrap else "parts", k, v[len(v) // 2], v[0], v[-1], f.refills, queued, held), flush=True)
    mg, mc = sorted(ms["gather"])[ROUNDS // 2], sorted(ms["composed"])[ROUNDS // 2]
    print("%-5s gather / composed = %.3f (median rounds)" % ("wrap" if wrap else "parts", mg / mc), flush=True)
    del feeds
    torch.cuda.empty_cache()
