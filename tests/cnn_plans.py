"""Python restatement of the launch plans of the Conv2D models (sm_hpss_mtl_amd/csrc/smh_cnn_plan.h, with the layer
graphs of smh_cnn_impl.h) -- TEST INFRASTRUCTURE.

It computes no numbers: it only says which split-K / reduction branch a layer takes at a given shape and batch, so
that tests/test_cnn_plans.py can show that every case of tests/test_cnn_gpu.py and tests/test_cnn_train_plans_gpu.py
reaches the branch it is named for.  Each function cites the C++ function it copies; a change there must be mirrored
here.  tests/test_cnn_plan_gpu.py compares every value with the library's own plan (smh_internal_cnn_plan), and the
hand-computed pins in tests/test_cnn_plans.py catch a mirror that drifts from what it claims.
"""
from __future__ import annotations

BM, BK, BKB = 128, 16, 32      # smh_cnn_plan.h: BM, BK, BKB
K_CHUNK = 64                   # kChunk
K_MAX_RED = 1024               # kMaxRed
K_SMALL_K = 32                 # kSmallK
MIN_TRAINER_CAP = 48           # cnn_training.py: CnnTrainingMixin._MIN_TRAINER_CAP


def _cdiv(a, b):
    return -(-a // b)


def _bn_width(OC):
    return 64 if OC <= 64 else 128


def tiles(rows, cols):
    """gemm_plan: (bn, mt, nt) -- the column tile width and the x / y grid of a rows x cols GEMM."""
    bn = _bn_width(cols)
    return bn, _cdiv(rows, BM), _cdiv(cols, bn)


# ---- layer graph (build_graph): the Conv2D / Dense layers with their GEMM geometry ------------------------------
def graph(kind, H, W, fc=4096, n_mels=None, single=False):
    """[layer dict] of the Conv2D / Dense layers in graph order.  `index` is the position in m->layers (pooling, LRN
    and the mel-scale layer count too): the data gradient runs for every layer with index > 0.  single: the
    single-task kind -- the same trunk for Doukhan and Papakostas, a graph of its own for Jang."""
    layers, pos = [], [0]

    def other(n=1):
        pos[0] += n

    def conv(name, h, w, c, kh, kw, oc, s, same, bn):
        if same:
            OH, OW = _cdiv(h, s), _cdiv(w, s)
            pt, pl = max((OH - 1) * s + kh - h, 0) // 2, max((OW - 1) * s + kw - w, 0) // 2
        else:
            OH, OW, pt, pl = (h - kh) // s + 1, (w - kw) // s + 1, 0, 0
        K = kh * kw * c
        layers.append(dict(name=name, H=h, W=w, C=c, OH=OH, OW=OW, OC=oc, kh=kh, kw=kw, s=s, pt=pt, pl=pl, K=K,
                           Kp=_cdiv(K, 32) * 32, bn=bn, index=pos[0]))
        pos[0] += 1
        return OH, OW, oc

    def dense(name, D, oc):
        layers.append(dict(name=name, H=1, W=1, C=D, OH=1, OW=1, OC=oc, kh=1, kw=1, s=1, pt=0, pl=0, K=D,
                           Kp=_cdiv(D, 32) * 32, bn=True, index=pos[0]))
        pos[0] += 1
        return oc

    if kind == "Doukhan":
        h, w, c = conv("conv1", H, W, 1, 4, 5, 64, 1, False, True)
        other(); h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1          # pool 2x2 valid
        h, w, c = conv("conv2", h, w, c, 3, 3, 128, 1, False, True)
        h, w, c = conv("conv3", h, w, c, 3, 3, 128, 1, False, True)
        other(); h, w = _cdiv(h, 2), _cdiv(w, 2)                    # pool 2x2 same
        h, w, c = conv("conv4", h, w, c, 3, 3, 256, 1, False, True)
        other(); w = (w - 12) // 12 + 1                             # pool 1x12 valid
        D = h * w * c
        for i in range(4):
            D = dense("fc%d" % (i + 1), D, 512)
    elif kind == "Papakostas":
        h, w, c = conv("conv1", H, W, 1, 5, 5, 96, 2, False, False)
        other(2); h, w = _cdiv(h, 2), _cdiv(w, 2)                   # LRN, pool 3x3/2 same
        h, w, c = conv("conv2", h, w, c, 3, 3, 384, 2, False, False)
        other(2); h, w = _cdiv(h, 2), _cdiv(w, 2)
        h, w, c = conv("conv3", h, w, c, 3, 3, 512, 1, True, False)
        other(); h, w = _cdiv(h, 2), _cdiv(w, 2)
        D = dense("fc1", h * w * c, fc)
        dense("fc2", D, fc)
    elif kind == "Jang" and single:
        other()                                  # one mel-scale layer over the whole image: (n_mels, W, 3)
        h, w, c = n_mels or 64, W, 3
        for i, oc in enumerate((32, 64, 128)):
            h, w, c = conv("conv%d" % (i + 1), h, w, c, 3, 3, oc, 1, True, True)
            other(); h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1      # pool 2x2 valid; no Dense: Flatten feeds the head
    elif kind == "Jang":
        other()                                  # the mel-scale layer: (2 n_mels, W, 3)
        h, w, c = 2 * (n_mels or 120), W, 3
        for i, oc in enumerate((32, 64, 128)):
            h, w, c = conv("conv%d" % (i + 1), h, w, c, 3, 3, oc, 1, True, True)
            other(); h, w = _cdiv(h, 2), _cdiv(w, 2)                # pool 2x2 same
        D = dense("fc1", h * w * c, 2048)
        dense("fc2", D, 1024)
    else:
        raise ValueError(kind)
    return layers


def layer(kind, H, W, name, **kw):
    return next(L for L in graph(kind, H, W, **kw) if L["name"] == name)


# ---- forward (inference) ----------------------------------------------------------------------------------------
def choose_split(mtiles, ntiles, ksteps):
    """choose_split."""
    s = 1
    blocks = mtiles * ntiles
    if 1 <= blocks < 256 and ksteps >= 32:
        s = max(min(_cdiv(512, blocks), 16, ksteps // 8), 1)
    return s


def plan_images(n, single=False):
    """plan_images: the single-task kinds plan the split of every pass as that of a full one."""
    return K_CHUNK if single else n


def forward_plan(L, n, bf16=False, single=False):
    """plan_forward for one pass of n images: the split is chosen on the f32 k-steps (Kp / 16) for both precisions
    and on the rows of plan_images; it never exceeds the bf16 kernel's Kp / 32 k-steps (at most Kp / 128 slices).
    `empty`: slices whose k range starts at or past ksteps -- they still write zeros to the partial buffer."""
    M = n * L["OH"] * L["OW"]
    mt, nt = _cdiv(plan_images(n, single) * L["OH"] * L["OW"], BM), _cdiv(L["OC"], _bn_width(L["OC"]))
    ksteps = L["Kp"] // (BKB if bf16 else BK)
    ksplit = choose_split(mt, nt, L["Kp"] // BK)
    per = _cdiv(ksteps, ksplit)
    return dict(M=M, ksteps=ksteps, ksplit=ksplit, ksteps_per=per, empty=ksplit - _cdiv(ksteps, per))


def passes(N):
    """forward_impl: passes of kChunk images, the last one ragged."""
    return [min(K_CHUNK, N - n0) for n0 in range(0, N, K_CHUNK)]


def forward_partial_floats(layers, N, single=False):
    """forward_partial_floats: the largest block of split partials over the passes of a forward of N images."""
    part = 0
    for n in set(passes(max(N, 1))):
        for L in layers:
            p = forward_plan(L, n, single=single)
            if p["ksplit"] > 1:
                part = max(part, p["ksplit"] * p["M"] * L["OC"])
    return part


def workspace_bytes(layers, H, W, N, single=False):
    """carve: two activation buffers for a pass and the split partials, each aligned to 256 bytes.  The largest
    activation is the input or a Conv2D / Dense output: pooling only shrinks, LRN keeps the size, and the mel-scale
    layer's 3 channels are fewer than conv1's 32 on the same pixels."""
    def align(v):
        return (v + 255) & ~255
    max_act = max([H * W] + [L["OH"] * L["OW"] * L["OC"] for L in layers])
    return 2 * align(4 * max_act * min(max(N, 1), K_CHUNK)) + align(4 * forward_partial_floats(layers, N, single))


# ---- training -----------------------------------------------------------------------------------------------------
def trainer_cap(N):
    """TrainingMixin._get_trainer: a fresh trainer has room for max(N, 48) images."""
    return max(N, MIN_TRAINER_CAP)


def trainer_partial_floats(layers, cap):
    """trainer_partial_floats."""
    p = 48 << 20
    for L in layers:
        p = max(p, 16 * min(cap * L["OH"] * L["OW"], 4096) * L["OC"])
    return p


def train_forward_plan(L, N, partial_floats):
    """plan_train_forward: the split of the batch's own rows, capped by the partial buffer."""
    M = N * L["OH"] * L["OW"]
    ksteps = L["Kp"] // BK
    ksplit = choose_split(_cdiv(M, BM), _cdiv(L["OC"], _bn_width(L["OC"])), ksteps)
    while ksplit > 1 and ksplit * M * L["OC"] > partial_floats:
        ksplit -= 1
    return dict(M=M, ksteps=ksteps, ksplit=ksplit, ksteps_per=_cdiv(ksteps, ksplit),
                partial=ksplit * M * L["OC"] if ksplit > 1 else 0)


def wgrad_split(blocks, ksteps, out_floats, cap_floats):
    """wgrad_split."""
    s = 1
    if blocks < 1024 and ksteps >= 32:
        s = min(_cdiv(1024, blocks), ksteps // 16, 256)
        while s > 1 and s * out_floats > cap_floats:
            s -= 1
        s = max(s, 1)
    return s


def wgrad_plan(L, N, partial_floats, env=None, mfma=False):
    """plan_wgrad: the VALU small-K kernel (K <= 32, unless SMH_CNN_WGRAD_MFMA is set) or the MODE-1
    GEMM with ordered split partials; env = SMH_CNN_WSPLIT.  A forced split is capped by the partial buffer like the
    automatic one (`cap_cut`), then cut so that no slice is empty (`empty_cut`)."""
    M = N * L["OH"] * L["OW"]
    outf = L["K"] * L["OC"]
    if L["K"] <= K_SMALL_K and not mfma:
        nb = max(1, min(1024, M // 512))
        while nb > 1 and nb * outf > partial_floats:
            nb -= 1
        rpb = _cdiv(_cdiv(M, nb), 64) * 64
        nb = _cdiv(M, rpb)
        return dict(kind="smallk", M=M, blocks=nb, rows_per_block=rpb, partial=nb * outf)
    ksteps = _cdiv(M, BK)
    mt, nt = _cdiv(L["K"], BM), _cdiv(L["OC"], _bn_width(L["OC"]))
    ksplit = wgrad_split(mt * nt, ksteps, outf, partial_floats)
    forced, cap_cut = ksplit, False
    if env is not None:
        ksplit = forced = max(1, min(int(env), ksteps))
        while ksplit > 1 and ksplit * outf > partial_floats:
            ksplit -= 1
        cap_cut = ksplit < forced
    requested = ksplit
    per = _cdiv(ksteps, ksplit)
    ksplit = _cdiv(ksteps, per)
    return dict(kind="mfma", M=M, ksteps=ksteps, forced=forced, ksplit=ksplit, ksteps_per=per,
                empty_cut=requested - ksplit, cap_cut=cap_cut, partial=ksplit * outf if ksplit > 1 else 0)


def dgrad_plan(L, N, partial_floats, env=None):
    """plan_dgrad (layers with index > 0): dZ is the image, the depth is kh*kw*Cout, the columns Cin
    padded to a multiple of 4; env = SMH_CNN_DSPLIT.  Unlike the weight gradient there is no rule against empty
    slices: an empty slice writes zeros to its partial block."""
    ldc = (L["C"] + 3) & ~3
    ksteps = _cdiv(L["kh"] * L["kw"] * L["OC"], BK)
    M = N * L["H"] * L["W"]
    ksplit = choose_split(_cdiv(M, BM), _cdiv(ldc, _bn_width(ldc)), ksteps)
    if env is not None:
        ksplit = max(1, min(int(env), ksteps))
    while ksplit > 1 and ksplit * M * ldc > partial_floats:
        ksplit -= 1
    per = _cdiv(ksteps, ksplit)
    return dict(M=M, ldc=ldc, ksteps=ksteps, ksplit=ksplit, ksteps_per=per, empty=ksplit - _cdiv(ksteps, per),
                partial=ksplit * M * ldc if ksplit > 1 else 0)


def col_reduce_plan(M, C):
    """plan_col_reduce (and colred_kernel's own test): vectorised when C/4 divides 256 or is a multiple
    of 256 (then C/1024 column slabs on blockIdx.y), scalar otherwise; the row blocks are re-blocked when more than
    kMaxRed would be needed."""
    cq = C >> 2
    vec = (C & 3) == 0 and ((cq <= 256 and 256 % cq == 0) or cq % 256 == 0)
    rows_per_pass = (256 // cq if cq < 256 else 1) if vec else 1
    slabs = cq // 256 if vec and cq > 256 else 1
    rpb = rows_per_pass * 16 if vec else 64
    nb = _cdiv(M, rpb)
    reblocked = nb > K_MAX_RED
    if reblocked:
        rpb = _cdiv(_cdiv(M, K_MAX_RED), rows_per_pass) * rows_per_pass
        nb = _cdiv(M, rpb)
    return dict(vec=vec, slabs=slabs, rows_per_pass=rows_per_pass, rows_per_block=rpb, blocks=nb, reblocked=reblocked)


def col_reduce_plans(kind, H, W, N, **kw):
    """{layer name: col_reduce plan} over the (N*OH*OW x OC) matrix of every Conv2D / Dense layer: the BatchNorm
    statistics (train_forward, backward_conv) or, without a BatchNorm, the bias gradient (backward_conv)."""
    return {L["name"]: col_reduce_plan(N * L["OH"] * L["OW"], L["OC"]) for L in graph(kind, H, W, **kw)}
