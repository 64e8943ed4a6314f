"""torch (CPU, autograd; float64 or float32) restatement of the single-task Conv2D baselines -- TEST INFRASTRUCTURE, not a test file.

  get_Doukhan_model      lib/baseline_architectures.py:62-108     Doukhan's trunk, Dense(n_classes) softmax; Adam(1e-4)
  get_Papakostas_model   lib/baseline_architectures.py:147-175    Papakostas' trunk, Dense(n_classes) softmax; SGD(ExponentialDecay)
  get_Jang_model         lib/baseline_architectures.py:358-442    ONE mel-scale layer over the (n_fft/2 + 1, W) image (tanh), three
                         [Conv2D 3x3 'same' + BN + ReLU + Dropout(0.4) + MaxPooling2D 2x2 'valid'], Flatten, Dense; l1_l2() (Keras
                         defaults l1 = l2 = 0.01) on the mel kernels and nowhere else; Adam(1e-3)

compiled at :114-117 with binary_crossentropy for two classes -- on BOTH softmax outputs, so Keras' 'accuracy' is binary accuracy over
the N x 2 outputs -- and categorical_crossentropy for three.  Keras / TensorFlow are absent: the layer semantics are restated from
their published definitions as in oracle/cnn_mtl_train.py, whose primitives this file uses ("parity unpinned").  One graph serves
inference (moving statistics, no dropout) and training (batch statistics, masks as INPUTS, 0 or 1 / (1 - rate)).
Weight names and their order are the library's (smh_cnn_tensor_info)."""
import numpy as np
import torch
import torch.nn.functional as Fnn

from oracle import cnn_mtl as oc
from oracle.cnn_mtl_train import BN_EPS, BN_MOMENTUM, KERAS_EPS, _bn_train, _conv, _conv_s, _lrn, _pool, _pool_s

L1 = L2 = 0.01  # tf.keras.regularizers.l1_l2() defaults
KINDS = ("Doukhan", "Papakostas", "Jang")


def jang_shapes(W, n_mels=64):
    h, w_ = n_mels, W
    for _ in range(3):
        h, w_ = h // 2, w_ // 2  # 2x2 stride 2 'valid'
    return h, w_, h * w_ * 128


def feat_dim(kind, H, W, fc=4096, n_mels=64):
    if kind == "Doukhan":
        return 512
    if kind == "Papakostas":
        return fc
    return jang_shapes(W, n_mels)[2]


def init_weights(kind, H, W, n_classes, seed=0, fc=4096, n_mels=64, n_fft=512, fs=16000, mel_signs=False):
    """Generic seeded values (randomised biases and BatchNorm tensors) in the library's tensor order.  Jang: the mel kernels are the
    Slaney weights of the reference's Constant initialiser; mel_signs=True flips the sign of every third weight and zeroes every
    seventh, so that the l1 term sees both signs and exact zeros."""
    rng = np.random.default_rng(seed)
    w = {}
    if kind == "Doukhan":
        full = oc.init_doukhan(seed, H, W, 3, randomize=False)
    elif kind == "Papakostas":
        full = oc.init_papakostas(seed, H, W, 3, randomize=False, fc=fc)
    else:
        M, bins = oc.mel_filter_bins(fs, n_fft, n_mels)
        for i in range(n_mels):
            k = np.repeat(M[i, bins[i, 0]:bins[i, 1] + 1][:, None], 5, axis=1)[:, :, None, None]
            k = np.repeat(k, 3, axis=3).astype(np.float32)
            if mel_signs:
                flat = k.reshape(-1).copy()
                flat[::3] *= -1.0
                flat[::7] = 0.0
                k = flat.reshape(k.shape)
            w["melCl%d/kernel" % i] = k
        full = {}
        for i, (cin, cout) in enumerate([(3, 32), (32, 64), (64, 128)]):
            oc._conv(full, rng, "conv%d" % (i + 1), 3, 3, cin, cout)
            oc._bn(full, "bn%d" % (i + 1), cout)
    for k, v in full.items():
        if k.split("/")[0] not in ("S", "M", "N", "R", "3C"):
            w[k] = v
    D = feat_dim(kind, H, W, fc, n_mels)
    oc._dense_w(w, rng, "dense", D, n_classes)
    mel = {k: v for k, v in w.items() if k.startswith("melCl")}
    oc._randomize(w, rng)
    w.update(mel)
    return w


def _trunk(kind, xt, W, bn, drop, dt, n_mels, n_fft, fs):
    N = xt.shape[0]
    mask = (lambda h, i: h if drop is None else h * torch.tensor(np.asarray(drop[i], dt)).reshape(h.shape))
    if kind == "Doukhan":
        h = torch.relu(bn(_conv(xt, W, "conv1"), "bn1", True))
        h = _pool(h, (2, 2), False)
        h = torch.relu(bn(_conv(h, W, "conv2"), "bn2", True))
        h = torch.relu(bn(_conv(h, W, "conv3"), "bn3", True))
        h = _pool(h, (2, 2), True)
        h = torch.relu(bn(_conv(h, W, "conv4"), "bn4", True))
        h = _pool(h, (1, 12), False).reshape(N, -1)
        for i in range(4):
            p = "fc%d" % (i + 1)
            h = mask(torch.relu(bn(h @ W[p + "/kernel"] + W[p + "/bias"], p + "_bn", False)), i)
        return h
    if kind == "Papakostas":
        h = torch.relu(_lrn(_conv_s(xt, W, "conv1", 2, False)))
        h = _pool_s(h, 3, 2, True)
        h = torch.relu(_lrn(_conv_s(h, W, "conv2", 2, False)))
        h = _pool_s(h, 3, 2, True)
        h = torch.relu(_conv_s(h, W, "conv3", 1, True))
        h = _pool_s(h, 3, 2, True).reshape(N, -1)
        for i in range(2):
            p = "fc%d" % (i + 1)
            h = mask(torch.relu(bn(h @ W[p + "/kernel"] + W[p + "/bias"], p + "_bn", False)), i)
        return h
    _, bins = oc.mel_filter_bins(fs, n_fft, n_mels)
    xn = xt.permute(0, 3, 1, 2)  # (N, 1, K, W)
    rows = []
    for i in range(n_mels):
        k = W["melCl%d/kernel" % i]  # (width, 5, 1, 3): stride (width, 1), 'same' -> one row
        band = xn[:, :, int(bins[i, 0]):int(bins[i, 1]) + 1]
        rows.append(Fnn.conv2d(band, k.permute(3, 2, 0, 1), padding=(0, k.shape[1] // 2)))
    h = torch.tanh(torch.cat(rows, dim=2)).permute(0, 2, 3, 1)  # (N, n_mels, W, 3)
    for i in range(3):
        h = mask(torch.relu(bn(_conv_s(h, W, "conv%d" % (i + 1), 1, True), "bn%d" % (i + 1), True)), i)
        h = _pool_s(h, 2, 2, False)
    return h.reshape(N, -1)


def _graph(kind, x, w, train, drop, dtype, n_mels, n_fft, fs):
    W = {k: torch.tensor(np.asarray(v, dtype), requires_grad=train and not k.endswith(("moving_mean", "moving_variance")))
         for k, v in w.items()}
    stats = {}

    def bn(z, p, fused):
        if train:
            return _bn_train(z, W, p, stats, fused)
        return (z - W[p + "/moving_mean"]) / torch.sqrt(W[p + "/moving_variance"] + BN_EPS) * W[p + "/gamma"] + W[p + "/beta"]

    xt = torch.tensor(np.asarray(x, dtype)).reshape(len(x), np.shape(x)[1], np.shape(x)[2], 1)
    feat = _trunk(kind, xt, W, bn, drop, dtype, n_mels, n_fft, fs)
    probs = torch.softmax(feat @ W["dense/kernel"] + W["dense/bias"], dim=1)
    return W, stats, feat, probs


def forward(kind, x, w, dtype=np.float64, n_mels=64, n_fft=512, fs=16000):
    """Inference: x (N, H, W[, 1]) -> (softmax (N, n_classes), features (N, D)) as float64 arrays."""
    with torch.no_grad():
        _, _, feat, probs = _graph(kind, x, w, False, None, dtype, n_mels, n_fft, fs)
    return probs.double().numpy(), feat.double().numpy()


def loss_and_accuracy(probs, t, n_classes):
    """Keras' loss and 'accuracy' metric of the compiled single-task model on torch tensors (autograd passes through the loss)."""
    pc = torch.clamp(probs, KERAS_EPS, 1 - KERAS_EPS)
    if n_classes == 2:
        loss = torch.mean(-(t * torch.log(pc + KERAS_EPS) + (1 - t) * torch.log(1 - pc + KERAS_EPS)))
        acc = float(((probs > 0.5) == (t > 0.5)).double().mean())
    else:
        pc = torch.clamp(probs / probs.sum(dim=1, keepdim=True), KERAS_EPS, 1 - KERAS_EPS)
        loss = torch.mean(-torch.sum(t * torch.log(pc), dim=1))
        acc = float((probs.argmax(1) == t.argmax(1)).double().mean())
    return loss, acc


def penalty(kind, w):
    """l1_l2() on Jang's mel kernels: 0.01 * sum w^2 + 0.01 * sum |w|; no other kernel of the three models is regularised."""
    if kind != "Jang":
        return 0.0
    return float(sum(L2 * np.sum(np.asarray(v, np.float64) ** 2) + L1 * np.sum(np.abs(np.asarray(v, np.float64)))
                     for k, v in w.items() if k.startswith("melCl")))


def forward_backward(kind, x, y, w, n_classes, drop=None, dtype=np.float64, n_mels=64, n_fft=512, fs=16000):
    """One training forward + backward.  y one-hot (N, n_classes).  Returns dict(loss (data loss), acc, penalty, grads (without the
    regulariser's term), bn_batch {name: (mean, variance for the moving update)}, probs, features)."""
    W, stats, feat, probs = _graph(kind, x, w, True, drop, dtype, n_mels, n_fft, fs)
    t = torch.tensor(np.asarray(y, dtype)).reshape(probs.shape)
    loss, acc = loss_and_accuracy(probs, t, n_classes)
    loss.backward()
    grads = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in W.items() if v.requires_grad}
    return dict(loss=float(loss.detach()), acc=acc, penalty=penalty(kind, w), grads=grads, bn_batch=stats,
                probs=probs.detach().double().numpy(), features=feat.detach().double().numpy())


def inference_losses(kind, x, y, w, n_classes, **kw):
    """[loss + penalty, accuracy] in inference mode: what `evaluate` reports."""
    probs, _ = forward(kind, x, w, **kw)
    loss, acc = loss_and_accuracy(torch.tensor(probs), torch.tensor(np.asarray(y, np.float64)), n_classes)
    return [float(loss) + penalty(kind, w), acc]


def _reg_grad(kind, k, val):
    """d penalty / d w of tensor k: 2 l2 w + l1 sign(w), sign(0) = 0 as tf.abs differentiates."""
    return 2 * L2 * val + L1 * np.sign(val) if (kind == "Jang" and k.startswith("melCl")) else 0.0


def _moving(k, val, bn_batch):
    mean, var = bn_batch[k.rsplit("/", 1)[0]]
    return BN_MOMENTUM * val + (1 - BN_MOMENTUM) * (mean if k.endswith("moving_mean") else var)


def sgd_step(kind, w, grads, bn_batch, lr):
    """Keras SGD without momentum + the regulariser's term + the BatchNorm moving statistics."""
    nw = {}
    for k, val in w.items():
        val = np.asarray(val, np.float64)
        moving = k.endswith(("moving_mean", "moving_variance"))
        nw[k] = _moving(k, val, bn_batch) if moving else val - lr * (grads[k] + _reg_grad(kind, k, val))
    return nw


def adam_step(kind, w, grads, m, v, bn_batch, step, lr, beta1=0.9, beta2=0.999, eps=1e-7):
    """Keras Adam (`step` counts from 1) + the regulariser's term + the moving statistics -> (new_w, new_m, new_v)."""
    alpha = lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    nw, nm, nv = {}, {}, {}
    for k, val in w.items():
        val = np.asarray(val, np.float64)
        if k.endswith(("moving_mean", "moving_variance")):
            nw[k] = _moving(k, val, bn_batch)
            continue
        g = grads[k] + _reg_grad(kind, k, val)
        nm[k] = beta1 * np.asarray(m.get(k, 0.0)) + (1 - beta1) * g
        nv[k] = beta2 * np.asarray(v.get(k, 0.0)) + (1 - beta2) * g * g
        nw[k] = val - alpha * nm[k] / (np.sqrt(nv[k]) + eps)
    return nw, nm, nv
