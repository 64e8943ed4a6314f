"""Late fusion (Late_Fusion_Results.py:388-513): an ensemble of two complete models of one architecture -- model H trained on the
harmonic half of the H||P featuregram ('LogMelHarmSpec'), model P on the percussive half ('LogMelPercSpec') -- whose '3C' outputs
are blended on the device:

    pred = alpha * pred_H + (1 - alpha) * pred_P,    pred_lab = argmax(pred)          (:422-423, alpha = 0.5 at :646)

`LateFusion` runs both models as ONE launch of the B3_MTL forward kernel (a second grid row is model P) and the blend as one small
kernel behind it (csrc/smh_late_fusion.hip); nothing crosses to the host.  The blend rounds as numpy does on float32 arrays -- two
rounded products, one rounded sum -- so `predict` equals the reference's expression bit for bit on the two models' own outputs.
Each model is trained alone (`fit` on its half feature); the ensemble only borrows them and follows their weights.

`predict_file` / `test_model` restate the driver's file-wise test loop with ONE featuregram pass per file: both half feature names
produce the same H||P array (lib/preprocessing.py:414-424), which the reference computes (or loads) once per model.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .host import f32_cuda, ptr, to_f32_cuda, workspace
from .model import B3MTL


class LateFusion:
    """LateFusion(model_H, model_P, alpha=0.5): two B3MTL or two CascadedMTL models of one geometry (n_feat = the width of ONE
    half).  Inputs are [x_H, x_P] or {'harm_input': x_H, 'perc_input': x_P}, each (N, W, n_feat) time-major.  The one output is the
    blended '3C' (N, n_classes); the models' own outputs come back through `heads=` / `predict_heads`.  f32 only; no training."""

    LATE_FUSION = True
    INPUT_NAMES = ("harm_input", "perc_input")
    output_names = ["3C"]
    block_variant = 0

    def __init__(self, model_H, model_P, alpha=0.5):
        for m in (model_H, model_P):
            if not isinstance(m, B3MTL):
                raise TypeError("LateFusion takes two B3MTL or CascadedMTL models, got %s" % type(m).__name__)
        self.lib = _lib.require_gpu()
        self.models = (model_H, model_P)  # (kept alive: the C handle borrows them)
        self.alpha = alpha
        h = C.c_void_p()
        _lib.check(self.lib.smh_late_fusion_create(model_H._h, model_P._h, C.byref(h)), "smh_late_fusion_create")
        self._h = h
        self.n_feat, self.patch_size, self.n_classes = model_H.n_feat, model_H.patch_size, model_H.n_classes
        self.out_dim = self.n_classes
        self.heads_dim = model_H.out_dim  # width of each model's own [S|M|(N)|R|3C]

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.smh_late_fusion_destroy(h)
            self._h = None

    @property
    def alpha(self):
        return self._alpha

    @alpha.setter
    def alpha(self, value):
        value = float(value)
        if not 0.0 <= value <= 1.0:  # (a NaN fails both comparisons)
            raise ValueError("late-fusion alpha must lie in [0, 1], got %r" % (value,))
        self._alpha = value

    def split_outputs(self, out):
        """(N, n_classes) -> ['3C'] (the ensemble has the one blended output)."""
        return [out]

    def _sync_weights(self):
        for m in self.models:
            m._sync_weights()

    def _call(self, entry, *args):
        return _lib.check(getattr(self.lib, entry)(*args, _lib.current_stream()), entry)

    def check_status(self):
        """Wait for the current stream and raise RuntimeError if a forward recorded in either model's device error word that its
        outputs are not results (smh_model_status on each model)."""
        for m in self.models:
            m.check_status()

    # ---- inputs and outputs ----
    def _pair(self, x):
        if isinstance(x, dict):
            if set(x) != set(self.INPUT_NAMES):
                raise ValueError("the late-fusion ensemble takes the inputs %s, got %s" % (list(self.INPUT_NAMES), sorted(x)))
            x = [x[k] for k in self.INPUT_NAMES]
        if not isinstance(x, (list, tuple)) or len(x) != 2:
            raise TypeError("the late-fusion ensemble takes two inputs: [x_H, x_P] or {'harm_input': x_H, 'perc_input': x_P}")
        for a in x:
            if not isinstance(a, (np.ndarray, torch.Tensor)):
                raise TypeError("inputs must be numpy arrays or torch tensors, got %s" % type(a).__name__)
        xh, xp = (self.models[0]._check_patches(to_f32_cuda(a), "each input") for a in x)
        if xh.shape[0] != xp.shape[0]:
            raise ValueError("harm_input has %d patches, perc_input %d" % (xh.shape[0], xp.shape[0]))
        return xh, xp

    def _outputs(self, N, device, out, labels, heads):
        """The three output tensors, checked when given: pred (N, n_classes) f32, labels (N) int32 or None, heads (2, N, heads_dim)
        f32 or None."""
        if out is None:
            out = torch.empty((N, self.n_classes), dtype=torch.float32, device=device)
        for t, shape, dt, what in ((out, (N, self.n_classes), torch.float32, "out"), (labels, (N,), torch.int32, "labels"),
                                   (heads, (2, N, self.heads_dim), torch.float32, "heads")):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and tuple(t.shape) == shape
                                      and t.is_contiguous()):
                raise ValueError("%s must be a contiguous %s CUDA tensor of shape %s" % (what, str(dt).replace("torch.", ""), shape))
        return out

    def _run(self, entry, ws_entry, ws_args, head_args, N, device, out, labels, heads):
        nbytes = getattr(self.lib, ws_entry)(self._h, *ws_args)
        work = workspace(nbytes, device)
        return self._call(entry, self._h, *head_args, C.c_double(self._alpha), ptr(work), nbytes, ptr(out), ptr(labels), ptr(heads))

    # ---- the three entries ----
    def forward_device(self, x, out=None, labels=None, heads=None):
        """x: [x_H, x_P] (or the dict) -> the blended '3C' (N, n_classes) on the device (smh_late_fusion_forward_f32).  labels: int32
        (N) tensor that receives argmax(pred); heads: (2, N, heads_dim) tensor that receives model H's and model P's own
        [S|M|(N)|R|3C] -- bit for bit what their forward_device returns."""
        xh, xp = self._pair(x)
        self._sync_weights()
        N = xh.shape[0]
        out = self._outputs(N, xh.device, out, labels, heads)
        if N:
            self._run("smh_late_fusion_forward_f32", "smh_late_fusion_workspace_bytes", (N,), (ptr(xh), ptr(xp), N), N, xh.device,
                      out, labels, heads)
        return out

    def w0_ptr(self):
        """Device address of the (2 * n_feat, 32) layer-0 kernels, model H's then model P's (smh_late_fusion_w0_ptr): the `w0` of
        Frontend.features_l0 for the ensemble.  Follows the weights of both models."""
        self._sync_weights()
        w0 = self.lib.smh_late_fusion_w0_ptr(self._h, _lib.current_stream())
        if not w0:
            raise RuntimeError("smh_late_fusion_w0_ptr: " + _lib.last_error())
        return w0

    def forward_from_x0_halves(self, x0p, out=None, labels=None, heads=None):
        """x0p (N, 2, W, 32) as Frontend.features_l0(..., model=self) wrote it -- half 0 is model H's complete first layer, half 1
        model P's -- -> the blended '3C' (N, n_classes) (smh_late_fusion_forward_x0_f32)."""
        x0p = self.models[0]._check_x0p(f32_cuda(x0p, "forward_from_x0_halves"))
        self._sync_weights()
        N = x0p.shape[0]
        out = self._outputs(N, x0p.device, out, labels, heads)
        if N:
            self._run("smh_late_fusion_forward_x0_f32", "smh_late_fusion_x0_workspace_bytes", (N,), (ptr(x0p), N), N, x0p.device,
                      out, labels, heads)
        return out

    def forward_dense(self, fv, shift=1, out=None, labels=None, heads=None, dtype="f32"):
        """Every hop-`shift` patch of a standardised H||P featuregram fv (2 * n_feat, Tc) through both models and the blend without
        building the patches (smh_late_fusion_forward_dense_f32): layer 0 of both models once per frame, every patch a window of it.
        Returns (nP, n_classes), nP = tools.extract_patches' count for Tc frames.  Needs Tc >= patch_size and n_feat % 4 == 0.
        dtype: "f32" only (B3_MTL is the only model with a bf16 path)."""
        if dtype == "bf16":
            raise ValueError("dtype='bf16': B3_MTL with the keras-tcn 2.3.x block is the only model with a bf16 path; the late-fusion "
                             "ensemble has the f32 forward only")
        if dtype != "f32":
            raise ValueError("dtype must be 'f32' or 'bf16' (split bf16 operands), got %r" % (dtype,))
        fv = f32_cuda(fv, "forward_dense")
        if fv.dim() != 2 or fv.shape[0] != 2 * self.n_feat:
            raise ValueError("expected the H||P featuregram (%d, Tc), got %s" % (2 * self.n_feat, tuple(fv.shape)))
        Tc, shift = int(fv.shape[1]), int(shift)
        self._sync_weights()
        nP = self.lib.smh_num_patches(Tc, self.patch_size, shift) if Tc >= self.patch_size else -1
        if nP < 0:
            raise ValueError("forward_dense needs shift >= 1 and at least patch_size=%d frames, got Tc=%d shift=%d" % (self.patch_size, Tc, shift))
        out = self._outputs(nP, fv.device, out, labels, heads)
        if nP:
            got = self._run("smh_late_fusion_forward_dense_f32", "smh_late_fusion_dense_workspace_bytes", (Tc, shift),
                            (ptr(fv), Tc, shift), nP, fv.device, out, labels, heads)
            if got != nP:
                raise RuntimeError("smh_late_fusion_forward_dense_f32 produced %d patches, expected %d" % (got, nP))
        return out

    # ---- the reference's predict surface ----
    def predict(self, x, batch_size=None, verbose=0):
        """The reference's `pred` (:422): the blended '3C' as a float32 numpy array (N, n_classes)."""
        out = self.forward_device(x)
        self.check_status()
        return out.cpu().numpy()

    def predict_classes(self, x):
        """The reference's `pred_lab` (:423): np.argmax(pred, axis=1), computed on the device."""
        xh, xp = self._pair(x)
        labels = torch.empty((xh.shape[0],), dtype=torch.int32, device=xh.device)
        self.forward_device([xh, xp], labels=labels)
        self.check_status()
        return labels.cpu().numpy().astype(np.int64)

    def predict_heads(self, x):
        """[model_H.predict(x_H), model_P.predict(x_P)]: each model's own output list [S, M, (N,) R, 3C], from the same launch."""
        xh, xp = self._pair(x)
        heads = torch.empty((2, xh.shape[0], self.heads_dim), dtype=torch.float32, device=xh.device)
        self.forward_device([xh, xp], heads=heads)
        self.check_status()
        host = heads.cpu().numpy()
        return [[np.ascontiguousarray(o) for o in m.split_outputs(host[i])] for i, m in enumerate(self.models)]


# ---- the driver's file-wise test loop ----------------------------------------------------------------------------------------------
def _file_patches(PARAMS, file_name_sp, file_name_mu, target_dB):
    """The two models' inputs for ONE test file, (nP, W, n_feat) time-major device tensors each: test_file_wise_generator (:344-381) for
    PARAMS_H and PARAMS_P (:393-399) with one featuregram pass."""
    from .generators import harm_perc_sibling
    from .lib import preprocessing as pp
    model = PARAMS['Model']
    names = PARAMS['featName'][model]
    if isinstance(names, str) or len(names) != 2:
        raise ValueError("late fusion: PARAMS['featName'][Model] is the pair [H feature name, P feature name], got %r" % (names,))
    if harm_perc_sibling(names[0]) != harm_perc_sibling(names[1]) or 'HarmSpec' not in names[0] or 'PercSpec' not in names[1]:
        raise ValueError("late fusion: %r are not the harmonic and the percussive half of one feature" % (list(names),))
    if PARAMS.get('frame_level_scaling') or PARAMS.get('skewness_vector'):
        raise ValueError("frame_level_scaling / skewness_vector are not wired into this path")
    if file_name_mu == '':
        spec = ('speech', file_name_sp, '', None)
    elif file_name_sp == '':
        spec = ('music', '', file_name_mu, None)
    else:
        spec = ('speech_music', file_name_sp, file_name_mu, target_dB)
    # both names give the H||P featuregram (lib/preprocessing.py:414-424): computed, or loaded from the H cache, once
    fv = pp.get_featuregram(PARAMS, spec[0], PARAMS['feature_opDir_H'], spec[1], spec[2], spec[3], PARAMS['n_fft'][model],
                            PARAMS['n_mels'][model], names[0], save_feat=True)
    fe = pp._frontend_for(pp._fe.FrontendConfig())
    d = to_f32_cuda(np.asarray(fv))
    R = d.shape[0] // 2
    # get_feature_patches per half (:359): tile if short, StandardScaler over the file, hop-W_shift patches, transposed for the TCN (:369)
    return [fe.extract_patches(fe.standardize_rows(rows)[None], PARAMS['W'], PARAMS['W_shift'], time_major=True)
            for rows in (d[:R], d[R:])]


def predict_file(PARAMS, ensemble, file_name_sp, file_name_mu, target_dB):
    """(pred, pred_lab) of one test file (:412-429, 469-485): `pred` float32 (nP, n_classes), `pred_lab` = argmax.  PARAMS as the
    driver builds it: featName[Model] = [H name, P name], feature_opDir_H (the featuregram cache), W, W_shift, late_fusion_alpha
    (when present it is the alpha of this call; the ensemble's own alpha is left as it was)."""
    own = ensemble.alpha
    try:
        if 'late_fusion_alpha' in PARAMS:
            ensemble.alpha = PARAMS['late_fusion_alpha']
        xh, xp = _file_patches(PARAMS, file_name_sp, file_name_mu, target_dB)
        labels = torch.empty((xh.shape[0],), dtype=torch.int32, device=xh.device)
        pred = ensemble.forward_device([xh, xp], labels=labels)
    finally:
        ensemble.alpha = own
    ensemble.check_status()
    return pred.cpu().numpy(), labels.cpu().numpy().astype(np.int64)


def confusion_matrix(PtdLabels, GroundTruth, n_classes):
    """Count table C[i][j] = patches of true class i predicted as class j (sklearn.metrics.confusion_matrix's orientation)."""
    cm = np.zeros((n_classes, n_classes), np.int64)
    np.add.at(cm, (np.asarray(GroundTruth, np.int64), np.asarray(PtdLabels, np.int64)), 1)
    return cm


def test_model(PARAMS, ensemble, target_dB):
    """The driver's test loop (:388-513) over PARAMS['test_files'] -> (PtdLabels, Predictions, GroundTruth, ConfMat).  target_dB None:
    the music and speech files, then (3 classes) the speech+music pairs at their annotated SMR; else the pairs alone at target_dB.
    ConfMat: plain counts (`confusion_matrix`)."""
    import os
    preds, labs, truth = [], [], []

    def add(pred, lab, cls):
        preds.append(pred), labs.append(lab), truth.append(np.full(len(lab), cls, np.int64))

    if target_dB is None:
        for classname, cls in (('music', 0), ('speech', 1)):
            for fl in PARAMS['test_files'][classname]:
                fName = PARAMS['folder'] + '/' + classname + '/' + fl
                if not os.path.exists(fName):
                    continue
                sp, mu = (fName, '') if classname == 'speech' else ('', fName)
                add(*predict_file(PARAMS, ensemble, sp, mu, None), cls)
    if len(PARAMS['classes']) == 3:
        for info in PARAMS['test_files']['speech+music']:
            smr = info['SMR'] if target_dB is None else target_dB
            add(*predict_file(PARAMS, ensemble, PARAMS['folder'] + '/speech/' + info['speech'],
                              PARAMS['folder'] + '/music/' + info['music'], smr), 2)
    n_classes = len(PARAMS['classes'])
    if not preds:
        return np.zeros((0,), np.int64), np.zeros((0, n_classes), np.float32), np.zeros((0,), np.int64), confusion_matrix([], [], n_classes)
    PtdLabels, Predictions, GroundTruth = np.concatenate(labs), np.concatenate(preds, 0), np.concatenate(truth)
    return PtdLabels, Predictions, GroundTruth, confusion_matrix(PtdLabels, GroundTruth, n_classes)


test_model.__test__ = False  # (the reference's function name; not a pytest case)
