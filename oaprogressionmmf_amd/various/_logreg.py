"""scikit-learn's LogisticRegression (L2, fit_intercept, the lbfgs defaults of koafusion/run/train_prog_clin.py) on the device.

The objective is strictly convex, so its minimiser is unique; scikit-learn's lbfgs stops at a projected gradient of 1e-4 on a
nearly collinear design (every one-hot group sums to the intercept column) and is therefore far from that minimiser in coefficient
space and close in probability space.  The device solves for the minimiser itself, with a damped Newton step in fp64
(ops.logreg_fit): parity with scikit-learn is a statement about decision_function and predict_proba, never about
coef_.  All problems of a call -- every fold times every class weight -- are fitted by one launch, one block each: a sample-weight
row per problem, where 0 takes a row out, carries fold membership and class weights alike.
"""
import numpy as np
import torch

from .. import ops
from ._metrics import _device, _on_device

DEFAULT_TOL = 1e-10          # on |grad|_inf of the scaled objective; Newton usually lands orders of magnitude below it
DEFAULT_MAX_ITER = 100


def _is_dev(a):
    return torch.is_tensor(a) and a.is_cuda


def _matrix(X, dev):
    X = _on_device(X, dev)
    if X.dim() != 2:
        raise ValueError(f"Expected 2D array, got {X.dim()}D array instead")
    return X.to(torch.float64).contiguous()


def _back(t, as_device):
    return t if as_device else t.cpu().numpy()


def class_weight_rows(y01, class_weight):
    """fp64 [n] device weights of one class_weight setting over the rows of y01 (a 0 / 1 device vector): None -> 1, "balanced" ->
    n / (2 count(y_i)) as compute_class_weight gives it, {0: a, 1: b} -> a or b.  Nothing is read back."""
    n = int(y01.numel())
    if class_weight is None:
        return torch.ones(n, dtype=torch.float64, device=y01.device)
    if isinstance(class_weight, dict):
        w = torch.tensor([float(class_weight.get(0, 1.0)), float(class_weight.get(1, 1.0))], dtype=torch.float64, device=y01.device)
    elif class_weight == "balanced":
        n1 = y01.sum().to(torch.float64)
        w = float(n) / (2.0 * torch.stack([float(n) - n1, n1]))
    else:
        raise ValueError(f"class_weight must be None, 'balanced' or a dict, got {class_weight!r}")
    return w[y01.long()]


def fold_weight_rows(y01, folds, class_weights):
    """sw [len(class_weights) * len(folds), n] on the device: problem ci * F + f holds the training rows of fold f under class
    weight ci (computed on that fold's training rows, as a fit on X[train] computes it) and 0 everywhere else."""
    n, F = int(y01.numel()), len(folds)
    sw = torch.zeros((len(class_weights) * F, n), dtype=torch.float64, device=y01.device)
    for f, (tr, _) in enumerate(folds):
        tr = _on_device(np.asarray(tr) if not torch.is_tensor(tr) else tr, y01.device).long()
        for ci, cw in enumerate(class_weights):
            sw[ci * F + f, tr] = class_weight_rows(y01[tr], cw)
    return sw


def fit_logreg_folds(X, y, folds, class_weights=(None,), C=1.0, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, flag=None):
    """The batched fit: every (class weight, fold) problem in ONE koaf_logreg_fit launch.  X (n, D) and y (n,) of 0 / 1 are numpy
    arrays or device tensors, folds the reference's list of (train_idx, val_idx) pairs.
    -> (W [len(class_weights) * len(folds), D + 1] with the intercept last, report [.., 4]) as device tensors, problem
    ci * len(folds) + f being fold f under class_weights[ci].  flag: an ops.clin_flag() word to raise into instead of the own one
    that is read back here."""
    dev = _device(X, y)
    Xd = _matrix(X, dev)
    y01 = _on_device(y, dev).reshape(-1).to(torch.int32).contiguous()
    if int(y01.numel()) != int(Xd.shape[0]):
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{int(Xd.shape[0])}, {int(y01.numel())}]")
    if len(folds) < 1 or len(class_weights) < 1:
        raise ValueError("fit_logreg_folds: at least one fold and one class weight")
    sw = fold_weight_rows(y01, folds, class_weights)
    return ops.logreg_fit(Xd, y01, sw, C=C, max_iter=max_iter, tol=tol, flag=flag)


class LogisticRegression(object):
    """sklearn.linear_model.LogisticRegression for binary targets: penalty "l2", fit_intercept, no multi_class.  Takes numpy arrays
    or device tensors and returns the same kind.  tol bounds |grad|_inf of the objective scaled by 1 / sum(sample weights), which
    is not scikit-learn's lbfgs criterion: the default is set for the minimiser, not for parity of stopping points."""

    def __init__(self, C=1.0, class_weight=None, random_state=None, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER):
        self.C, self.class_weight, self.random_state, self.tol, self.max_iter = C, class_weight, random_state, tol, max_iter

    def get_params(self, deep=True):
        return {"C": self.C, "class_weight": self.class_weight, "random_state": self.random_state, "tol": self.tol,
                "max_iter": self.max_iter}

    def fit(self, X, y, sample_weight=None):
        labels = (y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)).reshape(-1)
        classes = np.unique(labels)
        if classes.shape[0] > 2:
            raise ValueError(f"LogisticRegression here is binary: the target holds {classes.shape[0]} classes")
        if classes.shape[0] < 2:
            raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: "
                             f"{classes[0]!r}")
        dev = _device(X, y)
        self._dev_out = _is_dev(X)
        Xd = _matrix(X, dev)
        if int(Xd.shape[0]) != labels.shape[0]:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{int(Xd.shape[0])}, {labels.shape[0]}]")
        y01 = torch.from_numpy((labels == classes[1]).astype(np.int32)).to(dev)
        cw = self.class_weight
        if isinstance(cw, dict):
            cw = {0: cw.get(classes[0].item(), 1.0), 1: cw.get(classes[1].item(), 1.0)}
        sw = class_weight_rows(y01, cw)
        if sample_weight is not None:
            sw = sw * _on_device(sample_weight, dev).reshape(-1).to(torch.float64)
        W, report = ops.logreg_fit(Xd, y01, sw.reshape(1, -1).contiguous(), C=self.C, max_iter=self.max_iter, tol=self.tol)
        self._W = W
        self.classes_ = classes
        self.coef_ = _back(W[:, :-1], self._dev_out)
        self.intercept_ = _back(W[:, -1], self._dev_out)
        self.n_features_in_ = int(Xd.shape[1])
        rep = report.cpu().numpy()
        self.n_iter_ = np.array([int(rep[0, 0])], np.int32)
        self.grad_norm_, self.objective_ = float(rep[0, 1]), float(rep[0, 2])
        return self

    def _predict(self, X):
        dev = self._W.device
        return ops.logreg_predict(self._W, _matrix(X, dev)), _is_dev(X)

    def decision_function(self, X):
        res, d = self._predict(X)
        return _back(res["decision"][0], d)

    def predict_proba(self, X):
        res, d = self._predict(X)
        return _back(res["proba"][0], d)

    def predict_log_proba(self, X):
        p = self.predict_proba(X)
        return torch.log(p) if torch.is_tensor(p) else np.log(p)

    def predict(self, X):
        res, d = self._predict(X)
        idx = (res["decision"][0] > 0).long()
        if d:
            return torch.from_numpy(self.classes_).to(idx.device)[idx] if self.classes_.dtype.kind in "iufb" else idx
        return self.classes_[idx.cpu().numpy()]
