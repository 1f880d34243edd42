"""The logistic-regression half of koafusion/run/train_prog_clin.py on the device: the clinical baselines (age, sex, BMI and,
optionally, KL grade, injury, surgery, WOMAC) every fusion model of the paper is compared against.

clin_design is ProgressionPrediction.fit's preprocessing (:91-149): StandardScaler for age / BMI / WOMAC, OneHotEncoder for sex /
KL / injury / surgery, fitted on the train-validation rows, the columns in the reference's order.  clin_fit is the rest of it for
"LR" (:151-239): the grid over class_weight by mean held-out score (or the "previous best"), the per-fold fits with their
held-out test_score, and the fold ensemble on the test set, returned in the dict layout the reference pickles.

All fits of a call are one launch (various.fit_logreg_folds), the held-out scores come from the metric kernels the fusion models
are scored with, and nothing is read back between the fit and the scores: one host copy fetches the flag words and the scores.

Not here, on purpose: the DecisionTreeClassifier half.  Its "previous best" uses max_features="log2", so every split draws its
candidate features from scikit-learn's private per-tree generator stream, and ties between equal splits are broken by that
stream as well; reproducing it is a project of its own.  Reading the OAI tables, hydra, pickling and the fold splitter stay the
reference's too: `folds` comes in as its list of (train_idx, val_idx) pairs.
"""
import numpy as np
import torch

from .. import ops
from ..various._logreg import DEFAULT_MAX_ITER, DEFAULT_TOL, _is_dev, _matrix, fit_logreg_folds
from ..various._metrics import _device, _on_device, macro_recall_from_counts

VAR_TO_COL = {"age": "AGE", "sex": "P02SEX", "bmi": "P01BMI", "kl": "XRKL", "inj": "P01INJ-", "surg": "P01KSURG-", "womac": "WOMTS-"}
VAR_ORDER = ("age", "sex", "bmi", "kl", "inj", "surg", "womac")      # age, sex, bmi always; the others when the model asks
VAR_ONEHOT = {"age": False, "sex": True, "bmi": False, "kl": True, "inj": True, "surg": True, "womac": False}
CRITERIA = ("average_precision", "roc_auc", "balanced_accuracy", "neg_log_loss")
PARAM_GRID = {"LR": {"class_weight": [None, "balanced"]}}
PREV_BEST = {"LR": {"class_weight": "balanced"}}
DT_REASON = ("the DecisionTreeClassifier baseline is not implemented: its max_features='log2' setting draws the candidate features "
             "of every split from scikit-learn's private per-tree generator stream, which also breaks ties between equal splits")


def _column(columns, name):
    col = columns[name]
    col = col.detach().cpu().numpy() if torch.is_tensor(col) else np.asarray(col)
    return np.ascontiguousarray(col, np.float64).reshape(-1)


def clin_vars(vars=()):
    """the reference's variable order for a model: age, sex, bmi, then kl / inj / surg / womac where `vars` names them"""
    unknown = [v for v in vars if v not in VAR_ORDER]
    if unknown:
        raise ValueError(f"Unknown clinical variables: {unknown} (of {VAR_ORDER})")
    return tuple(v for v in VAR_ORDER if v in ("age", "sex", "bmi") or v in vars)


def clin_design(columns_trainval, columns_test, vars=(), device=None):
    """-> (X_trainval [n, D], X_test [m, D]) fp64 design matrices.  columns_* map the reference's column names (VAR_TO_COL) to 1-D
    arrays: a DataFrame works, and so does a dict of numpy arrays or tensors.  The scalers and encoders are fitted on the
    train-validation rows; a category of the test rows that those lack raises ValueError, as OneHotEncoder does, and so does a
    NaN.  numpy columns give numpy matrices; device=... (or device tensors as columns) leaves them on the device."""
    names = clin_vars(vars)
    tv = np.stack([_column(columns_trainval, VAR_TO_COL[v]) for v in names])
    te = np.stack([_column(columns_test, VAR_TO_COL[v]) for v in names])
    on_dev = device is not None or any(_is_dev(columns_trainval[VAR_TO_COL[v]]) for v in names)
    dev = torch.device(device) if device is not None else _device(*[columns_trainval[VAR_TO_COL[v]] for v in names])
    cats = [np.unique(tv[i]) if VAR_ONEHOT[v] else None for i, v in enumerate(names)]
    ncat = [0 if c is None else int(c.shape[0]) for c in cats]
    flag = ops.clin_flag(dev)
    X_tv, stats = ops.clin_design(torch.from_numpy(tv).to(dev), ncat, cats, flag=flag)
    X_te, _ = ops.clin_design(torch.from_numpy(te).to(dev), ncat, cats, stats=stats, flag=flag)
    ops.clin_raise(flag.item())
    return (X_tv, X_te) if on_dev else (X_tv.cpu().numpy(), X_te.cpu().numpy())


def pack_result(proba_foldw, ens_proba, ens_pred, target, extra=None):
    """the dict the reference pickles per classifier (:224-239): `extra` (its vars_test.to_dict(orient="list")) first, then
    predict_proba__k / predict__k per fold, predict_proba, predict, target"""
    out = dict(extra) if extra is not None else {}
    for f in range(len(proba_foldw)):
        p = proba_foldw[f]
        out[f"predict_proba__{f}"] = p
        out[f"predict__{f}"] = torch.argmax(p, dim=1) if torch.is_tensor(p) else np.argmax(p, axis=1)
    out.update({"predict_proba": ens_proba, "predict": ens_pred, "target": target})
    return out


def _check_request(criterion, params_init, clfs):
    for name in clfs:
        if name == "DT":
            raise NotImplementedError(DT_REASON)
        if name != "LR":
            raise ValueError(f"Unknown classifier: {name!r} (LR; DT is not implemented)")
    if criterion not in CRITERIA:
        raise ValueError(f"Unknown criterion: {criterion!r} (one of {CRITERIA})")
    if params_init not in ("prev_best", "grid_search"):
        raise ValueError(f"Unknown `params_init`: {params_init}")


def heldout_scores(criterion, W, X, y01, folds, n_weights, mflag):
    """The held-out score of every problem of W (problem ci * F + f scored on fold f's validation rows), all launches queued and
    nothing read back: -> a device tensor that score_values turns into numbers on the host.  average_precision and roc_auc rank
    the DECISION values (scikit-learn's scorers take decision_function for this estimator) through ops.score_ranks /
    ops.curve_metrics; balanced_accuracy counts decision > 0 against the labels with ops.confusion; neg_log_loss is
    koaf_logreg_predict's masked log-loss."""
    F, n, dev = len(folds), int(X.shape[0]), X.device
    K = F * n_weights
    vals = [_on_device(np.asarray(va) if not torch.is_tensor(va) else va, dev).long() for _, va in folds]
    if criterion == "neg_log_loss":
        mask = torch.zeros((K, n), dtype=torch.int32, device=dev)
        for k in range(K):
            mask[k, vals[k % F]] = 1
        return ops.logreg_predict(W, X, y=y01, mask=mask)["logloss"]
    dec = ops.logreg_predict(W, X)["decision"]
    if criterion == "balanced_accuracy":
        out = torch.zeros((K, 2, 2), dtype=torch.int64, device=dev)
        for k in range(K):
            va = vals[k % F]
            ops.confusion(y01[va].contiguous(), (dec[k, va] > 0).to(torch.int32), 2, out=out[k], flag=mflag)
        return out
    out = torch.empty((K, 8), dtype=torch.float64, device=dev)
    for k in range(K):
        va = vals[k % F]
        _, packed = ops.score_ranks(dec[k, va].contiguous(), y01[va].contiguous(), flag=mflag)
        ops.curve_metrics(packed, out=out[k:k + 1], flag=mflag)
    return out


def score_values(criterion, host):
    """the numbers behind heldout_scores' tensor, once it is on the host: -> fp64 [K], greater is better"""
    host = host.numpy()
    if criterion == "neg_log_loss":
        return -host
    if criterion == "balanced_accuracy":
        return np.array([macro_recall_from_counts(cm) for cm in host], np.float64)
    return host[:, 3 if criterion == "average_precision" else 2].copy()


def clin_fit(X_trainval, y_trainval, X_test, y_test, folds, criterion, params_init="prev_best", clfs=("LR",), extra=None, C=1.0,
             tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER):
    """ProgressionPrediction.fit for "LR" on design matrices (clin_design): numpy arrays in, numpy arrays out; device tensors in,
    device tensors out.  y_* hold 0 / 1.  folds: the reference's list of (train_idx, val_idx) pairs over the train-validation rows.
    params_init "grid_search": class_weight in [None, "balanced"] by the mean held-out `criterion` (the first of equal means wins,
    as in GridSearchCV); "prev_best": {"class_weight": "balanced"}.
    -> {"raw_ens": {"LR": the reference's dict: `extra`, predict_proba__k, predict__k, predict_proba, predict, target},
        "params": {"LR": ...}, "test_score": {"LR": fp64 [F], cross_validate's}, "grid_scores": {"LR": fp64 [2, F] or None},
        "coef": {"LR": [F, D + 1], the intercept last}, "n_iter": {"LR": int [F]}}"""
    _check_request(criterion, params_init, clfs)
    as_dev = _is_dev(X_trainval)
    dev = _device(X_trainval, X_test, y_trainval)
    X, Xt = _matrix(X_trainval, dev), _matrix(X_test, dev)
    y01 = _on_device(y_trainval, dev).reshape(-1).to(torch.int32).contiguous()
    F = len(folds)
    res = {"raw_ens": {}, "params": {}, "test_score": {}, "grid_scores": {}, "coef": {}, "n_iter": {}}
    for name in clfs:
        weights = PARAM_GRID[name]["class_weight"] if params_init == "grid_search" else [PREV_BEST[name]["class_weight"]]
        flag, mflag = ops.clin_flag(dev), ops.metrics_flag(dev)
        W, report = fit_logreg_folds(X, y01, folds, weights, C=C, tol=tol, max_iter=max_iter, flag=flag)
        scores_dev = heldout_scores(criterion, W, X, y01, folds, len(weights), mflag)
        ops.clin_raise(flag.item())                         # the first read since the fit was queued
        ops.metrics_raise(mflag.item())
        scores = score_values(criterion, scores_dev.cpu()).reshape(len(weights), F)
        best = int(np.argmax(scores.mean(axis=1)))          # the first maximum
        Wb = W[best * F:(best + 1) * F].contiguous()
        pred = ops.logreg_predict(Wb, Xt, ensemble=True)
        proba, ens, ens_pred = pred["proba"], pred["ens_proba"], pred["ens_pred"].long()
        target = y_test
        if not as_dev:
            proba, ens, ens_pred = proba.cpu().numpy(), ens.cpu().numpy(), ens_pred.cpu().numpy()
            target = y_test.cpu().numpy() if torch.is_tensor(y_test) else np.asarray(y_test)
        res["raw_ens"][name] = pack_result([proba[f] for f in range(F)], ens, ens_pred, target, extra)
        res["params"][name] = {"class_weight": weights[best]}
        res["test_score"][name] = scores[best].copy()
        res["grid_scores"][name] = scores if params_init == "grid_search" else None
        res["coef"][name] = Wb if as_dev else Wb.cpu().numpy()
        res["n_iter"][name] = report[best * F:(best + 1) * F, 0].cpu().numpy().astype(np.int64)
    return res
