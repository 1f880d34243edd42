"""The clinical logistic-regression baseline: design matrix, fit and prediction (koaf_clin.hip)."""
import ctypes
import math

import numpy as np
import torch

from .._lib import KoafError, check, defines, lib
from ._base import FlagWord, _ptr, _stream, check_tensor

LOGREG_MAX_P = defines()["KOAF_LOGREG_MAX_P"]
CLIN_FLAG_TEXT = {1: "Input contains NaN or infinity", 2: "Found unknown categories during transform",
                  4: "This solver needs samples of at least 2 classes in the data, but the data contains only one class",
                  8: "a label other than 0 / 1, a negative sample weight or a fitting-row index outside the table"}
_FLAG = FlagWord(CLIN_FLAG_TEXT)
clin_flag = _FLAG.new           # a zeroed flag word for clin_design / logreg_fit (koaf.h: bit 0 non-finite, 1 unknown category, 2 one class, 3 bad label)
clin_raise = _FLAG.raise_       # the ValueError of a clin flag word read back from the device (scikit-learn raises one in each of these cases)


def _f64(what, name, t, shape=None, like=None):
    check_tensor(what, name, t, torch.float64, shape, like, nonempty=True)


def clin_design(raw, ncat, cats, fit_idx=None, stats=None, flag=None):
    """The design matrix of a clinical table (koaf_clin_design): raw fp64 [V, n] holds one column per variable, ncat[v] is 0 for a
    continuous variable (StandardScaler: (x - mean) / population std, std 0 -> 1) and the number of categories otherwise
    (OneHotEncoder: one 0 / 1 column per entry of the sorted list cats[v], in that order).  stats None: mean and std are computed
    over the rows fit_idx (int32 device indices; None: all rows) and returned; stats [V, 2]: they are read.  -> (X [n, D], stats).
    flag: a clin_flag() word; None: an own word is read back here (a host sync), and a NaN / Inf or an unknown category raises
    ValueError as scikit-learn does."""
    _f64("clin_design", "raw", raw)
    if raw.dim() != 2:
        raise KoafError(f"clin_design: raw is [V, n], got {tuple(raw.shape)}")
    V, n = int(raw.shape[0]), int(raw.shape[1])
    ncat = [int(c) for c in ncat]
    lists = [np.asarray(cats[v], np.float64).reshape(-1) if ncat[v] else np.zeros(0) for v in range(min(V, len(ncat)))]
    D = sum(c if c else 1 for c in ncat)
    if len(ncat) != V or V > 32 or D + 1 > LOGREG_MAX_P or any(c < 0 for c in ncat) or any(len(l) != c for l, c in zip(lists, ncat)):
        raise KoafError(f"clin_design: {V} variables with category counts {ncat} (D = {D}): at most 32 variables, D + 1 <= {LOGREG_MAX_P}, "
                        f"and one list of categories per categorical variable")
    for l in lists:
        if l.size and (np.isnan(l).any() or (np.diff(l) <= 0).any()):
            raise KoafError("clin_design: a category list is strictly increasing (np.unique)")
    fit = stats is None
    if fit:
        stats = torch.empty((V, 2), dtype=torch.float64, device=raw.device)
        if fit_idx is not None:
            check_tensor("clin_design", "fit_idx", fit_idx, torch.int32, None, raw)
            if fit_idx.dim() != 1 or fit_idx.numel() == 0:
                raise KoafError("clin_design: fit_idx is a non-empty 1-D index vector")
    else:
        _f64("clin_design", "stats", stats, (V, 2), raw)
    nc = (ctypes.c_int32 * V)(*ncat)
    flat = np.concatenate(lists) if lists else np.zeros(0)
    cs = (ctypes.c_double * max(1, flat.size))(*flat.tolist())
    nfit = int(fit_idx.numel()) if (fit and fit_idx is not None) else n
    with _FLAG.own("clin_design", flag, raw) as flag:
        X = torch.empty((n, D), dtype=torch.float64, device=raw.device)
        check(lib().koaf_clin_design(_ptr(raw), n, V, ctypes.addressof(nc), ctypes.addressof(cs), _ptr(fit_idx) if fit else None, nfit,
                                     1 if fit else 0, _ptr(stats), _ptr(X), _ptr(flag), _stream()), "clin_design")
    return X, stats


def logreg_fit(X, y, sw, C=1.0, max_iter=100, tol=1e-10, out=None, flag=None):
    """K L2-penalised logistic regressions over the same rows in one launch (koaf_logreg_fit, one block per problem): X fp64
    [n, D], y int32 [n] of 0 / 1, sw fp64 [K, n] one sample-weight row per problem, a weight of 0 taking the row out of it.
    Damped Newton in fp64 on (1/S) sum s_i [log(1 + e^r_i) - y_i r_i] + |w|^2 / (2 C S) until |grad|_inf <= tol.
    -> (W [K, D + 1] with the intercept last, report [K, 4] = (steps, final |grad|_inf, final objective, step halvings)).
    out: a contiguous fp64 [K, D + 1] tensor to write W into.  flag as in clin_design (a one-class problem raises)."""
    _f64("logreg_fit", "X", X)
    if X.dim() != 2:
        raise KoafError(f"logreg_fit: X is [n, D], got {tuple(X.shape)}")
    n, D = int(X.shape[0]), int(X.shape[1])
    if D + 1 > LOGREG_MAX_P or n < 2:
        raise KoafError(f"logreg_fit: at least 2 rows and D + 1 <= {LOGREG_MAX_P} columns with the intercept, got n = {n}, D = {D}")
    check_tensor("logreg_fit", "y", y, torch.int32, (n,), X)
    _f64("logreg_fit", "sw", sw, None, X)
    if sw.dim() != 2 or int(sw.shape[1]) != n:
        raise KoafError(f"logreg_fit: sw is [K, {n}], got {tuple(sw.shape)}")
    K = int(sw.shape[0])
    if not (float(C) > 0.0 and math.isfinite(float(C))) or int(max_iter) < 0 or not float(tol) >= 0.0:
        raise KoafError(f"logreg_fit: C > 0, max_iter >= 0 and tol >= 0, got {C}, {max_iter}, {tol}")
    if out is None:
        out = torch.empty((K, D + 1), dtype=torch.float64, device=X.device)
    else:
        _f64("logreg_fit", "out", out, (K, D + 1), X)
    report = torch.empty((K, 4), dtype=torch.float64, device=X.device)
    with _FLAG.own("logreg_fit", flag, X) as flag:
        check(lib().koaf_logreg_fit(_ptr(X), _ptr(y), _ptr(sw), n, D, K, float(C), int(max_iter), float(tol), _ptr(out), _ptr(report),
                                    _ptr(flag), _stream()), "logreg_fit")
    return out, report


def logreg_predict(W, Xt, y=None, mask=None, ensemble=False):
    """The K models W [K, D + 1] on the rows Xt [m, D] (koaf_logreg_predict) -> dict of decision [K, m], proba [K, m, 2] =
    (1 - p, p); with y (int32 [m]) and mask (int32 [K, m]) also logloss [K], sklearn.metrics.log_loss of model k over the rows its
    mask selects; with ensemble also ens_proba [m, 2], the mean over the K models, and ens_pred [m] (int32), its argmax."""
    _f64("logreg_predict", "W", W)
    _f64("logreg_predict", "Xt", Xt, None, W)
    if W.dim() != 2 or Xt.dim() != 2 or int(W.shape[1]) != int(Xt.shape[1]) + 1 or int(W.shape[1]) > LOGREG_MAX_P:
        raise KoafError(f"logreg_predict: W [K, D + 1] and Xt [m, D] with D + 1 <= {LOGREG_MAX_P}, got {tuple(W.shape)} and {tuple(Xt.shape)}")
    K, m, D = int(W.shape[0]), int(Xt.shape[0]), int(Xt.shape[1])
    if (y is None) != (mask is None):
        raise KoafError("logreg_predict: the log-loss needs both y and mask")
    dev = W.device
    res = {"decision": torch.empty((K, m), dtype=torch.float64, device=dev), "proba": torch.empty((K, m, 2), dtype=torch.float64, device=dev)}
    if y is not None:
        check_tensor("logreg_predict", "y", y, torch.int32, (m,), W)
        check_tensor("logreg_predict", "mask", mask, torch.int32, (K, m), W)
        res["logloss"] = torch.empty(K, dtype=torch.float64, device=dev)
    if ensemble:
        res["ens_proba"] = torch.empty((m, 2), dtype=torch.float64, device=dev)
        res["ens_pred"] = torch.empty(m, dtype=torch.int32, device=dev)
    check(lib().koaf_logreg_predict(_ptr(W), _ptr(Xt), m, D, K, _ptr(y), _ptr(mask), 1 if ensemble else 0, _ptr(res["decision"]),
                                    _ptr(res["proba"]), _ptr(res.get("logloss")), _ptr(res.get("ens_proba")), _ptr(res.get("ens_pred")),
                                    _stream()), "logreg_predict")
    return res
