"""Calibration and clinical utility of the predicted probabilities on the device: the companion of _metrics.py, which measures
discrimination only.  The reference has no such code; the definitions are scikit-learn's (brier_score_loss, log_loss,
calibration_curve) and the usual ones of clinical prediction models (ECE / MCE, calibration intercept and slope,
calibration-in-the-large, temperature scaling, net benefit / decision curves).

It matters here more than usual: the reference's fold ensemble is softmax(mean_folds(predict_proba)), a softmax over
probabilities, whose output lies in [1 / (1 + e), e / (1 + e)] = [0.269, 0.731] whatever the folds say; the default loss is focal;
and the train sampler re-weights the classes.  None of that moves a ranking, so ROC-AUC and AP cannot see it.

One device pass (ops.calib_edges, ops.calib_metrics, ops.recalib_fit): the scores are read in place, the sample and every
bootstrap resample are one block each, all sums are fp64 in a fixed order, and everything lands in one fp64 buffer that is copied
to the host once.  The resample matrix is _metrics.bootstrap_indices': with equal seeds the intervals are over the very resamples
calc_metrics_v2's are.

Inputs are numpy arrays or device tensors (device tensors are read in place).  Scalars and curve arrays come back as numpy
values -- they pass through the one host copy anyway; Recalibrator.transform returns a device tensor for a device tensor and a
numpy array for a numpy array.
"""
import copy

import numpy as np
import torch

from .. import ops
from ._metrics import TARGETS, _device, _host_labels, _no_weights, _on_device, _scores, bootstrap_indices, summarize_bootstrap

STRATEGIES = ("uniform", "quantile")
EPS = ops.CALIB_EPS
FIT_METRICS = {"calib_intercept": ("slope_intercept", 0), "calib_slope": ("slope_intercept", 1), "citl": ("intercept", 0)}
ROW_METRICS = {"brier": 2, "log_loss": 3, "ece": 5, "mce": 6}     # where a metric sits in the 8-value rows of ops.calib_metrics
FIT_TOL, FIT_MAX_ITER = 1e-10, 50


# ---- argument checks that need no device ---------------------------------------------------------------------------------------
def _check_bins(n_bins, strategy):
    if strategy not in STRATEGIES:
        raise ValueError(f"Invalid entry to 'strategy' input. Strategy must be either 'quantile' or 'uniform', got {strategy!r}")
    if int(n_bins) != n_bins or not 1 <= int(n_bins) <= ops.CALIB_MAX_BINS:
        raise ValueError(f"n_bins is an integer in [1, {ops.CALIB_MAX_BINS}], got {n_bins!r}")
    return int(n_bins)


def _check_thresholds(thresholds):
    if thresholds is None:
        return None
    t = np.array(thresholds, np.float64).reshape(-1)         # (a copy: it is uploaded and handed back)
    if t.shape[0] > ops.CALIB_MAX_THR:
        raise ValueError(f"at most {ops.CALIB_MAX_THR} thresholds, got {t.shape[0]}")
    if not np.all((t > 0.0) & (t < 1.0)):
        raise ValueError(f"every threshold lies in (0, 1): the odds t / (1 - t) weigh the false positives, got {t}")
    return t


def _check_binary(y_true):
    """labels given on the host are checked there; device labels are checked by the kernels (flag bit 1)"""
    if not torch.is_tensor(y_true):
        u = np.unique(np.asarray(y_true))
        if not np.all((u == 0) | (u == 1)):
            raise ValueError(f"Expected binary target, got: {u}")


def _column(y_prob):
    if not torch.is_tensor(y_prob):
        y_prob = np.asarray(y_prob)
    if y_prob.ndim != 1:
        raise ValueError(f"the probabilities of class 1 are a 1-D column, got {tuple(y_prob.shape)}")
    return y_prob


def _uniform_edges(n_bins):
    return np.linspace(0.0, 1.0, n_bins + 1)


def _quantile_fractions(n_bins):
    """the fractions np.percentile makes of scikit-learn's `np.linspace(0, 1, n_bins + 1) * 100`: data-independent bookkeeping"""
    return np.linspace(0, 1, n_bins + 1) * 100 / 100


class _Pass(object):
    """The device pass over one column of class-1 probabilities: bin edges, ops.calib_metrics of the sample and of every row of
    idx, the recalibration fits asked for (`fits`: mode names) -- then ONE device-to-host copy."""

    def __init__(self, y_true, y_prob, n_bins=10, strategy="uniform", thresholds=None, idx=None, fits=(), eps=EPS):
        dev = _device(y_prob, y_true)
        s = _scores(_on_device(y_prob, dev))
        labels = _on_device(y_true, dev).reshape(-1).to(torch.int32)
        n = int(labels.numel())
        if s.dim() != 1 or int(s.numel()) != n:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{n}, {tuple(s.shape)}]")
        idx_dev = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
        rows = 1 + (0 if idx is None else int(idx.shape[0]))
        T = 0 if thresholds is None else int(thresholds.shape[0])
        sizes = [n_bins + 1, rows * 8, rows * n_bins * 3, rows * T * 4] + [rows * 8] * len(fits) + [1]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        buf = torch.zeros(int(offs[-1]), dtype=torch.float64, device=dev)
        part = [buf[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
        flag = part[-1].view(torch.int32)[:1]
        if strategy == "quantile":
            ops.calib_edges(s, torch.from_numpy(_quantile_fractions(n_bins)).to(dev), out=part[0], flag=flag)
        else:
            part[0].copy_(torch.from_numpy(_uniform_edges(n_bins)))
        thr_dev = None if thresholds is None else torch.from_numpy(thresholds).to(dev)
        ops.calib_metrics(s, labels, part[0], thr_dev, idx_dev, True, eps, out=part[1].view(rows, 8), bins=part[2].view(rows, n_bins, 3),
                          nb=part[3].view(rows, T, 4) if thresholds is not None else None, flag=flag)
        for k, mode in enumerate(fits):
            ops.recalib_fit(s, labels, "proba", mode, None, idx_dev, True, eps, FIT_TOL, FIT_MAX_ITER, out=part[4 + k].view(rows, 8),
                            flag=flag)
        host = buf.cpu()                                   # the one synchronisation
        ops.calib_raise(int(host[-1:].view(torch.int32)[0].item()) & 7)       # (bit 3, a fit that failed, is read from the reports)
        host = host.numpy()
        part = [host[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
        self.n, self.rows, self.edges = n, rows, part[0]
        self.out, self.bins = part[1].reshape(rows, 8), part[2].reshape(rows, n_bins, 3)
        self.nb = part[3].reshape(rows, T, 4) if thresholds is not None else None
        self.fit = {mode: part[4 + k].reshape(rows, 8) for k, mode in enumerate(fits)}

    def curve(self, row=0):
        """calibration_curve's (prob_true, prob_pred) over the non-empty bins, and their counts"""
        b = self.bins[row]
        used = b[:, 0] != 0
        return b[used, 1] / b[used, 0], b[used, 2] / b[used, 0], b[used, 0].astype(np.int64)


# ---- scikit-learn's functions ---------------------------------------------------------------------------------------------------
def brier_score_loss(y_true, y_proba, sample_weight=None):
    """sklearn.metrics.brier_score_loss of binary 0 / 1 targets: mean((p - y)^2), summed in fp64 whatever the scores' dtype"""
    _no_weights(sample_weight)
    _check_binary(y_true)
    return np.float64(_Pass(y_true, _column(y_proba), 1).out[0, 2])


def log_loss(y_true, y_pred, eps=EPS, sample_weight=None):
    """sklearn.metrics.log_loss of binary 0 / 1 targets and the probabilities of class 1: mean(-log(clip(p_y, eps, 1 - eps))).
    The arithmetic is fp64 whatever the scores' dtype and eps defaults to fp64's 2**-52: scikit-learn clips an fp32 column at
    fp32's eps (1.19e-7) and computes in fp32; this function does not."""
    _no_weights(sample_weight)
    _check_binary(y_true)
    if not 0.0 <= float(eps) < 0.5:
        raise ValueError(f"0 <= eps < 0.5, got {eps!r}")
    return np.float64(_Pass(y_true, _column(y_pred), 1, eps=float(eps)).out[0, 3])


def calibration_curve(y_true, y_prob, n_bins=5, strategy="uniform"):
    """sklearn.calibration.calibration_curve -> (prob_true, prob_pred) over the non-empty bins.  A score on an inner edge goes to
    the lower bin (searchsorted, side left), the quantile edges are np.percentile's (an fp32 column is widened first)."""
    n_bins = _check_bins(n_bins, strategy)
    _check_binary(y_true)
    pt, pp, _ = _Pass(y_true, _column(y_prob), n_bins, strategy).curve()
    return pt, pp


def expected_calibration_error(y_true, y_prob, n_bins=10, strategy="uniform"):
    """-> (ece, mce): sum_b (n_b / n) |mean y - mean p| and max_b |mean y - mean p| over calibration_curve's bins"""
    n_bins = _check_bins(n_bins, strategy)
    _check_binary(y_true)
    out = _Pass(y_true, _column(y_prob), n_bins, strategy).out
    return np.float64(out[0, 5]), np.float64(out[0, 6])


def _fit_value(report, k, what):
    status = int(report[5])
    if status != 0:
        raise ValueError(f"{what}: the logistic recalibration ended with status {status} ({ops.RECALIB_STATUS[status]})")
    return np.float64(report[k])


def calibration_slope_intercept(y_true, y_prob):
    """The logistic recalibration of the labels on logit(p): {"intercept", "slope"} of the free fit (1 is a perfect slope; above 1
    the probabilities are too flat), "citl" the intercept with the slope held at 1 (calibration in the large) and "mean_diff" =
    mean(p) - prevalence.  ValueError when a fit has no finite optimum (separable data, one class)."""
    _check_binary(y_true)
    t = _Pass(y_true, _column(y_prob), 1, fits=("slope_intercept", "intercept"))
    free, large = t.fit["slope_intercept"][0], t.fit["intercept"][0]
    return {"intercept": _fit_value(free, 0, "calibration_slope_intercept"), "slope": _fit_value(free, 1, "calibration_slope_intercept"),
            "citl": _fit_value(large, 0, "calibration_slope_intercept"), "mean_diff": np.float64(t.out[0, 4] - t.out[0, 0] / t.n)}


def decision_curve(y_true, y_prob, thresholds):
    """Net benefit of treating `y_prob >= t` per threshold t in (0, 1): tp / n - (fp / n) * t / (1 - t) -> {"thresholds",
    "net_benefit", "treat_all" (the same expression with everyone treated), "treat_none" (zeros)}"""
    thr = _check_thresholds(thresholds)
    if thr is None or thr.shape[0] == 0:
        raise ValueError("decision_curve: at least one threshold")
    _check_binary(y_true)
    nb = _Pass(y_true, _column(y_prob), 1, thresholds=thr).nb[0]
    return {"thresholds": thr, "net_benefit": nb[:, 2].copy(), "treat_all": nb[:, 3].copy(), "treat_none": np.zeros_like(thr)}


# ---- recalibration ---------------------------------------------------------------------------------------------------------------
def _fit_columns(scores, kind):
    """-> (device column, second device column or None, kind, whether the input was a tensor)"""
    was_tensor = torch.is_tensor(scores)
    if not was_tensor:
        scores = np.asarray(scores)
    if scores.ndim == 2 and scores.shape[1] == 2:
        if kind not in (None, "logit"):
            raise ValueError("a (B, 2) input holds logits: kind is 'logit'")
        t = _scores(_on_device(scores, _device(scores)))
        return t[:, 1], t[:, 0], "logit", was_tensor
    if scores.ndim != 1:
        raise ValueError(f"scores are a 1-D column or a (B, 2) logits matrix, got {tuple(scores.shape)}")
    return _scores(_on_device(scores, _device(scores))), None, kind or "proba", was_tensor


class Recalibrator(object):
    """Logistic recalibration p' = sigmoid(a + b x), fitted on validation or out-of-fold predictions and applied to the test
    ensemble.  mode "slope_intercept": a and b free; "temperature": a = 0, b = 1 / T; "intercept": b = 1.  x is logit(p) for a 1-D
    column of class-1 probabilities, and z1 - z0 for a (B, 2) logits matrix (kind "logit"; a 1-D column of logits: kind="logit").
    state_dict() is two floats, the mode and the kind: storable beside a checkpoint."""

    def __init__(self, mode="slope_intercept", kind=None):
        if mode not in ops.RECALIB_MODES:
            raise ValueError(f"mode is one of {tuple(ops.RECALIB_MODES)}, got {mode!r}")
        if kind not in (None,) + tuple(ops.RECALIB_KINDS):
            raise ValueError(f"kind is None or one of {tuple(ops.RECALIB_KINDS)}, got {kind!r}")
        self.mode, self.kind, self.a, self.b, self.report = mode, kind, None, None, None

    def fit(self, y_true, scores, tol=FIT_TOL, max_iter=FIT_MAX_ITER):
        _check_binary(y_true)
        s, s0, kind, _ = _fit_columns(scores, self.kind)
        labels = _on_device(y_true, s.device).reshape(-1).to(torch.int32)
        if int(labels.numel()) != int(s.numel()):
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{int(labels.numel())}, {int(s.numel())}]")
        buf = torch.zeros(9, dtype=torch.float64, device=s.device)
        ops.recalib_fit(s, labels, kind, self.mode, s0, None, True, EPS, tol, max_iter, out=buf[:8].view(1, 8),
                        flag=buf[8:].view(torch.int32)[:1])
        host = buf.cpu()
        ops.calib_raise(int(host[8:].view(torch.int32)[0].item()) & 7)
        self.report = host.numpy()[:8].copy()
        self.a, self.b = float(_fit_value(self.report, 0, "Recalibrator.fit")), float(_fit_value(self.report, 1, "Recalibrator.fit"))
        self.kind = kind
        return self

    def transform(self, scores):
        if self.a is None:
            raise ValueError("Recalibrator.transform before fit / load_state_dict")
        s, s0, kind, was_tensor = _fit_columns(scores, self.kind)
        out = ops.recalib_apply(s, self.a, self.b, kind, s0, EPS)
        return out if was_tensor else out.cpu().numpy()

    @property
    def temperature(self):
        return 1.0 / self.b

    def state_dict(self):
        return {"mode": self.mode, "kind": self.kind, "a": self.a, "b": self.b}

    def load_state_dict(self, state):
        r = Recalibrator(state["mode"], state["kind"])
        self.mode, self.kind, self.a, self.b = r.mode, r.kind, float(state["a"]), float(state["b"])
        return self


def fit_temperature(logits, y_true):
    """The temperature T that minimises the log-loss of softmax(logits / T) for two classes: logits is a (B, 2) matrix (read in
    place on the device) or the 1-D logit difference z1 - z0.  T > 1 softens, T < 1 sharpens."""
    return np.float64(Recalibrator("temperature", "logit").fit(y_true, logits).temperature)


# ---- the companion table of calc_metrics_v2 ------------------------------------------------------------------------------------
def calc_calibration(prog_target, prog_pred_proba, target, n_bins=10, strategy="uniform", thresholds=None, bootstrap=False,
                     kws_bs=None):
    """The calibration table that goes with calc_metrics_v2's discrimination table: same `target` names, same inputs
    (prog_target (sample,), prog_pred_proba (sample, class), numpy or device tensors; class 1 is the event), same kws_bs keys
    (n_bootstrap 1000, seed 0, stratified True, alpha 95, ddof 0) and the same resample matrix (bootstrap_indices), so with equal
    seeds the intervals are over the very resamples calc_metrics_v2 used.

    Keys: sample_size, num_pos, num_neg, prevalence, mean_predicted, brier, log_loss, ece, mce, calib_intercept, calib_slope,
    citl, then the reliability arrays of the sample bin_edges, prob_true, prob_pred, bin_count (non-empty bins), and net_benefit
    (decision_curve's dict) when `thresholds` is given.  bootstrap=True: each of the seven scalars from brier on is a
    (value, std_err, ci_l, ci_h) tuple by summarize_bootstrap's percentile rule, and n_fit_failed counts, per fitted metric, the
    resamples whose fit ended with a status other than 0 (separable or one-class resamples): they are dropped from that metric's
    interval.  The binning is fixed BEFORE resampling: resamples share the sample's bin edges, also for strategy "quantile".
    A fit of the sample itself that has no finite optimum gives NaN.  Nothing is rounded."""
    n_bins = _check_bins(n_bins, strategy)
    thr = _check_thresholds(thresholds)
    if target not in TARGETS:
        raise ValueError(f"Unknown target: {target}")
    kws = {"n_bootstrap": 1000, "seed": 0, "stratified": True, "alpha": 95, "ddof": 0}
    if kws_bs is not None:
        kws.update(copy.deepcopy(dict(kws_bs)))
    kws.pop("verbose", None)
    if prog_pred_proba.ndim != 2 or prog_pred_proba.shape[1] < 2:
        raise ValueError(f"prog_pred_proba is (sample, class) with at least two classes, got {tuple(prog_pred_proba.shape)}")
    _check_binary(prog_target)
    idx = None
    if bootstrap:
        y_host = _host_labels(prog_target)
        if len(np.unique(y_host)) > 2:
            raise ValueError(f"Expected binary target, got: {np.unique(y_host)}")
        idx = bootstrap_indices(y_host, kws["n_bootstrap"], kws["seed"], kws["stratified"])
    proba = _on_device(prog_pred_proba, _device(prog_pred_proba, prog_target))
    labels = prog_target.reshape(-1) if torch.is_tensor(prog_target) else np.asarray(prog_target).reshape(-1)
    t = _Pass(labels, proba[:, 1], n_bins, strategy, thr, idx, fits=("slope_intercept", "intercept"))

    def scalar(name):
        if name in ROW_METRICS:
            vals, ok = t.out[:, ROW_METRICS[name]], np.ones(t.rows, bool)
        else:
            mode, k = FIT_METRICS[name]
            vals, ok = t.fit[mode][:, k], t.fit[mode][:, 5] == 0
        point = np.float64(vals[0]) if ok[0] else np.float64(np.nan)
        if not bootstrap:
            return point, 0
        keep = ok[1:]
        return summarize_bootstrap(vals[1:][keep], t.out[1:, 0][keep], t.out[1:, 1][keep], point, kws["alpha"], kws["ddof"]), int((~keep).sum())

    out = dict()
    out["sample_size"] = t.n
    out["num_pos"], out["num_neg"] = np.int64(t.out[0, 0]), np.int64(t.out[0, 1])
    out["prevalence"] = out["num_pos"] / t.n
    out["mean_predicted"] = np.float64(t.out[0, 4])
    failed = dict()
    for name in tuple(ROW_METRICS) + tuple(FIT_METRICS):
        out[name], miss = scalar(name)
        if name in FIT_METRICS:
            failed[name] = miss
    out["bin_edges"] = t.edges.copy()
    out["prob_true"], out["prob_pred"], out["bin_count"] = t.curve()
    if thr is not None:
        nb = t.nb[0]
        out["net_benefit"] = {"thresholds": thr, "net_benefit": nb[:, 2].copy(), "treat_all": nb[:, 3].copy(), "treat_none": np.zeros_like(thr)}
    if bootstrap:
        out["n_fit_failed"] = failed
    return out
