"""calc_metrics_v2 / calc_bootstrap of koafusion/various/_metrics_stat_anlys.py:28-216 (with average_precision_score_calib of
_metrics_wissam.py:113-172) on the device: no scikit-learn, no scipy, no per-metric argsort.

The scores are ranked once per probability column (ops.score_ranks); the point estimates and all bootstrap resamples of the
four curve metrics are then two launches of ops.curve_metrics (column 1 / positive class 1: roc_auc, avg_precision,
avg_ppv_calib; column 0 / positive class 0: avg_npv), and ops.point_metrics gives the Youden cutoff and both confusion matrices.
Everything lands in one fp64 device buffer that is copied to the host once: the only synchronisation of a call.

The resampling indices come from the HOST: the reference seeds numpy's legacy generator with the same seed for each of its four
metrics, so one index matrix serves all four, and drawing it with that very generator (frozen across numpy versions) is what
makes the bootstrap a replay of the reference's and not a different sample of the same distribution.  The matrix is copied up
once.  The summary of the R per-resample values (percentiles, standard error) stays numpy: it is the reference's own arithmetic
on a thousand numbers.
"""
import copy

import numpy as np
import torch

from .. import ops

TARGETS = ("prog_kl_12", "prog_kl_24", "prog_kl_36", "prog_kl_48", "prog_kl_72", "prog_kl_96", "tiulpin2019_prog_bin")
METRICS = ("roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv")
ROUNDED = ("prevalence", "roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv", "cutoff", "youdens_index", "b_accuracy")
# where a metric sits in the 8-value rows of ops.curve_metrics, and which launch computes it (1: column 1 with positive class 1,
# 0: column 0 with positive class 0)
_SLOT = {"roc_auc": (1, 2), "avg_precision": (1, 3), "avg_ppv_calib": (1, 4), "avg_npv": (0, 3)}
_ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def bootstrap_indices(y_true, n_bootstrap, seed, stratified):
    """The index sets calc_bootstrap (:54-69) draws, as an int32 [n_bootstrap, n] matrix: numpy's legacy generator seeded with
    `seed`; per resample choice(ind_pos, n_pos) then choice(ind_neg, n_neg), laid side by side -- or one choice(n, n) when not
    stratified.  A private RandomState(seed) yields the stream np.random.seed(seed) would, without touching the global one.
    Resamples the reference would skip (no positives) are drawn and returned like the others: skipping is the summary's job."""
    y_true = np.asarray(y_true).reshape(-1)
    n = y_true.shape[0]
    rs = np.random.RandomState(seed)
    ind_pos = np.where(y_true == 1)[0]
    ind_neg = np.where(y_true == 0)[0]
    if stratified and ind_pos.shape[0] + ind_neg.shape[0] != n:
        raise ValueError(f"Expected binary target, got: {np.unique(y_true)}")
    out = np.empty((int(n_bootstrap), n), np.int32)
    for r in range(int(n_bootstrap)):
        if stratified:
            out[r, :ind_pos.shape[0]] = rs.choice(ind_pos, ind_pos.shape[0])
            out[r, ind_pos.shape[0]:] = rs.choice(ind_neg, ind_neg.shape[0])
        else:
            out[r] = rs.choice(n, n)
    return out


def summarize_bootstrap(vals, n_label1, n_label0, point, alpha=95., ddof=0):
    """calc_bootstrap's tail (:71-80) on the per-resample values of one metric: resamples without a sample of class 1 are dropped,
    a kept one without a sample of class 0 raises what sklearn's roc_auc_score raises there; then
    ci_l = percentile((100 - alpha) // 2), ci_h = percentile(alpha + (100 - alpha) // 2) -- the 2nd and the 97th at alpha = 95,
    as the reference computes them -- and the standard deviation with `ddof`.  -> (value, std_err, ci_l, ci_h)"""
    vals, n_label1, n_label0 = np.asarray(vals, np.float64), np.asarray(n_label1), np.asarray(n_label0)
    keep = n_label1 != 0
    if (n_label0[keep] == 0).any():
        raise ValueError(_ONE_CLASS)
    metric_vals = list(vals[keep])
    ci_l = np.percentile(metric_vals, (100 - alpha) // 2)
    ci_h = np.percentile(metric_vals, alpha + (100 - alpha) // 2)
    std_err = np.std(metric_vals, ddof=ddof)
    return np.float64(point), std_err, ci_l, ci_h


def _device(*things):
    """the device of the first device tensor among `things`, else the current one"""
    for t in things:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _on_device(a, dev):
    """a numpy array or a tensor -> a device tensor (device tensors pass through: nothing is copied to the host)"""
    if torch.is_tensor(a):
        return a if a.is_cuda else a.to(dev)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scores(col):
    """a score column the kernels read in place: fp32 and fp64 as they are, everything else widened to fp64"""
    return col if col.dtype in (torch.float32, torch.float64) else col.to(torch.float64)


def _host_labels(y):
    return (y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)).reshape(-1)


class _Tables(object):
    """The device pass: ranks of the score columns asked for, the curve metrics of the sample and of every row of idx, the point
    quantities -- then ONE device-to-host copy.  cols: {1: scores of class 1, 0: scores of class 0} (either may be missing)."""

    def __init__(self, labels, cols, idx=None, pi0=0.12, point=False):
        dev = _device(*cols.values(), labels)
        labels = _on_device(labels, dev).reshape(-1).to(torch.int32)
        n = int(labels.numel())
        idx_dev = None
        if idx is not None:
            idx_dev = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
        rows = 1 + (0 if idx is None else int(idx.shape[0]))
        which = sorted(cols)
        nbuf = len(which) * rows * 8 + 9 + 1
        buf = torch.zeros(nbuf, dtype=torch.float64, device=dev)
        flag = buf[nbuf - 1:].view(torch.int32)[:1]
        off = 0
        for c in which:
            s = _scores(_on_device(cols[c], dev))
            if s.dim() != 1 or int(s.numel()) != n:
                raise ValueError(f"Found input variables with inconsistent numbers of samples: [{n}, {tuple(s.shape)}]")
            _, packed = ops.score_ranks(s, labels, pos_label=c, flag=flag)
            ops.curve_metrics(packed, idx_dev, True, pi0, out=buf[off:off + rows * 8].view(rows, 8), flag=flag)
            if point and c == 1:
                ops.point_metrics(s, packed, 0.5, out=buf[nbuf - 10:nbuf - 1], flag=flag)
            off += rows * 8
        host = buf.cpu()                                   # the one synchronisation
        ops.metrics_raise(host[nbuf - 1:].view(torch.int32)[0].item())
        host = host.numpy()
        self.n, self.rows = n, rows
        self.curve = {c: host[i * rows * 8:(i + 1) * rows * 8].reshape(rows, 8) for i, c in enumerate(which)}
        self.point = host[nbuf - 10:nbuf - 1]
        first = self.curve[which[0]]
        # counts of label 1 / label 0 per row, whichever class the launch called positive
        self.n1, self.n0 = (first[:, 0], first[:, 1]) if which[0] == 1 else (first[:, 1], first[:, 0])
        self.score_dtype = {c: (cols[c].dtype if torch.is_tensor(cols[c]) else np.asarray(cols[c]).dtype) for c in which}

    def value(self, metric):
        c, k = _SLOT[metric]
        return np.float64(self.curve[c][0, k])

    def resamples(self, metric):
        c, k = _SLOT[metric]
        return self.curve[c][1:, k]

    def bootstrap(self, metric, alpha, ddof):
        return summarize_bootstrap(self.resamples(metric), self.n1[1:], self.n0[1:], self.value(metric), alpha, ddof)


def _np_dtype(dt):
    if isinstance(dt, torch.dtype):
        return np.dtype({torch.float32: np.float32, torch.float64: np.float64}.get(dt, np.float64))
    return np.dtype(dt) if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.float64)) else np.dtype(np.float64)


def calc_bootstrap(metric, y_true, y_pred, n_bootstrap=100, seed=0, stratified=True, alpha=95., ddof=0, verbose=True, pi0=0.12):
    """calc_bootstrap (:28-80) with the metric given by NAME: "roc_auc" | "avg_precision" | "avg_ppv_calib" (calibrated to the
    prevalence `pi0`) | "avg_npv" (y_pred then holds the scores of class 0, which is the positive one, as the reference's driver
    passes them).  y_true / y_pred: numpy arrays or device tensors.  All resamples and the point estimate are one launch; `verbose`
    is accepted and has nothing to report.  -> (metric_val, std_err, ci_l, ci_h)"""
    if metric not in METRICS:
        raise ValueError(f"Unknown metric: {metric!r} (one of {METRICS})")
    y_host = _host_labels(y_true)                       # the index draw needs the labels on the host
    if len(np.unique(y_host)) > 2:
        raise ValueError(f"Expected binary target, got: {np.unique(y_host)}")
    idx = bootstrap_indices(y_host, n_bootstrap, seed, stratified)
    c = _SLOT[metric][0]
    if not torch.is_tensor(y_pred):
        y_pred = np.asarray(y_pred).reshape(-1)
    t = _Tables(y_true if torch.is_tensor(y_true) else y_host, {c: y_pred}, idx, pi0)
    if t.n1[0] == 0 or t.n0[0] == 0:
        raise ValueError(_ONE_CLASS)
    return t.bootstrap(metric, alpha, ddof)


def _single_class(n, num_pos, num_neg):
    out = dict()
    out["sample_size"] = n
    out["num_pos"] = num_pos
    out["num_neg"] = num_neg
    for k in ("prevalence", "roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv", "cutoff", "youdens_index", "b_accuracy",
              "roc_curve", "pr_curve"):
        out[k] = np.nan
    return out


def calc_metrics_v2(prog_target, prog_pred_proba, target, with_curves=False, bootstrap=False, kws_ppv=None, kws_bs=None):
    """The reference's calc_metrics_v2 (:83-216): same signature, defaults, keys, key order, value types and rounding.

    prog_target (sample,) and prog_pred_proba (sample, class) are numpy arrays or device tensors; device tensors are read in
    place (a probability column is ranked through its stride).  fp32 and fp64 probabilities are ranked in their own precision.
    bootstrap=True: (value, std_err, ci_l, ci_h) per metric, rounded into a 4-array, over kws_bs["n_bootstrap"] (1000) resamples
    drawn as the reference draws them; the labels are then also copied to the host, where the indices are drawn.
    with_curves=True is not built (the curve arrays are never formed here)."""
    out = calc_metrics_unrounded(prog_target, prog_pred_proba, target, with_curves, bootstrap, kws_ppv, kws_bs)
    for k, v in out.items():
        if k in ROUNDED:
            out[k] = np.round(v, 3)
    return out


def calc_metrics_unrounded(prog_target, prog_pred_proba, target, with_curves=False, bootstrap=False, kws_ppv=None, kws_bs=None):
    """calc_metrics_v2 before its closing `np.round(v, 3)` (:207-214): what the tests compare at full precision"""
    if with_curves:
        raise NotImplementedError("calc_metrics_v2: with_curves=True -- the roc / pr curve arrays are not built on the device path")
    kws_bs_all = {"n_bootstrap": 1000, "seed": 0, "stratified": True, "alpha": 95}
    if kws_bs is not None:
        kws_bs_all.update(copy.deepcopy(dict(kws_bs)))
    kws_ppv_all = {"pi0": 0.12}
    if kws_ppv is not None:
        kws_ppv_all.update(copy.deepcopy(dict(kws_ppv)))
    kws_bs_all.pop("verbose", None)

    on_host = not torch.is_tensor(prog_target)
    y_host = None
    if on_host or bootstrap or target not in TARGETS:
        y_host = _host_labels(prog_target)
        if len(np.unique(y_host)) < 2:
            return _single_class(y_host.shape[0], np.sum(y_host == 1), np.sum(y_host == 0))
    if target not in TARGETS:
        raise ValueError(f"Unknown target: {target}")
    if prog_pred_proba.ndim != 2 or prog_pred_proba.shape[1] < 2:
        raise ValueError(f"prog_pred_proba is (sample, class) with at least two classes, got {tuple(prog_pred_proba.shape)}")

    idx = None
    if bootstrap:
        if len(np.unique(y_host)) > 2:
            raise ValueError(f"Expected binary target, got: {np.unique(y_host)}")
        idx = bootstrap_indices(y_host, kws_bs_all["n_bootstrap"], kws_bs_all["seed"], kws_bs_all["stratified"])
    proba = _on_device(prog_pred_proba, _device(prog_pred_proba, prog_target))
    t = _Tables(prog_target if not on_host else y_host, {1: proba[:, 1], 0: proba[:, 0]}, idx, kws_ppv_all["pi0"],
                point=not bootstrap)
    n, num_pos, num_neg = t.n, np.int64(t.n1[0]), np.int64(t.n0[0])
    if num_pos == 0 or num_neg == 0:                  # (device targets: known only now)
        return _single_class(n, num_pos, num_neg)

    out = dict()
    out["sample_size"] = n
    out["num_pos"] = num_pos
    out["num_neg"] = num_neg
    out["prevalence"] = num_pos / n
    for m in METRICS:
        out[m] = t.bootstrap(m, kws_bs_all["alpha"], kws_bs_all.get("ddof", 0)) if bootstrap else t.value(m)
    if not bootstrap:
        out["cutoff"] = _np_dtype(t.score_dtype[1]).type(t.point[0])
        tn, fp, fn, tp = t.point[5:9]
        out["youdens_index"] = tp / (tp + fn) + tn / (tn + fp) - 1.
        tn, fp, fn, tp = t.point[1:5]
        out["b_accuracy"] = np.mean(np.array([tn / (tn + fp), tp / (tp + fn)]))
    return out
