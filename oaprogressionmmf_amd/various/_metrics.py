"""calc_metrics_v2 / calc_bootstrap of koafusion/various/_metrics_stat_anlys.py:28-216 (with average_precision_score_calib of
_metrics_wissam.py:113-172) on the device: no scikit-learn, no scipy, no per-metric argsort.

The scores are ranked once per probability column (ops.score_ranks); the point estimates and all bootstrap resamples of the
four curve metrics are then two launches of ops.curve_metrics (column 1 / positive class 1: roc_auc, avg_precision,
avg_ppv_calib; column 0 / positive class 0: avg_npv), and ops.point_metrics gives the Youden cutoff and both confusion matrices.
Everything lands in one fp64 device buffer that is copied to the host once: the only synchronisation of a call.

The curves themselves (calc_metrics_curves, roc_curve, precision_recall_curve, precision_recall_curve_calib) are the
same walk with its points written out (ops.curve_points): the buffer's length follows from n alone, so it rides in that one copy,
and the host only slices and reverses.  avg_precision_at_recall_range and bestf1score_calib, and their bootstraps, are one launch
of ops.range_metrics; f1score_calib and mc_bacc read the integer counts of ops.confusion.

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
# calc_bootstrap's further metrics, and where they sit in the 8-value rows of ops.range_metrics
RANGE_METRICS = {"avg_precision_at_recall_range": 2, "best_f1_calib": 3}
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

    def __init__(self, labels, cols, idx=None, pi0=0.12, point=False, curves=False):
        dev = _device(*cols.values(), labels)
        labels = _on_device(labels, dev).reshape(-1).to(torch.int32)
        n = int(labels.numel())
        idx_dev = None
        if idx is not None:
            idx_dev = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
        rows = 1 + (0 if idx is None else int(idx.shape[0]))
        which = sorted(cols)
        ncurve = ops.curve_points_len(n) if curves else 0        # (sized from n alone: part of the same copy)
        nbuf = len(which) * rows * 8 + ncurve + 9 + 1
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
            if curves and c == 1:
                ops.curve_points(s, packed, pi0, out=buf[nbuf - 10 - ncurve:nbuf - 10], flag=flag)
            off += rows * 8
        host = buf.cpu()                                   # the one synchronisation
        ops.metrics_raise(host[nbuf - 1:].view(torch.int32)[0].item())
        host = host.numpy()
        self.n, self.rows = n, rows
        self.curve = {c: host[i * rows * 8:(i + 1) * rows * 8].reshape(rows, 8) for i, c in enumerate(which)}
        self.point = host[nbuf - 10:nbuf - 1]
        self.points = ops.parse_curve_points(host[nbuf - 10 - ncurve:nbuf - 10]) if curves and 1 in cols else None
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


def calc_bootstrap(metric, y_true, y_pred, n_bootstrap=100, seed=0, stratified=True, alpha=95., ddof=0, verbose=True, pi0=0.12,
                   recall_range=(0., 1.)):
    """calc_bootstrap (:28-80) with the metric given by NAME: "roc_auc" | "avg_precision" | "avg_ppv_calib" (calibrated to the
    prevalence `pi0`) | "avg_npv" (y_pred then holds the scores of class 0, which is the positive one, as the reference's driver
    passes them) | "avg_precision_at_recall_range" (over `recall_range`) | "best_f1_calib" (bestf1score_calib(pi0); pi0 None: not
    calibrated).  y_true / y_pred: numpy arrays or device tensors.  All resamples and the point estimate are one launch; `verbose`
    is accepted and has nothing to report.  -> (metric_val, std_err, ci_l, ci_h)"""
    if metric not in METRICS and metric not in RANGE_METRICS:
        raise ValueError(f"Unknown metric: {metric!r} (one of {METRICS + tuple(RANGE_METRICS)})")
    if metric in RANGE_METRICS:
        _check_recall_range(recall_range)
    y_host = _host_labels(y_true)                       # the index draw needs the labels on the host
    if len(np.unique(y_host)) > 2:
        raise ValueError(f"Expected binary target, got: {np.unique(y_host)}")
    idx = bootstrap_indices(y_host, n_bootstrap, seed, stratified)
    if metric in RANGE_METRICS:
        rows = _range_rows(y_true if torch.is_tensor(y_true) else y_host, y_pred, idx, pi0, recall_range)
        if rows[0, 0] == 0 or rows[0, 1] == 0:
            raise ValueError(_ONE_CLASS)
        k = RANGE_METRICS[metric]
        return summarize_bootstrap(rows[1:, k], rows[1:, 0], rows[1:, 1], rows[0, k], alpha, ddof)
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
    with_curves=True still raises NotImplementedError here, as it always has: the table with the reference's three curve keys is
    calc_metrics_curves, which takes the same arguments."""
    if with_curves:
        raise NotImplementedError("calc_metrics_v2: with_curves=True -- the roc / pr curve arrays come from calc_metrics_curves")
    return _rounded(calc_metrics_unrounded(prog_target, prog_pred_proba, target, False, bootstrap, kws_ppv, kws_bs))


def calc_metrics_curves(prog_target, prog_pred_proba, target, kws_ppv=None):
    """What the reference's calc_metrics_v2(..., with_curves=True) returns (:83-216): the plain table of calc_metrics_v2 and, after
    b_accuracy, roc_curve = (fpr, tpr), pr_curve = (prec, rec) -- sklearn's precision_recall_curve: every distinct threshold -- and
    pr_calib_curve = (prec, rec) -- the reference's precision_recall_curve_calib: calibrated to pi0 and cut at full recall --,
    tuples of fp64 numpy arrays.  They come out of the same device buffer and the same single copy as the table; the host only
    slices and reverses them.  The single-class return is calc_metrics_v2's."""
    return _rounded(calc_metrics_unrounded(prog_target, prog_pred_proba, target, True, False, kws_ppv, None))


def _rounded(out):
    for k, v in out.items():
        if k in ROUNDED:
            out[k] = np.round(v, 3)
    return out


def calc_metrics_unrounded(prog_target, prog_pred_proba, target, with_curves=False, bootstrap=False, kws_ppv=None, kws_bs=None):
    """calc_metrics_v2 before its closing `np.round(v, 3)` (:207-214): what the tests compare at full precision.  with_curves
    (ignored when bootstrap, as in the reference) adds the three curve keys of calc_metrics_curves."""
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
                point=not bootstrap, curves=bool(with_curves) and not bootstrap)
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
    if with_curves and not bootstrap:
        c = t.points
        out["roc_curve"] = (c["fpr"].copy(), c["tpr"].copy())
        out["pr_curve"] = (c["prec"][::-1].copy(), c["rec"][::-1].copy())
        out["pr_calib_curve"] = (c["prec_cal"][c["last_ind"] + 1::-1].copy(), c["rec"][c["last_ind"] + 1::-1].copy())
    return out


# ---- the curve functions of sklearn.metrics / _metrics_wissam.py the reference's notebook draws with --------------------------
def _no_weights(sample_weight):
    if sample_weight is not None:
        raise NotImplementedError("sample_weight is not built on the device path: the rank histograms count samples")


def _pos(pos_label):
    if pos_label is None:
        return 1
    if pos_label not in (0, 1):
        raise ValueError(f"pos_label is None, 1 or 0 (binary 0 / 1 targets), got {pos_label!r}")
    return int(pos_label)


def _check_recall_range(recall_range):
    lo, hi = (float(v) for v in recall_range)
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f"recall_range is (lo, hi) with 0 <= lo <= hi <= 1, got {tuple(recall_range)}")
    return lo, hi


def _ranked(y_true, y_score, pos_label, nbuf):
    """The sample ranked with `pos_label` positive, and a zeroed fp64 device buffer of nbuf values with the flag word behind it
    -> (scores, packed, buf, flag, numpy dtype of the scores)"""
    dev = _device(y_score, y_true)
    if not torch.is_tensor(y_score):
        y_score = np.asarray(y_score).reshape(-1)
    dtype = _np_dtype(y_score.dtype)
    s = _scores(_on_device(y_score, dev))
    labels = _on_device(y_true, dev).reshape(-1).to(torch.int32)
    if s.dim() != 1 or s.numel() != labels.numel():
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{int(labels.numel())}, {tuple(s.shape)}]")
    buf = torch.zeros(nbuf + 1, dtype=torch.float64, device=dev)
    flag = buf[nbuf:].view(torch.int32)[:1]
    _, packed = ops.score_ranks(s, labels, pos_label=pos_label, flag=flag)
    return s, packed, buf, flag, dtype


def _read_back(buf):
    """the one device-to-host copy of a buffer of _ranked: raises what the flag word says -> the values as numpy"""
    host = buf.cpu()
    ops.metrics_raise(host[-1:].view(torch.int32)[0].item())
    return host.numpy()[:-1]


def _points(y_true, y_score, pos_label=1, pi0=None):
    """ops.curve_points of one sample, copied to the host once -> (parsed views, numpy dtype of the scores)"""
    n = int(y_true.numel() if torch.is_tensor(y_true) else np.asarray(y_true).size)
    s, packed, buf, flag, dtype = _ranked(y_true, y_score, pos_label, ops.curve_points_len(n))
    ops.curve_points(s, packed, 0.5 if pi0 is None else pi0, pi_of_negatives=pos_label == 0, out=buf[:-1], flag=flag)
    return ops.parse_curve_points(_read_back(buf)), dtype


def _range_rows(y_true, y_score, idx, pi0, recall_range, pos_label=1):
    """ops.range_metrics of the sample and of every row of idx, copied to the host once -> [1 + R, 8] numpy"""
    rows = 1 + (0 if idx is None else int(idx.shape[0]))
    s, packed, buf, flag, _ = _ranked(y_true, y_score, pos_label, rows * 8)
    idx_dev = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(s.device)
    ops.range_metrics(packed, idx_dev, True, pi0, recall_range, out=buf[:-1].view(rows, 8), flag=flag)
    return _read_back(buf).reshape(rows, 8)


def roc_curve(y_true, y_score, pos_label=None, sample_weight=None):
    """sklearn.metrics.roc_curve (drop_intermediate=True) of binary 0 / 1 targets -> (fpr, tpr, thresholds): fp64 rates behind the
    leading (0, 0, inf) point, thresholds in the scores' dtype.  numpy arrays or device tensors in, numpy out."""
    _no_weights(sample_weight)
    c, dtype = _points(y_true, y_score, _pos(pos_label))
    return c["fpr"].copy(), c["tpr"].copy(), c["roc_thr"].astype(dtype)


def precision_recall_curve(y_true, y_score, pos_label=None, sample_weight=None):
    """sklearn.metrics.precision_recall_curve (1.7: every distinct threshold, not cut at full recall) -> (precision, recall,
    thresholds): recall decreasing, closing (1, 0) point, thresholds increasing in the scores' dtype"""
    _no_weights(sample_weight)
    c, dtype = _points(y_true, y_score, _pos(pos_label))
    return c["prec"][::-1].copy(), c["rec"][::-1].copy(), c["thr"][::-1].astype(dtype)


def precision_recall_curve_calib(y_true, y_pred, pos_label=None, sample_weight=None, pi0=None):
    """precision_recall_curve_calib (_metrics_wissam.py:113-165): the precision calibrated to the prevalence pi0 (None: plain),
    cut at the first threshold of full recall -> (precision, recall, thresholds)"""
    _no_weights(sample_weight)
    c, dtype = _points(y_true, y_pred, _pos(pos_label), pi0)
    last = c["last_ind"]
    prec = c["prec" if pi0 is None else "prec_cal"]
    return prec[last + 1::-1].copy(), c["rec"][last + 1::-1].copy(), c["thr"][last::-1].astype(dtype)


def average_precision_score_calib(y_true, y_pred, pos_label=1, sample_weight=None, pi0=None):
    """average_precision_score_calib (_metrics_wissam.py:168-172): slot 4 of ops.curve_metrics' identity row (pi0 None: slot 3,
    the plain average precision -- the same sum with ratio 1)"""
    _no_weights(sample_weight)
    pos_label = _pos(pos_label)
    if pos_label == 0 and pi0 is not None:
        raise NotImplementedError("average_precision_score_calib: pos_label=0 with pi0 (the reference then calibrates with the "
                                  "prevalence of label 1, which ops.curve_metrics does not take)")
    if not torch.is_tensor(y_pred):
        y_pred = np.asarray(y_pred).reshape(-1)
    t = _Tables(y_true, {pos_label: y_pred}, None, 0.5 if pi0 is None else pi0)
    return np.float64(t.curve[pos_label][0, 3 if pi0 is None else 4])


def avg_precision_at_recall_range(y_true, probas_pred, recall_range=(0.0, 1.0), sample_weight=None):
    """avg_precision_at_recall_range (:11-25): the trapezoid of precision over recall along sklearn's PR curve from the last point
    with recall <= recall_range[0] to the first with recall >= recall_range[1], over the recall between those two points (a zero
    interval gives NaN, as on the host).  ValueError unless 0 <= lo <= hi <= 1."""
    _no_weights(sample_weight)
    _check_recall_range(recall_range)
    return np.float64(_range_rows(y_true, probas_pred, None, None, recall_range)[0, 2])


def bestf1score_calib(y_true, y_pred, pi0=None):
    """bestf1score_calib (_metrics_wissam.py:215-231): the largest F1 along the calibrated PR curve"""
    return np.float64(_range_rows(y_true, y_pred, None, pi0, (0.0, 1.0))[0, 3])


def _class_counts(y_true, y_pred, K):
    """ops.confusion of two label vectors (numpy or device; booleans count as 0 / 1) -> int64 [K, K] numpy"""
    dev = _device(y_true, y_pred)
    t = _on_device(y_true, dev).reshape(-1).to(torch.int32)
    p = _on_device(y_pred, dev).reshape(-1).to(torch.int32)
    if t.numel() != p.numel():
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{int(t.numel())}, {int(p.numel())}]")
    buf = torch.zeros(K * K + 1, dtype=torch.int64, device=dev)
    flag = buf[-1:].view(torch.int32)[:1]
    ops.confusion(t, p, K, out=buf[:-1].view(K, K), flag=flag)
    host = buf.cpu()
    if int(host[-1:].view(torch.int32)[0].item()) & 2:
        raise ValueError(f"a class label outside [0, {K})")
    return host.numpy()[:-1].reshape(K, K)


def f1_from_counts(tn, fp, fn, tp, pi0=None):
    """f1score_calib's arithmetic (_metrics_wissam.py:193-212) on the four counts, in its order"""
    pos = fn + tp
    with np.errstate(divide="ignore", invalid="ignore"):
        recall = tp / np.float64(pos)
        if pi0 is not None:
            pi = pos / np.float64(tn + fn + tp + fp)
            ratio = pi * (1 - pi0) / (pi0 * (1 - pi))
            precision = tp / np.float64(tp + ratio * fp)
        else:
            precision = tp / np.float64(tp + fp)
    if np.isnan(precision):
        precision = 0
    if (precision + recall) == 0.0:
        return 0.0
    return (2 * precision * recall) / (precision + recall)


def f1score_calib(y_true, y_pred, pi0=None):
    """f1score_calib (_metrics_wissam.py:175-212) of BINARY predictions (0 / 1 or booleans): the four counts come from the device"""
    cm = _class_counts(y_true, y_pred, 2)
    return f1_from_counts(cm[0, 0], cm[0, 1], cm[1, 0], cm[1, 1], pi0)


def macro_recall_from_counts(cm):
    """recall_score(average="macro") on a confusion matrix: over the classes present in y_true or y_pred, a class without a true
    sample counting 0"""
    cm = np.asarray(cm, np.int64)
    true_sum, tp = cm.sum(axis=1), np.diag(cm)
    present = (true_sum + cm.sum(axis=0)) != 0
    rec = np.zeros(cm.shape[0], np.float64)
    np.divide(tp, true_sum, out=rec, where=true_sum != 0)
    return np.float64(np.average(rec[present]))


def mc_bacc(y_true, y_pred):
    """mc_bacc (:219-221): macro-averaged recall of integer class labels in [0, 32)"""
    return macro_recall_from_counts(_class_counts(y_true, y_pred, 32))
