"""Calibration of predicted probabilities on the device -- Brier score, log-loss, reliability bins with ECE / MCE, net benefit,
quantile bin edges and logistic recalibration (koaf_calib.hip)."""
import torch

from .._lib import KoafError, check, defines, lib
from ._base import FlagWord, _ptr, _stream, check_tensor, out_buffer
from .metrics import METRICS_FLAG_TEXT, _metric_scores

CALIB_MAX_BINS = defines()["KOAF_CALIB_MAX_BINS"]
CALIB_MAX_THR = defines()["KOAF_CALIB_MAX_THR"]
RECALIB_MAX_ITER = defines()["KOAF_RECALIB_MAX_ITER"]
CALIB_EPS = 2.0 ** -52          # the clip of log-loss and of the logit: fp64's eps, whatever the scores' dtype
RECALIB_KINDS = {"proba": 0, "logit": 1}
RECALIB_MODES = {"slope_intercept": 0, "temperature": 1, "intercept": 2}
RECALIB_STATUS = {0: "converged", 1: "iteration cap reached", 2: "no finite optimum (separable data)", 3: "one class only"}
CALIB_FLAG_TEXT = dict(METRICS_FLAG_TEXT)
CALIB_FLAG_TEXT[8] = "a logistic recalibration did not converge (iteration cap, separable data or one class only)"
_WHERE = "the scores' device"
_FLAG = FlagWord(CALIB_FLAG_TEXT, _WHERE)
calib_flag = _FLAG.new          # a zeroed flag word for the calibration kernels (koaf.h: bits 0-2 the metric kernels', bit 3 a fit that did not converge)
calib_raise = _FLAG.raise_      # the ValueError of a flag word read back from the device


def _f64(s):
    return 1 if s.dtype == torch.float64 else 0


def _rows(what, scores, labels, idx, with_identity):
    """what calib_metrics and recalib_fit check alike -> (n, stride, R, m, rows)"""
    n, stride = _metric_scores(what, scores)
    check_tensor(what, "labels", labels, torch.int32, (n,), scores, where=_WHERE)
    R = m = 0
    if idx is not None:
        check_tensor(what, "idx", idx, torch.int32, None, scores, where=_WHERE)
        if idx.dim() != 2 or idx.numel() == 0:
            raise KoafError(f"{what}: idx is a non-empty [R, m] matrix, got {tuple(idx.shape)}")
        R, m = int(idx.shape[0]), int(idx.shape[1])
    rows = R + (1 if with_identity else 0)
    if rows == 0:
        raise KoafError(f"{what}: neither the identity row nor an index matrix")
    return n, stride, R, m, rows


def _second(what, scores, scores0, kind):
    """the optional second column of kind "logit" -> its stride (0 without one)"""
    if kind not in RECALIB_KINDS:
        raise KoafError(f"{what}: kind is one of {tuple(RECALIB_KINDS)}, got {kind!r}")
    if scores0 is None:
        return 0
    n0, stride0 = _metric_scores(what, scores0)
    if kind != "logit" or n0 != int(scores.numel()) or scores0.dtype != scores.dtype or scores0.device != scores.device:
        raise KoafError(f"{what}: scores0 is the second column of kind 'logit': one length, dtype and device with the scores, got "
                        f"{n0} {scores0.dtype} {scores0.device} for kind {kind!r}")
    return stride0


def calib_edges(scores, q, out=None, flag=None):
    """edges [nbins + 1] fp64 = np.percentile(scores, 100 * q) (numpy's default linear method) of a 1-D fp32 / fp64 device vector of
    any positive stride, n <= METRICS_MAX_N, for the nbins + 1 fractions q (fp64 device vector, nbins <= CALIB_MAX_BINS;
    calibration_curve's quantile strategy passes linspace(0, 1, nbins + 1)).  koaf_calib_edges: one block, order statistics by
    all-pairs counting, numpy's two-sided lerp -- bit-equal to numpy on fp64 scores (fp32 scores are widened first).  flag: a
    calib_flag() word; None: an own word is read back here (a host sync) and a non-finite score raises ValueError."""
    n, stride = _metric_scores("calib_edges", scores)
    check_tensor("calib_edges", "q", q, torch.float64, None, scores, nonempty=True, where=_WHERE)
    if q.dim() != 1 or q.numel() < 2:
        raise KoafError(f"calib_edges: q holds nbins + 1 >= 2 fractions, got {tuple(q.shape)}")
    nbins = int(q.numel()) - 1
    out = out_buffer("calib_edges", out, (nbins + 1,), torch.float64, scores, _WHERE)
    with _FLAG.own("calib_edges", flag, scores) as flag:
        check(lib().koaf_calib_edges(_ptr(scores), _f64(scores), stride, n, _ptr(q), nbins, _ptr(out), _ptr(flag), _stream()), "calib_edges")
    return out


def calib_metrics(scores, labels, edges, thr=None, idx=None, with_identity=True, eps=CALIB_EPS, out=None, bins=None, nb=None,
                  want_bins=True, flag=None):
    """-> (out, bins, nb).  out [rows, 8] fp64, row r = (n_pos, n_neg, brier, log_loss, mean_p, ece, mce, bins in use) of one
    resample of the n scored samples (scores as in score_ranks, labels int32 [n] of 0 / 1): row 0 the sample itself when
    with_identity, then one row per row of idx (int32 [R, m] device indices, m <= METRICS_MAX_N).  edges: fp64 device [nbins + 1],
    nbins <= CALIB_MAX_BINS; a score's bin is the number of inner edges below it (a score on an edge goes to the lower bin).
    bins [rows, nbins, 3] = (count, positives, score sum) per bin (want_bins=False and no buffer: None).  thr: fp64 device [T],
    T <= CALIB_MAX_THR, each in (0, 1) -> nb [rows, T, 4] = (tp, fp, net benefit, net benefit of treating all) of `scores >= t`;
    None: no nb.  koaf_calib_metrics: one block per row, integer counts, fixed-order fp64 sums -- identical bits from run to run.
    A one-class row keeps finite values.  flag as in calib_edges (a wild index is skipped and raises)."""
    n, stride, R, m, rows = _rows("calib_metrics", scores, labels, idx, with_identity)
    check_tensor("calib_metrics", "edges", edges, torch.float64, None, scores, where=_WHERE)
    if edges.dim() != 1 or edges.numel() < 2:
        raise KoafError(f"calib_metrics: edges holds nbins + 1 >= 2 values, got {tuple(edges.shape)}")
    nbins, T = int(edges.numel()) - 1, 0
    if thr is not None:
        check_tensor("calib_metrics", "thr", thr, torch.float64, None, scores, where=_WHERE)
        if thr.dim() != 1:
            raise KoafError(f"calib_metrics: thr is a [T] vector, got {tuple(thr.shape)}")
        T = int(thr.numel())
    elif nb is not None:
        raise KoafError("calib_metrics: nb without thresholds")
    out = out_buffer("calib_metrics", out, (rows, 8), torch.float64, scores, _WHERE)
    if bins is not None or want_bins:
        bins = out_buffer("calib_metrics", bins, (rows, nbins, 3), torch.float64, scores, _WHERE)
    if T > 0:
        nb = out_buffer("calib_metrics", nb, (rows, T, 4), torch.float64, scores, _WHERE)
    elif thr is not None:
        nb = out_buffer("calib_metrics", nb, (rows, 0, 4), torch.float64, scores, _WHERE)     # (T = 0: nothing to launch for)
    with _FLAG.own("calib_metrics", flag, scores) as flag:
        check(lib().koaf_calib_metrics(_ptr(scores), _f64(scores), stride, _ptr(labels), n, _ptr(edges), nbins,
                                       _ptr(thr) if T > 0 else None, T, _ptr(idx), R, m, 1 if with_identity else 0, float(eps),
                                       _ptr(out), _ptr(bins), _ptr(nb) if T > 0 else None, _ptr(flag), _stream()), "calib_metrics")
    return out, bins, nb


def recalib_fit(scores, labels, kind="proba", mode="slope_intercept", scores0=None, idx=None, with_identity=True, eps=CALIB_EPS,
                tol=1e-10, max_iter=50, out=None, flag=None):
    """report [rows, 8] fp64, row r = (a, b, steps, max|g_free| / draws, L / draws, status, n_pos, n_neg) of the unpenalised
    logistic regression of the labels on a + b * x over one resample (rows / idx / with_identity as in calib_metrics).
    kind "proba": x = logit(clip(score, eps, 1 - eps)); "logit": x = score (- scores0, a second column of the same dtype: the two
    columns of a (B, 2) logits tensor in place).  mode "slope_intercept": a and b free; "temperature": a = 0 (T = 1 / b);
    "intercept": b = 1.  koaf_recalib_fit: Newton from (0, 1) with step halving, one block per row, fixed-order fp64 sums; stops at
    max|g_free| / draws <= tol or after max_iter <= RECALIB_MAX_ITER steps.  status: RECALIB_STATUS; a and b are NaN for status >= 2.
    A status other than 0 raises flag bit 3: pass an own calib_flag() word to read the statuses instead of raising."""
    n, stride, R, m, rows = _rows("recalib_fit", scores, labels, idx, with_identity)
    stride0 = _second("recalib_fit", scores, scores0, kind)
    if mode not in RECALIB_MODES:
        raise KoafError(f"recalib_fit: mode is one of {tuple(RECALIB_MODES)}, got {mode!r}")
    out = out_buffer("recalib_fit", out, (rows, 8), torch.float64, scores, _WHERE)
    with _FLAG.own("recalib_fit", flag, scores) as flag:
        check(lib().koaf_recalib_fit(_ptr(scores), _f64(scores), stride, _ptr(scores0), stride0, _ptr(labels), n, RECALIB_KINDS[kind],
                                     RECALIB_MODES[mode], _ptr(idx), R, m, 1 if with_identity else 0, float(eps), float(tol),
                                     int(max_iter), _ptr(out), _ptr(flag), _stream()), "recalib_fit")
    return out


def recalib_apply(scores, a, b, kind="proba", scores0=None, eps=CALIB_EPS, out=None, flag=None):
    """out [n] fp64 = sigmoid(a + b * x), x of the scores as in recalib_fit (koaf_recalib_apply, element-wise); a, b: host floats"""
    n, stride = _metric_scores("recalib_apply", scores)
    stride0 = _second("recalib_apply", scores, scores0, kind)
    out = out_buffer("recalib_apply", out, (n,), torch.float64, scores, _WHERE)
    with _FLAG.own("recalib_apply", flag, scores) as flag:
        check(lib().koaf_recalib_apply(_ptr(scores), _f64(scores), stride, _ptr(scores0), stride0, n, RECALIB_KINDS[kind], float(a),
                                       float(b), float(eps), _ptr(out), _ptr(flag), _stream()), "recalib_apply")
    return out
