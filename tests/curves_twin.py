"""Plain-numpy restatement of koaf_curve_points / koaf_range_metrics / koaf_confusion (include/koaf.h) -- a test helper like
metrics_twin.py: the CPU tests check it against the reference's recorded curves and values (fixture F22), the GPU tests use it
where the fixture has no case (the cap n = 16384) and to pin the kernels' summation order.

Every curve value is one IEEE operation chain on integers, so the arrays agree with the device's -- and the reference's -- to the
last bit.  The range sum is taken in the kernel's order: per thread over its contiguous run of bins, then the 256-leaf tree.
"""
import numpy as np

import metrics_twin as M


def _walk(tg, fg):
    """the thresholds (non-empty bins, descending score) -> (bins, tp, fp) with tp / fp the running counts including the bin"""
    g = np.flatnonzero(tg + fg)
    return g, np.cumsum(tg[g]), np.cumsum(fg[g])


def _ratio(P, N, pi0, pi_of_negatives=False):
    pi = np.float64(N if pi_of_negatives else P) / np.float64(P + N)
    with np.errstate(divide="ignore", invalid="ignore"):
        return pi * (1.0 - pi0) / (pi0 * (1.0 - pi))


def curve_points(s, y, pos_label=1, pi0=0.12, pi_of_negatives=False):
    """what ops.parse_curve_points makes of koaf_curve_points' buffer: n_pos, n_neg, T, K, last_ind and the arrays thr [T],
    rec / prec / prec_cal [T + 1], fpr / tpr / roc_thr [K + 1], all fp64"""
    s, y = np.asarray(s), np.asarray(y).reshape(-1)
    n = s.shape[0]
    rank, pos = M.ranks(s), y == pos_label
    tg, fg = M.hist(rank, pos, n)
    P, N = int(tg.sum()), int(fg.sum())
    g, tp, fp = _walk(tg, fg)
    T = g.shape[0]
    by_bin = np.zeros(n, np.float64)
    by_bin[rank] = s.astype(np.float64)
    thr = by_bin[g]
    dtp, dfp = tp.astype(np.float64), fp.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = dtp / np.float64(P)
        prec = dtp / (tp + fp).astype(np.float64)
        cal = dtp / (dtp + _ratio(P, N, pi0, pi_of_negatives) * dfp)
        cal[np.isnan(cal)] = 0.0
        fpr = dfp / np.float64(N)
    keep = np.ones(T, bool)
    if T > 2:
        keep[1:-1] = (tg[g][2:] != tg[g][1:-1]) | (fg[g][2:] != fg[g][1:-1])
    return {"n_pos": P, "n_neg": N, "T": T, "K": int(keep.sum()), "last_ind": int(np.searchsorted(tp, P)), "thr": thr,
            "rec": np.r_[0.0, rec], "prec": np.r_[1.0, prec], "prec_cal": np.r_[1.0, cal],
            "fpr": np.r_[0.0, fpr[keep]], "tpr": np.r_[0.0, rec[keep]], "roc_thr": np.r_[np.inf, thr[keep]]}


def range_row(rank, pos, n, idx=None, pi0=0.12, lo=0.0, hi=1.0):
    """-> (P, N, ap_range, best_f1_calib, rec_at_low, rec_at_high) of one resample; pi0 None: the F1 is not calibrated"""
    tg, fg = M.hist(rank, pos, n, idx)
    P, N = int(tg.sum()), int(fg.sum())
    if P == 0 or N == 0:
        return P, N, np.nan, np.nan, np.nan, np.nan
    g, tp, fp = _walk(tg, fg)
    dtp, dfp = tp.astype(np.float64), fp.astype(np.float64)
    rec, prec = dtp / np.float64(P), dtp / (tp + fp).astype(np.float64)
    rec_p, prec_p = np.r_[0.0, rec[:-1]], np.r_[1.0, prec[:-1]]
    terms = np.zeros(n, np.float64)
    terms[g] = np.where((rec > lo) & (rec_p < hi), (rec - rec_p) * (prec + prec_p) / 2.0, 0.0)
    rlo = max(0.0, rec[rec <= lo].max(initial=0.0))
    rhi = rec[rec >= hi].min()
    ratio = 1.0 if pi0 is None else _ratio(P, N, pi0)
    with np.errstate(divide="ignore", invalid="ignore"):
        cal = dtp / (dtp + ratio * dfp)
        cal[np.isnan(cal)] = 0.0
        f = (2.0 * cal * rec) / (cal + rec)
        ap = M._thread_tree(terms, n) / (rhi - rlo)
    f = np.where(np.isfinite(f) & ((tp - tg[g]) < P), f, 0.0)
    return P, N, ap, max(0.0, f.max()), rlo, rhi


def range_rows(s, y, idx=None, pi0=0.12, recall_range=(0.0, 1.0), pos_label=1):
    """[1 + R, 6]: the identity row, then one row per row of idx -- the first six columns of ops.range_metrics"""
    s, y = np.asarray(s), np.asarray(y).reshape(-1)
    rank, pos, n = M.ranks(s), y == pos_label, s.shape[0]
    rows = [range_row(rank, pos, n, None, pi0, *recall_range)]
    for r in range(0 if idx is None else idx.shape[0]):
        rows.append(range_row(rank, pos, n, idx[r], pi0, *recall_range))
    return np.array(rows, np.float64)


def confusion(y_true, y_pred, K):
    """int64 [K, K] counts of the (true, pred) pairs inside [0, K), and whether a label fell outside"""
    t, p = np.asarray(y_true).astype(np.int64), np.asarray(y_pred).astype(np.int64)
    ok = (t >= 0) & (t < K) & (p >= 0) & (p < K)
    return np.bincount(t[ok] * K + p[ok], minlength=K * K).reshape(K, K).astype(np.int64), bool((~ok).any())
