"""Plain-numpy fp64 restatement of koaf_calib.hip (include/koaf.h: koaf_calib_edges, koaf_calib_metrics, koaf_recalib_fit,
koaf_recalib_apply) -- a test helper like metrics_twin.py: the CPU tests check it against scikit-learn's and numpy's recorded
values (fixture F25), the GPU tests use it to pin the kernels' summation order and their Newton iteration.

Every fp64 sum is taken in the kernels' order: thread t adds the draws [t L, (t + 1) L) of the row, L = ceil(draws / 256), in row
order, then the 256-leaf tree (metrics_twin._thread_tree).  A skipped draw (an index outside [0, n)) adds +0.0, which changes no
bit.  The Newton iteration has the kernel's start (0, 1), step rule (the full step, then at most 30 halvings until L does not
increase) and stopping rule; only exp / log / log1p may differ from the device's in their last places.
"""
import numpy as np

from metrics_twin import _thread_tree

EPS = 2.0 ** -52
L_SLACK = 2.0 ** -45        # the rounding of L itself that "L does not increase" allows (koaf_calib.hip CB_L_SLACK)
MODES = {"slope_intercept": 0, "temperature": 1, "intercept": 2}


def edges(s, q):
    """np.percentile(s, 100 q), default linear method, restated: h = q (n - 1), the two neighbouring order statistics, numpy's lerp"""
    x = np.sort(np.asarray(s).astype(np.float64))
    n = x.shape[0]
    out = np.empty(len(q), np.float64)
    for k, qk in enumerate(np.asarray(q, np.float64)):
        h = qk * np.float64(n - 1)
        if h < 0:
            lo = hi = 0
        elif h < n - 1:
            lo = int(np.floor(h))
            hi = lo + 1
        else:
            lo = hi = n - 1
        a, b, t = x[lo], x[hi], h - np.float64(lo)
        d = b - a
        out[k] = b - d * (1.0 - t) if t >= 0.5 else a + d * t
    return out


def bin_of(p, edge):
    """#{k in 1 .. nbins - 1 : edge[k] < p}: np.searchsorted(edge[1:-1], p, side="left")"""
    return (np.asarray(edge, np.float64)[None, 1:-1] < np.asarray(p, np.float64)[:, None]).sum(axis=1)


def _draws(n, idx):
    """-> (the row's indices, which of them are followed)"""
    i = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    ok = (i >= 0) & (i < n)
    return np.where(ok, i, 0), ok


def metrics_row(s, y, edge, thr=None, idx=None, eps=EPS):
    """-> (out [8], bins [nbins, 3], nb [T, 4] or None) of one row, as koaf_calib_metrics writes them"""
    s64, y = np.asarray(s).astype(np.float64), np.asarray(y).reshape(-1)
    i, ok = _draws(s64.shape[0], idx)
    draws = i.shape[0]
    p, pos = s64[i], (y[i] == 1) & ok
    neg = ok & ~pos
    dm = np.float64(draws)
    e = p - pos.astype(np.float64)
    py = np.where(pos, p, 1.0 - p)
    with np.errstate(divide="ignore"):
        ll = -np.log(np.clip(py, eps, 1.0 - eps))
    brier, logloss, sp = (_thread_tree(np.where(ok, t, 0.0), draws) for t in (e * e, ll, p))
    nbins = len(edge) - 1
    b = bin_of(p, edge)
    bins = np.zeros((nbins, 3), np.float64)
    ece, mce, used = np.float64(0.0), np.float64(0.0), 0
    for k in range(nbins):
        inb = ok & (b == k)
        bins[k] = (inb.sum(), (inb & pos).sum(), _thread_tree(np.where(inb, p, 0.0), draws))
        if bins[k, 0]:
            gap = abs(bins[k, 1] - bins[k, 2])
            ece = ece + gap
            mce = max(mce, gap / bins[k, 0])
            used += 1
    P, N = np.float64(pos.sum()), np.float64(neg.sum())
    out = np.array([P, N, brier / dm, logloss / dm, sp / dm, ece / dm, mce, used], np.float64)
    nb = None
    if thr is not None:
        thr = np.asarray(thr, np.float64)
        nb = np.empty((thr.shape[0], 4), np.float64)
        for k, t in enumerate(thr):
            tp, fp = np.float64((pos & (p >= t)).sum()), np.float64((neg & (p >= t)).sum())
            w = t / (1.0 - t)
            nb[k] = (tp, fp, tp / dm - (fp / dm) * w, P / dm - (N / dm) * w)
    return out, bins, nb


def metrics_rows(s, y, edge, thr=None, idx=None, with_identity=True, eps=EPS):
    """the three buffers of ops.calib_metrics: out [rows, 8], bins [rows, nbins, 3], nb [rows, T, 4] (None without thresholds)"""
    rows = ([None] if with_identity else []) + ([] if idx is None else list(idx))
    got = [metrics_row(s, y, edge, thr, r, eps) for r in rows]
    return (np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), None if thr is None else np.stack([g[2] for g in got]))


def x_of(s, kind="proba", s0=None, eps=EPS):
    """the regressor of the recalibration: the logit of the clipped probability, or the score (minus the second column)"""
    v = np.asarray(s).astype(np.float64)
    if kind == "proba":
        p = np.clip(v, eps, 1.0 - eps)
        return np.log(p) - np.log1p(-p)
    return v if s0 is None else v - np.asarray(s0).astype(np.float64)


def _sigmoid(eta):
    e = np.exp(-np.abs(eta))
    den = 1.0 + e
    return np.where(eta >= 0.0, 1.0 / den, e / den), np.maximum(eta, 0.0) + np.log1p(e)


def evaluate(x, pos, ok, a, b):
    """L, (g_a, g_b), (h_aa, h_ab, h_bb) and the number of draws the line does not put strictly on their side, at (a, b)"""
    draws = x.shape[0]
    eta = a + b * x
    sig, spl = _sigmoid(eta)
    res, w = sig - pos.astype(np.float64), sig * (1.0 - sig)
    wx = w * x
    terms = (np.where(pos, spl - eta, spl), res, res * x, w, wx, wx * x)
    L, ga, gb, haa, hab, hbb = (_thread_tree(np.where(ok, t, 0.0), draws) for t in terms)
    sep = int((ok & ~np.where(pos, eta > 0.0, eta < 0.0)).sum())
    return L, (ga, gb), (haa, hab, hbb), sep


def fit_row(x, y, mode="slope_intercept", idx=None, tol=1e-10, max_iter=50):
    """koaf_recalib_fit's row: (a, b, steps, max|g_free| / draws, L / draws, status, P, N); x is x_of the whole sample"""
    mode = MODES.get(mode, mode)
    y = np.asarray(y).reshape(-1)
    i, ok = _draws(x.shape[0], idx)
    xr, pos = x[i], (y[i] == 1) & ok
    dm = np.float64(i.shape[0])
    P, N = float(pos.sum()), float((ok & ~pos).sum())
    nan = np.float64(np.nan)
    if P == 0 or N == 0:
        return np.array([nan, nan, 0, nan, nan, 3, P, N], np.float64)
    a, b, status, it = np.float64(0.0), np.float64(1.0), 1, 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        L, (ga, gb), (haa, hab, hbb), sep = evaluate(xr, pos, ok, a, b)
        while True:
            gmax = max(0.0 if mode == 1 else abs(ga), 0.0 if mode == 2 else abs(gb)) / dm
            if not (np.isfinite(L) and np.isfinite(gmax)) or (mode != 2 and sep == 0):
                status = 2
                break
            if gmax <= tol:
                status = 0
                break
            if it == max_iter:
                break
            da = db = np.float64(0.0)
            if mode == 0:
                det = haa * hbb - hab * hab
                if not (haa > 0.0 and det > 0.0):
                    status = 2
                    break
                da, db = (hbb * ga - hab * gb) / det, (haa * gb - hab * ga) / det
            elif mode == 1:
                if not hbb > 0.0:
                    status = 2
                    break
                db = gb / hbb
            else:
                if not haa > 0.0:
                    status = 2
                    break
                da = ga / haa
            step, took = np.float64(1.0), False
            for _ in range(31):
                na, nb = a - step * da, b - step * db
                if evaluate(xr, pos, ok, na, nb)[0] <= L + L_SLACK * abs(L):
                    took = True
                    break
                step = step * 0.5
            if not took:
                break
            if not (np.isfinite(na) and np.isfinite(nb)):
                status = 2
                break
            a, b, it = na, nb, it + 1
            L, (ga, gb), (haa, hab, hbb), sep = evaluate(xr, pos, ok, a, b)
    if status >= 2:
        a = b = nan
    return np.array([a, b, it, gmax, L / dm, status, P, N], np.float64)


def fit_rows(x, y, mode="slope_intercept", idx=None, with_identity=True, tol=1e-10, max_iter=50):
    rows = ([None] if with_identity else []) + ([] if idx is None else list(idx))
    return np.stack([fit_row(x, y, mode, r, tol, max_iter) for r in rows])


def apply(x, a, b):
    return _sigmoid(a + b * x)[0]


def gradient(x, y, a, b, idx=None):
    """(g_a, g_b, H [2, 2]) at (a, b) over the row's own draws, plain numpy sums: what the GPU tests judge a fit by"""
    i = np.arange(x.shape[0]) if idx is None else np.asarray(idx)
    xr, yr = x[i], (np.asarray(y).reshape(-1)[i] == 1).astype(np.float64)
    sig = _sigmoid(a + b * xr)[0]
    w = sig * (1.0 - sig)
    return np.sum(sig - yr), np.sum((sig - yr) * xr), np.array([[w.sum(), (w * xr).sum()], [(w * xr).sum(), (w * xr * xr).sum()]])
