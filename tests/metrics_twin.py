"""Plain-numpy restatement of the arithmetic of koaf_metrics.hip (include/koaf.h: koaf_score_ranks, koaf_curve_metrics,
koaf_point_metrics) -- a test helper: the CPU tests check it against the reference's recorded values (fixture F18), the GPU tests
use it where the fixture has no case (sizes that reach the large-histogram kernels).

The fp64 sums are taken in the kernel's order -- per thread over its contiguous run of bins, then the 256-leaf tree -- so that
the values agree with the device's to the last bit where its divisions are correctly rounded.
"""
import numpy as np

BLOCK = 256


def ranks(s):
    """rank[i] = #{j : s[j] > s[i]}, in s's own dtype: by counting; beyond 4096 samples from the sorted scores (the same number)"""
    s = np.asarray(s)
    if s.shape[0] > 4096:
        return (s.shape[0] - np.searchsorted(np.sort(s), s, side="right")).astype(np.int32)
    out = np.empty(s.shape[0], np.int32)
    for i0 in range(0, s.shape[0], 512):
        out[i0:i0 + 512] = (s[None, :] > s[i0:i0 + 512, None]).sum(axis=1)
    return out


def hist(rank, pos, n, idx=None):
    """(tp_g, fp_g) per rank bin of the resample idx (None: the identity)"""
    if idx is not None:
        rank, pos = rank[idx], pos[idx]
    return (np.bincount(rank[pos], minlength=n).astype(np.int64), np.bincount(rank[~pos], minlength=n).astype(np.int64))


def _thread_tree(terms, n):
    """sum of per-bin terms as the kernel forms it: thread t adds bins [t L, (t + 1) L) in order, then a tree over the threads"""
    L = -(-n // BLOCK)
    pad = np.zeros(BLOCK * L, terms.dtype)
    pad[:n] = terms
    pad = pad.reshape(BLOCK, L)
    acc = np.zeros(BLOCK, terms.dtype)
    for k in range(L):
        acc = acc + pad[:, k]
    o = BLOCK // 2
    while o:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o //= 2
    return acc[0]


def curve_row(rank, pos, n, idx=None, pi0=0.12):
    """-> (P, N, roc_auc, avg_precision, calibrated avg_precision) of one resample"""
    tg, fg = hist(rank, pos, n, idx)
    P, N = int(tg.sum()), int(fg.sum())
    if P == 0 or N == 0:
        return P, N, np.nan, np.nan, np.nan
    tp, fp = np.cumsum(tg), np.cumsum(fg)
    auc = int((fg * (2 * (tp - tg) + tg)).sum()) / (2.0 * float(P) * float(N))
    dP = np.float64(P)
    pi = dP / np.float64(P + N)
    ratio = pi * (1.0 - pi0) / (pi0 * (1.0 - pi))
    dr = tg.astype(np.float64) / dP
    dtp, dfp = tp.astype(np.float64), fp.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(tg != 0, dtp / (tp + fp).astype(np.float64), 0.0)
        den = dtp + ratio * dfp
        cal = np.where((tg != 0) & (den != 0.0), dtp / den, 0.0)
    return P, N, auc, _thread_tree(dr * prec, n), _thread_tree(dr * cal, n)


def curve_rows(s, y, pos_label=1, idx=None, pi0=0.12):
    """[1 + R, 5]: the identity row, then one row per row of idx -- what ops.curve_metrics(..., with_identity=True) leaves in the
    first five columns"""
    s, y = np.asarray(s), np.asarray(y).reshape(-1)
    rank, pos, n = ranks(s), y == pos_label, s.shape[0]
    rows = [curve_row(rank, pos, n, None, pi0)]
    for r in range(0 if idx is None else idx.shape[0]):
        rows.append(curve_row(rank, pos, n, idx[r], pi0))
    return np.array(rows, np.float64)


def point(s, y, thr=0.5):
    """-> (cutoff in s's dtype, [tn, fp, fn, tp] at s > thr, the same at s >= cutoff): the identity resample with class 1 positive"""
    s, y = np.asarray(s), np.asarray(y).reshape(-1)
    n = s.shape[0]
    rank, pos = ranks(s), y == 1
    tg, fg = hist(rank, pos, n)
    P, N = int(tg.sum()), int(fg.sum())
    g = np.flatnonzero(tg + fg)                                  # the thresholds, by descending score
    tgk, fgk = tg[g], fg[g]
    keep = np.ones(g.shape[0], bool)
    if g.shape[0] > 2:
        keep[1:-1] = (tgk[2:] != tgk[1:-1]) | (fgk[2:] != fgk[1:-1])
    j = np.cumsum(tgk) / np.float64(P) - np.cumsum(fgk) / np.float64(N)
    j = np.where(keep, j, -np.inf)
    k = int(np.argmax(j))
    if not j[k] > 0.0:                                           # the leading (0, 0, inf) point comes first and is worth 0
        cutoff = s.dtype.type(np.inf)
    else:
        cutoff = s[np.flatnonzero(rank == g[k])[0]]

    def confusion(pred):
        return [int((~pos & ~pred).sum()), int((~pos & pred).sum()), int((pos & ~pred).sum()), int((pos & pred).sum())]
    return cutoff, confusion(s.astype(np.float64) > thr), confusion(s >= cutoff)


def calc_metrics_plain(y, proba, pi0=0.12):
    """the eight unrounded values of calc_metrics_v2(bootstrap=False) after sample_size / num_pos / num_neg, in key order"""
    y = np.asarray(y).reshape(-1)
    r1 = curve_rows(proba[:, 1], y, 1, None, pi0)[0]
    r0 = curve_rows(proba[:, 0], y, 0, None, pi0)[0]
    cutoff, c5, cc = point(proba[:, 1], y)
    youden = cc[3] / (cc[3] + cc[2]) + cc[0] / (cc[0] + cc[1]) - 1.0
    bacc = (c5[0] / (c5[0] + c5[1]) + c5[3] / (c5[3] + c5[2])) / 2
    return [y.sum() / y.shape[0], r1[2], r1[3], r1[4], r0[3], cutoff, youden, bacc]
