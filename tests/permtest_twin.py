"""Plain-numpy restatement of koaf_pair_ranks / koaf_perm_metrics (include/koaf.h) -- a test helper next to tests/metrics_twin.py,
whose pieces it uses: the CPU tests check it against fixture F20 (scikit-learn's per-permutation values), the GPU tests use it
where the fixture has no case and for bit equality.

Same bin ownership and summation order as the kernel: 2n union bins, thread t owns bins [t L, (t + 1) L) with L = ceil(2n / 256),
then the 256-leaf tree.
"""
import numpy as np

import metrics_twin as T


def unpack_masks(masks, n):
    """uint32 [R, ceil(n / 32)] -> bool [R, n]: sample i is bit i & 31 of word i >> 5"""
    masks = np.asarray(masks, np.uint32)
    i = np.arange(n)
    return ((masks[:, i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def pair_ranks(a, b):
    """rank[j] = #{k : s[k] > s[j]} over the union s = (a, b), in the columns' own dtype (int32 [2n])"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return T.ranks(np.concatenate([a, b]))


def packed(a, b, y, pos_label=1):
    y = np.asarray(y).reshape(-1)
    return ((pair_ranks(a, b).astype(np.int32) << 1) | np.tile(y == pos_label, 2)).astype(np.int32)


def side_row(rank, pos, n):
    """-> (P, N, U, ap) of one side: the n ranks it counts, over the 2n bins"""
    tg, fg = T.hist(rank, pos, 2 * n)
    P, N = int(tg.sum()), int(fg.sum())
    if P == 0 or N == 0:
        return P, N, np.nan, np.nan
    tp, fp = np.cumsum(tg), np.cumsum(fg)
    U = int((fg * (2 * (tp - tg) + tg)).sum())
    dr = tg.astype(np.float64) / np.float64(P)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(tg != 0, tp.astype(np.float64) / (tp + fp).astype(np.float64), 0.0)
    return P, N, float(U), T._thread_tree(dr * prec, 2 * n)


def perm_rows(a, b, y, masks=None, with_identity=True, pos_label=1):
    """[rows, 8]: what ops.perm_metrics leaves -- (P, N, U_ref, U_cmp, ap_ref, ap_cmp, 0, 0) of the identity row (when asked for)
    and of every mask row"""
    y = np.asarray(y).reshape(-1)
    n = y.shape[0]
    rank, pos = pair_ranks(a, b), y == pos_label
    swaps = np.zeros((0, n), bool) if masks is None else unpack_masks(masks, n)
    if with_identity:
        swaps = np.concatenate([np.zeros((1, n), bool), swaps])
    out = np.zeros((swaps.shape[0], 8), np.float64)
    for r, sw in enumerate(swaps):
        P, N, ua, pa = side_row(np.where(sw, rank[n:], rank[:n]), pos, n)
        _, _, ub, pb = side_row(np.where(sw, rank[:n], rank[n:]), pos, n)
        out[r, :6] = (P, N, ua, ub, pa, pb)
    return out
