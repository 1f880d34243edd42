"""Validation / evaluation metrics on the device -- calc_metrics_v2, calc_bootstrap, the curve arrays and the paired permutation
test (koaf_metrics.hip)."""
import torch

from .._lib import KoafError, check, defines, lib
from ._base import FlagWord, _ptr, _stream, check_tensor, out_buffer

METRICS_MAX_N = defines()["KOAF_METRICS_MAX_N"]
METRICS_FLAG_TEXT = {1: "Input contains NaN or infinity.", 2: "a label other than 0 / 1 (binary targets only)",
                     4: "an index of the resampling matrix lies outside [0, n)"}      # (or a rank of `packed` outside its bins)
_WHERE = "the scores' device"   # how this family's refusals name the device its arguments share
_FLAG = FlagWord(METRICS_FLAG_TEXT, _WHERE)
metrics_flag = _FLAG.new        # a zeroed flag word for the metric kernels (koaf.h: bit 0 a non-finite score, 1 a non-binary label, 2 a wild index)
metrics_raise = _FLAG.raise_    # the ValueError of a flag word read back from the device (sklearn raises one for non-finite scores)


def _metric_scores(what, s):
    """(n, stride) of a 1-D fp32 / fp64 device vector with a positive stride: a column of an (n, classes) tensor is read in place"""
    if not torch.is_tensor(s) or s.dtype not in (torch.float32, torch.float64) or s.dim() != 1 or s.numel() == 0 or s.stride(0) < 1:
        raise KoafError(f"{what}: the scores are a non-empty 1-D fp32 / fp64 device vector with a positive stride, got "
                        f"{(tuple(s.shape), s.dtype, s.stride()) if torch.is_tensor(s) else type(s)}")
    return int(s.numel()), int(s.stride(0))


def _int32(what, name, t, like, shape=None):
    check_tensor(what, name, t, torch.int32, shape, like, where=_WHERE)


def _resample_args(what, packed, mat, with_identity, out, pair=False):
    """what curve_metrics / range_metrics (mat = idx) and perm_metrics (pair: mat = masks, packed of pair_ranks) check alike
    -> (n, R, m, out): the samples behind packed, the [R, m] of mat (0, 0 without one) and the fp64 [rows, 8] result buffer"""
    name, kind, src = ("masks", "a mask", "pair_ranks") if pair else ("idx", "an index", "score_ranks")
    if not torch.is_tensor(packed) or not packed.is_cuda:
        raise KoafError(f"{what}: packed is the device tensor {src} returns")
    _int32(what, "packed", packed, packed)
    if pair and (packed.dim() != 1 or packed.numel() == 0 or packed.numel() % 2):
        raise KoafError(f"{what}: packed holds 2n words, got {tuple(packed.shape)}")
    n = int(packed.numel()) // (2 if pair else 1)
    R = m = 0
    if mat is not None:
        _int32(what, name, mat, packed)
        if mat.dim() != 2 or mat.numel() == 0 or (pair and int(mat.shape[1]) != (n + 31) // 32):
            raise KoafError(f"{what}: {name} is a non-empty [R, {(n + 31) // 32 if pair else 'm'}] matrix, got {tuple(mat.shape)}")
        R, m = int(mat.shape[0]), int(mat.shape[1])
    rows = R + (1 if with_identity else 0)
    if rows == 0:
        raise KoafError(f"{what}: neither the identity row nor {kind} matrix")
    return n, R, m, out_buffer(what, out, (rows, 8), torch.float64, packed, "packed's device")


def score_ranks(scores, labels=None, pos_label=1, flag=None):
    """rank[i] = #{j : scores[j] > scores[i]} (int32; ties share a rank, the comparison is made in the scores' own dtype) of a
    1-D fp32 / fp64 device vector of any positive stride, n <= METRICS_MAX_N (koaf_score_ranks: all-pairs counting).  With labels
    (int32 [n], values 0 / 1) also packed[i] = rank[i] << 1 | (labels[i] == pos_label), what curve_metrics / point_metrics read:
    -> (rank, packed).  flag: a metrics_flag() word the kernel raises bits of; None: an own word is read back here (a host
    sync) and a non-finite score or a non-binary label raises ValueError."""
    n, stride = _metric_scores("score_ranks", scores)
    if labels is not None:
        _int32("score_ranks", "labels", labels, scores, (n,))
    with _FLAG.own("score_ranks", flag, scores) as flag:
        rank = torch.empty(n, dtype=torch.int32, device=scores.device)
        packed = torch.empty(n, dtype=torch.int32, device=scores.device) if labels is not None else None
        check(lib().koaf_score_ranks(_ptr(scores), 1 if scores.dtype == torch.float64 else 0, stride, n, _ptr(labels), int(pos_label),
                                     _ptr(rank), _ptr(packed), _ptr(flag), _stream()), "score_ranks")
    return rank if labels is None else (rank, packed)


def curve_metrics(packed, idx=None, with_identity=True, pi0=0.12, out=None, flag=None):
    """out [rows, 8] fp64, row r = (n_pos, n_neg, roc_auc, avg_precision, avg_precision calibrated to the prevalence pi0, 0, 0, 0)
    of one resample of the n samples behind packed (score_ranks): row 0 the sample itself when with_identity, then one row per
    row of idx (int32 [R, m] device indices into the sample, m <= METRICS_MAX_N; None: no resamples).  One block per row
    (koaf_curve_metrics: integer histograms, fixed-order fp64 sums -- identical bits from run to run).  A row without positives or
    without negatives holds its counts and NaN.  flag as in score_ranks (a wild index is skipped and raises)."""
    n, R, m, out = _resample_args("curve_metrics", packed, idx, with_identity, out)
    with _FLAG.own("curve_metrics", flag, packed) as flag:
        check(lib().koaf_curve_metrics(_ptr(packed), n, _ptr(idx), R, m, 1 if with_identity else 0, float(pi0), _ptr(out), _ptr(flag),
                                       _stream()), "curve_metrics")
    return out


def point_metrics(scores, packed, thr=0.5, out=None, flag=None):
    """out [9] fp64 of the sample itself: out[0] the Youden cutoff as the reference's sensitivity_specificity_cutoff picks it
    (first maximum over the points roc_curve(drop_intermediate=True) keeps; a score value, or +inf), out[1:5] = (tn, fp, fn, tp)
    of `scores > thr`, out[5:9] the same of `scores >= cutoff` (koaf_point_metrics, one block).  scores / packed as in score_ranks."""
    n, stride = _metric_scores("point_metrics", scores)
    _int32("point_metrics", "packed", packed, scores, (n,))
    out = out_buffer("point_metrics", out, (9,), torch.float64, scores, _WHERE)
    with _FLAG.own("point_metrics", flag, scores) as flag:
        check(lib().koaf_point_metrics(_ptr(scores), 1 if scores.dtype == torch.float64 else 0, stride, _ptr(packed), n, float(thr),
                                       _ptr(out), _ptr(flag), _stream()), "point_metrics")
    return out


def curve_points_len(n):
    """the fp64 length of curve_points' buffer for n samples: 8 + 8 * (n + 1), known before anything is computed"""
    return int(lib().koaf_curve_points_len(int(n)))


def curve_points(scores, packed, pi0=0.12, pi_of_negatives=False, out=None, flag=None):
    """The ROC / PR curve points of the sample itself in one fp64 buffer [curve_points_len(n)] (koaf_curve_points, one block): a
    header (n_pos, n_neg, T thresholds, K kept ROC thresholds, last_ind, 0, 0, 0) and eight arrays of n + 1 slots -- thr, rec,
    prec, prec calibrated to the prevalence pi0, roc fpr, roc tpr, roc thr, scratch; see koaf.h and parse_curve_points.
    pi_of_negatives: the calibration takes the share of the NEGATIVES as the sample's prevalence (the reference's
    np.sum(y_true) / n when class 0 is the positive one).  scores / packed / flag as in score_ranks."""
    n, stride = _metric_scores("curve_points", scores)
    _int32("curve_points", "packed", packed, scores, (n,))
    out = out_buffer("curve_points", out, (curve_points_len(n),), torch.float64, scores, _WHERE)
    with _FLAG.own("curve_points", flag, scores) as flag:
        check(lib().koaf_curve_points(_ptr(scores), 1 if scores.dtype == torch.float64 else 0, stride, _ptr(packed), n, float(pi0),
                                      1 if pi_of_negatives else 0, _ptr(out), _ptr(flag), _stream()), "curve_points")
    return out


def parse_curve_points(buf):
    """the views into a HOST copy (numpy fp64) of curve_points' buffer: dict of n_pos, n_neg, T, K, last_ind and the arrays
    thr [T]; rec / prec / prec_cal [T + 1] (slot 0 the closing (0, 1) point); fpr / tpr / roc_thr [K + 1] (slot 0 the leading
    (0, 0, inf) point).  Slicing only: nothing is computed here."""
    n = (buf.shape[0] - 8) // 8 - 1
    P, N, T, K, last = (int(v) for v in buf[:5])
    a = buf[8:].reshape(8, n + 1)
    return {"n_pos": P, "n_neg": N, "T": T, "K": K, "last_ind": last, "thr": a[0, :T], "rec": a[1, :T + 1], "prec": a[2, :T + 1],
            "prec_cal": a[3, :T + 1], "fpr": a[4, :K + 1], "tpr": a[5, :K + 1], "roc_thr": a[6, :K + 1]}


def range_metrics(packed, idx=None, with_identity=True, pi0=0.12, recall_range=(0.0, 1.0), out=None, flag=None):
    """out [rows, 8] fp64, row r = (n_pos, n_neg, average precision over the recall range, best calibrated F1, the recall at the
    low end, at the high end, 0, 0) of one resample; rows / idx / with_identity / flag as in curve_metrics (koaf_range_metrics:
    one block per row, fixed-order fp64 sums).  pi0 None: the F1 is not calibrated."""
    n, R, m, out = _resample_args("range_metrics", packed, idx, with_identity, out)
    lo, hi = recall_range
    with _FLAG.own("range_metrics", flag, packed) as flag:
        check(lib().koaf_range_metrics(_ptr(packed), n, _ptr(idx), R, m, 1 if with_identity else 0, 0.0 if pi0 is None else float(pi0),
                                       float(lo), float(hi), _ptr(out), _ptr(flag), _stream()), "range_metrics")
    return out


def confusion(y_true, y_pred, K, out=None, flag=None):
    """counts [K, K] int64, counts[t, p] = #{i : y_true[i] == t and y_pred[i] == p} of two int32 device vectors of class indices,
    K <= 32 (koaf_confusion: integer atomics only).  out: a ZEROED int64 [K, K] to add into.  A label outside [0, K) is skipped and
    raises flag bit 1 (flag as in score_ranks)."""
    if not torch.is_tensor(y_true) or not y_true.is_cuda or y_true.dim() != 1 or y_true.numel() == 0:
        raise KoafError("confusion: y_true is a non-empty 1-D int32 device vector")
    _int32("confusion", "y_true", y_true, y_true)
    _int32("confusion", "y_pred", y_pred, y_true, tuple(y_true.shape))
    K = int(K)
    out = out_buffer("confusion", out, (max(K, 0), max(K, 0)), torch.int64, y_true, "the labels' device", fresh=torch.zeros)     # (K < 1: the library refuses)
    with _FLAG.own("confusion", flag, y_true) as flag:
        check(lib().koaf_confusion(_ptr(y_true), _ptr(y_pred), int(y_true.numel()), K, _ptr(out), _ptr(flag), _stream()), "confusion")
    return out


def pair_ranks(scores_a, scores_b, labels=None, pos_label=1, flag=None):
    """score_ranks over the UNION of two score columns of the same n samples (koaf_pair_ranks): element j < n is scores_a[j],
    element n + j is scores_b[j]; rank[j] = #{k : union[k] > union[j]} (int32 [2n]), so equal scores of the two models share a
    rank.  Both columns are 1-D device vectors of one dtype (fp32 or fp64), each read through its own positive stride,
    n <= METRICS_MAX_N // 2.  With labels (int32 [n]) also packed[j] = rank[j] << 1 | (labels[j mod n] == pos_label), what
    perm_metrics reads: -> (rank, packed).  flag as in score_ranks."""
    n, stride_a = _metric_scores("pair_ranks", scores_a)
    nb, stride_b = _metric_scores("pair_ranks", scores_b)
    if nb != n or scores_b.dtype != scores_a.dtype or scores_b.device != scores_a.device:
        raise KoafError(f"pair_ranks: two columns of one length, dtype and device, got {n} {scores_a.dtype} {scores_a.device} and "
                        f"{nb} {scores_b.dtype} {scores_b.device}")
    if labels is not None:
        _int32("pair_ranks", "labels", labels, scores_a, (n,))
    with _FLAG.own("pair_ranks", flag, scores_a) as flag:
        rank = torch.empty(2 * n, dtype=torch.int32, device=scores_a.device)
        packed = torch.empty(2 * n, dtype=torch.int32, device=scores_a.device) if labels is not None else None
        check(lib().koaf_pair_ranks(_ptr(scores_a), stride_a, _ptr(scores_b), stride_b, 1 if scores_a.dtype == torch.float64 else 0, n,
                                    _ptr(labels), int(pos_label), _ptr(rank), _ptr(packed), _ptr(flag), _stream()), "pair_ranks")
    return rank if labels is None else (rank, packed)


def perm_metrics(packed, masks=None, with_identity=True, out=None, flag=None):
    """out [rows, 8] fp64, row r = (n_pos, n_neg, U_ref, U_cmp, ap_ref, ap_cmp, 0, 0) of one paired permutation of the n samples
    behind packed (pair_ranks, int32 [2n]): row 0 the sample as it is when with_identity, then one row per row of masks (int32
    [R, ceil(n / 32)] device words holding the bits of a uint32 matrix: sample i changes sides when bit i & 31 of word i >> 5 is
    set; None: no permutations).  U is the Mann-Whitney sum 2 * n_pos * n_neg * roc_auc as an exact integer, ap the average
    precision (koaf_perm_metrics: two blocks per row, integer histograms over the 2n union bins, fixed-order fp64 sums --
    identical bits from run to run).  flag as in score_ranks."""
    n, R, _, out = _resample_args("perm_metrics", packed, masks, with_identity, out, pair=True)
    with _FLAG.own("perm_metrics", flag, packed) as flag:
        check(lib().koaf_perm_metrics(_ptr(packed), n, _ptr(masks), R, 1 if with_identity else 0, _ptr(out), _ptr(flag), _stream()),
              "perm_metrics")
    return out
