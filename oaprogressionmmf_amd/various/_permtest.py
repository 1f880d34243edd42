"""The paired permutation test of the "Permutation testing" cell of koafusion/run/Analysis_Visualization.ipynb on the device:
is model `cmp` better than model `ref` on the same knees?  The reference calls, for ROC-AUC and for average precision,
    scipy.stats.permutation_test(data=(x_ref, x_cmp), permutation_type="samples", n_resamples=1000, alternative="two-sided",
                                 statistic=metric(cmp) - metric(ref))
which is 2 x 1000 scikit-learn evaluations per call, each with its own argsort.  Here: no scipy, no scikit-learn, no sort.

A permutation swaps the two predictions of some samples.  That does not change the order of the union of the 2n scores, so the
union is ranked once (ops.pair_ranks) and every permutation is, per side, an integer histogram over the 2n rank bins
(ops.perm_metrics: all rows, both sides and both metrics in one launch).  The labels do not move, so P and N are the same on both
sides of every row, and ROC-AUC differences are compared as the integers U_cmp - U_ref (U = 2 P N roc_auc, the Mann-Whitney sum):
equal statistics are equal integers, whatever their quotient rounds to.  One fp64 device buffer is copied to the host once: the
only synchronisation of a call.

The swap masks come from the HOST.  The reference hands scipy no generator, so its own draws differ from run to run and there is
no stream to replay; a seeded numpy draw (swap_masks) is the contract here, and passing the same seed gives the same p-value.
The p-value arithmetic on the R statistics is scipy's own (its `less` / `greater` / `two_sided` closures).
"""
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from ._metrics import _ONE_CLASS, _device, _on_device, _scores

PERM_METRICS = ("roc_auc", "avg_precision")
ALTERNATIVES = ("two-sided", "less", "greater")
PermutationTestResult = namedtuple("PermutationTestResult", ("statistic", "pvalue", "null_distribution"))


def pack_masks(bits):
    """a 0 / 1 matrix [R, n] -> uint32 [R, ceil(n / 32)]: sample i is bit i & 31 of word i >> 5"""
    bits = np.asarray(bits, np.uint8)
    R, n = bits.shape
    W = (n + 31) // 32
    pad = np.zeros((R, W * 32), np.uint8)
    pad[:, :n] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<u4")


def swap_masks(n, n_resamples, seed=0):
    """The permutations of a paired test of n samples as swap masks: -> (masks uint32 [R, ceil(n / 32)], exact).
    Sample i changes sides in row r when bit i & 31 of masks[r, i >> 5] is set.
    exact (scipy's rule for paired samples: 2 ** n <= n_resamples): all R = 2 ** n assignments, row r swapping sample i iff bit i
    of r is set, so row 0 is the sample as observed.
    Otherwise R = n_resamples rows drawn as np.random.default_rng(seed).integers(0, 2, size=(R, n), dtype=np.uint8).  The
    reference passes scipy no generator, so its own draws are not reproducible and there is nothing to replay: this seeded host
    draw is the contract."""
    n, n_resamples = int(n), int(n_resamples)
    if n < 1 or n_resamples < 0:
        raise ValueError(f"swap_masks: n >= 1 and n_resamples >= 0, got {n}, {n_resamples}")
    if n < 63 and 2 ** n <= n_resamples:
        r = np.arange(2 ** n, dtype=np.int64)
        return pack_masks((r[:, None] >> np.arange(n)[None, :]) & 1), True
    bits = np.random.default_rng(seed).integers(0, 2, size=(n_resamples, n), dtype=np.uint8)
    return pack_masks(bits), False


def permutation_pvalues(null, observed, exact, gamma):
    """scipy.stats.permutation_test's p-values of the statistics `null` (one per permutation) around `observed`:
    less = (#{null <= observed + gamma} + adj) / (R + adj), greater = (#{null >= observed - gamma} + adj) / (R + adj),
    two-sided = min(1, 2 min(less, greater)); adj = 0 for an exact test, 1 for a randomized one.
    -> {"less": ..., "greater": ..., "two-sided": ...}"""
    null = np.asarray(null)
    adj = 0 if exact else 1
    R = null.shape[0]
    less = (np.count_nonzero(null <= observed + gamma) + adj) / (R + adj)
    greater = (np.count_nonzero(null >= observed - gamma) + adj) / (R + adj)
    return {"less": np.float64(less), "greater": np.float64(greater),
            "two-sided": np.float64(min(1.0, 2.0 * min(less, greater)))}


def results_from_rows(rows, exact, metrics=PERM_METRICS, alternative="two-sided"):
    """the host end of the test: rows [1 + R, 8] of ops.perm_metrics (row 0 the sample as observed; for an exact test the R rows
    behind it are all assignments) -> {metric: PermutationTestResult}.
    roc_auc: the integers D = U_cmp - U_ref are compared, gamma = 0; statistic and null distribution are D / (2 P N).
    avg_precision: the fp64 differences, with scipy's gamma = |100 eps observed|."""
    rows = np.asarray(rows, np.float64)
    P, N = rows[0, 0], rows[0, 1]
    out = {}
    for m in metrics:
        if m == "roc_auc":
            d = np.rint(rows[:, 3] - rows[:, 2]).astype(np.int64)             # (both < 2^27: the difference is exact)
            pv = permutation_pvalues(d[1:], d[0], exact, 0)
            stat, null = d[0] / (2.0 * P * N), d[1:] / (2.0 * P * N)
        else:
            d = rows[:, 5] - rows[:, 4]
            pv = permutation_pvalues(d[1:], d[0], exact, np.abs(100.0 * np.finfo(np.float64).eps * d[0]))
            stat, null = d[0], d[1:].copy()
        out[m] = PermutationTestResult(np.float64(stat), pv[alternative], null)
    return out


def _as_masks(masks, n):
    masks = np.ascontiguousarray(masks)
    if masks.dtype != np.uint32 or masks.ndim != 2 or masks.shape[1] != (n + 31) // 32:
        raise ValueError(f"masks is a uint32 [R, {(n + 31) // 32}] matrix (swap_masks), got {masks.dtype} {masks.shape}")
    return masks


def _test(y_true, y_pred_ref, y_pred_cmp, metrics, n_resamples, alternative, seed, masks):
    for m in metrics:
        if m not in PERM_METRICS:
            raise ValueError(f"Unknown metric: {m!r} (one of {PERM_METRICS})")
    if alternative not in ALTERNATIVES:
        raise ValueError(f"Unknown alternative: {alternative!r} (one of {ALTERNATIVES})")
    dev = _device(y_pred_ref, y_pred_cmp, y_true)
    labels = _on_device(y_true, dev).reshape(-1).to(torch.int32)
    a, b = _on_device(y_pred_ref, dev), _on_device(y_pred_cmp, dev)
    n = int(labels.numel())
    if a.dim() != 1 or b.dim() != 1 or int(a.numel()) != n or int(b.numel()) != n:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{n}, {tuple(a.shape)}, {tuple(b.shape)}]")
    if a.dtype != b.dtype:
        a, b = a.to(torch.float64), b.to(torch.float64)
    a, b = (s if s.stride(0) >= 1 else s.contiguous() for s in (_scores(a), _scores(b)))    # (an expanded column: copied)
    if masks is None:
        masks, exact = swap_masks(n, n_resamples, seed)
    else:
        masks, exact = _as_masks(masks, n), False
    R = int(masks.shape[0])
    rows = 1 + R
    buf = torch.zeros(rows * 8 + 1, dtype=torch.float64, device=dev)
    flag = buf[rows * 8:].view(torch.int32)[:1]
    masks_dev = torch.from_numpy(masks.view(np.int32)).to(dev) if R else None
    _, packed = ops.pair_ranks(a, b, labels, flag=flag)
    ops.perm_metrics(packed, masks_dev, True, out=buf[:rows * 8].view(rows, 8), flag=flag)
    host = buf.cpu()                                       # the one synchronisation
    ops.metrics_raise(host[rows * 8:].view(torch.int32)[0].item())
    table = host.numpy()[:rows * 8].reshape(rows, 8)
    if table[0, 0] == 0 or table[0, 1] == 0:
        raise ValueError(_ONE_CLASS)
    return results_from_rows(table, exact, metrics, alternative)


def permutation_test_paired(y_true, y_pred_ref, y_pred_cmp, metrics=PERM_METRICS, n_resamples=1000, alternative="two-sided", seed=0,
                            masks=None):
    """scipy.stats.permutation_test(data=(y_pred_ref, y_pred_cmp), permutation_type="samples", n_resamples=n_resamples,
    alternative=alternative, statistic=metric(y_true, cmp) - metric(y_true, ref)) for each metric of `metrics` ("roc_auc":
    roc_auc_score, "avg_precision": average_precision_score), all of them from one device pass.
    -> {metric: PermutationTestResult(statistic, pvalue, null_distribution)} (scipy's attribute names).

    y_true (sample,) holds 0 / 1 and is narrowed to int32 as calc_metrics_v2 narrows it: a fractional label is truncated, not
    reported.  The two score vectors are numpy arrays or device tensors; a device tensor with a positive stride is read in place
    through it (proba[:, 1]), one without (an expanded scalar) is copied.  Two fp32 or two fp64 vectors are ranked in that
    precision, anything else is widened to fp64.  At most ops.METRICS_MAX_N // 2 = 8192 samples.
    2 ** n <= n_resamples: the exact test over all 2 ** n assignments (p = count / 2 ** n); otherwise a randomized test of
    n_resamples permutations drawn by swap_masks(n, n_resamples, seed) (p = (count + 1) / (n_resamples + 1)).  masks: a uint32
    [R, ceil(n / 32)] matrix to use in place of that draw, counted as a random draw of R permutations.
    ROC-AUC statistics are compared as exact integers; average-precision statistics with scipy's tolerance |100 eps observed|."""
    return _test(y_true, y_pred_ref, y_pred_cmp, tuple(metrics), n_resamples, alternative, seed, masks)


def compare_predictions(prog_target, proba_ref, proba_cmp, n_resamples=1000, alternative="two-sided", seed=0):
    """One row of the notebook's table: column 1 of two (sample, class) probability tables of the same samples, both metrics from
    one device pass.  -> {"pvalue__roc_auc", "statistic__roc_auc", "pvalue__ap", "statistic__ap"}"""
    for p in (proba_ref, proba_cmp):
        if p.ndim != 2 or p.shape[1] < 2:
            raise ValueError(f"predict_proba is (sample, class) with at least two classes, got {tuple(p.shape)}")
    res = permutation_test_paired(prog_target, proba_ref[:, 1], proba_cmp[:, 1], PERM_METRICS, n_resamples, alternative, seed)
    return {"pvalue__roc_auc": res["roc_auc"].pvalue, "statistic__roc_auc": res["roc_auc"].statistic,
            "pvalue__ap": res["avg_precision"].pvalue, "statistic__ap": res["avg_precision"].statistic}
