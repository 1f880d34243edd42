#!/usr/bin/env python3
"""Generate fixture F20 (tests/golden/f20_permtest.npz): the paired permutation test of two models' ROC-AUC / average precision,
as scipy.stats.permutation_test(permutation_type="samples") evaluates it around scikit-learn's roc_auc_score /
average_precision_score -- per swap-mask row, so that a device run over the SAME masks can be compared row by row.
Needs scikit-learn and scipy (written with scikit-learn 1.7.2, scipy 1.15.3); nothing else of this project or of the reference.

Cases (scores: sigmoid of a shared base logit plus each model's own noise; see case_inputs):
  a    n = 300, prevalence 0.12, fp64, continuous scores, R = 1000
  b    n = 300, fp32, logits quantised to 1/8 (few distinct values, ties across the two models), R = 1000
  c    n = 9, exact: all 512 assignments, row r swaps sample i iff bit i of r is set; p-values from scipy.stats.permutation_test
  d32, d33   n = 32 / 33, R = 64: the two sides of the mask word boundary
  e    n = 3000, fp32, logits quantised to 1/64, R = 200: 6000 union bins
Per case <c> the file holds
  <c>:y int64 [n], <c>:ref / <c>:cmp [n] (fp32 or fp64), <c>:masks uint32 [R, ceil(n / 32)] (sample i swapped in row r when bit
  i & 31 of word i >> 5 is set; drawn by default_rng(7).integers(0, 2, (R, n), uint8) unless exact), <c>:exact
  <c>:auc, <c>:ap [1 + R, 2] fp64   scikit-learn's metric of the (ref side, cmp side); row 0 is the unswapped sample
  <c>:U [1 + R, 2] int64            the Mann-Whitney sums 2 P N roc_auc of both sides, from an integer recount
  <c>:stat [2]                      the observed statistics metric(cmp) - metric(ref): roc_auc, avg_precision
  <c>:p [2, 3]                      p-values (roc_auc, avg_precision) x (less, greater, two-sided), scipy's arithmetic
The generator asserts, for every case and both metrics, that for every row | |null_r| - |obs| | is either below gamma / 4 (gamma =
|100 eps obs|, scipy's tie tolerance) or above 1e-9, and that the ROC-AUC rows of the first kind are exactly those whose integer
|U_cmp - U_ref| equals the observed one: the classification of a row then does not hang on last bits.

Usage:  python tests/golden/make_golden_permtest.py
"""
import sys
from pathlib import Path

import numpy as np
from scipy import stats
from sklearn.metrics import average_precision_score, roc_auc_score

HERE = Path(__file__).resolve().parent
MASK_SEED = 7
EPS100 = 100.0 * np.finfo(np.float64).eps


def case_inputs(name):
    """-> (y int64 [n], ref [n], cmp [n], R, exact)"""
    n, prev, dtype, quant, R, seed, exact = {
        "a": (300, 0.12, np.float64, None, 1000, 11, False),
        "b": (300, 0.12, np.float32, 8, 1000, 12, False),
        "c": (9, 0.4, np.float64, None, 512, 13, True),
        "d32": (32, 0.3, np.float32, None, 64, 14, False),
        "d33": (33, 0.3, np.float32, None, 64, 15, False),
        "e": (3000, 0.12, np.float32, 64, 200, 16, False),
    }[name]
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < prev).astype(np.int64)
    if y.sum() < 2:
        y[:2] = 1
    if y.sum() > n - 2:
        y[-2:] = 0
    base = rng.standard_normal(n) + 1.0 * y
    lg_ref = base + 0.8 * rng.standard_normal(n)
    small = n < 100                                  # (a clear gap at small n keeps |obs| and so gamma away from one ulp)
    lg_cmp = base + (0.5 if small else 0.7) * rng.standard_normal(n) + (0.3 if small else 0.05) * y
    if quant:
        lg_ref, lg_cmp = np.round(lg_ref * quant) / quant, np.round(lg_cmp * quant) / quant
    sig = lambda z: (1.0 / (1.0 + np.exp(-z))).astype(dtype)
    return y, sig(lg_ref), sig(lg_cmp), R, exact


def pack(bits):
    R, n = bits.shape
    W = (n + 31) // 32
    words = np.zeros((R, W), np.uint64)
    for i in range(n):
        words[:, i >> 5] |= bits[:, i].astype(np.uint64) << np.uint64(i & 31)
    return words.astype(np.uint32)


def mann_whitney_2x(y, s):
    """2 P N roc_auc as an integer: 2 #{pos > neg} + #{pos == neg}, compared in s's own dtype"""
    pos, neg = np.sort(s[y == 1]), np.sort(s[y == 0])
    below = np.searchsorted(neg, pos, side="left")
    upto = np.searchsorted(neg, pos, side="right")
    return int(2 * below.sum() + (upto - below).sum())


def pvalues(null, obs, exact):
    gamma = np.abs(EPS100 * obs)
    adj = 0 if exact else 1
    less = ((null <= obs + gamma).sum() + adj) / (null.shape[0] + adj)
    greater = ((null >= obs - gamma).sum() + adj) / (null.shape[0] + adj)
    return np.array([less, greater, min(1.0, 2.0 * min(less, greater))])


def run_case(name, out):
    y, ref, cmp_, R, exact = case_inputs(name)
    n = y.shape[0]
    assert ref.dtype == cmp_.dtype and 0 < y.sum() < n
    if exact:
        assert R == 2 ** n
        bits = ((np.arange(R)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.uint8)
    else:
        bits = np.random.default_rng(MASK_SEED).integers(0, 2, size=(R, n), dtype=np.uint8)
    swaps = np.concatenate([np.zeros((1, n), bool), bits.astype(bool)])
    auc, ap, U = np.empty((R + 1, 2)), np.empty((R + 1, 2)), np.empty((R + 1, 2), np.int64)
    for r, sw in enumerate(swaps):
        for k, s in enumerate((np.where(sw, cmp_, ref), np.where(sw, ref, cmp_))):
            auc[r, k], ap[r, k], U[r, k] = roc_auc_score(y, s), average_precision_score(y, s), mann_whitney_2x(y, s)
    P, N = int(y.sum()), int(n - y.sum())
    assert np.abs(U / (2.0 * P * N) - auc).max() < 1e-12, "the integer recount is not scikit-learn's ROC-AUC"
    p = np.empty((2, 3))
    stat = np.empty(2)
    for m, vals in enumerate((auc, ap)):
        d = vals[:, 1] - vals[:, 0]
        obs, null = d[0], d[1:]
        gamma = np.abs(EPS100 * obs)
        gap = np.abs(np.abs(null) - np.abs(obs))
        tie = gap < gamma / 4
        assert (tie | (gap > 1e-9)).all(), f"case {name}, metric {m}: a near-tie, change the seed: {np.sort(gap[~tie])[:3]}"
        if m == 0:
            D = U[:, 1] - U[:, 0]
            assert np.array_equal(tie, np.abs(D[1:]) == abs(D[0])), f"case {name}: ROC-AUC ties are not the integer ties"
        stat[m], p[m] = obs, pvalues(null, obs, exact)
        print(f"  case {name} metric {m}: obs {obs:+.6f} gamma {gamma:.2e} ties {int(tie.sum())} "
              f"smallest other gap {np.sort(gap[~tie])[:1]} p {p[m]}")
    if exact:                      # scipy itself: its p-values do not depend on the order in which it enumerates
        for m, fn in enumerate((roc_auc_score, average_precision_score)):
            def statistic(x0, x1, fn=fn):
                return fn(y, x1) - fn(y, x0)
            for k, alt in enumerate(("less", "greater", "two-sided")):
                res = stats.permutation_test(data=(ref, cmp_), permutation_type="samples", n_resamples=1000, alternative=alt,
                                             statistic=statistic)
                assert res.null_distribution.shape[0] == R and res.statistic == stat[m]
                assert res.pvalue == p[m, k], f"case {name}: scipy gives {res.pvalue}, the row count {p[m, k]}"
    out[f"{name}:y"], out[f"{name}:ref"], out[f"{name}:cmp"] = y, ref, cmp_
    out[f"{name}:masks"], out[f"{name}:exact"] = pack(bits), np.bool_(exact)
    out[f"{name}:auc"], out[f"{name}:ap"], out[f"{name}:U"] = auc, ap, U
    out[f"{name}:stat"], out[f"{name}:p"] = stat, p
    both = np.concatenate([ref, cmp_])
    print(f"  case {name}: n = {n}, R = {R}, {len(np.unique(both))} distinct union values, "
          f"{len(np.intersect1d(ref, cmp_))} values shared by the two models")


def main():
    if len(sys.argv) != 1:
        sys.exit(__doc__)
    out = {}
    for name in ("a", "b", "c", "d32", "d33", "e"):
        run_case(name, out)
    path = HERE / "f20_permtest.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
