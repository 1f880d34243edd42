"""CPU: the numpy twin of koaf_curve_points / koaf_range_metrics / koaf_confusion (tests/curves_twin.py) against fixture F22 (the
reference's own curves and values, written by tests/golden/make_golden_curves.py), and the host side that needs no device.
 * every curve array of every case is BIT-equal to the reference's: each value is one correctly rounded IEEE operation chain on
   integers, which is also why the GPU tests ask the kernel for equality;
 * best_f1_calib (a maximum of such chains) is equal, point value and per resample; ap_range is within 1e-10 absolute -- a sum of
   at most n <= 16384 terms in [0, 1] (n * 2^-53 <= 1.8e-12 per sum) and one division, the reference summing pairwise, the twin
   in the kernel's per-thread-run-then-tree order;
 * mc_bacc / f1score_calib host arithmetic on given counts; sample_weight, a bad recall_range and an unknown metric name raise."""
from pathlib import Path

import numpy as np
import pytest

import curves_twin as C
import metrics_twin as M

GOLD = Path(__file__).resolve().parent / "golden" / "f22_curves.npz"
CASES = ("a", "b", "c", "d", "f", "g", "k", "l", "m", "p", "q")
RANGES = ((0.0, 1.0), (0.2, 0.8), (0.75, 1.0))
TOL = 1e-10


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def case(F, c):
    R, seed, strat, pi0 = (int(v) for v in F[f"{c}:par"])
    return F[f"{c}:target"], F[f"{c}:proba"], R, seed, bool(strat), pi0 / 1e6


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_points(F, c, pts, dtype):
    """the slices the host takes of a parsed curve-points buffer against the reference's arrays, bit for bit"""
    T, K, last = pts["T"], pts["K"], pts["last_ind"]
    assert T == F[f"{c}:pr_thr"].shape[0] and K + 1 == F[f"{c}:roc_fpr"].shape[0] and last + 2 == F[f"{c}:prc_prec"].shape[0]
    assert same_bits(pts["fpr"], F[f"{c}:roc_fpr"]) and same_bits(pts["tpr"], F[f"{c}:roc_tpr"])
    assert same_bits(pts["roc_thr"].astype(dtype), F[f"{c}:roc_thr"])
    assert same_bits(pts["prec"][::-1], F[f"{c}:pr_prec"]) and same_bits(pts["rec"][::-1], F[f"{c}:pr_rec"])
    assert same_bits(pts["thr"][::-1].astype(dtype), F[f"{c}:pr_thr"])
    assert same_bits(pts["prec_cal"][last + 1::-1], F[f"{c}:prc_prec"]) and same_bits(pts["rec"][last + 1::-1], F[f"{c}:prc_rec"])
    assert same_bits(pts["thr"][last::-1].astype(dtype), F[f"{c}:prc_thr"])
    assert same_bits(pts["prec"][last + 1::-1], F[f"{c}:prn_prec"]) and same_bits(pts["rec"][last + 1::-1], F[f"{c}:prn_rec"])
    assert (pts["thr"].astype(dtype).astype(np.float64) == pts["thr"]).all(), "the thresholds are score values"


def test_fixture_is_what_the_issue_asks_for(F):
    assert [v.split()[0] for v in F["versions"]] == ["scikit-learn", "scipy", "numpy"]
    assert F["b:pr_prec"].shape[0] == 301 and F["b:prc_prec"].shape[0] == 270        # not truncated / cut at full recall
    assert F["f:pr_prec"].shape[0] == 2 and F["f:roc_fpr"].shape[0] == 2               # all scores equal
    assert F["k:target"].shape[0] == 257 and F["k:pr_thr"].shape[0] == 257             # no ties
    assert F["l:target"].shape[0] == 5000 and F["q:target"].shape[0] == 2
    assert F["p:prc_prec"].shape[0] == F["p:pr_prec"].shape[0] == 61                   # the lowest score is a positive
    assert F["m:prc_prec"].shape[0] == 10 and F["m:roc_fpr"].shape[0] == 4             # perfectly separated
    assert 0 < int(F["g:kept"]) < int(F["g:par"][0])
    assert 2 not in F["mc:true"] and 2 in F["mc:pred"]
    for c in CASES:
        assert list(F[f"{c}:keys"][-3:]) == ["roc_curve", "pr_curve", "pr_calib_curve"] and F[f"{c}:keys"][-4] == "b_accuracy"


@pytest.mark.parametrize("c", CASES)
def test_twin_curves_equal_the_reference_bit_for_bit(F, c):
    y, p, _, _, _, pi0 = case(F, c)
    check_points(F, c, C.curve_points(p[:, 1], y, 1, pi0), p.dtype)


@pytest.mark.parametrize("c", CASES)
def test_twin_range_values_against_the_reference(F, c):
    from oaprogressionmmf_amd.various import bootstrap_indices
    y, p, R, seed, strat, pi0 = case(F, c)
    idx = bootstrap_indices(y, R, seed, strat)
    keep = y[idx].sum(axis=1) != 0
    assert int(keep.sum()) == int(F[f"{c}:kept"])
    for k, rr in enumerate(RANGES):
        rows = C.range_rows(p[:, 1], y, idx, pi0, rr)
        assert np.isnan(rows[1:, 2:][~keep]).all(), "a resample without positives is NaN"
        assert abs(rows[0, 2] - F[f"{c}:apr"][k]) < TOL
        err = np.abs(rows[1:, 2][keep] - F[f"{c}:rs_apr"][k]).max()
        assert err < TOL, f"case {c}, range {rr}: {err}"
        assert rows[0, 3] == F[f"{c}:bf1"][0] and np.array_equal(rows[1:, 3][keep], F[f"{c}:rs_bf1"])
    assert C.range_rows(p[:, 1], y, None, None)[0, 3] == F[f"{c}:bf1"][1]               # pi0=None: not calibrated


@pytest.mark.parametrize("c", CASES)
def test_bootstrap_summaries_from_the_recorded_values(F, c):
    from oaprogressionmmf_amd.various import bootstrap_indices, summarize_bootstrap
    y, _, R, seed, strat, _ = case(F, c)
    idx = bootstrap_indices(y, R, seed, strat)
    n1 = y[idx].sum(axis=1)
    keep = n1 != 0
    for vals, point, want in [(F[f"{c}:rs_apr"][k], F[f"{c}:apr"][k], F[f"{c}:bs_apr"][k]) for k in range(3)] + \
                             [(F[f"{c}:rs_bf1"], F[f"{c}:bf1"][0], F[f"{c}:bs_bf1"])]:
        full = np.full(R, np.nan)
        full[keep] = vals
        assert np.array_equal(np.array(summarize_bootstrap(full, n1, y.shape[0] - n1, point)), want)


def test_confusion_twin_and_host_arithmetic(F):
    from oaprogressionmmf_amd.various import _metrics as V
    cm, bad = C.confusion(F["mc:true"], F["mc:pred"], 4)
    assert not bad and np.array_equal(cm, F["mc:cm"])
    assert V.macro_recall_from_counts(cm) == F["mc:bacc"]
    wide = np.zeros((32, 32), np.int64)
    wide[:4, :4] = cm
    assert V.macro_recall_from_counts(wide) == F["mc:bacc"], "classes absent from both vectors do not count"
    assert C.confusion([0, 5, 1], [1, 1, -1], 4)[1]
    for c in CASES:
        y, p, *_ = case(F, c)
        cm, _ = C.confusion(y, p[:, 1] > 0.5, 2)
        assert V.f1_from_counts(cm[0, 0], cm[0, 1], cm[1, 0], cm[1, 1], 0.12) == F[f"{c}:f1c"][0]
        assert V.f1_from_counts(cm[0, 0], cm[0, 1], cm[1, 0], cm[1, 1], None) == F[f"{c}:f1c"][1]
    assert V.f1_from_counts(np.int64(5), np.int64(0), np.int64(3), np.int64(0)) == 0.0   # nothing predicted positive: NaN counts 0


def test_argument_errors(F):
    from oaprogressionmmf_amd import various as V
    y, p = F["a:target"], F["a:proba"][:, 1]
    w = np.ones(37)
    for fn in (V.roc_curve, V.precision_recall_curve, V.precision_recall_curve_calib, V.average_precision_score_calib,
               V.avg_precision_at_recall_range):
        with pytest.raises(NotImplementedError, match="sample_weight"):
            fn(y, p, sample_weight=w)
    for bad in ((-0.1, 0.5), (0.6, 0.5), (0.2, 1.5)):
        with pytest.raises(ValueError, match="recall_range"):
            V.avg_precision_at_recall_range(y, p, recall_range=bad)
        with pytest.raises(ValueError, match="recall_range"):
            V.calc_bootstrap("avg_precision_at_recall_range", y, p, recall_range=bad)
    with pytest.raises(ValueError, match="Unknown metric"):
        V.calc_bootstrap("best_f1", y, p)
    with pytest.raises(ValueError, match="pos_label"):
        V.roc_curve(y, p, pos_label=2)
    with pytest.raises(ValueError, match="Expected binary target"):
        V.calc_bootstrap("best_f1_calib", np.arange(37) % 3, p)
