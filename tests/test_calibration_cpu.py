"""CPU: the calibration feature's twin against fixture F25 (scikit-learn 1.7.2 and numpy, tests/golden/make_golden_calibration.py),
and everything about it that needs no device.
 * tests/calib_twin.py, which restates koaf_calib.hip in numpy and sums in the kernels' order, against the fixture: quantile
   edges BIT-equal to np.percentile; prob_true equal; brier and prob_pred within 1e-10 absolute (two sums of k <= 1031 terms in
   [0, 1], each off by at most k * 2^-53 in any order, and one division); log_loss within (2 m + 8) * 2^-53 * 36.05 (below);
   the Newton of the three modes reproduces the recorded parameters exactly (same code, same libm);
 * koaf.h declares the entry points and the caps, KOAF_VERSION is still 200, REST_SRCS lists koaf_calib.hip;
 * the refusals that need no device; Recalibrator's state_dict round trip; val_epoch's signature;
 * a sanity check of the twin's (intercept, slope) against scikit-learn's LogisticRegression(penalty=None, tol=1e-10,
   max_iter=1000): two references compared, not the code under test.  lbfgs stops on its own projected-gradient rule, which
   leaves the parameters open by up to 2.2e-8 on these cases (measured: 1031:ens; the others 2e-11 .. 1.8e-9); the bar is ten
   times the largest gap.  Skipped where scikit-learn is absent."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import calib_twin as C

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "f25_calibration.npz"
SIZES = (97, 257, 1031)
COLUMNS = ("p", "ens", "r2", "p01", "p32")
NBINS = 10
TOL = 1e-10
LBFGS_BAR = 2.2e-7          # ten times the largest gap measured between the twin's Newton and lbfgs on the fixture's cases


def logloss_tol(m):
    """log-loss terms lie in [0, -log 2^-52 = 36.05]; the device's log, the host's and scikit-learn's may each be off in the last
    place (2^-53 relative per term: m * 2^-53 * 36.05 over the sum, once per side), and two sums of m such terms in different
    orders differ by at most m * 2^-53 * 36.05 more -- (2 m + 8) * 2^-53 * 36.05 with the division and the clip's bound"""
    return (2 * m + 8) * 2.0 ** -53 * 36.05


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def fractions(nbins):
    return np.linspace(0, 1, nbins + 1) * 100 / 100


def edges_of(F, n, col, strategy):
    return np.linspace(0.0, 1.0, NBINS + 1) if strategy == "uniform" else F[f"{n}:{col}:edges"]


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


@pytest.mark.parametrize("col", COLUMNS)
@pytest.mark.parametrize("n", SIZES)
def test_twin_matches_scikit_learn_and_numpy(F, n, col):
    y, s = F[f"{n}:y"], F[f"{n}:{col}"]
    assert s.dtype == (np.float32 if col == "p32" else np.float64)
    assert same_bits(C.edges(s, fractions(NBINS)), F[f"{n}:{col}:edges"]), "quantile edges"
    for strategy in ("uniform", "quantile"):
        out, bins, _ = C.metrics_row(s, y, edges_of(F, n, col, strategy))
        used = bins[:, 0] != 0
        assert out[7] == used.sum() and bins[:, 0].sum() == n and bins[:, 1].sum() == y.sum()
        assert np.array_equal(bins[used, 1] / bins[used, 0], F[f"{n}:{col}:{strategy}:prob_true"])
        assert np.abs(bins[used, 2] / bins[used, 0] - F[f"{n}:{col}:{strategy}:prob_pred"]).max() <= TOL
        assert abs(out[2] - F[f"{n}:{col}:brier"]) <= TOL
        assert abs(out[3] - F[f"{n}:{col}:log_loss"]) <= logloss_tol(n)
        # ece / mce from the recorded curve: sum_b n_b |prob_true - prob_pred| / n and the largest gap
        gap = np.abs(F[f"{n}:{col}:{strategy}:prob_true"] - F[f"{n}:{col}:{strategy}:prob_pred"])
        assert abs(out[5] - (gap * bins[used, 0]).sum() / n) <= TOL and abs(out[6] - gap.max()) <= TOL
    if col == "p":
        assert (C.metrics_row(s, y, edges_of(F, n, col, "uniform"))[1][:, 0] > 0).all(), "all ten uniform bins are in use"
        assert (C.metrics_row(s, y, edges_of(F, n, col, "quantile"))[1][:, 0] > 0).all(), "all ten quantile bins are in use"


def test_ensemble_column_is_confined_and_flat(F):
    for n in SIZES:
        s = F[f"{n}:ens"]
        assert 1 / (1 + np.e) < s.min() and s.max() < np.e / (1 + np.e)
        assert F[f"{n}:ens:fit"][0, 1] > 1.5 * F[f"{n}:p:fit"][0, 1] > 1.5           # a far steeper calibration slope


@pytest.mark.parametrize("n", SIZES)
def test_twin_newton_reproduces_the_recorded_fits(F, n):
    y = F[f"{n}:y"]
    for col in COLUMNS:
        x = C.x_of(F[f"{n}:{col}"])
        for k, mode in enumerate(C.MODES):
            got, want = C.fit_row(x, y, mode, tol=1e-13, max_iter=100), F[f"{n}:{col}:fit"][k]
            assert want[5] == 0 and want[2] <= 10 and want[3] <= 1e-13, (col, mode, want)
            assert np.allclose(got[:2], want[:2], rtol=0, atol=1e-9) and got[5] == 0
            ga, gb, _ = C.gradient(x, y, want[0], want[1])
            free = [abs(ga) if mode != "temperature" else 0.0, abs(gb) if mode != "intercept" else 0.0]
            assert max(free) / n <= 1e-13 + 4 * 2.0 ** -52 * max(1.0, np.abs(x).max())
    # the stratified resamples the GPU tests use converge too, none failing
    from oaprogressionmmf_amd.various._metrics import bootstrap_indices
    idx = bootstrap_indices(y, 64 if n < 1000 else 8, 0, True)
    rows = C.fit_rows(C.x_of(F[f"{n}:p"]), y, "slope_intercept", idx, with_identity=False)
    assert (rows[:, 5] == 0).all() and rows[:, 2].max() <= 16


def test_twin_statuses(F):
    x, y = F["sep:logit"], F["sep:y"]
    want = F["sep:fit"]
    for k, mode in enumerate(C.MODES):
        got = C.fit_row(x, y, mode, tol=1e-13, max_iter=100)
        assert np.array_equal(got, want[k], equal_nan=True)
    assert want[0, 5] == 2 and np.isnan(want[0, :2]).all() and 0 < want[0, 2] < 50, "separable: found while walking, not at the start"
    assert want[1, 5] == 0 and want[2, 5] == 0, "the slope alone and the intercept alone have an optimum"
    one = C.fit_row(x, np.ones_like(y), "slope_intercept")
    assert one[5] == 3 and np.isnan(one[:2]).all() and one[6] == len(y) and one[7] == 0
    capped = C.fit_row(C.x_of(F["97:p"]), F["97:y"], "slope_intercept", tol=0.0, max_iter=2)
    assert capped[5] == 1 and capped[2] == 2 and np.isfinite(capped[:2]).all()


def test_twin_against_lbfgs(F):
    lm = pytest.importorskip("sklearn.linear_model")
    worst = 0.0
    for n in SIZES:
        for col in COLUMNS:
            x, f = C.x_of(F[f"{n}:{col}"]), F[f"{n}:{col}:fit"][0]
            lr = lm.LogisticRegression(penalty=None, tol=1e-10, max_iter=1000).fit(x[:, None], F[f"{n}:y"])
            worst = max(worst, abs(lr.intercept_[0] - f[0]), abs(lr.coef_[0, 0] - f[1]))
    print(f"largest |twin - lbfgs| over the fixture's cases: {worst:.3e}")
    assert worst <= LBFGS_BAR


def test_header_and_makefile():
    from oaprogressionmmf_amd import _lib
    protos, defs = _lib.parse_header(), _lib.defines()
    for name, nargs in (("koaf_calib_edges", 9), ("koaf_calib_metrics", 19), ("koaf_recalib_fit", 19), ("koaf_recalib_apply", 13)):
        assert name in protos and len(protos[name][1]) == nargs, name
    assert defs["KOAF_VERSION"] == 200
    assert defs["KOAF_CALIB_MAX_BINS"] == 64 and defs["KOAF_CALIB_MAX_THR"] == 128 and defs["KOAF_RECALIB_MAX_ITER"] >= 50
    mk = (ROOT / "oaprogressionmmf_amd" / "csrc" / "Makefile").read_text()
    rest = re.search(r"^REST_SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "koaf_calib.hip" in rest and (ROOT / "oaprogressionmmf_amd" / "csrc" / "koaf_calib.hip").exists()
    header = (ROOT / "include" / "koaf.h").read_text()
    assert "koaf_calib.hip" in header and "bit 3" in header[header.index("koaf_calib.hip"):]


def test_flag_family():
    from oaprogressionmmf_amd import ops
    assert set(ops.METRICS_FLAG_TEXT) == {1, 2, 4}, "the metric kernels' table stays as it is"
    assert set(ops.CALIB_FLAG_TEXT) == {1, 2, 4, 8} and all(ops.CALIB_FLAG_TEXT[b] == ops.METRICS_FLAG_TEXT[b] for b in (1, 2, 4))
    ops.calib_raise(0)
    ops.calib_raise(16)
    with pytest.raises(ValueError, match="did not converge"):
        ops.calib_raise(8)
    with pytest.raises(ValueError, match="NaN or infinity.*did not converge"):
        ops.calib_raise(9)


def test_refusals_that_need_no_device(F):
    from oaprogressionmmf_amd import various as V
    y, p = F["97:y"], F["97:p"]
    proba = np.stack([1 - p, p], axis=1)
    with pytest.raises(ValueError, match="Strategy must be either"):
        V.calibration_curve(y, p, strategy="kmeans")
    with pytest.raises(ValueError, match="Strategy must be either"):
        V.calc_calibration(y, proba, "prog_kl_72", strategy="kmeans")
    for bad in (0, -1, 65, 2.5):
        with pytest.raises(ValueError, match="n_bins"):
            V.expected_calibration_error(y, p, n_bins=bad)
        with pytest.raises(ValueError, match="n_bins"):
            V.calc_calibration(y, proba, "prog_kl_72", n_bins=bad)
    for bad in ([0.0, 0.5], [0.5, 1.0], [-0.1], [np.nan]):
        with pytest.raises(ValueError, match=r"lies in \(0, 1\)"):
            V.decision_curve(y, p, bad)
        with pytest.raises(ValueError, match=r"lies in \(0, 1\)"):
            V.calc_calibration(y, proba, "prog_kl_72", thresholds=bad)
    with pytest.raises(ValueError, match="at most 128 thresholds"):
        V.decision_curve(y, p, np.linspace(0.01, 0.99, 129))
    with pytest.raises(NotImplementedError, match="sample_weight"):
        V.brier_score_loss(y, p, sample_weight=np.ones_like(p))
    with pytest.raises(NotImplementedError, match="sample_weight"):
        V.log_loss(y, p, sample_weight=np.ones_like(p))
    with pytest.raises(ValueError, match="Unknown target"):
        V.calc_calibration(y, proba, "kl")
    y2 = y.copy()
    y2[3] = 2
    for call in (lambda: V.calc_calibration(y2, proba, "prog_kl_72"), lambda: V.brier_score_loss(y2, p),
                 lambda: V.calibration_slope_intercept(y2, p), lambda: V.Recalibrator().fit(y2, p)):
        with pytest.raises(ValueError, match="Expected binary target"):
            call()
    with pytest.raises(ValueError, match="mode is one of"):
        V.Recalibrator("isotonic")
    with pytest.raises(ValueError, match="before fit"):
        V.Recalibrator().transform(p)


def test_recalibrator_state_dict_round_trip():
    from oaprogressionmmf_amd.various import Recalibrator
    r = Recalibrator("temperature")
    assert r.state_dict() == {"mode": "temperature", "kind": None, "a": None, "b": None}
    r.load_state_dict({"mode": "slope_intercept", "kind": "proba", "a": -1.5, "b": 2.25})
    state = r.state_dict()
    assert state == {"mode": "slope_intercept", "kind": "proba", "a": -1.5, "b": 2.25}
    assert all(type(state[k]) is float for k in "ab") and r.temperature == 1 / 2.25
    again = Recalibrator().load_state_dict(state)
    assert again.state_dict() == state
    with pytest.raises(ValueError, match="mode is one of"):
        Recalibrator().load_state_dict({"mode": "platt", "kind": None, "a": 0.0, "b": 1.0})


def test_val_epoch_signature():
    from oaprogressionmmf_amd.run import val_epoch
    par = inspect.signature(val_epoch).parameters
    assert par["calibration"].default is None and par["calibration"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(par)[-2:] == ["kws_metrics", "calibration"]
