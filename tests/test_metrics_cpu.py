"""CPU: the host side of various.calc_metrics_v2 / calc_bootstrap against fixture F18 (the reference's own outputs, written by
tests/golden/make_golden_metrics.py), and the numpy twin of the kernels' arithmetic (tests/metrics_twin.py) against every case.
 * bootstrap_indices draws the index sets the reference drew (its kept resamples, in order), and leaves numpy's global
   generator alone;
 * summarize_bootstrap on the fixture's per-resample values gives the reference's (value, std_err, ci_l, ci_h): the 2nd / 97th
   percentile quirk, ddof, the skipped resamples of case g, the ValueError of a kept resample without negatives;
 * the twin reproduces every per-resample value, every unrounded output and all 400 Youden cutoffs of case e.  Its bound is the
   GPU tests' bound, 1e-10 absolute: each metric is a sum of at most n <= 16384 terms in [0, 1] in fp64 (n * 2^-53 * a small
   constant < 1e-11), and the reference's own rounding is of the same order;
 * the argument handling that needs no device: single-class return, unknown target, with_curves, unknown metric name."""
from pathlib import Path

import numpy as np
import pytest

import metrics_twin as T

GOLD = Path(__file__).resolve().parent / "golden" / "f18_metrics.npz"
CASES = ("a", "b", "c", "d", "f", "g")
KEYS_PLAIN = ("prevalence", "roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv", "cutoff", "youdens_index", "b_accuracy")
TOL = 1e-10


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def case(F, c):
    R, seed, strat, pi0 = (int(v) for v in F[f"{c}:par"])
    return F[f"{c}:target"], F[f"{c}:proba"], R, seed, bool(strat), pi0 / 1e6


@pytest.mark.parametrize("c", CASES)
def test_bootstrap_indices_replay_the_reference(F, c):
    from oaprogressionmmf_amd.various import bootstrap_indices
    y, _, R, seed, strat, _ = case(F, c)
    np.random.seed(4242)
    state = np.random.get_state()[1].copy()
    idx = bootstrap_indices(y, R, seed, strat)
    assert (np.random.get_state()[1] == state).all(), "the global generator was touched"
    assert idx.dtype == np.int32 and idx.shape == (R, y.shape[0]) and idx.min() >= 0 and idx.max() < y.shape[0]
    keep = y[idx].sum(axis=1) != 0
    assert int(keep.sum()) == int(F[f"{c}:kept"])
    assert np.array_equal(idx[keep], F[f"{c}:idx_kept"])
    if c == "g":
        assert 0 < int((~keep).sum()) < R


@pytest.mark.parametrize("c", CASES)
def test_twin_reproduces_the_reference(F, c):
    from oaprogressionmmf_amd.various import bootstrap_indices
    y, p, R, seed, strat, pi0 = case(F, c)
    idx = bootstrap_indices(y, R, seed, strat)
    r1, r0 = T.curve_rows(p[:, 1], y, 1, idx, pi0), T.curve_rows(p[:, 0], y, 0, idx, pi0)
    assert np.array_equal(r1[:, 0], y[np.vstack([np.arange(y.shape[0]), idx])].sum(axis=1))       # n_pos exact
    assert np.array_equal(r1[:, 0], r0[:, 1]) and np.array_equal(r1[:, 1], r0[:, 0])
    keep = r1[1:, 0] != 0
    vals = np.array([r1[1:, 2][keep], r1[1:, 3][keep], r1[1:, 4][keep], r0[1:, 3][keep]])
    assert vals.shape == F[f"{c}:vals"].shape
    assert np.abs(vals - F[f"{c}:vals"]).max() < TOL
    plain = T.calc_metrics_plain(y, p, pi0)
    want = F[f"{c}:plain_raw"]
    assert plain[5] == want[5] and np.asarray(plain[5]).dtype == p.dtype, "cutoff"
    for k in (0, 1, 2, 3, 4, 6, 7):
        assert abs(float(plain[k]) - want[k]) < TOL, KEYS_PLAIN[k]


def test_twin_ranks_in_the_scores_precision(F):
    """case d: pairs 1e-12 apart are distinct ranks in fp64 and tie in fp32"""
    p = F["d:proba"][:, 1]
    assert len(np.unique(T.ranks(p))) == 200 and len(np.unique(T.ranks(p.astype(np.float32)))) <= 100


def test_twin_youden_cutoffs_of_case_e(F):
    off = F["e:off"]
    got = np.array([T.point(F["e:score"][a:b], F["e:target"][a:b])[0] for a, b in zip(off[:-1], off[1:])], np.float32)
    assert np.array_equal(got, F["e:cutoff"])
    assert np.isinf(got).any() and not np.isinf(got).all()


@pytest.mark.parametrize("c", CASES)
def test_summary_of_the_recorded_resamples(F, c):
    """the host summary alone: fed the reference's per-resample values it returns the reference's tuples (rounded: exactly)"""
    from oaprogressionmmf_amd.various import bootstrap_indices, summarize_bootstrap
    y, p, R, seed, strat, _ = case(F, c)
    idx = bootstrap_indices(y, R, seed, strat)
    n1 = y[idx].sum(axis=1)
    n0 = y.shape[0] - n1
    full = np.full((4, R), -7.0)                     # values of skipped resamples must never be looked at
    full[:, n1 != 0] = F[f"{c}:vals"]
    for k in range(4):
        got = summarize_bootstrap(full[k], n1, n0, F[f"{c}:plain_raw"][1 + k])
        assert all(isinstance(v, np.float64) for v in got)
        assert np.abs(np.array(got) - F[f"{c}:bs_raw"][1 + k]).max() < 1e-15
        assert np.array_equal(np.round(got, 3), F[f"{c}:bs"][1 + k])


def test_summary_percentiles_ddof_and_one_class():
    from oaprogressionmmf_amd.various import summarize_bootstrap
    v = np.arange(101, dtype=np.float64)
    ones = np.ones(101)
    val, se, lo, hi = summarize_bootstrap(v, ones, ones, 0.25)
    assert (val, lo, hi) == (0.25, 2.0, 97.0), "(100 - 95) // 2 = 2 and 95 + 2 = 97: not the 2.5th / 97.5th percentiles"
    assert se == np.std(v) and summarize_bootstrap(v, ones, ones, 0.0, ddof=1)[1] == np.std(v, ddof=1)
    _, _, lo, hi = summarize_bootstrap(v, ones, ones, 0.0, alpha=90.)
    assert (lo, hi) == (5.0, 95.0)
    skip = ones.copy()
    skip[50:] = 0                                                   # no positives: dropped
    assert summarize_bootstrap(v, skip, ones, 0.0)[3] == np.percentile(v[:50], 97)
    none0 = ones.copy()
    none0[3] = 0
    with pytest.raises(ValueError, match="Only one class"):
        summarize_bootstrap(v, ones, none0, 0.0)
    none0[3], skip[3] = 0, 0                                        # ... unless that resample is skipped anyway
    summarize_bootstrap(v, skip, none0, 0.0)


def test_single_class_return(F):
    from oaprogressionmmf_amd.various import calc_metrics_v2
    for bootstrap in (False, True):
        out = calc_metrics_v2(F["h:target"], F["h:proba"], "prog_kl_72", bootstrap=bootstrap)
        assert list(out) == [str(k) for k in F["h:keys"]]
        assert np.array_equal(np.array([float(v) for v in out.values()]), F["h:values"], equal_nan=True)
        assert out["sample_size"] == 12 and isinstance(out["sample_size"], int)
        assert out["num_pos"] == 12 and out["num_neg"] == 0 and isinstance(out["num_pos"], np.integer)
    # the reference looks at the classes before it looks at the target's name
    assert list(calc_metrics_v2(F["h:target"], F["h:proba"], "no_such_target")) == [str(k) for k in F["h:keys"]]


def test_argument_errors(F):
    from oaprogressionmmf_amd.various import calc_bootstrap, calc_metrics_v2
    y, p = F["a:target"], F["a:proba"]
    with pytest.raises(ValueError, match="Unknown target: prog_kl_13"):
        calc_metrics_v2(y, p, "prog_kl_13")
    with pytest.raises(NotImplementedError, match="curve"):
        calc_metrics_v2(y, p, "prog_kl_72", with_curves=True)
    with pytest.raises(ValueError, match="Unknown metric"):
        calc_bootstrap("f1", y, p[:, 1])
    with pytest.raises(ValueError, match="Expected binary target"):
        calc_bootstrap("roc_auc", np.arange(37) % 3, p[:, 1])


def test_exports():
    from oaprogressionmmf_amd import ops, run, various
    assert callable(run.val_epoch) and "val_epoch" in run.__all__
    for name in ("calc_metrics_v2", "calc_bootstrap", "bootstrap_indices"):
        assert callable(getattr(various, name))
    assert ops.METRICS_MAX_N == 16384


def test_metric_entry_points_are_declared_and_built():
    """koaf.h declares the three entry points, the binding derives their prototypes from it and the library exports them"""
    import ctypes
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    assert protos["koaf_score_ranks"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
    assert protos["koaf_curve_metrics"][1][6] is ctypes.c_double and len(protos["koaf_curve_metrics"][1]) == 10
    assert protos["koaf_point_metrics"][1][5] is ctypes.c_double and len(protos["koaf_point_metrics"][1]) == 9
    handle = _lib.lib()
    for name in ("koaf_score_ranks", "koaf_curve_metrics", "koaf_point_metrics"):
        assert getattr(handle, name).argtypes == protos[name][1]
    # refusals ahead of any launch: the library's own argument checks need no device
    assert handle.koaf_score_ranks(None, 0, 1, _lib.defines()["KOAF_METRICS_MAX_N"] + 1, None, 1, None, None, None, None) == _lib.defines()["KOAF_EINVAL"]
    assert b"1 <= n <= 16384" in handle.koaf_last_error()
