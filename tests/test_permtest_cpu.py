"""CPU: the host side of various.permutation_test_paired / compare_predictions against fixture F20 (scikit-learn's metrics per swap
mask and scipy's p-values, written by tests/golden/make_golden_permtest.py), and the numpy twin of the two kernels
(tests/permtest_twin.py) against every fixture row.
 * swap_masks: the bit packing, the enumeration order of the exact test, scipy's exactness rule (2 ** n <= n_resamples) on both
   sides of it at n = 9 / 10 with 1000 resamples, the seeded draw (the fixture's masks are seed 7's);
 * the p-value arithmetic on the fixture's recorded statistics gives the recorded p-values exactly, for all three alternatives;
   case c's are scipy.stats.permutation_test's own;
 * the twin reproduces every row: the Mann-Whitney sums exactly, average precision within 1e-10 absolute -- the project's bound
   for a fixed-order fp64 sum of at most 16384 terms in [0, 1] (n * 2^-53 * a small constant < 1e-11; here 2n <= 16384 bins);
 * argument errors that need no device; the header declares the two entry points and the library exports them."""
from pathlib import Path

import numpy as np
import pytest

import permtest_twin as PT

GOLD = Path(__file__).resolve().parent / "golden" / "f20_permtest.npz"
CASES = ("a", "b", "c", "d32", "d33", "e")
ALTS = ("less", "greater", "two-sided")
TOL = 1e-10


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def test_swap_masks_packing_and_enumeration():
    from oaprogressionmmf_amd.various import swap_masks
    from oaprogressionmmf_amd.various._permtest import pack_masks
    bits = np.zeros((3, 70), np.uint8)
    bits[0, [0, 31]] = 1
    bits[1, [32, 63, 64]] = 1
    bits[2, 69] = 1
    m = pack_masks(bits)
    assert m.dtype == np.uint32 and m.shape == (3, 3)
    assert m.tolist() == [[0x80000001, 0, 0], [0, 0x80000001, 1], [0, 0, 1 << 5]]
    assert np.array_equal(PT.unpack_masks(m, 70), bits.astype(bool))
    masks, exact = swap_masks(9, 1000)
    assert exact and masks.shape == (512, 1) and masks.dtype == np.uint32
    assert np.array_equal(masks[:, 0], np.arange(512)), "row r swaps sample i iff bit i of r is set; row 0 is the identity"
    masks, exact = swap_masks(10, 1000)
    assert not exact and masks.shape == (1000, 1) and int(masks.max()) < 1 << 10
    assert swap_masks(10, 1024)[1] and swap_masks(10, 1024)[0].shape == (1024, 1)
    assert not swap_masks(100, 1000)[1]
    with pytest.raises(ValueError):
        swap_masks(0, 10)


@pytest.mark.parametrize("c", CASES)
def test_swap_masks_seeded_draw(F, c):
    from oaprogressionmmf_amd.various import swap_masks
    n, R = F[f"{c}:y"].shape[0], F[f"{c}:masks"].shape[0]
    masks, exact = swap_masks(n, 1000 if c == "c" else R, seed=7)
    assert exact == bool(F[f"{c}:exact"]) == (c == "c")
    assert masks.dtype == np.uint32 and np.array_equal(masks, F[f"{c}:masks"])
    if not exact:
        again, _ = swap_masks(n, R, seed=7)
        other, _ = swap_masks(n, R, seed=8)
        assert np.array_equal(again, masks) and not np.array_equal(other, masks)
        bits = np.random.default_rng(7).integers(0, 2, size=(R, n), dtype=np.uint8)
        assert np.array_equal(PT.unpack_masks(masks, n), bits.astype(bool))
        if n % 32:
            assert int(masks[:, -1].max()) < 1 << (n % 32), "no bit at or beyond n"


@pytest.mark.parametrize("c", CASES)
def test_pvalue_arithmetic_on_the_recorded_statistics(F, c):
    from oaprogressionmmf_amd.various._permtest import permutation_pvalues, results_from_rows
    exact = bool(F[f"{c}:exact"])
    auc, ap, U = F[f"{c}:auc"], F[f"{c}:ap"], F[f"{c}:U"]
    d = ap[:, 1] - ap[:, 0]
    got = permutation_pvalues(d[1:], d[0], exact, abs(100 * np.finfo(np.float64).eps * d[0]))
    assert [got[a] for a in ALTS] == F[f"{c}:p"][1].tolist()
    D = U[:, 1] - U[:, 0]
    got = permutation_pvalues(D[1:], D[0], exact, 0)
    assert [got[a] for a in ALTS] == F[f"{c}:p"][0].tolist(), "integer comparison of the Mann-Whitney sums"
    # the same through the table the device pass leaves
    y = F[f"{c}:y"]
    rows = np.zeros((U.shape[0], 8))
    rows[:, 0], rows[:, 1] = y.sum(), (y == 0).sum()
    rows[:, 2:4], rows[:, 4:6] = U, ap
    for k, a in enumerate(ALTS):
        res = results_from_rows(rows, exact, alternative=a)
        for m, name in enumerate(("roc_auc", "avg_precision")):
            r = res[name]
            assert r.pvalue == F[f"{c}:p"][m, k] and isinstance(r.pvalue, np.float64)
            assert abs(r.statistic - F[f"{c}:stat"][m]) < 1e-14 and r.null_distribution.shape == (U.shape[0] - 1,)
    if c == "c":
        assert results_from_rows(rows, exact)["roc_auc"].pvalue == 0.375 and U.shape[0] == 513


def test_pvalue_adjustment_and_clip():
    from oaprogressionmmf_amd.various._permtest import permutation_pvalues
    null = np.array([-2, -1, 0, 1, 2, 2])
    p = permutation_pvalues(null, 2, False, 0)
    assert (p["less"], p["greater"], p["two-sided"]) == (7 / 7, 3 / 7, 6 / 7)
    p = permutation_pvalues(null, 2, True, 0)
    assert (p["less"], p["greater"], p["two-sided"]) == (1.0, 2 / 6, 4 / 6)
    p = permutation_pvalues(null, 0, True, 0)
    assert p["two-sided"] == 1.0, "2 * 4 / 6 is clipped"
    p = permutation_pvalues(np.array([0.5 + 1e-16, 0.5, 0.6]), 0.5, True, 100 * np.finfo(np.float64).eps * 0.5)
    assert (p["less"], p["greater"]) == (2 / 3, 1.0), "values within gamma of the observed one count on both sides"


@pytest.mark.parametrize("c", CASES)
def test_twin_reproduces_every_row(F, c):
    y, a, b, masks = F[f"{c}:y"], F[f"{c}:ref"], F[f"{c}:cmp"], F[f"{c}:masks"]
    rows = PT.perm_rows(a, b, y, masks, True)
    assert rows.shape == (masks.shape[0] + 1, 8)
    assert (rows[:, 0] == y.sum()).all() and (rows[:, 1] == (y == 0).sum()).all() and (rows[:, 6:] == 0).all()
    assert np.array_equal(rows[:, 2:4], F[f"{c}:U"]), "Mann-Whitney sums: exact"
    err = np.abs(rows[:, 4:6] - F[f"{c}:ap"]).max()
    assert err < TOL, err
    assert np.abs(rows[:, 2:4] / (2 * rows[:, :1] * rows[:, 1:2]) - F[f"{c}:auc"]).max() < TOL
    if c == "b":
        r = PT.pair_ranks(a, b)
        assert len(np.unique(r)) < 100 and len(np.intersect1d(r[:300], r[300:])) > 10, "ties between the two models share a bin"


def test_argument_errors(F):
    """refused ahead of any device work"""
    from oaprogressionmmf_amd.various import compare_predictions, permutation_test_paired
    y, a, b = F["a:y"], F["a:ref"], F["a:cmp"]
    with pytest.raises(ValueError, match="Unknown metric"):
        permutation_test_paired(y, a, b, metrics=("roc_auc", "f1"))
    with pytest.raises(ValueError, match="Unknown alternative"):
        permutation_test_paired(y, a, b, alternative="two_sided")
    with pytest.raises(ValueError, match="at least two classes"):
        compare_predictions(y, a[:, None], b[:, None])


def test_exports():
    from oaprogressionmmf_amd import ops, various
    for name in ("swap_masks", "permutation_test_paired", "compare_predictions"):
        assert callable(getattr(various, name))
    assert callable(ops.pair_ranks) and callable(ops.perm_metrics)


def test_entry_points_are_declared_and_built():
    """koaf.h declares the two entry points, the binding derives their prototypes from it, the library exports them and is of the
    header's version; its argument checks refuse ahead of any launch"""
    import ctypes
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert protos["koaf_pair_ranks"] == (ctypes.c_int, [vp, i64, vp, i64, i32, i32, vp, i32, vp, vp, vp, vp])
    assert protos["koaf_perm_metrics"] == (ctypes.c_int, [vp, i32, vp, i32, i32, vp, vp, vp])
    handle = _lib.lib()
    for name in ("koaf_pair_ranks", "koaf_perm_metrics"):
        assert getattr(handle, name).argtypes == protos[name][1]
    d = _lib.defines()
    assert handle.koaf_version() == d["KOAF_VERSION"]
    assert handle.koaf_pair_ranks(None, 1, None, 1, 0, d["KOAF_METRICS_MAX_N"] // 2 + 1, None, 1, None, None, None, None) == d["KOAF_EINVAL"]
    assert b"koaf_pair_ranks: 1 <= n <= 8192" in handle.koaf_last_error()
    assert handle.koaf_perm_metrics(None, 0, None, 0, 1, None, None, None) == d["KOAF_EINVAL"]
    assert b"koaf_perm_metrics: 1 <= n <= 8192" in handle.koaf_last_error()
    assert handle.koaf_perm_metrics(None, 8, None, 0, 1, None, None, None) == d["KOAF_EINVAL"]
    assert b"packed, out and flag are required" in handle.koaf_last_error()
