"""GPU: koaf_score_ranks / koaf_curve_metrics / koaf_point_metrics (ops.score_ranks, ops.curve_metrics, ops.point_metrics)
against fixture F18 -- the reference's own per-resample values -- and, where the fixture has no case, against the numpy twin that
the CPU tests pin to the same fixture (tests/metrics_twin.py).
 * ranks equal the counting definition exactly, read through a stride (a probability column in place) and contiguously, fp32 and
   fp64 (case d: pairs 1e-12 apart that fp32 would tie);
 * every per-resample value of cases a-d, f, g is within 1e-10 absolute of the fixture; n_pos / n_neg are exact; two launches
   give identical bits.  The bound is derived, not measured: each metric is a sum of at most n <= 16384 terms in [0, 1] in fp64,
   so the error is about n * 2^-53 * a small constant < 1e-11, and the reference's own rounding is of the same order;
 * the 400 Youden cutoffs of case e equal the reference's exactly (the drop_intermediate tie rule);
 * the kernels with the 16384-bin histogram (n > 4096), at n = 5000 and at the cap n = 16384, and an index matrix narrower than
   the sample, against the twin, same bound;
 * a non-finite score, a non-binary label and a wild index raise ValueError; n above the cap is the library's error status."""
from pathlib import Path

import numpy as np
import pytest
import torch

import metrics_twin as T

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "f18_metrics.npz"
TOL = 1e-10


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def case(F, c):
    R, seed, strat, pi0 = (int(v) for v in F[f"{c}:par"])
    return F[f"{c}:target"], F[f"{c}:proba"], R, seed, bool(strat), pi0 / 1e6


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _labels(y, dev):
    return _dev(np.asarray(y, np.int32), dev)


@pytest.mark.parametrize("c", ("a", "b", "c", "d", "f"))
def test_ranks_equal_the_counting_definition(F, dev, c):
    from oaprogressionmmf_amd import ops
    y, p, *_ = case(F, c)
    pd = _dev(p, dev)
    assert pd.dtype == (torch.float64 if c == "d" else torch.float32)
    for col in (0, 1):
        want = T.ranks(p[:, col])
        strided = ops.score_ranks(pd[:, col])                          # stride 2: the column in place
        assert pd[:, col].stride(0) == 2 and strided.dtype == torch.int32
        assert np.array_equal(strided.cpu().numpy(), want)
        rank, packed = ops.score_ranks(pd[:, col].contiguous(), _labels(y, dev), pos_label=col)
        assert np.array_equal(rank.cpu().numpy(), want)
        assert np.array_equal(packed.cpu().numpy(), (want << 1) | (y == col))
    if c == "d":
        assert len(np.unique(want)) == 200
        assert len(np.unique(ops.score_ranks(pd[:, 1].float()).cpu().numpy())) <= 100


@pytest.mark.parametrize("c", ("a", "b", "c", "d", "f", "g"))
def test_per_resample_values_against_the_reference(F, dev, c):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.various import bootstrap_indices
    y, p, R, seed, strat, pi0 = case(F, c)
    idx = bootstrap_indices(y, R, seed, strat)
    pd, yd, idxd = _dev(p, dev), _labels(y, dev), _dev(idx, dev)
    flag = ops.metrics_flag(dev)
    rows = {}
    for col in (1, 0):
        _, packed = ops.score_ranks(pd[:, col], yd, pos_label=col, flag=flag)
        out = ops.curve_metrics(packed, idxd, True, pi0, flag=flag)
        again = ops.curve_metrics(packed, idxd, True, pi0, flag=flag)
        assert out.shape == (R + 1, 8)
        assert torch.equal(out.view(torch.int64), again.view(torch.int64)), "two launches, different bits"
        rows[col] = out.cpu().numpy()
    assert int(flag.item()) == 0
    n1 = np.concatenate([[y.sum()], y[idx].sum(axis=1)])
    assert np.array_equal(rows[1][:, 0], n1) and np.array_equal(rows[1][:, 1], y.shape[0] - n1), "n_pos / n_neg"
    assert np.array_equal(rows[0][:, 0], y.shape[0] - n1) and np.array_equal(rows[0][:, 1], n1)
    keep = n1[1:] != 0
    assert int(keep.sum()) == int(F[f"{c}:kept"])
    assert np.isnan(rows[1][1:, 2:5][~keep]).all() and np.isnan(rows[0][1:, 2:5][~keep]).all(), "a resample without positives is NaN"
    got = np.array([rows[1][1:, 2][keep], rows[1][1:, 3][keep], rows[1][1:, 4][keep], rows[0][1:, 3][keep]])
    err = np.abs(got - F[f"{c}:vals"]).max(axis=1)
    print(f"case {c}: max |device - reference| per metric {err}")
    assert (err < TOL).all()
    point = np.array([rows[1][0, 2], rows[1][0, 3], rows[1][0, 4], rows[0][0, 3]])
    assert np.abs(point - F[f"{c}:plain_raw"][1:5]).max() < TOL
    # the identity row alone (no index matrix) is the same launch with R = 0
    _, packed = ops.score_ranks(pd[:, 1], yd, pos_label=1, flag=flag)
    alone = ops.curve_metrics(packed, pi0=pi0, flag=flag).cpu().numpy()
    assert alone.shape == (1, 8) and np.array_equal(alone[0], rows[1][0])


def test_point_quantities_against_the_reference(F, dev):
    """cutoff and both confusion matrices of cases a-d, f, g (the fixture's youdens_index / b_accuracy follow from them)"""
    from oaprogressionmmf_amd import ops
    for c in ("a", "b", "c", "d", "f", "g"):
        y, p, *_ = case(F, c)
        pd, yd = _dev(p, dev), _labels(y, dev)
        _, packed = ops.score_ranks(pd[:, 1], yd)
        out = ops.point_metrics(pd[:, 1], packed).cpu().numpy()
        cutoff, c5, cc = T.point(p[:, 1], y)
        assert out[0] == F[f"{c}:plain_raw"][5] == float(cutoff), f"case {c}: cutoff"      # (a score value: exact in fp64)
        assert out[1:5].tolist() == c5 and out[5:9].tolist() == cc, f"case {c}: confusion counts"
        tn, fp, fn, tp = out[5:9]
        assert abs(tp / (tp + fn) + tn / (tn + fp) - 1.0 - F[f"{c}:plain_raw"][6]) < TOL
        tn, fp, fn, tp = out[1:5]
        assert abs((tn / (tn + fp) + tp / (tp + fn)) / 2 - F[f"{c}:plain_raw"][7]) < TOL
    assert np.isinf(F["f:cutoff"])


def test_youden_cutoffs_of_case_e(F, dev):
    from oaprogressionmmf_amd import ops
    off = F["e:off"]
    s, y = _dev(F["e:score"], dev), _labels(F["e:target"], dev)
    flag = ops.metrics_flag(dev)
    out = torch.empty((400, 9), dtype=torch.float64, device=dev)
    for k, (a, b) in enumerate(zip(off[:-1].tolist(), off[1:].tolist())):
        _, packed = ops.score_ranks(s[a:b], y[a:b], flag=flag)
        ops.point_metrics(s[a:b], packed, out=out[k], flag=flag)
    got = out[:, 0].cpu().numpy().astype(np.float32)
    assert int(flag.item()) == 0
    wrong = np.flatnonzero(got != F["e:cutoff"])
    assert wrong.size == 0, f"{wrong.size} of 400 cutoffs differ, first at set {wrong[:5]}"


@pytest.mark.parametrize("n,m,R", [(5000, 5000, 3), (16384, 16384, 2), (4096, 4096, 2), (4097, 1000, 3), (300, 77, 4)])
def test_large_histograms_and_narrow_index_matrices_against_the_twin(dev, n, m, R):
    """n > 4096 takes the 16384-bin kernels (4096 / 4097: both sides of that switch); m != n: an index matrix of its own width"""
    from oaprogressionmmf_amd import ops
    rng = np.random.RandomState(n + m)
    y = (rng.rand(n) < 0.2).astype(np.int64)
    s = (np.round((rng.randn(n) + 0.7 * y) * 64) / 64).astype(np.float32)           # tie groups and singletons
    s = (1.0 / (1.0 + np.exp(-s))).astype(np.float32)
    idx = rng.randint(0, n, size=(R, m)).astype(np.int32)
    sd, yd = _dev(s, dev), _labels(y, dev)
    rank, packed = ops.score_ranks(sd, yd)
    assert np.array_equal(rank.cpu().numpy(), T.ranks(s))
    got = ops.curve_metrics(packed, _dev(idx, dev), True, 0.12).cpu().numpy()
    want = T.curve_rows(s, y, 1, idx, 0.12)
    assert np.array_equal(got[:, :2], want[:, :2])
    err = np.abs(got[:, 2:5] - want[:, 2:5]).max()
    print(f"n = {n}, m = {m}: max |device - twin| {err}, bit-equal {np.array_equal(got[:, 2:5], want[:, 2:5])}")
    assert err < TOL and (got[:, 5:] == 0).all()
    out = ops.point_metrics(sd, packed).cpu().numpy()
    cutoff, c5, cc = T.point(s, y)
    assert np.float32(out[0]) == cutoff and out[1:5].tolist() == c5 and out[5:9].tolist() == cc


def test_flag_word_raises(F, dev):
    from oaprogressionmmf_amd import ops
    y, p, *_ = case(F, "a")
    yd = _labels(y, dev)
    for bad in (np.nan, np.inf, -np.inf):
        q = p[:, 1].copy()
        q[11] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            ops.score_ranks(_dev(q, dev))
        flag = ops.metrics_flag(dev)
        ops.score_ranks(_dev(q.astype(np.float64), dev), yd, flag=flag)      # a caller's flag word: no sync, no raise here
        assert int(flag.item()) == 1
    y3 = y.astype(np.int32).copy()
    y3[5] = 2
    with pytest.raises(ValueError, match="label other than 0 / 1"):
        ops.score_ranks(_dev(p[:, 1], dev), _dev(y3, dev))
    _, packed = ops.score_ranks(_dev(p[:, 1], dev), yd)
    idx = np.tile(np.arange(37, dtype=np.int32), (2, 1))
    idx[1, 3], idx[1, 9] = 37, -1                                            # not followed: flagged and left out of the counts
    flag = ops.metrics_flag(dev)
    out = ops.curve_metrics(packed, _dev(idx, dev), False, flag=flag).cpu().numpy()
    assert int(flag.item()) == 4 and out[0, 0] + out[0, 1] == 37 and out[1, 0] + out[1, 1] == 35
    with pytest.raises(ValueError, match=r"outside \[0, n\)"):
        ops.curve_metrics(packed, _dev(idx, dev), False)


def test_cap_and_argument_checks(dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    n = ops.METRICS_MAX_N + 1
    s = torch.rand(n, device=dev)
    with pytest.raises(KoafError, match="koaf_score_ranks: 1 <= n <= 16384"):
        ops.score_ranks(s)
    with pytest.raises(KoafError, match="koaf_curve_metrics: 1 <= n <= 16384"):
        ops.curve_metrics(torch.zeros(n, dtype=torch.int32, device=dev))
    with pytest.raises(KoafError, match="koaf_point_metrics: 1 <= n <= 16384"):
        ops.point_metrics(s, torch.zeros(n, dtype=torch.int32, device=dev))
    ok = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(KoafError, match="1 <= m <= 16384"):
        ops.curve_metrics(ok, torch.zeros((1, n), dtype=torch.int32, device=dev))
    with pytest.raises(KoafError, match="0 < pi0 < 1"):
        ops.curve_metrics(ok, pi0=1.0)
    with pytest.raises(KoafError, match="fp32 / fp64"):
        ops.score_ranks(s[:8].half())
    with pytest.raises(KoafError, match="int32"):
        ops.score_ranks(s[:8], torch.zeros(8, dtype=torch.int64, device=dev))
    with pytest.raises(KoafError):
        ops.score_ranks(torch.rand(8))                                       # a host tensor: no CPU fallback
