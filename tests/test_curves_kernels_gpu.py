"""GPU: koaf_curve_points / koaf_range_metrics / koaf_confusion (ops.curve_points, ops.range_metrics, ops.confusion) against
fixture F22 -- the reference's own curves and per-resample values -- and against the numpy twin the CPU tests pin to the same
fixture (tests/curves_twin.py).
 * curve points: T, K, last_ind and every array BIT-equal to the fixture, for fp32 and fp64 scores, read through a stride of 2 (a
   probability column in place) and contiguously; bit-equal to the twin on both sides of the histogram switch (n = 4096 / 4097),
   at n = 5000 and at the cap n = 16384, and where tie groups and the ROC keep-rule cross thread-run boundaries (n = 257 without
   ties: two bins per run; n = 2503 with ties); two launches leave identical buffers.  Equality is the bar because every value is
   one correctly rounded IEEE operation chain on integers;
 * range metrics: best_f1_calib per resample EQUAL to the fixture; ap_range per resample within 1e-10 absolute of it -- derived,
   not measured: a sum of at most n <= 16384 terms in [0, 1] is off by at most n * 2^-53 <= 1.8e-12, there are two such sums
   (the reference's pairwise one and the kernel's) and one division; all six columns equal to the twin (NaN where it is NaN), which sums
   in the kernel's order; rows without positives are NaN (case g's skipped resamples); two launches give identical bits;
 * confusion: exact counts over several blocks; a label outside [0, K) is skipped and flagged;
 * the flag bits and the cap (n = 16385 is the library's error status) for all three."""
import numpy as np
import pytest
import torch

import curves_twin as C
from test_curves_cpu import CASES, GOLD, RANGES, TOL, case, check_points, same_bits

pytestmark = pytest.mark.gpu
FIELDS = ("thr", "rec", "prec", "prec_cal", "fpr", "tpr", "roc_thr")


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _labels(y, dev):
    return _dev(np.asarray(y, np.int32), dev)


def _same(a, b):
    """equal values, NaN where NaN (a NaN's sign and payload are the one thing the host's and the device's division differ in)"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _points(ops, s, yd, pi0, pos_label=1, **kw):
    """ranks + curve points into a zeroed buffer, twice -> the parsed host views; the two buffers hold the same bits"""
    flag = ops.metrics_flag(s.device)
    _, packed = ops.score_ranks(s, yd, pos_label=pos_label, flag=flag)
    n = int(s.numel())
    assert ops.curve_points_len(n) == 8 + 8 * (n + 1)
    a = torch.zeros(ops.curve_points_len(n), dtype=torch.float64, device=s.device)
    b = torch.zeros_like(a)
    ops.curve_points(s, packed, pi0, out=a, flag=flag, **kw)
    ops.curve_points(s, packed, pi0, out=b, flag=flag, **kw)
    assert int(flag.item()) == 0
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two launches, different bits"
    return ops.parse_curve_points(a.cpu().numpy())


def _synthetic(n, ties, seed):
    rng = np.random.RandomState(seed)
    y = (rng.rand(n) < 0.2).astype(np.int64)
    lg = rng.randn(n) + 0.7 * y
    if ties:
        lg = np.round(lg * 64) / 64                                     # tie groups and singletons
    return y, (1.0 / (1.0 + np.exp(-lg))).astype(np.float32)


@pytest.mark.parametrize("c", CASES)
def test_curve_points_equal_the_reference_bit_for_bit(F, dev, c):
    from oaprogressionmmf_amd import ops
    y, p, _, _, _, pi0 = case(F, c)
    pd, yd = _dev(p, dev), _labels(y, dev)
    assert pd[:, 1].stride(0) == 2
    check_points(F, c, _points(ops, pd[:, 1], yd, pi0), p.dtype)                        # the column in place, its own dtype
    wide = pd[:, 1].to(torch.float64).contiguous()                     # fp32 widened exactly: the same ranks, the fp64 kernel
    check_points(F, c, _points(ops, wide, yd, pi0), p.dtype)


@pytest.mark.parametrize("n,ties", [(257, False), (2503, True), (4096, True), (4097, True), (5000, False), (16384, True)])
def test_curve_points_equal_the_twin_across_run_boundaries_and_histogram_sizes(dev, n, ties):
    from oaprogressionmmf_amd import ops
    y, s = _synthetic(n, ties, 5 * n + 1)
    for pos_label in (1, 0):
        got = _points(ops, _dev(s, dev), _labels(y, dev), 0.12, pos_label, pi_of_negatives=pos_label == 0)
        want = C.curve_points(s, y, pos_label, 0.12, pi_of_negatives=pos_label == 0)
        assert [got[k] for k in ("n_pos", "n_neg", "T", "K", "last_ind")] == [want[k] for k in ("n_pos", "n_neg", "T", "K", "last_ind")]
        for k in FIELDS:
            assert same_bits(got[k], want[k]), f"n = {n}, pos_label = {pos_label}: {k}"
    if not ties:
        assert got["T"] == len(np.unique(s))
    else:
        assert got["K"] < got["T"] < n


@pytest.mark.parametrize("c", CASES)
def test_range_metrics_against_the_reference_and_the_twin(F, dev, c):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.various import bootstrap_indices
    y, p, R, seed, strat, pi0 = case(F, c)
    idx = bootstrap_indices(y, R, seed, strat)
    keep = y[idx].sum(axis=1) != 0
    assert int(keep.sum()) == int(F[f"{c}:kept"])
    pd, yd, idxd = _dev(p, dev), _labels(y, dev), _dev(idx, dev)
    flag = ops.metrics_flag(dev)
    _, packed = ops.score_ranks(pd[:, 1], yd, flag=flag)
    worst = 0.0
    for k, rr in enumerate(RANGES):
        out = ops.range_metrics(packed, idxd, True, pi0, rr, flag=flag)
        again = ops.range_metrics(packed, idxd, True, pi0, rr, flag=flag)
        assert out.shape == (R + 1, 8) and torch.equal(out.view(torch.int64), again.view(torch.int64)), "two launches, different bits"
        got = out.cpu().numpy()
        want = C.range_rows(p[:, 1], y, idx, pi0, rr)
        assert _same(got[:, :6], want), f"case {c}, range {rr}: not the twin's bits"
        if k == 0:
            ap01 = got[0, 2]
        assert (got[:, 6:] == 0).all()
        assert np.isnan(got[1:, 2:6][~keep]).all() and np.array_equal(got[1:, 0][~keep], np.zeros(int((~keep).sum())))
        err = max(np.abs(got[1:, 2][keep] - F[f"{c}:rs_apr"][k]).max(), abs(got[0, 2] - F[f"{c}:apr"][k]))
        worst = max(worst, err)
        assert err < TOL, f"case {c}, range {rr}: ap_range off by {err}"
        assert got[0, 3] == F[f"{c}:bf1"][0] and np.array_equal(got[1:, 3][keep], F[f"{c}:rs_bf1"]), "best_f1_calib is exact"
    print(f"case {c}: max |device - reference| of ap_range {worst}")
    plain = ops.range_metrics(packed, pi0=None, flag=flag).cpu().numpy()                 # the identity row alone, not calibrated
    assert plain.shape == (1, 8) and plain[0, 3] == F[f"{c}:bf1"][1] and plain[0, 2] == ap01
    assert int(flag.item()) == 0
    if c == "g":
        assert 0 < int((~keep).sum()) < R


@pytest.mark.parametrize("n,m,R", [(5000, 5000, 3), (16384, 16384, 2), (4096, 4096, 2), (4097, 1000, 3), (257, 257, 3)])
def test_range_metrics_equal_the_twin_at_both_histogram_sizes(dev, n, m, R):
    from oaprogressionmmf_amd import ops
    y, s = _synthetic(n, n != 257, n + m)
    idx = np.random.RandomState(n).randint(0, n, size=(R, m)).astype(np.int32)
    _, packed = ops.score_ranks(_dev(s, dev), _labels(y, dev))
    for rr, pi0 in (((0.0, 1.0), 0.12), ((0.2, 0.8), None), ((0.75, 1.0), 0.3), ((0.5, 0.5), 0.12)):
        got = ops.range_metrics(packed, _dev(idx, dev), True, pi0, rr).cpu().numpy()
        assert _same(got[:, :6], C.range_rows(s, y, idx, pi0, rr)), f"n = {n}, m = {m}, range {rr}, pi0 = {pi0}"
    only = np.flatnonzero(y == 0)[:m].astype(np.int32)[None, :]                          # a resample without positives
    got = ops.range_metrics(packed, _dev(only, dev), False).cpu().numpy()
    assert got[0, 0] == 0 and got[0, 1] == only.shape[1] and np.isnan(got[0, 2:6]).all()


def test_confusion_counts(F, dev):
    from oaprogressionmmf_amd import ops
    t, p = F["mc:true"], F["mc:pred"]
    got = ops.confusion(_labels(t, dev), _labels(p, dev), 4)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), F["mc:cm"])
    rng = np.random.RandomState(9)
    n = 300001                                                                            # several blocks, a ragged tail
    t, p = rng.randint(0, 32, n), rng.randint(0, 32, n)
    td, pd = _labels(t, dev), _labels(p, dev)
    want, _ = C.confusion(t, p, 32)
    out = torch.zeros((32, 32), dtype=torch.int64, device=dev)
    assert ops.confusion(td, pd, 32, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    ops.confusion(td, pd, 32, out=out)                                                    # adds into a caller's counts
    assert np.array_equal(out.cpu().numpy(), 2 * want)
    flag = ops.metrics_flag(dev)
    got = ops.confusion(td, pd, 7, flag=flag).cpu().numpy()                               # labels >= 7 are skipped and flagged
    want7, bad = C.confusion(t, p, 7)
    assert bad and int(flag.item()) == 2 and np.array_equal(got, want7)
    t2 = t.copy()
    t2[5] = -1
    with pytest.raises(ValueError):
        ops.confusion(_labels(t2, dev), pd, 32)


def test_flag_word_and_wild_indices(F, dev):
    from oaprogressionmmf_amd import ops
    y, p, *_ = case(F, "a")
    s, yd = _dev(p[:, 1], dev), _labels(y, dev)
    _, packed = ops.score_ranks(s, yd)
    idx = np.tile(np.arange(37, dtype=np.int32), (2, 1))
    idx[1, 3], idx[1, 9] = 37, -1                                                         # not followed: flagged and left out
    flag = ops.metrics_flag(dev)
    out = ops.range_metrics(packed, _dev(idx, dev), False, flag=flag).cpu().numpy()
    assert int(flag.item()) == 4 and out[0, 0] + out[0, 1] == 37 and out[1, 0] + out[1, 1] == 35
    with pytest.raises(ValueError, match=r"outside \[0, n\)"):
        ops.range_metrics(packed, _dev(idx, dev), False)
    wild = packed.clone()
    wild[4] = (37 << 1) | 1                                                               # a rank outside the bins: skipped, flagged
    flag = ops.metrics_flag(dev)
    pts = ops.parse_curve_points(ops.curve_points(s, wild, flag=flag).cpu().numpy())
    assert int(flag.item()) == 4 and pts["n_pos"] + pts["n_neg"] == 36
    with pytest.raises(ValueError, match=r"outside"):
        ops.curve_points(s, wild)


def test_cap_and_argument_checks(dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    n = ops.METRICS_MAX_N + 1
    s = torch.rand(n, device=dev)
    big = torch.zeros(n, dtype=torch.int32, device=dev)
    with pytest.raises(KoafError, match="koaf_curve_points: 1 <= n <= 16384"):
        ops.curve_points(s, big)
    with pytest.raises(KoafError, match="koaf_range_metrics: 1 <= n <= 16384"):
        ops.range_metrics(big)
    ok = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(KoafError, match="1 <= m <= 16384"):
        ops.range_metrics(ok, torch.zeros((1, n), dtype=torch.int32, device=dev))
    with pytest.raises(KoafError, match="0 <= lo <= hi <= 1"):
        ops.range_metrics(ok, recall_range=(0.5, 0.25))
    with pytest.raises(KoafError, match="0 <= pi0 < 1"):
        ops.range_metrics(ok, pi0=1.0)
    with pytest.raises(KoafError, match="0 < pi0 < 1"):
        ops.curve_points(s[:8], ok, pi0=0.0)
    with pytest.raises(KoafError, match=r"out is contiguous fp64 \[80\]"):
        ops.curve_points(s[:8], ok, out=torch.zeros(79, dtype=torch.float64, device=dev))
    with pytest.raises(KoafError, match="1 <= K <= 32"):
        ops.confusion(ok, ok, 33)
    with pytest.raises(KoafError, match="int32"):
        ops.confusion(ok, ok.long(), 2)
    with pytest.raises(KoafError):
        ops.curve_points(torch.rand(8), ok)                                               # a host tensor: no CPU fallback
