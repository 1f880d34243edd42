"""GPU: koaf_pair_ranks / koaf_perm_metrics (ops.pair_ranks, ops.perm_metrics) against fixture F20 -- scikit-learn's metrics per
swap mask -- and against the numpy twin that the CPU tests pin to the same fixture (tests/permtest_twin.py).
 * the union ranks equal the counting definition exactly, through a stride of 2 and contiguously, fp32, fp64 and fp32 widened
   to fp64;
 * every row of cases a-e: P, N and both Mann-Whitney sums exact; average precision within 1e-10 absolute of the fixture and
   bit-equal to the twin.  The bound is derived, not measured: a fixed-order fp64 sum of at most 2n <= 16384 terms in [0, 1],
   n * 2^-53 * a small constant < 1e-11, the reference's own rounding of the same order;
 * an all-zero mask row is the identity row, an all-one row the identity with its sides exchanged, bit for bit; two launches
   give identical bits;
 * side A of the identity row against ops.curve_metrics of column a alone: U / (2 P N) bit-equal, average precision within
   1e-12 (n <= 3000 bins summed in another partition: two roundings of order n * 2^-53 ~ 3e-13 apart at most);
 * n = 2048 / 2049 (the two sides of the 4096- / 16384-bin switch) and n = 8192 (the cap) against the twin;
 * flag bits 0, 1 and 2; n = 8193 and R = 2^20 + 1 are the library's error status, ahead of any launch."""
from pathlib import Path

import numpy as np
import pytest
import torch

import permtest_twin as PT

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "f20_permtest.npz"
CASES = ("a", "b", "c", "d32", "d33", "e")
TOL = 1e-10


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _masks(m, dev):
    return _dev(np.ascontiguousarray(m, np.uint32).view(np.int32), dev)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _rows(a, b, y, masks, dev, with_identity=True):
    from oaprogressionmmf_amd import ops
    flag = ops.metrics_flag(dev)
    _, packed = ops.pair_ranks(_dev(a, dev), _dev(b, dev), _dev(np.asarray(y, np.int32), dev), flag=flag)
    out = ops.perm_metrics(packed, None if masks is None else _masks(masks, dev), with_identity, flag=flag)
    assert int(flag.item()) == 0
    return packed, out


@pytest.mark.parametrize("c", CASES)
def test_pair_ranks_equal_the_counting_definition(F, dev, c):
    from oaprogressionmmf_amd import ops
    y, a, b = F[f"{c}:y"], F[f"{c}:ref"], F[f"{c}:cmp"]
    n = y.shape[0]
    want = PT.pair_ranks(a, b)
    table = _dev(np.stack([b, a], axis=1), dev)                      # [n, 2]: both columns read in place, stride 2
    assert table[:, 1].stride(0) == 2
    rank = ops.pair_ranks(table[:, 1], table[:, 0])
    assert rank.dtype == torch.int32 and rank.shape == (2 * n,)
    assert np.array_equal(rank.cpu().numpy(), want)
    yd = _dev(y.astype(np.int32), dev)
    rank, packed = ops.pair_ranks(_dev(a, dev), table[:, 0], yd)     # one contiguous, one strided
    assert np.array_equal(rank.cpu().numpy(), want)
    assert np.array_equal(packed.cpu().numpy(), PT.packed(a, b, y))
    _, packed0 = ops.pair_ranks(_dev(a, dev), _dev(b, dev), yd, pos_label=0)
    assert np.array_equal(packed0.cpu().numpy(), PT.packed(a, b, y, 0))
    r64 = ops.pair_ranks(table[:, 1].double(), table[:, 0].double())  # widening is exact: the same ranks in fp64
    assert np.array_equal(r64.cpu().numpy(), want)
    if c == "a":                                                     # fp64 scores are not narrowed
        assert len(np.unique(want)) == 2 * n and a.dtype == np.float64
        a2, b2 = a.copy(), a + 1e-12
        assert len(np.unique(ops.pair_ranks(_dev(a2, dev), _dev(b2, dev)).cpu().numpy())) == 2 * n
        assert len(np.unique(ops.pair_ranks(_dev(a2, dev).float(), _dev(b2, dev).float()).cpu().numpy())) <= n


@pytest.mark.parametrize("c", CASES)
def test_every_row_against_the_fixture_and_the_twin(F, dev, c):
    from oaprogressionmmf_amd import ops
    y, a, b, masks = F[f"{c}:y"], F[f"{c}:ref"], F[f"{c}:cmp"], F[f"{c}:masks"]
    packed, out = _rows(a, b, y, masks, dev)
    again = ops.perm_metrics(packed, _masks(masks, dev), True)
    assert torch.equal(_bits(out), _bits(again)), "two launches, different bits"
    got = out.cpu().numpy()
    assert got.shape == (masks.shape[0] + 1, 8)
    assert (got[:, 0] == y.sum()).all() and (got[:, 1] == (y == 0).sum()).all() and (got[:, 6:] == 0).all()
    assert np.array_equal(got[:, 2:4], F[f"{c}:U"]), "Mann-Whitney sums: exact"
    err = np.abs(got[:, 4:6] - F[f"{c}:ap"]).max()
    twin = PT.perm_rows(a, b, y, masks, True)
    print(f"case {c}: max |device - scikit-learn| of average precision {err}; bit-equal to the twin "
          f"{np.array_equal(got, twin)}, max |device - twin| {np.abs(got - twin).max()}")
    assert err < TOL
    assert np.array_equal(got.view(np.int64), twin.view(np.int64)), "not the twin's bits"
    # no identity row: the mask rows alone
    alone = ops.perm_metrics(packed, _masks(masks, dev), False)
    assert torch.equal(_bits(alone), _bits(out[1:]))
    only = ops.perm_metrics(packed)
    assert only.shape == (1, 8) and torch.equal(_bits(only), _bits(out[:1]))


@pytest.mark.parametrize("c", ("b", "d32", "d33", "e"))
def test_all_zero_and_all_one_rows(F, dev, c):
    y, a, b = F[f"{c}:y"], F[f"{c}:ref"], F[f"{c}:cmp"]
    n = y.shape[0]
    W = (n + 31) // 32
    masks = np.zeros((3, W), np.uint32)
    masks[1] = 0xffffffff                                            # bits at and beyond n set as well: ignored
    masks[2] = 0xffffffff
    if n % 32:
        masks[2, -1] = (1 << (n % 32)) - 1
    _, out = _rows(a, b, y, masks, dev)
    out = out.cpu().numpy().view(np.int64)
    assert np.array_equal(out[1], out[0]), "an all-zero row is the identity"
    swapped = out[0][[0, 1, 3, 2, 5, 4, 6, 7]]
    assert np.array_equal(out[2], swapped) and np.array_equal(out[3], swapped), "an all-one row exchanges the sides"


@pytest.mark.parametrize("c", CASES)
def test_identity_row_against_curve_metrics(F, dev, c):
    from oaprogressionmmf_amd import ops
    y, a, b = F[f"{c}:y"], F[f"{c}:ref"], F[f"{c}:cmp"]
    _, out = _rows(a, b, y, None, dev)
    out = out.cpu().numpy()[0]
    yd = _dev(y.astype(np.int32), dev)
    for k, s in enumerate((a, b)):
        _, packed = ops.score_ranks(_dev(s, dev), yd)
        one = ops.curve_metrics(packed).cpu().numpy()[0]
        assert out[0] == one[0] and out[1] == one[1]
        assert out[2 + k] / (2.0 * out[0] * out[1]) == one[2], "ROC-AUC: the same integers, the same quotient"
        assert abs(out[4 + k] - one[3]) < 1e-12


@pytest.mark.parametrize("n,R", [(2048, 3), (2049, 3), (8192, 8), (1, 2), (257, 5)])
def test_bin_switch_and_cap_against_the_twin(dev, n, R):
    """2n = 4096 is the last size of the 4096-bin kernel, 2n = 4098 the first of the 16384-bin one; n = 8192 fills it"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.various import swap_masks
    rng = np.random.default_rng(n)
    y = (rng.random(n) < 0.2).astype(np.int64)
    if n == 1:
        y[:] = 1                                                     # a single class: counts and NaN
    base = rng.standard_normal(n) + 0.8 * y
    sig = lambda z: (1.0 / (1.0 + np.exp(-np.round(z * 64) / 64))).astype(np.float32)
    a, b = sig(base + 0.6 * rng.standard_normal(n)), sig(base + 0.6 * rng.standard_normal(n))
    masks, exact = swap_masks(n, R, seed=n)
    assert exact == (n == 1) and masks.shape[0] == (2 if n == 1 else R)
    packed, out = _rows(a, b, y, masks, dev)
    assert np.array_equal(packed.cpu().numpy(), PT.packed(a, b, y))
    got, twin = out.cpu().numpy(), PT.perm_rows(a, b, y, masks, True)
    assert np.array_equal(got[:, :4], twin[:, :4], equal_nan=True)
    if n == 1:
        assert got[:, :2].tolist() == [[1, 0]] * 3 and np.isnan(got[:, 2:6]).all()
    else:
        assert np.array_equal(got.view(np.int64), twin.view(np.int64)), "not the twin's bits"


def test_flag_word(F, dev):
    from oaprogressionmmf_amd import ops
    y, a, b = F["b:y"], F["b:ref"], F["b:cmp"]
    yd = _dev(y.astype(np.int32), dev)
    for bad, which in ((np.nan, 0), (np.inf, 1), (-np.inf, 1)):
        q = [a.copy(), b.copy()]
        q[which][17] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            ops.pair_ranks(_dev(q[0], dev), _dev(q[1], dev))
        flag = ops.metrics_flag(dev)
        ops.pair_ranks(_dev(q[0], dev), _dev(q[1], dev), yd, flag=flag)       # a caller's flag word: no sync, no raise here
        assert int(flag.item()) == 1
    y3 = y.astype(np.int32).copy()
    y3[5] = 2
    with pytest.raises(ValueError, match="label other than 0 / 1"):
        ops.pair_ranks(_dev(a, dev), _dev(b, dev), _dev(y3, dev))
    n = y.shape[0]
    _, packed = ops.pair_ranks(_dev(a, dev), _dev(b, dev), yd)
    wild = packed.clone()
    wild[3] = (2 * n) << 1 | 1                                      # ranks outside [0, 2n): skipped, never followed
    wild[n + 9] = -2
    flag = ops.metrics_flag(dev)
    masks = np.zeros((1, (n + 31) // 32), np.uint32)
    masks[0, 0] = 1 << 9                                            # row 1 moves the second wild word to side A
    out = ops.perm_metrics(wild, _masks(masks, dev), True, flag=flag).cpu().numpy()
    assert int(flag.item()) == 4
    assert out[0, 0] + out[0, 1] == n - 1 and out[1, 0] + out[1, 1] == n - 2, "side A's counts leave the skipped words out"
    with pytest.raises(ValueError, match="outside"):
        ops.perm_metrics(wild)


def test_cap_and_argument_checks(dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    n = ops.METRICS_MAX_N // 2 + 1
    s = torch.rand(n, device=dev)
    with pytest.raises(KoafError, match="koaf_pair_ranks: 1 <= n <= 8192"):
        ops.pair_ranks(s, s)
    with pytest.raises(KoafError, match="koaf_perm_metrics: 1 <= n <= 8192"):
        ops.perm_metrics(torch.zeros(2 * n, dtype=torch.int32, device=dev))
    ok = torch.zeros(16, dtype=torch.int32, device=dev)
    with pytest.raises(KoafError, match=r"koaf_perm_metrics: 0 <= R <= 2\^20"):
        ops.perm_metrics(ok, torch.zeros(((1 << 20) + 1, 1), dtype=torch.int32, device=dev))
    with pytest.raises(KoafError, match="neither the identity row nor a mask matrix"):
        ops.perm_metrics(ok, None, False)
    with pytest.raises(KoafError, match=r"\[R, 1\] matrix"):
        ops.perm_metrics(ok, torch.zeros((2, 2), dtype=torch.int32, device=dev))
    with pytest.raises(KoafError, match="2n words"):
        ops.perm_metrics(ok[:15])
    with pytest.raises(KoafError, match="one length, dtype and device"):
        ops.pair_ranks(s[:8], s[:8].double())
    with pytest.raises(KoafError, match="one length, dtype and device"):
        ops.pair_ranks(s[:8], s[:9])
    with pytest.raises(KoafError, match="fp32 / fp64"):
        ops.pair_ranks(s[:8].half(), s[:8].half())
    with pytest.raises(KoafError):
        ops.pair_ranks(torch.rand(8), torch.rand(8))                 # host tensors: no CPU fallback
