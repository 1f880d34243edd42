"""GPU: the four kernels of koaf_mriprep.hip (ops.t2_fit, series_hist, series_quantiles, series_pack) against fixture F21 -- the
reference's fit_t2_map and numpy's percentile / clip / astype (tests/golden/make_golden_mriprep.py).
T2, every case:
 * the zero / non-zero pattern equals the fixture's;
 * |t_dev - t_ref| <= 32 kappa 2^-53 |t_ref| on the kept voxels.  Derived, not measured: at most 16 terms per sum,
   about a dozen roundings per term including log at 1 ulp, then two products and a difference whose cancellation kappa counts;
   four times the margin the generator holds the reference itself to against a longdouble evaluation;
 * decimals = 6 is bit-equal to np.round of the unrounded device map; layout 1 and the margin are pure index moves of layout 0;
   two launches give identical bits; a base pointer 2 / 6 / 8 bytes off 16-byte alignment (a slice of a larger buffer) gives the same
   bits; R * C is no multiple of 64 in any case and C - 2m crosses a 64-column run in case b;
 * uint16, int16, float32 and float64 copies of the same integer data give identical bits; val_low / val_high / nan_to are honoured.
Compression, every case: the bins are np.bincount's (also at shifts 2 and 8, on a constant volume -- every lane on one bin -- and at
n = one block's 2048-element step + 1 from an unaligned base, all four dtypes); the quantile pair is np.percentile's bit for bit;
the packed volume is bit-equal, through the 8-wide path and the element-wise one; flag bit 0 for a NaN, bit 1 for 70000.0."""
from pathlib import Path

import numpy as np
import pytest
import torch

import mriprep_twin as TW

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "f21_mriprep.npz"
T2_CASES = ("a", "b", "c", "d", "e", "f")
PACK_CASES = ("u1001", "u2002", "u1701", "const", "top", "i16", "m16")
ALL_CASES = PACK_CASES + ("dess_hi",)
U53 = 2.0 ** -53
TORCH_OUT = {"uint8": torch.uint8, "uint16": torch.uint16}


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int64).cpu().numpy()


def _off(a, dev, elems):
    """the same values in a contiguous view that starts `elems` elements into a 16-byte aligned buffer"""
    a = np.ascontiguousarray(a)
    host = np.zeros(a.size + 16, a.dtype)
    host[elems:elems + a.size] = a.ravel()
    buf = _dev(host, dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[elems:elems + a.size].view(a.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (elems * a.itemsize) % 16
    return v


@pytest.fixture(scope="module")
def maps(F, dev):
    """the unrounded layout-0 device map of every T2 case, computed once"""
    from oaprogressionmmf_amd import ops
    out = {c: ops.t2_fit(_dev(F[f"{c}:vol"], dev), _dev(F[f"{c}:tes"], dev)) for c in T2_CASES}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", T2_CASES)
def test_t2_fit_against_the_reference(F, maps, c):
    ref, kappa = F[f"{c}:t"], F[f"{c}:kappa"]
    t = maps[c].cpu().numpy()
    assert t.shape == ref.shape and t.dtype == np.float64
    kept = ref != 0.0
    assert np.array_equal(t != 0.0, kept)
    err = np.abs(t[kept] - ref[kept]) / (kappa[kept] * U53 * np.abs(ref[kept]))
    print(f"case {c}: device vs reference {err.max():.3f} kappa 2^-53 (bound 32), {int((t[kept] != ref[kept]).sum())} of "
          f"{int(kept.sum())} kept voxels differ in bits")
    assert err.max() <= 32.0


@pytest.mark.parametrize("c", T2_CASES)
def test_t2_fit_rounding_layout_margin_repeat(F, maps, dev, c):
    from oaprogressionmmf_amd import ops
    vol, tes = _dev(F[f"{c}:vol"], dev), _dev(F[f"{c}:tes"], dev)
    t = maps[c]
    assert np.array_equal(_bits(ops.t2_fit(vol, tes)), _bits(t))                      # two launches
    r = ops.t2_fit(vol, tes, decimals=6)
    want = np.round(t.cpu().numpy(), 6)
    assert np.array_equal(_bits(r), want.view(np.int64))
    assert np.array_equal(_bits(ops.t2_fit(vol, tes, layout=1)), _bits(t.permute(1, 2, 0)))
    for m in (1, 2):
        crop = t[:, m:-m, m:-m]
        assert np.array_equal(_bits(ops.t2_fit(vol, tes, margin=m)), _bits(crop))
        assert np.array_equal(_bits(ops.t2_fit(vol, tes, margin=m, layout=1, decimals=6)),
                              np.ascontiguousarray(np.moveaxis(want[:, m:-m, m:-m], [0, 1, 2], [2, 0, 1])).view(np.int64))


@pytest.mark.parametrize("c", ("b", "d", "e", "a"))
def test_t2_fit_unaligned_base(F, maps, dev, c):
    from oaprogressionmmf_amd import ops
    vol, tes = F[f"{c}:vol"], _dev(F[f"{c}:tes"], dev)
    for elems in (1, 3) if vol.itemsize == 2 else (1,):
        v = _off(vol, dev, elems)
        assert v.data_ptr() % 16 != 0
        assert np.array_equal(_bits(ops.t2_fit(v, tes)), _bits(maps[c]))
        assert np.array_equal(_bits(ops.t2_fit(v, tes, layout=1, margin=1)), _bits(maps[c][:, 1:-1, 1:-1].permute(1, 2, 0)))


def test_t2_fit_dtypes_give_identical_bits(F, maps, dev):
    from oaprogressionmmf_amd import ops
    vol, tes = F["b:vol"], _dev(F["b:tes"], dev)
    assert vol.dtype == np.uint16 and vol.max() < 32768
    for dt in (np.int16, np.float32, np.float64):
        for layout in (0, 1):
            got = ops.t2_fit(_dev(vol.astype(dt), dev), tes, layout=layout)
            assert np.array_equal(_bits(got), _bits(maps["b"] if layout == 0 else maps["b"].permute(1, 2, 0))), (dt, layout)
    neg = F["f:vol"]
    assert neg.dtype == np.int16 and (neg < 0).any()
    tf = _dev(F["f:tes"], dev)
    assert np.array_equal(_bits(ops.t2_fit(_dev(neg.astype(np.float64), dev), tf)), _bits(maps["f"]))


def test_t2_fit_limits_and_nan_to(F, maps, dev):
    from oaprogressionmmf_amd import ops
    vol, tes = _dev(F["b:vol"], dev), _dev(F["b:tes"], dev)
    t = maps["b"].cpu().numpy()
    kappa = TW.t2_kappa(F["b:vol"], F["b:tes"])[0]
    for kw in (dict(val_high=10.0), dict(val_low=0.03, val_high=0.06), dict(nan_to=7.0), dict(val_low=-1.0, val_high=1.0)):
        got = ops.t2_fit(vol, tes, **kw).cpu().numpy()
        want = TW.t2_fit(F["b:vol"], F["b:tes"], **kw)
        assert np.array_equal(got != 0.0, want != 0.0), kw
        both = (t != 0.0) & (got != 0.0)
        assert np.array_equal(got[both], t[both]), kw                 # a kept voxel keeps the bits of the default map
        kept = want != 0.0
        assert (np.abs(got[kept] - want[kept]) <= 32.0 * kappa[kept] * U53 * np.abs(want[kept])).all(), kw


def test_t2_fit_refusals(F, dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    tes = _dev(F["d:tes"], dev)
    vol = _dev(F["d:vol"], dev)
    for bad in (lambda: ops.t2_fit(_dev(F["d:vol"][..., :1], dev), _dev(F["d:tes"][:, :1], dev)),
                lambda: ops.t2_fit(_dev(np.zeros((2, 9, 9, 17), np.uint16), dev), torch.zeros((2, 17), dtype=torch.float64, device=dev)),
                lambda: ops.t2_fit(vol, tes, margin=5),
                lambda: ops.t2_fit(vol, tes.float()),
                lambda: ops.t2_fit(torch.zeros(tuple(vol.shape), dtype=torch.int32, device=dev), tes),
                lambda: ops.t2_fit(vol, tes, layout=2),
                lambda: ops.t2_fit(vol.cpu(), tes)):
        with pytest.raises(KoafError):
            bad()


@pytest.mark.parametrize("c", ALL_CASES)
def test_series_hist_quantiles_pack(F, dev, c):
    from oaprogressionmmf_amd import ops
    image, p = F[f"{c}:image"], F[f"{c}:p"]
    x = _dev(image, dev)
    u = image.view(np.uint16) if image.dtype == np.int16 else image
    flag = ops.series_flag(dev)
    for shift in (3, 2, 8):
        bins = ops.series_hist(x, shift, flag=flag)
        assert bins.dtype == torch.int32 and np.array_equal(bins.cpu().numpy(), np.bincount((u >> shift).ravel(), minlength=65536 >> shift))
    bins = ops.series_hist(x, 3, flag=flag)
    q = ops.series_quantiles(bins, image.size)
    assert np.array_equal(_bits(q), p.view(np.int64))
    qs = (0.0, 99.9, 50.0, 2.5, 100.0)
    assert np.array_equal(_bits(ops.series_quantiles(bins, image.size, qs)), np.percentile(u >> 3, q=qs).view(np.int64))
    assert int(flag.item()) == 0
    if c == "dess_hi":
        return
    want, margin = F[f"{c}:out"], int(F[f"{c}:margin"])
    got = ops.series_pack(x, q, 3, margin, TORCH_OUT[str(want.dtype)])
    assert got.dtype == TORCH_OUT[str(want.dtype)] and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.series_pack(_off(image, dev, 1), q, 3, margin, TORCH_OUT[str(want.dtype)]).cpu().numpy(), want)


def test_series_hist_block_edges_and_dtypes(dev):
    """one block's step is 256 threads x 16 bytes: n = 2048 + 1 two-byte elements from a base 2 bytes off alignment leaves a head, a
    body and a tail; all four dtypes count alike; a constant volume puts every lane on one bin"""
    from oaprogressionmmf_amd import ops
    rng = np.random.default_rng(3)
    for n in (2049, 4 * 2048 + 9, 7):
        a = rng.integers(0, 65536, n).astype(np.uint16)
        want = np.bincount(a >> 3, minlength=8192)
        for dt in (np.uint16, np.int16, np.float32, np.float64):
            src = a.view(np.int16) if dt == np.int16 else a.astype(dt)
            for elems in (0, 1):
                assert np.array_equal(ops.series_hist(_off(src, dev, elems), 3).cpu().numpy(), want), (n, dt, elems)
    const = np.full(70001, 4321, np.uint16)
    bins = ops.series_hist(_dev(const, dev), 3).cpu().numpy()
    assert bins[4321 >> 3] == 70001 and bins.sum() == 70001
    bins2 = ops.series_hist(_dev(const, dev), 3, bins=ops.series_hist(_dev(const, dev), 3)).cpu().numpy()      # adds into given bins
    assert bins2[4321 >> 3] == 140002


def test_series_pack_wide_path_is_the_elementwise_one(dev):
    """rows of (C - 2m) * S and m * S multiples of 8 from an aligned base take 8 voxels per thread; one element off they go one
    by one: the same bytes, for every input dtype and both outputs"""
    from oaprogressionmmf_amd import ops
    rng = np.random.default_rng(4)
    a = np.minimum(rng.gamma(1.2, 900.0, (12, 14, 16)), 65535).astype(np.uint16)
    lim = np.percentile(a >> 3, q=(0., 99.9))
    for od, nd in ((torch.uint8, np.uint8), (torch.uint16, np.uint16)):
        hi = min(lim[1], 255.0) if nd == np.uint8 else lim[1]
        l2 = np.array([lim[0] + 1.5, hi])
        want = np.clip(a >> 3, l2[0], l2[1]).astype(nd)[2:-2, 2:-2, :]
        for dt in (np.uint16, np.float32, np.float64):
            for elems in (0, 1):
                got = ops.series_pack(_off(a.astype(dt), dev, elems), _dev(l2, dev), 3, 2, od)
                assert np.array_equal(got.cpu().numpy(), want), (od, dt, elems)


def test_series_flags(F, dev):
    from oaprogressionmmf_amd import ops
    image = F["u1701:image"].astype(np.float32)
    clean = ops.series_hist(_dev(image + np.float32(0.75), dev), 3).cpu().numpy()
    assert np.array_equal(clean, np.bincount((F["u1701:image"] >> 3).ravel(), minlength=8192))
    for dt in (np.float32, np.float64):
        for value, bit in ((np.nan, 1), (np.inf, 1), (70000.0, 2), (-1.0, 2)):
            x = image.astype(dt)
            x[3, 4, 5] = value
            flag = ops.series_flag(dev)
            bins = ops.series_hist(_dev(x, dev), 3, flag=flag)
            assert int(flag.item()) == bit and int(bins.sum().item()) == x.size - 1, (dt, value)
            with pytest.raises(ValueError, match="NaN or infinity" if bit == 1 else "outside"):
                ops.series_hist(_dev(x, dev), 3)
