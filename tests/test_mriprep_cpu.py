"""CPU: the numpy twin of koaf_mriprep.hip (tests/mriprep_twin.py) against fixture F21 (the reference's fit_t2_map and numpy's
percentile / clip / astype, written by tests/golden/make_golden_mriprep.py), and everything of the feature that needs no device.
 * T2: the twin's zero / non-zero pattern equals the reference's on every voxel, and |t - t_ref| <= 32 kappa 2^-53 |t_ref| on the
   voxels it keeps (the device's bound, derived in DESIGN 3.20; kappa is the fixture's condition number); the twin's own kappa is
   the fixture's; rounding, margin and layout are np.round / slicing / moveaxis of the plain map;
 * compression: histogram + order statistics give np.percentile's pair bit for bit, the packed volume is bit-equal, the DESS
   case with p99.9 > 255 raises;
 * the (k, gamma) restatement of np.percentile's linear method for every n in 2..3000, at q = 99.9 and four more;
 * rint(x * 1e6) / 1e6 == np.round(x, 6) bit for bit;
 * koaf.h declares the four entry points, KOAF_VERSION is 200, the Makefile's REST_SRCS lists koaf_mriprep.hip, and every
   bad-argument path of the four returns the error status from host code."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import mriprep_twin as TW

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "f21_mriprep.npz"
T2_CASES = ("a", "b", "c", "d", "e", "f")
PACK_CASES = ("u1001", "u2002", "u1701", "const", "top", "i16", "m16")
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("c", T2_CASES)
def test_twin_t2_against_the_reference(F, c):
    vol, tes, ref, kappa = F[f"{c}:vol"], F[f"{c}:tes"], F[f"{c}:t"], F[f"{c}:kappa"]
    t = TW.t2_fit(vol, tes)
    kept = ref != 0.0
    assert kept.any() and (~kept).any()
    assert np.array_equal(t != 0.0, kept)
    err = np.abs(t[kept] - ref[kept]) / (kappa[kept] * U53 * np.abs(ref[kept]))
    print(f"case {c}: twin vs reference {err.max():.2f} kappa 2^-53 (bound 32)")
    assert err.max() <= 32.0
    assert np.allclose(TW.t2_kappa(vol, tes)[0][kept], kappa[kept], rtol=1e-12, atol=0.0)
    # what the device compares its map with: the longdouble value within the generator's 8 kappa 2^-53 of the reference
    ld = F[f"{c}:t_ld"]
    assert (np.abs(ref[kept] - ld[kept]) <= 8.0 * kappa[kept] * U53 * np.abs(ld[kept]) * (1 + 1e-9)).all()


def test_twin_t2_branches_rounding_margin_layout(F):
    vol, tes = F["b:vol"], F["b:tes"]
    t = TW.t2_fit(vol, tes)
    assert np.array_equal(_bits(TW.t2_fit(vol, tes, decimals=6)), _bits(np.round(t, 6)))
    m = TW.t2_fit(vol, tes, decimals=6, margin=3, layout=1)
    assert np.array_equal(_bits(m), _bits(np.moveaxis(np.round(t, 6)[:, 3:-3, 3:-3], [0, 1, 2], [2, 0, 1])))
    # val_high moves voxels into the map, nan_to never shows on finite data, planted voxels 0..3 are rejected
    wide = TW.t2_fit(vol, tes, val_high=10.0)
    assert (wide != 0).sum() > (t != 0).sum() and np.array_equal(wide[t != 0], t[t != 0])
    assert np.array_equal(_bits(TW.t2_fit(vol, tes, nan_to=7.0)), _bits(t))
    assert not t[0, 0, :4].any()


@pytest.mark.parametrize("c", PACK_CASES + ("dess_hi",))
def test_twin_compression_is_numpy(F, c):
    image, p, seq, margin = F[f"{c}:image"], F[f"{c}:p"], str(F[f"{c}:seq"]), int(F[f"{c}:margin"])
    bins, flag = TW.series_hist(image, 3)
    assert flag == 0 and bins.dtype == np.int32 and bins.sum() == image.size
    assert np.array_equal(bins, np.bincount((image.astype(np.uint16) >> 3).ravel(), minlength=8192))
    assert np.array_equal(_bits(TW.series_quantiles(bins, image.size)), _bits(p))
    if c == "dess_hi":
        assert p[1] > 255
        with pytest.raises(ValueError, match="Out-of-range intensity"):
            TW.compress_series(image, seq, margin)
        return
    out, pp = TW.compress_series(image, seq, margin)
    assert out.dtype == F[f"{c}:out"].dtype and np.array_equal(out, F[f"{c}:out"]) and np.array_equal(_bits(pp), _bits(p))


def test_twin_float_series_and_flags(F):
    image = F["u1701:image"]
    for dt in (np.float32, np.float64):
        x = image.astype(dt) + dt(0.75)                       # truncation toward zero drops the fraction
        assert np.array_equal(TW.series_hist(x, 3)[0], TW.series_hist(image, 3)[0])
        x[0, 0, 0], x[1, 1, 1], x[2, 2, 2] = np.nan, 70000.0, -1.0
        bins, flag = TW.series_hist(x, 3)
        assert flag == 3 and bins.sum() == image.size - 3
    neg = F["i16:image"]
    assert (neg < 0).any() and np.array_equal(TW.series_hist(neg, 3)[0], TW.series_hist(neg.view(np.uint16), 3)[0])


def test_percentile_index_is_numpys_rule():
    """lerp over (k, gamma) equals np.percentile bit for bit: every n in 2..3000, on data whose neighbours differ"""
    from oaprogressionmmf_amd import ops
    rng = np.random.default_rng(5)
    base = np.sort(rng.integers(0, 8192, 3000)).astype(np.uint16)
    qs = (0.0, 99.9, 50.0, 2.5, 100.0)
    for n in range(2, 3001):
        a = base[:n]
        want = np.percentile(a, q=qs)
        got = np.empty(len(qs))
        for j, q in enumerate(qs):
            k, g = ops.percentile_index(n, q)
            assert (k, g) == TW.percentile_index(n, q) and 0 <= k < n and 0.0 <= g < 1.0
            lo, hi = float(a[k]), float(a[min(k + 1, n - 1)])
            d = hi - lo
            got[j] = hi - d * (1.0 - g) if g >= 0.5 else lo + d * g
        assert np.array_equal(_bits(got), _bits(want)), n


def test_rint_scale_is_np_round():
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.uniform(0.0, 0.1, 200000), rng.uniform(0.0, 0.1, 1000).round(6) + 5e-7, [0.0, 0.1, 0.0000005, 0.0000015]])
    assert np.array_equal(_bits(np.rint(x * 1e6) / 1e6), _bits(np.round(x, 6)))
    assert 10.0 ** 6 == 1e6 and 10.0 ** 22 == 1e22


def test_exports():
    from oaprogressionmmf_amd import ops, preproc
    for name in ("fit_t2_map", "t2_map_series", "compress_series"):
        assert callable(getattr(preproc, name))
    for name in ("t2_fit", "series_hist", "series_quantiles", "series_pack", "series_flag", "series_raise"):
        assert callable(getattr(ops, name))
    with pytest.raises(NotImplementedError, match="SAG_3D_FOO"):
        preproc.compress_series(np.zeros((40, 40, 2), np.uint16), "SAG_3D_FOO")
    with pytest.raises(ValueError, match="margin 0"):
        preproc.compress_series(np.zeros((40, 40, 2), np.uint16), "COR_IW_TSE", margin=0)
    with pytest.raises(ValueError, match="holds NaN"):
        ops.series_raise(1)
    ops.series_raise(0)


def test_header_makefile_and_version():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert protos["koaf_t2_fit"] == (ctypes.c_int, [vp, i32, vp, i32, i32, i32, i32, f64, f64, f64, i32, i32, i32, vp, vp])
    assert protos["koaf_series_hist"] == (ctypes.c_int, [vp, i32, i64, i32, vp, vp, vp])
    assert protos["koaf_series_quantiles"] == (ctypes.c_int, [vp, i32, i64, vp, vp, i32, vp, vp])
    assert protos["koaf_series_pack"] == (ctypes.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp])
    assert list(protos)[-4:] == ["koaf_t2_fit", "koaf_series_hist", "koaf_series_quantiles", "koaf_series_pack"]   # appended
    assert _lib.defines()["KOAF_VERSION"] == 200
    mk = (ROOT / "oaprogressionmmf_amd" / "csrc" / "Makefile").read_text()
    rest = re.findall(r"^REST_SRCS\s*=(.*)$", mk, flags=re.M)
    assert len(rest) == 1 and "koaf_mriprep.hip" in rest[0].split()
    handle = _lib.lib()
    assert handle.koaf_version() == 200
    for name in ("koaf_t2_fit", "koaf_series_hist", "koaf_series_quantiles", "koaf_series_pack"):
        assert getattr(handle, name).argtypes == protos[name][1]


def test_bad_arguments_are_refused_on_the_host():
    """every refusal comes from host code ahead of any launch: the pointers are host buffers no kernel ever sees"""
    from oaprogressionmmf_amd import _lib
    handle, d = _lib.lib(), _lib.defines()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ks, gs = (ctypes.c_int64 * 2)(0, 5), (ctypes.c_double * 2)(0.0, 0.5)
    pk, pg = ctypes.addressof(ks), ctypes.addressof(gs)

    def refused(rc, text):
        assert rc == d["KOAF_EINVAL"], (rc, text)
        assert text in handle.koaf_last_error(), handle.koaf_last_error()

    fit = lambda vol=p, dtype=2, tes=p, S=2, R=8, C=8, E=7, dec=6, m=0, layout=0, out=p: handle.koaf_t2_fit(
        vol, dtype, tes, S, R, C, E, 0.0, 0.0, 0.1, dec, m, layout, out, None)
    refused(fit(E=1), b"2..16 echoes")
    refused(fit(E=17), b"2..16 echoes")
    refused(fit(E=0), b"2..16 echoes")
    refused(fit(dtype=1), b"koaf_t2_fit: dtype")
    refused(fit(dtype=6), b"koaf_t2_fit: dtype")
    refused(fit(m=4), b"margin 4")
    refused(fit(m=-1), b"margin -1")
    refused(fit(S=0), b"bad shape")
    refused(fit(layout=2), b"layout")
    refused(fit(dec=23), b"22 decimals")
    refused(fit(vol=None), b"null pointer")
    refused(fit(tes=None), b"null pointer")
    refused(fit(out=None), b"null pointer")
    refused(fit(vol=p + 1), b"not aligned")

    hist = lambda x=p, dtype=2, n=100, shift=3, bins=p, flag=p: handle.koaf_series_hist(x, dtype, n, shift, bins, flag, None)
    refused(hist(shift=1), b"shift 2..8")
    refused(hist(shift=9), b"shift 2..8")
    refused(hist(dtype=1), b"koaf_series_hist: dtype")
    refused(hist(n=0), b"n < 2^31")
    refused(hist(n=1 << 31), b"n < 2^31")
    refused(hist(x=None), b"null pointer")
    refused(hist(bins=None), b"null pointer")
    refused(hist(flag=None), b"null pointer")

    quant = lambda bins=p, shift=3, n=10, k=pk, g=pg, K=2, out=p: handle.koaf_series_quantiles(bins, shift, n, k, g, K, out, None)
    refused(quant(shift=1), b"shift 2..8")
    refused(quant(K=0), b"1..8 quantiles")
    refused(quant(K=9), b"1..8 quantiles")
    refused(quant(n=5), b"pair 1")                          # k = 5 is not below n = 5
    refused(quant(bins=None), b"null pointer")
    refused(quant(k=None), b"null pointer")
    refused(quant(out=None), b"null pointer")

    pack = lambda x=p, dtype=2, R=8, C=8, S=3, shift=3, m=1, lim=p, out=p, o16=0: handle.koaf_series_pack(
        x, dtype, R, C, S, shift, m, lim, out, o16, None)
    refused(pack(shift=1), b"shift 2..8")
    refused(pack(m=0), b"margin 0")
    refused(pack(m=4), b"margin 4")
    refused(pack(dtype=1), b"koaf_series_pack: dtype")
    refused(pack(o16=2), b"out16")
    refused(pack(R=0), b"bad shape")
    refused(pack(x=None), b"null pointer")
    refused(pack(lim=None), b"null pointer")
    refused(pack(out=None), b"null pointer")
