"""GPU: preproc.fit_t2_map / t2_map_series / compress_series against fixture F21 and the numpy twin the CPU tests pin to it.
 * fit_t2_map: numpy in / numpy out and tensor in / tensor out, identical bits; the reference's zero pattern; kept voxels within
   32 kappa 2^-53 relative of the reference (the kernel test's derived bound);
 * t2_map_series: np.round(., 6) of fit_t2_map moved to (rows, cols, slices), bit for bit, with and without the margin;
 * compress_series: volume and percentile pair bit-equal to numpy's for every case and both calling conventions; SAG_T2_MAP is
   the crop; the DESS ValueError, NotImplementedError for another sequence, ValueError for margin 0;
 * one native-size run against the twin: T2 (27, 384, 384, 7) uint16 through t2_map_series with margin 16, and DESS
   (384, 384, 160).  Same bound on the fit, bit equality on the rest."""
from pathlib import Path

import numpy as np
import pytest
import torch

import mriprep_twin as TW

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "f21_mriprep.npz"
T2_CASES = ("a", "b", "c", "d", "e", "f")
PACK_CASES = ("u1001", "u2002", "u1701", "const", "top", "i16", "m16")
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("c", T2_CASES)
def test_fit_t2_map_and_series(F, dev, c):
    from oaprogressionmmf_amd.preproc import fit_t2_map, t2_map_series
    vol, tes, ref, kappa = F[f"{c}:vol"], F[f"{c}:tes"], F[f"{c}:t"], F[f"{c}:kappa"]
    t = fit_t2_map(vol, tes)
    assert isinstance(t, np.ndarray) and t.dtype == np.float64 and t.shape == ref.shape
    td = fit_t2_map(_dev(vol, dev), _dev(tes, dev))
    assert torch.is_tensor(td) and td.is_cuda and _same(td.cpu().numpy(), t)
    assert _same(fit_t2_map(vol.astype(np.float64), tes), t)              # the reference's call site widens first
    kept = ref != 0.0
    assert np.array_equal(t != 0.0, kept)
    assert (np.abs(t[kept] - ref[kept]) <= 32.0 * kappa[kept] * U53 * np.abs(ref[kept])).all()
    moved = np.ascontiguousarray(np.moveaxis(np.round(t, decimals=6), [0, 1, 2], [2, 0, 1]))
    assert _same(t2_map_series(vol, tes), moved)
    assert _same(t2_map_series(_dev(vol, dev), _dev(tes, dev), margin=1).cpu().numpy(), np.ascontiguousarray(moved[1:-1, 1:-1, :]))
    wide = fit_t2_map(vol, tes, 0.0, 0.0, 10.0)                           # positional, as the reference's signature has them
    assert (wide != 0).sum() > kept.sum()


@pytest.mark.parametrize("c", PACK_CASES)
def test_compress_series(F, dev, c):
    from oaprogressionmmf_amd.preproc import compress_series
    image, p, want, seq, margin = F[f"{c}:image"], F[f"{c}:p"], F[f"{c}:out"], str(F[f"{c}:seq"]), int(F[f"{c}:margin"])
    out, pp = compress_series(image, seq, margin)
    assert isinstance(out, np.ndarray) and _same(out, want) and _same(pp, p)
    tout, tp = compress_series(_dev(image, dev), seq, margin)
    assert tout.is_cuda and tp.is_cuda and _same(tout.cpu().numpy(), want) and _same(tp.cpu().numpy(), p)
    two, _ = TW.compress_series(image, seq, margin)
    assert _same(two, want)
    for dt in (np.float32, np.float64):
        if image.dtype == np.uint16:
            assert _same(compress_series(image.astype(dt), seq, margin)[0], want)


def test_compress_series_t2_map_and_refusals(F, dev):
    from oaprogressionmmf_amd.preproc import compress_series
    t2 = np.round(np.random.default_rng(8).uniform(0.0, 0.1, (40, 41, 5)), 6)
    out, p = compress_series(t2, "SAG_T2_MAP")
    assert p is None and _same(out, np.ascontiguousarray(t2[16:-16, 16:-16, :]))
    out, p = compress_series(_dev(t2, dev), "SAG_T2_MAP", margin=3)
    assert p is None and out.is_cuda and out.is_contiguous() and _same(out.cpu().numpy(), np.ascontiguousarray(t2[3:-3, 3:-3, :]))
    image = F["dess_hi:image"]
    assert F["dess_hi:p"][1] > 255
    with pytest.raises(ValueError, match="Out-of-range intensity after clipping"):
        compress_series(image, "SAG_3D_DESS", 1)
    with pytest.raises(ValueError, match="Out-of-range intensity after clipping"):
        compress_series(_dev(image, dev), "SAG_3D_DESS", 1)
    assert compress_series(image, "COR_IW_TSE", 1)[0].dtype == np.uint16          # the same series is fine as uint16
    with pytest.raises(NotImplementedError, match="SAG_IW_TSE"):
        compress_series(image, "SAG_IW_TSE", 1)
    with pytest.raises(ValueError, match="margin 0"):
        compress_series(image, "COR_IW_TSE", margin=0)
    with pytest.raises(ValueError, match="larger than its margins"):
        compress_series(image, "COR_IW_TSE", margin=4)
    bad = image.astype(np.float32)
    bad[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        compress_series(bad, "COR_IW_TSE", 1)


def test_native_size_against_the_twin(dev):
    """the sizes the reference prepares: a 27-slice 7-echo MESE series and a 160-slice DESS volume"""
    from oaprogressionmmf_amd.preproc import compress_series, t2_map_series
    rng = np.random.default_rng(9)
    S, R, C, E = 27, 384, 384, 7
    tes = np.tile(0.010 * np.arange(1, E + 1), (S, 1))
    A = rng.uniform(0.0, 3500.0, (S, R, C, 1)).astype(np.float32)
    T2 = rng.uniform(0.010, 0.120, (S, R, C, 1)).astype(np.float32)
    vol = np.clip(np.rint(A * np.exp(-tes[:, None, None, :].astype(np.float32) / T2) + rng.normal(0.0, 15.0, (S, R, C, E)).astype(np.float32)),
                  0, 4095).astype(np.uint16)
    got = t2_map_series(_dev(vol, dev), _dev(tes, dev), decimals=-1, margin=16).cpu().numpy()
    want = TW.t2_fit(vol, tes, margin=16, layout=1)
    kappa = np.ascontiguousarray(np.moveaxis(TW.t2_kappa(vol, tes, np.float64)[0][:, 16:-16, 16:-16], [0, 1, 2], [2, 0, 1]))
    assert got.shape == (352, 352, 27) == want.shape
    kept = want != 0.0
    assert 0.3 < kept.mean() < 0.95 and np.array_equal(got != 0.0, kept)
    err = np.abs(got[kept] - want[kept]) / (kappa[kept] * U53 * np.abs(want[kept]))
    print(f"native T2: device vs twin {err.max():.3f} kappa 2^-53 (bound 32) over {int(kept.sum())} kept voxels")
    assert err.max() <= 32.0
    rounded = t2_map_series(_dev(vol, dev), _dev(tes, dev), margin=16).cpu().numpy()
    assert _same(rounded, np.round(got, 6))

    dess = np.minimum(rng.gamma(1.2, 120.0, (384, 384, 160)), 65535).astype(np.uint16)
    out, p = compress_series(_dev(dess, dev), "SAG_3D_DESS")
    wout, wp = TW.compress_series(dess, "SAG_3D_DESS")
    assert out.shape == (352, 352, 160) and _same(out.cpu().numpy(), wout) and _same(p.cpu().numpy(), wp)
    assert _same(wp, np.percentile(dess >> 3, q=(0., 99.9))) and 0 < wp[1] <= 255
