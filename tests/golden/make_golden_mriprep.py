#!/usr/bin/env python3
"""Generate fixture F21 (tests/golden/f21_mriprep.npz): the T2 fit and the series compression of the reference's
run/prepare_data_mri_oai.py, for koaf_mriprep.hip.

The T2 cases run the reference's own koafusion/datasets/_mr_t2_mapping.py, loaded by path with a stand-in `numba` module (jit
returns the function, prange = range): the plain IEEE-754 evaluation of its source text, which is what the kernel restates.
The compression cases call numpy the way preproc_compress_series does (that module needs pydicom / nibabel and cannot be
imported).  Only arrays are stored.

T2 cases (S, R, C, E): a (3, 10, 12, 7) fp64; b (2, 33, 37, 7) uint16; c (33, 5, 6, 7) uint16; d (2, 9, 9, 2) uint16;
e (2, 9, 9, 16) uint16; f (2, 8, 9, 7) int16 with negative voxels.  Intensities are round(A exp(-te / T2) + noise) clipped to
[0, 4095] (f: [-60, 4095]), T2 in 10..120 ms, a fifth of the voxels with A near the noise (rising and flat curves), echo times in
seconds and slightly different per slice; voxels (0, 0, 0..3) are planted: all-zero, one zero echo, constant signal, a rising line.
Per case <c>:  <c>:vol, <c>:tes fp64 [S, E], <c>:t the reference's fit_t2_map(vol.astype(fp64), tes), <c>:t_ld the unbranched
t = -1 / b re-evaluated in np.longdouble (stored as fp64), <c>:kappa the condition number of tests/mriprep_twin.t2_kappa.
Asserted here: on every voxel the reference keeps, |t - t_ld| <= 8 kappa 2^-53 |t_ld|; and no voxel is borderline under four
times that error, i.e. with err_b = 32 * 2^-53 * kappa |b| (written without dividing by the numerator, so that it is finite for
the planted constant voxel whose numerator cancels to 0): the interval b +- err_b does not contain -1 / val_high (val_low = 0 is
the sign of b, and a sign change of b moves t between two rejected ranges), and |den| > 32 * 2^-53 * (|S_y S_x2y| + |S_xy^2|)
unless every term is 0.  Voxels with an intensity <= 0 are NaN by 0 * log(0) / log(negative) on any IEEE machine.  If an
assertion fires, change the seed.

Compression cases (R, C, S), the (p0, p99.9) pair and the packed volume as numpy makes them:
  u1001 (7, 11, 13) uint16 COR m 1, (n - 1) * 0.999 fractional part < 0.5;  u2002 (14, 11, 13) uint16 COR m 2, fractional part
  >= 0.5;  u1701 (7, 9, 27) uint16 COR m 1, fractional part 0.3;  const (7, 11, 13) DESS m 2;  top (7, 11, 13) COR m 1 with a
  65535 voxel;  i16 (7, 11, 13) int16 with negatives COR m 1;  dess_hi (7, 11, 13) DESS whose p99.9 > 255 (no volume: the reference
  raises);  m16 (34, 35, 3) DESS m 16.
Per case <c>: <c>:image, <c>:p fp64 [2], <c>:out, <c>:margin, <c>:seq.

Usage:  python tests/golden/make_golden_mriprep.py /path/to/reference
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import mriprep_twin as TW  # noqa: E402

SEED = 2101
U53 = 2.0 ** -53
T2_CASES = {"a": ((3, 10, 12, 7), np.float64), "b": ((2, 33, 37, 7), np.uint16), "c": ((33, 5, 6, 7), np.uint16),
            "d": ((2, 9, 9, 2), np.uint16), "e": ((2, 9, 9, 16), np.uint16), "f": ((2, 8, 9, 7), np.int16)}


def load_reference(root):
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda fn: fn)
    numba.prange = range
    sys.modules["numba"] = numba
    spec = importlib.util.spec_from_file_location("ref_t2", Path(root) / "koafusion" / "datasets" / "_mr_t2_mapping.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def t2_inputs(name, k):
    (S, R, C, E), dtype = T2_CASES[name]
    rng = np.random.default_rng(SEED + k)
    te0 = 0.010 * np.arange(1, E + 1) if E <= 8 else 0.005 * np.arange(1, E + 1)
    tes = te0[None, :] * (1.0 + 0.01 * np.arange(S))[:, None]
    A = rng.uniform(200.0, 3500.0, (S, R, C))
    weak = rng.random((S, R, C)) < 0.2
    A[weak] = rng.uniform(0.0, 60.0, int(weak.sum()))
    T2 = rng.uniform(0.010, 0.120, (S, R, C))
    sig = A[..., None] * np.exp(-tes[:, None, None, :] / T2[..., None]) + rng.normal(0.0, 15.0, (S, R, C, E))
    vol = np.clip(np.round(sig), -60 if dtype == np.int16 else 0, 4095)
    vol[0, 0, 0, :] = 0
    vol[0, 0, 1, :] = np.maximum(vol[0, 0, 1, :], 40)
    vol[0, 0, 1, E // 2] = 0
    vol[0, 0, 2, :] = 777
    vol[0, 0, 3, :] = 100 + 10 * np.arange(E)
    return vol.astype(dtype), tes


def run_t2(ref, name, k, out):
    vol, tes = t2_inputs(name, k)
    with np.errstate(all="ignore"):
        t = ref.fit_t2_map(vol.astype(np.float64), tes)
    t_ld = TW.t2_raw(vol, tes, np.longdouble)[0]
    _, _, b, _ = TW.t2_raw(vol, tes)
    kappa, err_b, ratio = TW.t2_kappa(vol, tes)
    kept = t != 0.0
    live = (vol > 0).all(axis=-1)                         # every other voxel is NaN -> 0 on any IEEE machine
    assert kept.sum() > 0 and not (kept & ~live).any()
    rel = np.abs(t[kept] - t_ld[kept]).astype(np.float64) / (kappa[kept] * U53 * np.abs(t_ld[kept]).astype(np.float64))
    assert rel.max() <= 8.0, f"case {name}: the reference is {rel.max():.2f} kappa 2^-53 from its longdouble evaluation"
    edge = np.abs(b[live] + 1.0 / 0.1) <= 32.0 * U53 * err_b[live]
    assert not edge.any(), f"case {name}: {int(edge.sum())} voxels within the error of val_high: change the seed"
    thin = ratio[live] <= 32.0 * U53
    assert not thin.any(), f"case {name}: {int(thin.sum())} voxels whose denominator may cancel: change the seed"
    assert np.array_equal(TW.t2_fit(vol, tes) != 0.0, kept), f"case {name}: the twin classifies differently"
    rising = int((b[live] > 0).sum())
    high = int(((b[live] < 0) & (b[live] > -10.0)).sum())
    print(f"  T2 case {name} {vol.shape} {vol.dtype}: kept {int(kept.sum())}, dead {int((~live).sum())}, rising {rising}, above val_high "
          f"{high}; reference vs longdouble {rel.max():.2f} kappa 2^-53, kappa max {kappa[kept].max():.1f}")
    assert rising > 0 and high > 0
    out[f"{name}:vol"], out[f"{name}:tes"], out[f"{name}:t"] = vol, tes, t
    out[f"{name}:t_ld"], out[f"{name}:kappa"] = t_ld.astype(np.float64), kappa


def compress_inputs(name, rng):
    heavy = lambda shape, top: np.minimum(rng.gamma(1.2, top / 8.0, shape), 65535).astype(np.uint16)
    if name == "u1001":
        return heavy((7, 11, 13), 20000.0), "COR_IW_TSE", 1
    if name == "u2002":
        return heavy((14, 11, 13), 20000.0), "COR_IW_TSE", 2
    if name == "u1701":
        return heavy((7, 9, 27), 20000.0), "COR_IW_TSE", 1
    if name == "const":
        return np.full((7, 11, 13), 1234, np.uint16), "SAG_3D_DESS", 2
    if name == "top":
        x = heavy((7, 11, 13), 9000.0)
        x[3, 4, 5] = 65535
        return x, "COR_IW_TSE", 1
    if name == "i16":
        return rng.normal(300.0, 250.0, (7, 11, 13)).round().astype(np.int16), "COR_IW_TSE", 1
    if name == "dess_hi":
        return heavy((7, 11, 13), 9000.0), "SAG_3D_DESS", 1
    if name == "m16":
        return heavy((34, 35, 3), 500.0), "SAG_3D_DESS", 16
    raise KeyError(name)


def run_compress(name, rng, out):
    image, seq, margin = compress_inputs(name, rng)
    tmp = image.astype(np.uint16) >> 3
    p = np.percentile(tmp, q=(0., 99.9))
    out[f"{name}:image"], out[f"{name}:p"] = image, p
    out[f"{name}:margin"], out[f"{name}:seq"] = np.int64(margin), np.str_(seq)
    n = image.size
    k, g = TW.percentile_index(n, 99.9)
    srt = np.sort(tmp.ravel())
    print(f"  compression case {name} {image.shape} {image.dtype} {seq}: n = {n}, (k, gamma) = ({k}, {g:.6f}), x_k = {srt[k]}, "
          f"x_k+1 = {srt[min(k + 1, n - 1)]}, p = {p}")
    if name in ("u1001", "u2002", "u1701"):
        assert srt[k] != srt[k + 1], f"case {name}: the two order statistics coincide, change the seed"
    if seq == "SAG_3D_DESS" and p[1] > 255:
        assert name == "dess_hi"
        return
    assert name != "dess_hi"
    tmp = np.clip(tmp, p[0], p[1]).astype(np.uint8 if seq == "SAG_3D_DESS" else np.uint16)
    out[f"{name}:out"] = np.ascontiguousarray(tmp[margin:-margin, margin:-margin, :])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    out = {}
    for k, name in enumerate(T2_CASES):
        run_t2(ref, name, k, out)
    rng = np.random.default_rng(SEED + 100)
    for name in ("u1001", "u2002", "u1701", "const", "top", "i16", "dess_hi", "m16"):
        run_compress(name, rng, out)
    fr = [TW.percentile_index(n, 99.9)[1] for n in (1001, 2002, 1701)]
    assert fr[1] >= 0.5 and fr[0] < 0.5 and fr[2] < 0.5, fr
    path = HERE / "f21_mriprep.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
