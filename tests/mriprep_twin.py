"""Vectorised numpy twin of koaf_mriprep.hip: the T2 fit (datasets/_mr_t2_mapping.py fit_t2_map, evaluated operation by operation
in fp64 over whole volumes), its conditioning, and the histogram / order-statistic / clip-narrow-crop steps of
run/prepare_data_mri_oai.py preproc_compress_series.  Pinned to fixture F21 by tests/test_mriprep_cpu.py; the GPU tests compare
the device against it where the fixture has no case (the native-size run)."""
import math

import numpy as np

U53 = 2.0 ** -53
SEQ_DTYPE = {"SAG_3D_DESS": np.uint8, "COR_IW_TSE": np.uint16}


def t2_sums(vol, tes, dtype=np.float64):
    """the five sums of fit_exp_linear in echo order, [S, R, C] each: (S_x2_y, S_y_lny, S_x_y, S_x_y_lny, S_y)"""
    vol = np.asarray(vol)
    S, R, C, E = vol.shape
    z = lambda: np.zeros((S, R, C), dtype)
    S_x2_y, S_y_lny, S_x_y, S_x_y_lny, S_y = z(), z(), z(), z(), z()
    with np.errstate(all="ignore"):
        for e in range(E):
            x = np.asarray(tes, dtype)[:, e][:, None, None]
            y = vol[..., e].astype(dtype)
            ly = np.log(y)
            S_x2_y = S_x2_y + x * x * y
            S_y_lny = S_y_lny + y * ly
            S_x_y = S_x_y + x * y
            S_x_y_lny = S_x_y_lny + x * y * ly
            S_y = S_y + y
    return S_x2_y, S_y_lny, S_x_y, S_x_y_lny, S_y


def t2_raw(vol, tes, dtype=np.float64):
    """-> (t, a, b, denom) before any branch, in `dtype` (np.longdouble: the yardstick the fixture holds the reference to)"""
    S_x2_y, S_y_lny, S_x_y, S_x_y_lny, S_y = t2_sums(vol, tes, dtype)
    with np.errstate(all="ignore"):
        denom = S_y * S_x2_y - S_x_y * S_x_y
        a = (S_x2_y * S_y_lny - S_x_y * S_x_y_lny) / denom
        b = (S_y * S_x_y_lny - S_x_y * S_y_lny) / denom
        t = -1.0 / b
    return t, a, b, denom


def t2_fit(vol, tes, nan_to=0.0, val_low=0.0, val_high=0.1, decimals=-1, margin=0, layout=0):
    """koaf_t2_fit: the branches of fit_t2_map in the reference's order, np.round, the margin crop and the layout move"""
    t, a, b, denom = t2_raw(vol, tes)
    with np.errstate(all="ignore"):
        out = np.where((t < val_low) | (t > val_high), 0.0, t)
        out = np.where(np.isnan(t), nan_to, out)
        out = np.where((denom == 0.0) | np.isnan(a) | np.isnan(b), 0.0, out)
        if decimals >= 0:
            scale = 10.0 ** decimals
            out = np.rint(out * scale) / scale
    if margin:
        out = out[:, margin:-margin, margin:-margin]
    if layout == 1:
        out = np.moveaxis(out, [0, 1, 2], [2, 0, 1])
    return np.ascontiguousarray(out)


def t2_kappa(vol, tes, dtype=np.longdouble):
    """-> (kappa, err_b, den_ratio) [S, R, C]: with num = S_y S_xylny - S_xy S_ylny and den = S_y S_x2y - S_xy^2,
    kappa = (|S_y S_xylny| + |S_xy S_ylny|) / |num| + (|S_y S_x2y| + |S_xy^2|) / |den|, the factor by which the relative rounding
    error of the products reaches t = -den / num;  err_b = kappa |b| written without the division by num (finite where num is 0);
    den_ratio = |den| / (|S_y S_x2y| + |S_xy^2|).  Evaluated in longdouble (fp64 serves where only kappa's size matters: its own
    relative error is kappa 2^-53); NaN where an intensity is <= 0."""
    S_x2_y, S_y_lny, S_x_y, S_x_y_lny, S_y = t2_sums(vol, tes, dtype)
    with np.errstate(all="ignore"):
        num = S_y * S_x_y_lny - S_x_y * S_y_lny
        den = S_y * S_x2_y - S_x_y * S_x_y
        tn = np.abs(S_y * S_x_y_lny) + np.abs(S_x_y * S_y_lny)
        td = np.abs(S_y * S_x2_y) + np.abs(S_x_y * S_x_y)
        kappa = tn / np.abs(num) + td / np.abs(den)
        err_b = (tn + np.abs(num / den) * td) / np.abs(den)
        ratio = np.abs(den) / td
    return kappa.astype(np.float64), err_b.astype(np.float64), ratio.astype(np.float64)


def as_u16(x):
    """-> (uint16 values, valid mask, flag word) of astype(np.uint16): integers reinterpreted, floats truncated toward zero; a float
    that is not finite raises bit 0, one outside [0, 65535] bit 1, and neither has a value"""
    x = np.asarray(x)
    if x.dtype in (np.uint16, np.int16):
        return x.view(np.uint16), np.ones(x.shape, bool), 0
    with np.errstate(all="ignore"):
        fin = np.isfinite(x)
        t = np.trunc(np.where(fin, x, 0).astype(np.float64))
        inr = (t >= 0) & (t <= 65535)
    ok = fin & inr
    return np.where(ok, t, 0).astype(np.uint16), ok, (0 if fin.all() else 1) | (0 if (inr | ~fin).all() else 2)


def series_hist(x, shift=3):
    """-> (int32 bins [65536 >> shift], flag word)"""
    u, ok, flag = as_u16(x)
    return np.bincount((u[ok] >> shift).ravel(), minlength=65536 >> shift).astype(np.int32), flag


def percentile_index(n, q):
    """(k, gamma) of np.percentile's linear method over n values"""
    v = (n - 1) * (float(q) / 100.0)
    k = math.floor(v)
    return int(k), v - k


def series_quantiles(bins, n, q=(0.0, 99.9)):
    """np.percentile of the n binned values from their histogram: numpy's _lerp over the order statistics (k, k + 1)"""
    cum = np.cumsum(bins.astype(np.int64))
    out = np.empty(len(q))
    for j, qq in enumerate(q):
        k, g = percentile_index(n, qq)
        lo = min(k, n - 1, int(cum[-1]) - 1)
        hi = min(k + 1, n - 1, int(cum[-1]) - 1)
        a = float(np.searchsorted(cum, lo, side="right"))
        b = float(np.searchsorted(cum, hi, side="right"))
        d = b - a
        out[j] = b - d * (1.0 - g) if g >= 0.5 else a + d * g
    return out


def series_pack(x, limits, shift=3, margin=16, out_dtype=np.uint8):
    u, _, _ = as_u16(x)
    w = np.minimum(np.maximum((u >> shift).astype(np.float64), limits[0]), limits[1])
    return np.ascontiguousarray(w.astype(np.int32).astype(out_dtype)[margin:-margin, margin:-margin, :])


def compress_series(image, sequence, margin=16):
    """-> (volume, (p0, p99.9)) as oaprogressionmmf_amd.preproc.compress_series gives them"""
    if sequence == "SAG_T2_MAP":
        return np.ascontiguousarray(image[margin:-margin, margin:-margin, :]), None
    bins, _ = series_hist(image, 3)
    p = series_quantiles(bins, image.size)
    if sequence == "SAG_3D_DESS" and p[1] > 255:
        raise ValueError("Out-of-range intensity after clipping")
    return series_pack(image, p, 3, margin, SEQ_DTYPE[sequence]), p
