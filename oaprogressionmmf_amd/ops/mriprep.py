"""Raw MRI series -> input volumes: T2 mapping and series compression (koaf_mriprep.hip)."""
import ctypes
import math

import torch

from .._lib import KoafError, check, lib
from ._base import FlagWord, _ptr, _stream, check_tensor, out_buffer

_SERIES_DTYPE = {torch.uint16: 2, torch.int16: 3, torch.float32: 4, torch.float64: 5}      # koaf.h: koaf_widen's codes and on
SERIES_FLAG_TEXT = {1: "the series holds NaN or infinity", 2: "the series holds a value outside [0, 65535]"}
_FLAG = FlagWord(SERIES_FLAG_TEXT)
series_flag = _FLAG.new         # a zeroed flag word for series_hist (koaf.h: bit 0 a non-finite voxel, bit 1 a voxel outside [0, 65535])
series_raise = _FLAG.raise_     # the ValueError of a series_hist flag word read back from the device


def _series_volume(what, x, ndim=None):
    """dtype code of a non-empty contiguous uint16 / int16 / fp32 / fp64 device tensor (of `ndim` axes)"""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype not in _SERIES_DTYPE or x.dim() != (ndim or x.dim()) or x.numel() == 0 \
            or not x.is_contiguous():
        raise KoafError(f"{what}: a non-empty contiguous {'' if ndim is None else str(ndim) + '-D '}uint16 / int16 / float32 / float64 tensor on the HIP device, got "
                        f"{(tuple(x.shape), x.dtype, x.device, x.is_contiguous()) if torch.is_tensor(x) else type(x)}")
    return _SERIES_DTYPE[x.dtype]


def _series_shift(what, shift):
    if not 2 <= int(shift) <= 8:
        raise KoafError(f"{what}: shift 2..8, got {shift}")
    return int(shift)


def t2_fit(vol, tes, nan_to=0.0, val_low=0.0, val_high=0.1, decimals=-1, margin=0, layout=0, out=None):
    """The reference's fit_t2_map on the device (koaf_t2_fit): vol (S, R, C, E) in its stored dtype (uint16 / int16 / fp32 / fp64,
    echo fastest), tes (S, E) fp64 -> fp64 T2 map, one launch.  decimals >= 0 also applies np.round(., decimals), margin > 0
    drops that many voxels at both ends of R and C, layout 0 gives (S, R', C'), layout 1 (R', C', S).  2 <= E <= 16."""
    dt = _series_volume("t2_fit", vol, 4)
    S, R, C, E = (int(v) for v in vol.shape)
    check_tensor("t2_fit", "tes", tes, torch.float64, (S, E), vol, where="vol's device")
    if not 2 <= E <= 16:
        raise KoafError(f"t2_fit: 2..16 echoes, got {E} (with one echo the reference's own answer is rounding noise)")
    margin, decimals = int(margin), int(decimals)
    if margin < 0 or 2 * margin >= R or 2 * margin >= C:
        raise KoafError(f"t2_fit: margin {margin} leaves nothing of {R} x {C}")
    if layout not in (0, 1):
        raise KoafError(f"t2_fit: layout 0 = (S, R, C), 1 = (R, C, S), got {layout}")
    if decimals > 22:
        raise KoafError(f"t2_fit: at most 22 decimals (10^d exact in fp64), got {decimals}")
    RO, CO = R - 2 * margin, C - 2 * margin
    shape = (S, RO, CO) if layout == 0 else (RO, CO, S)
    out = out_buffer("t2_fit", out, shape, torch.float64, vol, "vol's device")
    check(lib().koaf_t2_fit(vol.data_ptr(), dt, _ptr(tes), S, R, C, E, float(nan_to), float(val_low), float(val_high), decimals,
                            margin, int(layout), _ptr(out), _stream()), "t2_fit")
    return out


def series_hist(x, shift=3, bins=None, flag=None):
    """int32 [65536 >> shift] counts of astype(uint16)(x) >> shift over a contiguous uint16 / int16 / fp32 / fp64 device tensor
    (koaf_series_hist; integer atomics: deterministic).  bins: a tensor to add into (None: fresh zeros).  flag: a series_flag()
    word the kernel raises bits of; None: an own word is read back here (a host sync) and a non-finite or out-of-range voxel of a
    floating-point series raises ValueError."""
    dt = _series_volume("series_hist", x)
    shift = _series_shift("series_hist", shift)
    if x.numel() >= 1 << 31:
        raise KoafError(f"series_hist: fewer than 2^31 voxels, got {x.numel()}")
    nb = 65536 >> shift
    if bins is None:
        bins = torch.zeros(nb, dtype=torch.int32, device=x.device)
    check_tensor("series_hist", "bins", bins, torch.int32, (nb,), x)
    with _FLAG.own("series_hist", flag, x) as flag:
        check(lib().koaf_series_hist(x.data_ptr(), dt, x.numel(), shift, _ptr(bins), _ptr(flag), _stream()), "series_hist")
    return bins


def percentile_index(n, q):
    """(k, gamma) of np.percentile(a, q) (method "linear") over n values: the result is lerp(a_(k), a_(min(k + 1, n - 1)), gamma)"""
    v = (n - 1) * (float(q) / 100.0)
    k = math.floor(v)
    return int(k), v - k


def series_quantiles(bins, n, q=(0.0, 99.9), shift=3, out=None):
    """fp64 [len(q)] device tensor of np.percentile(x >> shift, q) from the histogram series_hist made of the n voxels of x
    (koaf_series_quantiles, one block; bit-equal to numpy, and nothing is read back)."""
    shift = _series_shift("series_quantiles", shift)
    if not torch.is_tensor(bins) or not bins.is_cuda:
        raise KoafError("series_quantiles: bins is the device tensor series_hist returns")
    check_tensor("series_quantiles", "bins", bins, torch.int32, (65536 >> shift,), bins)
    n, q = int(n), [float(v) for v in q]
    if not 0 < n < 1 << 31 or not 1 <= len(q) <= 8 or not all(0.0 <= v <= 100.0 for v in q):
        raise KoafError(f"series_quantiles: 0 < n < 2^31 and 1..8 percentiles within [0, 100], got n = {n}, q = {q}")
    pairs = [percentile_index(n, v) for v in q]
    out = out_buffer("series_quantiles", out, (len(q),), torch.float64, bins, "the bins' device")
    ks = (ctypes.c_int64 * len(q))(*[p[0] for p in pairs])
    gs = (ctypes.c_double * len(q))(*[p[1] for p in pairs])
    check(lib().koaf_series_quantiles(_ptr(bins), shift, n, ctypes.addressof(ks), ctypes.addressof(gs), len(q), _ptr(out), _stream()),
          "series_quantiles")
    return out


def series_pack(x, limits, shift=3, margin=16, out_dtype=torch.uint8):
    """(R - 2m, C - 2m, S) uint8 / uint16 tensor: x (R, C, S) shifted right, clipped in fp64 to the device pair `limits` (what
    series_quantiles returned), truncated toward zero and cropped by `margin` >= 1 on the first two axes (koaf_series_pack)."""
    dt = _series_volume("series_pack", x, 3)
    shift = _series_shift("series_pack", shift)
    R, C, S = (int(v) for v in x.shape)
    margin = int(margin)
    if margin < 1 or 2 * margin >= R or 2 * margin >= C:
        raise KoafError(f"series_pack: margin {margin} of {R} x {C}: at least 1 (numpy's [0:-0] is empty) and below half of both")
    if x.numel() >= 1 << 31:
        raise KoafError(f"series_pack: fewer than 2^31 voxels, got {x.numel()}")
    if out_dtype not in (torch.uint8, torch.uint16):
        raise KoafError(f"series_pack: uint8 or uint16 output, got {out_dtype}")
    check_tensor("series_pack", "limits", limits, torch.float64, (2,), x, where="x's device")
    out = torch.empty((R - 2 * margin, C - 2 * margin, S), dtype=out_dtype, device=x.device)
    check(lib().koaf_series_pack(x.data_ptr(), dt, R, C, S, shift, margin, _ptr(limits), out.data_ptr(),
                                 1 if out_dtype == torch.uint16 else 0, _stream()), "series_pack")
    return out
