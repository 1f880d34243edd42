"""From raw MRI series to the volumes the models read, on the device: the numerical bodies of the reference's
run/prepare_data_mri_oai.py (koaf_mriprep.hip).  Reading DICOM / writing NIfTI stays with the caller.

A device tensor in gives a device tensor out; a numpy array in is uploaded and a numpy array comes back, so the reference's call
sites work unchanged.  Series may stay in their stored integer dtype (uint16 / int16): the reference widens to fp64 first and the
values are the same.
"""
import numpy as np
import torch

from .. import ops

_SHIFT = 3                       # preproc_compress_series: image >> 3
_PERCENTS = (0.0, 99.9)
_PACKED = {"SAG_3D_DESS": torch.uint8, "COR_IW_TSE": torch.uint16}


def _device():
    if not torch.cuda.is_available():
        raise ops.KoafError("preproc: the MRI preparation runs on the HIP device (no CPU fallback exists)")
    return torch.device("cuda", torch.cuda.current_device())


def _upload(a, dtype=None):
    """-> (contiguous device tensor, came_from_numpy)"""
    if torch.is_tensor(a):
        return (a if dtype is None else a.to(dtype)).contiguous(), False
    a = np.ascontiguousarray(a, dtype=None if dtype is None else {torch.float64: np.float64}[dtype])
    return torch.from_numpy(a).to(_device()), True


def _download(t, as_numpy):
    return t.cpu().numpy() if as_numpy else t


def fit_t2_map(vol, tes, nan_to=0.0, val_low=0.0, val_high=0.1):
    """The reference's fit_t2_map (datasets/_mr_t2_mapping.py): vol (slices, rows, cols, echoes) multi-echo series, tes (slices,
    echoes) echo times -> (slices, rows, cols) fp64 T2 map; values outside [val_low, val_high] and unfittable voxels are 0."""
    v, from_np = _upload(vol)
    t, _ = _upload(tes, torch.float64)
    return _download(ops.t2_fit(v, t.to(v.device), nan_to, val_low, val_high), from_np)


def t2_map_series(vol, tes, decimals=6, margin=None):
    """The numerical body of dicom_series_to_t2_map_meta: fit_t2_map, np.round(., decimals) and the LAS+ -> IPR+ axis move, one
    launch -> (rows, cols, slices) fp64.  margin (16 in the reference) also applies the crop preproc_compress_series gives
    SAG_T2_MAP, in the same launch."""
    v, from_np = _upload(vol)
    t, _ = _upload(tes, torch.float64)
    return _download(ops.t2_fit(v, t.to(v.device), decimals=decimals, margin=margin or 0, layout=1), from_np)


def compress_series(image, sequence, margin=16):
    """preproc_compress_series for image (rows, cols, slices): "SAG_3D_DESS" -> uint8 and "COR_IW_TSE" -> uint16 (>> 3, clip to the
    (0, 99.9) percentiles, narrow, crop `margin` on the first two axes), "SAG_T2_MAP" crop only (a copy, no arithmetic).
    -> (volume, (p0, p99.9)); the pair is a device fp64 tensor (a numpy pair for a numpy image), None for SAG_T2_MAP.
    DESS raises the reference's ValueError when p99.9 > 255: the one host read-back of the call (COR_IW_TSE has none for an
    integer series; a floating-point series is also checked for NaN / out-of-range voxels)."""
    if sequence not in _PACKED and sequence != "SAG_T2_MAP":
        raise NotImplementedError(f"Preprocessing is not available: {sequence}")
    margin = int(margin)
    if margin < 1:
        raise ValueError(f"compress_series: margin {margin}: numpy's [0:-0] is empty, crop at least one voxel")
    x, from_np = _upload(image)
    if x.dim() != 3 or 2 * margin >= x.shape[0] or 2 * margin >= x.shape[1]:
        raise ValueError(f"compress_series: a (rows, cols, slices) volume larger than its margins, got {tuple(x.shape)} with margin {margin}")
    if sequence == "SAG_T2_MAP":
        return _download(x[margin:-margin, margin:-margin, :].contiguous(), from_np), None
    integer = x.dtype in (torch.uint16, torch.int16)
    flag = ops.series_flag(x.device) if integer else None            # an integer series cannot raise a bit: nothing to read back
    bins = ops.series_hist(x, _SHIFT, flag=flag)
    p = ops.series_quantiles(bins, x.numel(), _PERCENTS, _SHIFT)
    if sequence == "SAG_3D_DESS" and float(p[1].item()) > 255:
        raise ValueError("Out-of-range intensity after clipping")
    out = ops.series_pack(x, p, _SHIFT, margin, _PACKED[sequence])
    return _download(out, from_np), _download(p, from_np)
