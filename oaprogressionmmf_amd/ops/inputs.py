"""Input plumbing: slice folding, resizing, widening and augmentation (koaf_preproc.hip) and the stored-volume window pipeline
(koaf_inpipe.hip)."""
import ctypes
import functools
import math

import numpy as np
import torch

from .._lib import KoafError, check, lib
from ._base import _empty, _ptr, _stream


def slice_fold(x, B, R, Cc, S):
    out = _empty((B * S, R, Cc), x)
    check(lib().koaf_slice_fold(_ptr(x), _ptr(out), B, R, Cc, S, _stream()), "slice_fold")
    return out


def slice_unfold(g, B, R, Cc, S):
    """"(b s) r c -> b r c s": g [B*S,R,C] -> [B,R,C,S], the transpose of slice_fold (its backward)"""
    out = _empty((B, R, Cc, S), g)
    check(lib().koaf_slice_unfold(_ptr(g), _ptr(out), B, R, Cc, S, _stream()), "slice_unfold")
    return out


def rowdot(a, b):
    """per-sample sum(a * b) of two contiguous fp32 tensors of one shape (B, ...) -> [B] (koaf_rowdot: fixed-order, no atomics)"""
    if tuple(a.shape) != tuple(b.shape) or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise KoafError(f"rowdot: two fp32 tensors of one shape, got {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
    a, b = a.contiguous(), b.contiguous()
    B = int(a.shape[0])
    n = a.numel() // B
    out = _empty((B,), a)
    ws = torch.empty(B * lib().koaf_rowdot_ws(n) // 2, device=a.device, dtype=torch.float64)      # (the fp64 block sums)
    check(lib().koaf_rowdot(_ptr(a), _ptr(b), B, n, _ptr(out), _ptr(ws), _stream()), "rowdot")
    return out


def resize(x, out_size):
    """F.interpolate(x, size given as recompute_scale_factor computes it, linear | bilinear | trilinear, align_corners=False) of
    a contiguous fp32 (B, CH, d0[, d1[, d2]]) tensor -> (B, CH, *out_size)  (koaf_resize)"""
    nd = x.dim() - 2
    if nd < 1 or nd > 3 or len(out_size) != nd:
        raise KoafError(f"resize: (B, CH, 1..3 spatial dims) tensors, got {tuple(x.shape)} -> {tuple(out_size)}")
    out = _empty(tuple(x.shape[:2]) + tuple(int(v) for v in out_size), x)
    ins = (ctypes.c_int32 * nd)(*[int(v) for v in x.shape[2:]])
    outs = (ctypes.c_int32 * nd)(*[int(v) for v in out_size])
    check(lib().koaf_resize(_ptr(x), _ptr(out), int(x.shape[0]) * int(x.shape[1]), nd, ctypes.addressof(ins), ctypes.addressof(outs),
                            _stream()), "resize")
    return out


def downscale2(x, B, R, Cc, S, fs):
    out = _empty((B, R // 2, Cc // 2, S // fs), x)
    check(lib().koaf_downscale2(_ptr(x), _ptr(out), B, R, Cc, S, fs, _stream()), "downscale2")
    return out


_WIDEN = {torch.uint8: 1, torch.uint16: 2, torch.int16: 3}


def widen(x):
    """uint8 / uint16 / int16 device tensor -> fp32 (koaf_widen); fp32 passes through"""
    if x.dtype == torch.float32:
        return x
    if x.dtype not in _WIDEN or not x.is_cuda:
        raise KoafError(f"widen: uint8 / uint16 / int16 tensors on the HIP device, got {x.dtype} on {x.device}")
    x = x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    check(lib().koaf_widen(x.data_ptr(), _WIDEN[x.dtype], _ptr(y), x.numel(), _stream()), "widen")
    return y


def minmax(x, B):
    """per-sample (min, max) of a contiguous batch -> [B, 2]"""
    n = x.numel() // B
    mm = _empty((B, 2), x)
    ws = _empty((B * lib().koaf_minmax_ws(n),), x)
    check(lib().koaf_minmax(_ptr(x), B, n, _ptr(mm), _ptr(ws), _stream()), "minmax")
    return mm


def augment(x, mm, params, B, R, C, S, mean, std):
    y = torch.empty_like(x)
    check(lib().koaf_augment(_ptr(x), _ptr(y), _ptr(mm), _ptr(params), B, R, C, S, mean, std, _stream()), "augment")
    return y


_STORED = {torch.float32: 0, **_WIDEN}


def _upload_bytes(host, dev):
    """a small host uint8 array -> device tensor on torch's current stream, through pinned memory and without waiting: a pageable
    copy makes the host wait for everything the stream still holds, once per batch.  The pinned block comes from torch's caching
    host allocator, which does not hand it out again before the copy has run."""
    pin = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    pin.numpy()[:] = host
    return pin.to(dev, non_blocking=True)


class HostWindowTable(object):
    """The host form of the per-sample table of koaf.h (8 x int64 per sample) with, optionally, the (cos, sin, exponent, rotated)
    rows of ops.augment behind it in the same bytes: built and CHECKED once by `window_rows`, then `upload(volumes)` fills in the
    addresses of this batch's volumes and sends everything in one pinned copy.  A transform whose geometry does not change from
    batch to batch (validation: centre crop, nothing random) keeps one of these per (stored shapes, flip pattern)."""

    def __init__(self, rows, prm, shapes, dtype, dense_step, win):
        B = rows.shape[0]
        self.buf = np.empty(64 * B + (16 * B if prm is not None else 0), dtype=np.uint8)
        self.rows = self.buf[:64 * B].view(np.int64).reshape(B, 8)
        self.rows[:] = rows
        self.prm = None
        if prm is not None:
            self.prm = self.buf[64 * B:].view(np.float32).reshape(B, 4)
            self.prm[:] = prm
        self.B, self.shapes, self.dtype, self.win = B, shapes, dtype, win
        self.offsets = None if dense_step is None else np.arange(B, dtype=np.int64) * dense_step      # dense: bytes from sample 0

    def upload(self, volumes):
        """volumes: the tensor / list of tensors the table was built for, or others of the same shapes and dtype
        -> (table [B, 8] int64 on the device, dtype code, (R, C, S)[, params [B, 4] fp32 on the device])"""
        B = self.B
        if self.offsets is not None:
            v0 = volumes
            if tuple(volumes.shape) != self.shapes or not volumes.is_contiguous():
                raise KoafError(f"window_table: built for one contiguous tensor {self.shapes}, got {tuple(volumes.shape)}")
            self.rows[:, 0] = self.offsets
            self.rows[:, 0] += volumes.data_ptr()
        else:
            v0 = volumes[0]
            if len(volumes) != B:
                raise KoafError(f"window_table: built for {B} volumes, got {len(volumes)}")
            for b, v in enumerate(volumes):
                if tuple(v.shape) != self.shapes[b] or v.dtype != self.dtype or v.device != v0.device or not v.is_contiguous():
                    raise KoafError(f"window_table: volume {b} is not the contiguous {self.shapes[b]} {self.dtype} tensor the table was built for")
                self.rows[b, 0] = v.data_ptr()
        if v0.dtype != self.dtype or not v0.is_cuda:
            raise KoafError(f"window_table: {self.dtype} volumes on the HIP device, got {v0.dtype} on {v0.device}")
        both = _upload_bytes(self.buf, v0.device)
        table = both[:64 * B].view(torch.int64).view(B, 8)
        if self.prm is None:
            return table, _STORED[self.dtype], self.win
        return table, _STORED[self.dtype], self.win, both[64 * B:].view(torch.float32).view(B, 4)


def window_rows(volumes, origins, masks, window, params=None):
    """-> HostWindowTable for `volumes` (see window_table for the arguments): every window is checked against its volume HERE, on
    the host -- the kernels follow the addresses"""
    nd = len(window)
    dense = torch.is_tensor(volumes)
    B = int(volumes.shape[0]) if dense else len(volumes)
    if nd not in (2, 3) or B < 1 or len(origins) != B or len(masks) != B:
        raise KoafError(f"window_table: a (R, C[, S]) window and one origin and mask per volume, got {tuple(window)} for {B} volumes")
    win = tuple(int(v) for v in window) + (1,) * (3 - nd)
    dt = volumes.dtype if dense else volumes[0].dtype
    if dt not in _STORED:
        raise KoafError(f"window_table: fp32 / uint8 / uint16 / int16 volumes, got {dt}")
    rows = np.zeros((B, 8), dtype=np.int64)
    rows[:, 1:4] = 1
    if dense:
        if volumes.dim() < nd + 1 or volumes.numel() != B * math.prod(volumes.shape[-nd:]):
            raise KoafError(f"window_table: one contiguous (B, 1, ...) tensor of {nd} stored axes, got {tuple(volumes.shape)}")
        rows[:, 1:1 + nd] = tuple(volumes.shape[-nd:])
        shapes, step = tuple(volumes.shape), volumes.numel() // B * volumes.element_size()
    else:
        for b, v in enumerate(volumes):
            sp = v.shape[-nd:]
            if len(sp) != nd or v.numel() != math.prod(sp):
                raise KoafError(f"window_table: volumes of {nd} axes behind axes of size 1, got {tuple(v.shape)}")
            rows[b, 1:1 + nd] = sp
        shapes, step = [tuple(v.shape) for v in volumes], None
    rows[:, 4:4 + nd] = np.asarray(origins, dtype=np.int64).reshape(B, nd)
    rows[:, 7] = np.asarray(masks, dtype=np.int64)
    sp, org = rows[:, 1:4], rows[:, 4:7]
    last = org + (1 - 2 * ((rows[:, 7:8] >> np.arange(3)) & 1)) * (np.asarray(win, dtype=np.int64) - 1)
    ok = (org >= 0) & (org < sp) & (last >= 0) & (last < sp)
    if min(win) < 1 or not ok.all() or (rows[:, 7] >> nd).any() or (rows[:, 7] < 0).any():
        b = int(np.argmin(ok.all(1)))
        raise KoafError(f"window_table: window {win} from origin {org[b].tolist()} (backwards mask {int(rows[b, 7])}) leaves the stored "
                        f"volume {sp[b].tolist()} of sample {b}")
    if params is not None:
        params = np.asarray(params, dtype=np.float32)
        if params.shape != (B, 4):
            raise KoafError(f"window_table: params is one (cos, sin, exponent, rotated) row per volume, got {params.shape}")
    return HostWindowTable(rows, params, shapes, dt, step, win)


def window_table(volumes, origins, masks, window, params=None):
    """The per-sample device table koaf_window_minmax / koaf_input_pipeline read the stored volumes through (koaf.h): `volumes`
    is B contiguous device tensors of one dtype (fp32 / uint8 / uint16 / int16), each (R0, C0[, S0]) behind leading axes of
    size 1 -- or ONE contiguous tensor (B, 1, R0, C0[, S0]), whose samples are addressed in place; `origins` [B][nd] the stored
    index of window voxel 0 per axis, `masks` [B] the bit mask of the axes walked backwards (1 = R, 2 = C, 4 = S), `window` =
    (R, C[, S]).  Every window is checked against its volume on the host (window_rows) and the table goes up in one pinned copy.
    -> (table [B, 8] int64 on the device, dtype code, (R, C, S)); keep the volumes alive until the kernels that read them have
    run.  With `params` (B rows of (cos, sin, exponent, rotated), what ops.augment takes) those travel in the same copy and come
    back as a fourth element, [B, 4] fp32 on the device."""
    return window_rows(volumes, origins, masks, window, params).upload(volumes)


@functools.lru_cache(maxsize=None)
def _window_ws(n):
    return int(lib().koaf_window_minmax_ws(n))


def window_minmax(table, dtype, window):
    """per-sample (min, max) over the R x C x S window of the stored volumes, straight from the stored type -> [B, 2] fp32
    (koaf_window_minmax; `table, dtype, window` as window_table returns them)"""
    B, (R, C, S) = int(table.shape[0]), window
    nws = B * _window_ws(R * C * S)
    buf = torch.empty((nws + 2 * B,), device=table.device, dtype=torch.float32)          # the partials, then the result
    mm = buf[nws:].view(B, 2)
    check(lib().koaf_window_minmax(_ptr(table), dtype, B, R, C, S, _ptr(mm), _ptr(buf), _stream()), "window_minmax")
    return mm


def input_pipeline(table, dtype, window, mm, params, mean, std, pool=1, pool_s=1, layout="rcs"):
    """stored volumes -> mean over pool x pool x pool_s of ((gamma(rotate(unit(window)))) - mean) / std, fp32
    (koaf_input_pipeline): (B, R/pool, C/pool, S/pool_s) for layout "rcs", (B, S/pool_s, R/pool, C/pool) for "ncdhw".
    mm [B, 2] as window_minmax leaves it, params [B, 4] as ops.augment takes them."""
    if layout not in ("rcs", "ncdhw"):
        raise KoafError(f"input_pipeline: layout is 'rcs' or 'ncdhw', got {layout!r}")
    B, (R, C, S) = int(table.shape[0]), window
    if pool not in (1, 2) or pool_s not in (1, 2) or R % pool or C % pool or S % pool_s:
        raise KoafError(f"input_pipeline: pools of 1 or 2 that divide the window, got {pool}, {pool_s} for {window}")
    shape = (B, S // pool_s, R // pool, C // pool) if layout == "ncdhw" else (B, R // pool, C // pool, S // pool_s)
    y = torch.empty(shape, device=table.device, dtype=torch.float32)
    check(lib().koaf_input_pipeline(_ptr(table), dtype, _ptr(y), _ptr(mm), _ptr(params), B, R, C, S, pool, pool_s,
                                    1 if layout == "ncdhw" else 0, mean, std, _stream()), "input_pipeline")
    return y
