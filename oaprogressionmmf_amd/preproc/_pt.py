"""On-device "last-chance" downscale (reference: koafusion/preproc/_pt.py:175-200, called from
koafusion/run/train_prog_fus.py:111-116).  F.interpolate(scale 0.5, recompute_scale_factor=True,
align_corners=False, linear/bilinear/trilinear) on even sizes is exactly 2x average pooling -- one
HBM-bound HIP kernel here."""
import math
import random

import numpy as np
import torch

from .. import ops


class PTInterpolate(object):
    """F.interpolate(image, scale_factor, recompute_scale_factor=True, align_corners=False, mode = linear | bilinear |
    trilinear by rank) exactly as the reference's transform (preproc/_pt.py:175-200), for any scale factor: output size
    floor(in * scale) per dimension, coordinates from in / out.  The recipes' factors (0.5, 0.5[, 0.5 | 1.0]) on even
    single-channel inputs take the 2x-average-pooling kernel (identical values).  A mask raises ValueError, as in the
    reference: its mask branch hands align_corners=False to mode="nearest", which torch refuses (fixture F8 records it)."""

    def __init__(self, scale_factor):
        self.scale_factor = tuple(scale_factor) if not isinstance(scale_factor, (int, float)) else scale_factor

    def _factors(self, nd):
        sf = self.scale_factor
        if isinstance(sf, (int, float)):
            return (float(sf),) * nd
        if len(sf) != nd:
            raise ValueError(f"scale_factor {sf} does not match the {nd} spatial dimensions of the input")
        return tuple(float(v) for v in sf)

    def __call__(self, image, mask=None):
        """image: (B, CH, D0[, D1[, D2]]) device tensor -> resized image"""
        if image.ndim not in (3, 4, 5):
            raise KeyError(image.ndim)          # (the reference indexes {3: "linear", 4: "bilinear", 5: "trilinear"})
        if mask is not None:
            raise ValueError("align_corners option can only be set with the interpolating modes: linear | bilinear | bicubic | "
                             "trilinear")      # (what the reference's mask branch raises, _pt.py:193-197)
        sf = self._factors(image.ndim - 2)
        if all(s == 1.0 for s in sf):
            return image
        x = image.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        t = image
        if t.shape[1] == 1 and all(s in (0.5, 1.0) for s in sf):
            if t.ndim == 4 and sf == (0.5, 0.5) and t.shape[2] % 2 == 0 and t.shape[3] % 2 == 0:
                B, _, R, C = t.shape
                return ops.downscale2(x, B, R, C, 1, 1).view(B, 1, R // 2, C // 2)
            if t.ndim == 5 and sf[:2] == (0.5, 0.5) and t.shape[2] % 2 == 0 and t.shape[3] % 2 == 0 and (sf[2] == 1.0 or t.shape[4] % 2 == 0):
                B, _, R, C, S = t.shape
                fs = 2 if sf[2] == 0.5 else 1
                return ops.downscale2(x, B, R, C, S, fs).view(B, 1, R // 2, C // 2, S // fs)
        out_size = [int(math.floor(float(n) * s)) for n, s in zip(t.shape[2:], sf)]     # recompute_scale_factor=True
        if min(out_size) < 1:
            raise ValueError(f"scale_factor {sf} empties an input of spatial size {tuple(t.shape[2:])}")
        return ops.resize(x, out_size)


class PTBatchAugment(object):
    """The reference's per-sample tensor pipeline for one image modality
        PTToUnitRange -> PTRotate2D | PTRotate3DInSlice (prob) -> PTGammaCorrection (prob) -> PTNormalize
    (koafusion/datasets/_data_provider.py:295-335, transforms koafusion/preproc/_pt.py:75-345), applied to a whole
    BATCH already resident on the device: one min/max reduction and one fused HBM-bound kernel instead of four CPU
    passes per sample in the loader workers.  Validation / test = the same without the random parts
    (`rotate_prob = gamma_prob = 0`).

    Random state: like the reference's transforms, a rotation draws (p, theta) and a gamma correction (p, gamma) from
    Python's `random` per sample (`randomize()`, _pt.py:228-232, :305-307); `draw(B)` does that for a batch in sample
    order, or pass `states` explicitly ([(p_rot, theta_rad, p_gamma, gamma)] * B)."""

    def __init__(self, mean, std, degree_range=(-15., 15.), rotate_prob=0.5, gamma_range=(0.5, 2.0), gamma_prob=0.5,
                 clip_to_unit=False):
        if clip_to_unit:
            raise NotImplementedError("clip_to_unit=True is not built (the recipes use False)")
        self.mean = float(mean[0] if isinstance(mean, (list, tuple)) else mean)
        self.std = float(std[0] if isinstance(std, (list, tuple)) else std)
        self.theta_range = (math.radians(degree_range[0]), math.radians(degree_range[1]))
        self.rotate_prob, self.gamma_range, self.gamma_prob = rotate_prob, tuple(gamma_range), gamma_prob

    def draw(self, B):
        out = []
        for _ in range(B):
            # a transform that is not in the modality's list draws nothing (T2 maps have no gamma correction,
            # validation has neither: _data_provider.py:304-309,341-360), so the host RNG stream stays the reference's
            p_rot, theta = (random.random(), random.uniform(*self.theta_range)) if self.rotate_prob > 0 else (1.0, 0.0)
            p_gam, gamma = (random.random(), random.uniform(*self.gamma_range)) if self.gamma_prob > 0 else (1.0, 1.0)
            out.append((p_rot, theta, p_gam, gamma))
        return out

    def __call__(self, image, states=None):
        """image: (B, 1, R, C) or (B, 1, R, C, S) raw intensities on the device -> same shape, float32.  Integer volumes
        (uint8 radiographs, uint16 / int16 MRI, as stored on disk) are taken as they are -- 4x / 2x fewer PCIe bytes than
        the fp32 tensors of the reference's loader workers -- and widened on the device (koaf_widen)."""
        if image.ndim not in (4, 5) or image.shape[1] != 1:
            raise ValueError(f"Unsupported tensor shape: {tuple(image.shape)}")
        B, _, R, C = image.shape[:4]
        S = image.shape[4] if image.ndim == 5 else 1
        x = ops.widen(image) if image.dtype in (torch.uint8, torch.uint16, torch.int16) else image.contiguous().float()
        states = self.draw(B) if states is None else list(states)
        if len(states) != B:
            raise ValueError("one (p_rot, theta, p_gamma, gamma) tuple per sample")
        prm = []
        for p_rot, theta, p_gam, gamma in states:
            rot = p_rot < self.rotate_prob
            gam = p_gam < self.gamma_prob
            prm.append([math.cos(theta) if rot else 1.0, math.sin(theta) if rot else 0.0,
                        (1.0 / gamma) if gam else 0.0, 1.0 if rot else 0.0])
        prm = torch.tensor(prm, dtype=torch.float32).to(x.device)
        return ops.augment(x, ops.minmax(x, B), prm, B, R, C, S, self.mean, self.std)


def crop_geometry(in_shape, out_size, ratios=None, flip_axis=None):
    """Where the reference's `np.flip(image, axis=flip_axis)` -> RandomCrop | CenterCrop window lies in the STORED volume
    (datasets/oai/_dataset.py:298-321, preproc/_np_nd.py:62-144) -- pure host arithmetic, nothing is copied.

    in_shape: the stored spatial extents (d0, d1[, d2]); out_size: the crop size (an int: every axis); ratios: the RandomCrop
    state, one value in [0, 1) per axis (start = floor(ratio * (in - out)), _np_nd.py:91), or None for the CenterCrop
    ((in - out) // 2, :133); flip_axis: the axis of the reference's (ch, d0, ...) array that np.flip reverses (2 for COR_IW_TSE /
    XR_PA, -1 for SAG_3D_DESS / SAG_T2_MAP), or None.  The crop is taken AFTER the flip, so index i of a flipped axis of length N
    is stored index N - 1 - i.
    -> (origin, backwards): the stored index of window voxel 0 per axis, and the bit mask (1 << axis) of the axes the window
    walks backwards: window voxel i along an axis is stored index origin + i, or origin - i on a backwards axis."""
    ds_in = tuple(int(v) for v in in_shape)
    nd = len(ds_in)
    ds_out = (int(out_size),) * nd if isinstance(out_size, int) else tuple(int(v) for v in out_size)
    if len(ds_out) != nd:
        raise ValueError(f"crop size {ds_out!r} does not match the {nd} spatial dimensions of the input")
    for d_in, d_out in zip(ds_in, ds_out):
        if d_in < d_out:
            raise ValueError(f"Invalid crop size {ds_out!r} for input {ds_in!r}")
    if ratios is not None and len(ratios) != nd:
        raise ValueError(f"one crop ratio per spatial dimension, got {len(ratios)} for {nd}")
    flipped = None
    if flip_axis is not None:
        flipped = flip_axis - 1 if flip_axis >= 0 else nd + flip_axis        # (axis 0 of the reference's array is the channel)
        if not 0 <= flipped < nd:
            raise ValueError(f"flip_axis {flip_axis} is not a spatial axis of a (ch, {nd} x d) array")
    origin, back = [], 0
    for d in range(nd):
        start = (ds_in[d] - ds_out[d]) // 2 if ratios is None else math.floor(ratios[d] * (ds_in[d] - ds_out[d]))
        if d == flipped:
            origin.append(ds_in[d] - 1 - start)
            back |= 1 << d
        else:
            origin.append(start)
    return tuple(origin), back


_POOLED = {(0.5, 0.5): (2, 1), (0.5, 0.5, 0.5): (2, 2), (0.5, 0.5, 1.0): (2, 1)}


class PTBatchPipeline(object):
    """One image modality from the volumes AS STORED to the tensor the model consumes, on the device:
        np.flip (RIGHT knees) -> RandomCrop | CenterCrop -> NumpyToTensor -> PTToUnitRange (of the cropped window)
        -> PTRotate2D | PTRotate3DInSlice (prob) -> PTGammaCorrection (prob) -> PTNormalize -> PTInterpolate(scale_factor)
    (datasets/oai/_dataset.py:298-321, datasets/_data_provider.py:295-418, run/train_prog_fus.py:111-116) in two library calls (three kernels) that
    read the stored integers in place (ops.window_minmax, ops.input_pipeline): no flipped, cropped, stacked or widened copy on
    either side of PCIe.  Stored volumes are ragged (the dataset only checks shape >= the crop), so a batch may be a list of
    one tensor per sample.  Validation / test: `random_crop=False, rotate_prob=0, gamma_prob=0`.

    Random state, per sample and in the reference's transform order: the RandomCrop ratios (one random.random() per spatial
    axis), the rotation (p, theta), the gamma correction (p, gamma) -- the calls the reference's randomize() methods make
    (_np_nd.py:104-106, _pt.py:228-232, :305-307).  theta is drawn as the reference draws it, between the float32 bounds
    torch.deg2rad leaves and in float32, so that a seeded run reproduces the reference's recorded states exactly.  `draw(B)` does
    that for a batch, or pass `states` ([(ratios | None, p_rot, theta_rad, p_gamma, gamma)] * B)."""

    def __init__(self, crop_size, mean, std, flip_axis=None, random_crop=True, degree_range=(-15., 15.), rotate_prob=0.5,
                 gamma_range=(0.5, 2.0), gamma_prob=0.5, scale_factor=None, layout="rcs", clip_to_unit=False):
        if clip_to_unit:
            raise NotImplementedError("clip_to_unit=True is not built (the recipes use False)")
        self.crop_size = tuple(int(v) for v in crop_size)
        if len(self.crop_size) not in (2, 3):
            raise ValueError(f"crop_size is (R, C) or (R, C, S), got {crop_size!r}")
        if layout not in ("rcs", "ncdhw"):
            raise ValueError(f"layout is 'rcs' or 'ncdhw', got {layout!r}")
        self.mean = float(mean[0] if isinstance(mean, (list, tuple)) else mean)
        self.std = float(std[0] if isinstance(std, (list, tuple)) else std)
        self.flip_axis, self.random_crop, self.layout = flip_axis, bool(random_crop), layout
        self.theta_range = torch.deg2rad(torch.Tensor([float(degree_range[0]), float(degree_range[1])]))    # (_pt.py:259, :312)
        self.rotate_prob, self.gamma_range, self.gamma_prob = rotate_prob, tuple(gamma_range), gamma_prob
        nd = len(self.crop_size)
        if scale_factor is None or isinstance(scale_factor, (int, float)):
            sf = (1.0 if scale_factor is None else float(scale_factor),) * nd
        else:
            sf = tuple(float(v) for v in scale_factor)
        if len(sf) != nd:
            raise ValueError(f"scale_factor {scale_factor} does not match the {nd} spatial dimensions of the crop")
        self.scale_factor = sf
        # (pool, pool_s) of the fused pass; (0, 0): unpooled, then koaf_resize
        pools = (1, 1) if all(v == 1.0 for v in sf) else _POOLED.get(sf, (0, 0))
        self._pools = pools if all(n % 2 == 0 for n, v in zip(self.crop_size, sf) if v == 0.5) else (0, 0)
        self._static = not self.random_crop and not rotate_prob > 0 and not gamma_prob > 0       # nothing is drawn
        self._tables = {}

    def draw(self, B):
        nd, out = len(self.crop_size), []
        for _ in range(B):
            # a transform that is not in the modality's list draws nothing, so the host RNG stream stays the reference's
            ratios = tuple(random.random() for _ in range(nd)) if self.random_crop else None
            p_rot, theta = (random.random(), float(random.uniform(*self.theta_range))) if self.rotate_prob > 0 else (1.0, 0.0)
            p_gam, gamma = (random.random(), random.uniform(*self.gamma_range)) if self.gamma_prob > 0 else (1.0, 1.0)
            out.append((ratios, p_rot, theta, p_gam, gamma))
        return out

    def geometry(self, shapes, ratios, flip=None):
        """crop_geometry for a whole batch at once, in numpy (the same float64 products and floors): shapes [B][nd] stored
        extents, ratios one tuple per sample (ignored unless random_crop), flip per-sample booleans or None
        -> (origins int64 [B][nd], backwards masks int64 [B])"""
        shapes = np.asarray(shapes, dtype=np.int64)
        B, nd = shapes.shape
        out = np.asarray(self.crop_size, dtype=np.int64)
        if nd != len(out):
            raise ValueError(f"crop size {self.crop_size!r} does not match the {nd} spatial dimensions of the input")
        if (shapes < out).any():
            b = int(np.argmax((shapes < out).any(1)))
            raise ValueError(f"Invalid crop size {self.crop_size!r} for input {tuple(int(v) for v in shapes[b])!r}")
        if self.random_crop:
            if any(r is None for r in ratios):
                raise ValueError("random_crop=True needs the crop ratios of every sample")
            start = np.floor(np.array(ratios, dtype=np.float64).reshape(B, nd) * (shapes - out)).astype(np.int64)
        else:
            start = (shapes - out) // 2
        masks = np.zeros(B, dtype=np.int64)
        if flip is not None and self.flip_axis is not None:
            fd = self.flip_axis - 1 if self.flip_axis >= 0 else nd + self.flip_axis
            if not 0 <= fd < nd:
                raise ValueError(f"flip_axis {self.flip_axis} is not a spatial axis of a (ch, {nd} x d) array")
            fl = np.asarray(flip, dtype=bool)
            start[fl, fd] = shapes[fl, fd] - 1 - start[fl, fd]
            masks[fl] = 1 << fd
        return start, masks

    def __call__(self, images, flip=None, states=None):
        """images: a (B, 1, R0, C0[, S0]) device tensor, or a list of B device tensors (1, R0_b, C0_b[, S0_b]) of differing
        stored shapes -- fp32, uint8, uint16 or int16, one dtype for the batch; flip: per-sample booleans (side == RIGHT)
        -> (B, 1, R', C'[, S']) float32, or (B, 1, S', R', C') for layout="ncdhw"."""
        nd = len(self.crop_size)
        dense = torch.is_tensor(images)
        if dense:
            if images.ndim != nd + 2 or images.shape[1] != 1:
                raise ValueError(f"Unsupported tensor shape: {tuple(images.shape)}")
            vols = images.contiguous()
            B = int(vols.shape[0])
        else:
            vols = [v.contiguous() for v in images]
            for v in vols:
                if v.ndim != nd + 1 or v.shape[0] != 1:
                    raise ValueError(f"Unsupported tensor shape: {tuple(v.shape)}")
            B = len(vols)
        if flip is not None and len(flip) != B:
            raise ValueError("one flip flag per sample")
        if self._static:
            # nothing random (validation / test): the table depends on the stored shapes and the flip pattern only -- built and
            # checked once, then only the addresses change from batch to batch
            key = (tuple(vols.shape) if dense else tuple(tuple(v.shape) for v in vols), (vols if dense else vols[0]).dtype,
                   None if flip is None else tuple(bool(f) for f in flip))
            host = self._tables.get(key)
            if host is None:
                if len(self._tables) >= 64:
                    self._tables.clear()
                host = self._tables[key] = self._host_table(vols, dense, B, flip, [(None, 1.0, 0.0, 1.0, 1.0)] * B)
        else:
            states = self.draw(B) if states is None else list(states)
            if len(states) != B:
                raise ValueError("one (ratios, p_rot, theta, p_gamma, gamma) tuple per sample")
            host = self._host_table(vols, dense, B, flip, states)
        table, dtype, win, prm = host.upload(vols)                                     # one small copy
        mm = ops.window_minmax(table, dtype, win)
        pool, pool_s = self._pools
        if pool:
            y = ops.input_pipeline(table, dtype, win, mm, prm, self.mean, self.std, pool, pool_s, self.layout if nd == 3 else "rcs")
            return y.unsqueeze(1) if nd == 3 else y.view(B, 1, y.shape[1], y.shape[2])
        # any other factor, or an odd size: the fused pass unpooled, then the general resize (what PTInterpolate accepts)
        y = ops.input_pipeline(table, dtype, win, mm, prm, self.mean, self.std, 1, 1, "rcs")
        out_size = [int(math.floor(float(n) * s)) for n, s in zip(self.crop_size, self.scale_factor)]     # recompute_scale_factor=True
        if min(out_size) < 1:
            raise ValueError(f"scale_factor {self.scale_factor} empties a crop of size {self.crop_size}")
        y = ops.resize(y.view((B, 1) + self.crop_size), out_size)
        if nd == 3 and self.layout == "ncdhw":
            R, C, S = out_size
            y = ops.slice_fold(y, B, R, C, S).view(B, 1, S, R, C)
        return y

    def _host_table(self, vols, dense, B, flip, states):
        """geometry and augmentation parameters of one batch -> the checked host table (ops.window_rows)"""
        nd = len(self.crop_size)
        if dense:
            shapes = np.empty((B, nd), dtype=np.int64)
            shapes[:] = tuple(vols.shape[2:])
        else:
            shapes = np.array([tuple(v.shape[1:]) for v in vols], dtype=np.int64).reshape(B, nd)
        start, masks = self.geometry(shapes, [st[0] for st in states], flip)
        aug = np.array([st[1:] for st in states], dtype=np.float64).reshape(B, 4)            # p_rot, theta, p_gamma, gamma
        rot, gam = aug[:, 0] < self.rotate_prob, aug[:, 2] < self.gamma_prob
        prm = np.zeros((B, 4), dtype=np.float32)                                             # cos, sin, exponent or 0, rotated
        prm[:, 0] = 1.0
        if rot.any():
            prm[rot, 0], prm[rot, 1], prm[rot, 3] = np.cos(aug[rot, 1]), np.sin(aug[rot, 1]), 1.0
        if gam.any():
            prm[gam, 2] = 1.0 / aug[gam, 3]
        return ops.window_rows(vols, start, masks, self.crop_size, params=prm)


def _is_tensor_list(v):
    return isinstance(v, (list, tuple)) and len(v) > 0 and all(torch.is_tensor(t) for t in v)


class PinnedPrefetcher(object):
    """Host -> device upload of the next batch while the current step runs (the input side of _data_provider.py:460-498,
    whose DataLoader hands over pageable fp32 tensors): every tensor of a batch dict is staged in a pinned host buffer
    (two sets, reused) and copied on a dedicated HIP stream with non_blocking=True; `next()` makes the caller's stream
    wait for that copy only.  Integer volumes stay integer across PCIe (PTBatchAugment widens them on the device).  A value
    that is a list or tuple of tensors -- what a collate function returns for ragged stored volumes (PTBatchPipeline) -- is
    staged in one flat pinned block per key (the shapes change from batch to batch; the block grows to the largest batch seen
    and is reused), uploaded element by element, and arrives as the same kind of sequence.

        for batch in PinnedPrefetcher(loader, device): ...      # batch: same keys, device tensors (non-tensors pass through)
    """

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PinnedPrefetcher uploads to a HIP device")
        self.stream = torch.cuda.Stream(device=self.device)
        self._pinned = [{}, {}]
        self._done = [None, None]      # upload-finished event of the batch that last used each pinned set
        self._turn = 0

    def _stage(self, batch):
        turn = self._turn
        bufs, out = self._pinned[turn], {}
        self._turn ^= 1
        if self._done[turn] is not None:
            self._done[turn].synchronize()         # its previous upload has left the pinned buffers
        with torch.cuda.stream(self.stream):
            def upload(key, v):
                pb = bufs.get(key)
                if pb is None or pb.shape != v.shape or pb.dtype != v.dtype:
                    pb = bufs[key] = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                pb.copy_(v)
                return pb.to(self.device, non_blocking=True)

            def upload_list(key, vs):
                # shapes differ from batch to batch, so the elements share ONE flat pinned block per key, grown to the largest
                # batch seen and reused; each element is staged at a 16-byte offset of it and copied from there
                offs, total = [], 0
                for t in vs:
                    offs.append(total)
                    total += -(-t.numel() * t.element_size() // 16) * 16
                pb = bufs.get((key, "flat"))
                if pb is None or pb.numel() < total:
                    pb = bufs[(key, "flat")] = torch.empty(total, dtype=torch.uint8, pin_memory=True)
                res = []
                for t, o in zip(vs, offs):
                    stage = pb[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
                    stage.copy_(t)
                    res.append(stage.to(self.device, non_blocking=True))
                return res

            for k, v in batch.items():
                if torch.is_tensor(v):
                    out[k] = upload(k, v)
                elif _is_tensor_list(v):         # ragged stored volumes, one tensor per sample: element by element
                    out[k] = type(v)(upload_list(k, v))
                else:
                    out[k] = v
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self._done[turn] = ev
        return out, ev

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur, ev = nxt
            try:
                nxt = self._stage(next(it))          # the NEXT batch travels while the caller works on `cur`
            except StopIteration:
                nxt = None
            torch.cuda.current_stream(self.device).wait_event(ev)
            for v in cur.values():
                for t in ([v] if torch.is_tensor(v) else v if _is_tensor_list(v) else ()):
                    t.record_stream(torch.cuda.current_stream(self.device))
            yield cur
