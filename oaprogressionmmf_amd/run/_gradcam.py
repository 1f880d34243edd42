"""Grad-CAM volumes of the slice-wise encoders (not in the reference; the lab's earlier progression model was published with
such maps).  Every trunk ends in a global average pool in front of the tokens, so the gradient of a logit with respect to the
last feature map A is spatially constant, g[n, c] / HW with g the gradient with respect to the pooled token, and the map is

    cam[n, y, x] = sum_c A[n, y, x, c] * g[n, c] / HW

one per slice, stacked into a volume.  One forward that keeps no trunk activation but the last feature map, and the backward of
the fusion transformers only: the autograd graph is cut at the trunk outputs.  koaf_cam forms the maps, koaf_cam_upsample resizes
them to the slice size, normalises them and writes them in the layout the model received -- no arithmetic runs in torch ops."""
import re
from typing import NamedTuple

import torch

from .. import ops
from ..models import KoafTrunk
from ..models._common import mr_view
from ._explain import _forward_main, _targets

VIEWS = ("rc", "src", "cs", "rs")


class GradCam(NamedTuple):
    """map: shaped like the input ((B, K, h, w) with upsample=False); slice_scores (B, K): the sum of the un-normalised
    low-resolution map of every slice"""
    map: torch.Tensor
    slice_scores: torch.Tensor


def slice_dims(view, shape):
    """(K slices per sample, slice rows, slice columns) of an input of `shape` under `view` (None: a 2-D radiograph (B,1,H,W);
    rc / cs / rs: (B,1,R,C,S) volumes; src: a slice-major (B,1,S,R,C) volume) -- models/_common.fold_slices' images"""
    shape = tuple(int(s) for s in shape)
    if view is None:
        if len(shape) != 4 or shape[1] != 1:
            raise ValueError(f"a radiograph is (B, 1, H, W), got {shape}")
        return 1, shape[2], shape[3]
    if view not in VIEWS:
        raise ValueError(f"Unknown view: {view}")
    if len(shape) != 5 or shape[1] != 1:
        raise ValueError(f"a volume is (B, 1, d0, d1, d2), got {shape}")
    if view == "src":
        S, R, C = shape[2:]
        return S, R, C
    R, C, S = shape[2:]
    return {"rc": (S, R, C), "cs": (R, C, S), "rs": (C, R, S)}[view]


def cam_strides(view, volume_shape):
    """(K, sb, sk, si, sj): pixel (i, j) of slice image n = b * K + k, as the trunk receives the folded input, is element
    b * sb + k * sk + i * si + j * sj of the input tensor (strides in elements; sk is unused for a radiograph, K = 1).
    The inverse of models/_common.fold_slices."""
    K, H, W = slice_dims(view, volume_shape)
    sb = K * H * W
    if view is None:
        return K, sb, sb, W, 1
    if view == "src":
        return K, sb, H * W, W, 1
    R, C, S = (int(s) for s in volume_shape[2:])
    sk, si, sj = {"rc": (1, C * S, S), "cs": (C * S, S, 1), "rs": (S, C * S, 1)}[view]
    return K, sb, sk, si, sj


def _trunks(model):
    """{input position: trunk} over every KoafTrunk of the model.  The registry models hold the trunk of input i as the direct
    child `_fe{i}` (`_fe`: the only image input); a trunk anywhere else cannot be tied to an input and is refused, not skipped"""
    found = {}
    for name, mod in model.named_modules(remove_duplicate=False):
        if not isinstance(mod, KoafTrunk):
            continue
        m = re.fullmatch(r"_fe(\d*)", name)
        if not m:
            raise ValueError(f"gradcam: trunk `{name}` is not a `_fe` / `_fe{{i}}` child of the model: no input to map it to")
        found[int(m.group(1) or 0)] = mod
    if not found:
        raise ValueError("gradcam: the model has no encoder trunk (`_fe` / `_fe{i}` KoafTrunk children)")
    if len(set(map(id, found.values()))) != len(found):
        raise ValueError("gradcam: one trunk serves several inputs")
    return found


def _view_of(model, x):
    if x.dim() == 4:
        return None
    from ..models._mrN_cnn_trf import MR1CnnTrf
    return model.config["fe"]["dims_view"] if isinstance(model, MR1CnnTrf) else mr_view(model.config)


def gradcam(model, xs, target, *, relu=True, normalize="sample", upsample=True):
    """Grad-CAM of logit[b, target_b] at the last feature map of every encoder trunk, in whatever mode the model is in
    (explanations: eval()).  Returns a tuple shaped like `xs`: None for an input without a trunk (the clinical vector), else a
    GradCam with `.map` shaped like that input -- the slice maps resized to the slice size and laid out as the volume; with
    upsample=False the (B, K, h, w) low-resolution maps -- and `.slice_scores` (B, K), the sum of each slice's un-normalised
    low-resolution map.  relu: clamp the maps at 0 (False: signed maps).  normalize: "sample" divides by the largest magnitude of
    the sample's K slice maps, "image" by each slice's own, None leaves the values.  Parameters are frozen for the call and the
    inputs ask for no gradient: the trunks keep nothing for backward, no p.grad is touched.  Every KoafTrunk of the model is hooked;
    the trunk of input i must be the model's direct child `_fe{i}` (`_fe`: the only image input), as in the registry models -- a trunk
    nested deeper or named otherwise raises a ValueError."""
    if normalize not in ops.CAM_NORMALIZE:
        raise ValueError(f"Unknown normalize: {normalize}")
    xs = tuple(xs)
    trunks = _trunks(model)
    for i in trunks:
        if i >= len(xs) or xs[i].dim() not in (4, 5):
            raise ValueError(f"gradcam: trunk `_fe{i}` has no image input among the {len(xs)} inputs")
    tgt = _targets(target, xs)
    calls = {}                      # trunk -> (leaf, features, input shape); filled by the hooks in call order

    def hook(mod, args, out):
        if mod in calls:
            raise RuntimeError("gradcam: a trunk ran twice in one forward")
        leaf = out.detach().requires_grad_(True)
        calls[mod] = (leaf, mod.features, tuple(args[0].shape))
        mod.features = None
        return leaf

    params = [p for p in model.parameters() if p.requires_grad]
    handles = []
    try:
        for p in params:
            p.requires_grad_(False)
        for tr in trunks.values():
            tr.keep_features = True
            handles.append(tr.register_forward_hook(hook))
        with torch.enable_grad():
            sel = _forward_main(model, tuple(x.detach() for x in xs)).gather(1, tgt).sum()
            order = [i for i in sorted(trunks) if trunks[i] in calls]
            grads = torch.autograd.grad(sel, [calls[trunks[i]][0] for i in order])
    finally:
        for h in handles:
            h.remove()
        for tr in trunks.values():
            tr.__dict__.pop("keep_features", None)
            tr.__dict__.pop("features", None)
        for p in params:
            p.requires_grad_(True)
    res = [None] * len(xs)
    for i, g in zip(order, grads):
        _, (A, N, h, w, C), in_shape = calls[trunks[i]]
        x = xs[i]
        view = _view_of(model, x)
        K, H, W = slice_dims(view, x.shape)
        B = int(x.shape[0])
        if (N, H, W) != (B * K, in_shape[-2], in_shape[-1]):
            raise RuntimeError(f"gradcam: trunk `_fe{i}` received {in_shape}, input {i} folds to {(B * K, 1, H, W)} (view {view})")
        g = g.detach()
        g.record_stream(torch.cuda.current_stream())      # (it may come from an encoder lane's pool; it is read on this stream)
        if tuple(g.shape[2:]) == (1, 1):
            # behind the GAP the gradient of every pixel is g / HW (koaf_grad_fold mode 0: wv = (1 / HW) * g)
            wv = torch.empty(N * C, device=g.device, dtype=torch.float32)
            ops.grad_fold(wv, g.reshape(N * C).contiguous(), 1.0 / (h * w), 0)
        else:
            # with_gap false: the leaf is the (N, C, h, w) view of the map; the weights are the spatial mean of its gradient
            wv = ops.gap_fwd(g.permute(0, 2, 3, 1).contiguous(), N, h * w, C)
        low, img_sum, img_max = ops.cam(A, wv, N, h * w, C, relu=relu)
        if upsample:
            out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
            ops.cam_upsample(low, img_max, out, B, K, h, w, H, W, cam_strides(view, x.shape)[1:], normalize)
        elif normalize is None:
            out = low.view(B, K, h, w)
        else:
            out = torch.empty((B, K, h, w), device=x.device, dtype=torch.float32)
            ops.cam_upsample(low, img_max, out, B, K, h, w, h, w, (K * h * w, h * w, w, 1), normalize)
        res[i] = GradCam(out, img_sum.view(B, K))
    return tuple(res)
