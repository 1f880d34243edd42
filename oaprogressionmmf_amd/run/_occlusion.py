"""Occlusion sensitivity maps (captum's Occlusion; the third `explain_fn` the reference's recipe names, never built there;
DESIGN 3.27).  A window slides over one input at a time; what it covers is set to the baseline, every other input stays, and

    delta_m[k, b] = F(x)[b, t_b] - F(x with window k of input m at the baseline)[b, t_b]
    map_m[b, i]   = mean of delta_m[k, b] over the windows k that cover element i          (summed in ascending k, fp32)

The encoders are slice-wise and an eval()-mode trunk treats every slice image on its own, so a window that touches d of a
volume's S slices changes d rows of that trunk's output and no row of any other trunk's.  The sparse pass keeps the trunk outputs
of one forward of the intact inputs and, per window, encodes only the touched slice images: koaf_occl_slices gathers them from
the stored volume, koaf_occl_rows splices their feature rows into the kept ones, the fusion transformers run as they are, and
koaf_occl_fold forms the map from the score differences.  Nothing here reads a value back to the host."""
import math

import numpy as np
import torch

from .. import ops
from ._attr import _check_chunk, _inputs, resolve_baselines
from ._explain import _forward_main, _targets
from ._gradcam import _trunks, _view_of, cam_strides, slice_dims

_SLICE_AXIS = {"rc": 3, "cs": 1, "rs": 2, "src": 1}      # the slice dimension among the extents (1, d0, d1, d2) behind the batch


def _box(shape, window, strides):
    """(dims, window, strides) as int tuples over the dimensions behind the batch; strides None = the window (no overlap)"""
    dims = tuple(int(d) for d in shape[1:])
    try:
        window = tuple(int(w) for w in window)
        strides = window if strides is None else tuple(int(s) for s in strides)
    except TypeError:
        raise ValueError(f"occlusion: window and strides are sequences with one entry per dimension behind the batch {dims}") from None
    if not 1 <= len(dims) <= 4 or len(window) != len(dims) or len(strides) != len(dims):
        raise ValueError(f"occlusion: an input of shape {tuple(shape)} takes a window and strides of {len(dims)} entries (at most 4), "
                         f"got {window} and {strides}")
    for d, w, s in zip(dims, window, strides):
        if not 1 <= s <= w <= d:
            raise ValueError(f"occlusion: 1 <= strides <= window <= extents, got strides {strides}, window {window}, extents {dims}")
    return dims, window, strides


def occlusion_windows(shape, window, strides=None):
    """-> (counts, K): the number of windows along every dimension behind the batch of an input of `shape` (B, d1, ..., dr),
    cnt_i = 1 + ceil((d_i - w_i) / s_i), and their product.  Window k -- flat, row-major over counts, the last dimension fastest --
    covers [j_i s_i, min(j_i s_i + w_i, d_i)): the last window along a dimension is clipped.  1 <= s_i <= w_i <= d_i, else a
    ValueError.  strides None: the window itself."""
    dims, window, strides = _box(shape, window, strides)
    counts = tuple(1 + -(-(d - w) // s) for d, w, s in zip(dims, window, strides))
    return counts, math.prod(counts)


def _window(shape, window, strides, k):
    """[(lo, hi)] of window k along every dimension behind the batch"""
    dims, window, strides = _box(shape, window, strides)
    counts, K = occlusion_windows(shape, window, strides)
    if not 0 <= int(k) < K:
        raise ValueError(f"occlusion: window {k} of {K}")
    js, k = [], int(k)
    for c in reversed(counts):
        js.append(k % c)
        k //= c
    return [(j * s, min(j * s + w, d)) for j, d, w, s in zip(reversed(js), dims, window, strides)]


def touched_images(view, shape, window, strides, k):
    """the indices kk in [0, K_img) of the slice images (run.slice_dims / cam_strides: what models' fold_slices hands the trunk)
    that window k of an input of `shape` intersects, ascending.  view None: a radiograph, whose one image every window touches."""
    K_img = slice_dims(view, shape)[0]
    box = _window(shape, window, strides, k)
    if view is None:
        return [0]
    lo, hi = box[_SLICE_AXIS[view]]
    assert 0 <= lo < hi <= K_img
    return list(range(lo, hi))


class _Plan:
    """what the sparse pass of one volume needs, built on the host and uploaded once: `rows` [R, 2] -- (window, image) in (k, b, kk)
    order, off[k] its first row of window k -- and src [K, N], the row of window k's chunk-local fresh features that replaces
    cached row n, or -1"""

    def __init__(self, view, shape, window, strides, K, chunk, device):
        B = int(shape[0])
        self.K_img, self.H, self.W = slice_dims(view, shape)
        self.strides4 = cam_strides(view, shape)[1:]
        N = B * self.K_img
        rows, off = [], [0]
        src = np.full((K, N), -1, dtype=np.int32)
        for k in range(K):
            t = np.asarray(touched_images(view, shape, window, strides, k), dtype=np.int32)
            n = (np.arange(B, dtype=np.int32)[:, None] * self.K_img + t[None, :]).reshape(-1)
            k0 = k // chunk * chunk
            src[k, n] = off[k] - off[k0] + np.arange(n.size, dtype=np.int32)
            rows.append(np.stack([np.full(n.size, k, dtype=np.int32), n], axis=1))
            off.append(off[k] + n.size)
        self.off = off
        self.rows = torch.from_numpy(np.concatenate(rows)).to(device)
        self.src = torch.from_numpy(src).to(device)


def _feature_rows(t):
    """a trunk output (N, C, h, w) -- an NHWC buffer viewed as NCHW -- as the contiguous rows [N, h, w, C] koaf_occl_rows copies"""
    return t.permute(0, 2, 3, 1).contiguous()


def occlusion(model, xs, target, sliding_window_shapes, strides=None, baselines=None, chunk=1, sparse=True, return_deltas=False):
    """tuple shaped like `xs` of the fp32 occlusion maps of logit[b, target_b] (module docstring); captum's Occlusion semantics with
    one perturbation target per call.  sliding_window_shapes: per input the window with one entry per dimension behind the batch,
    the channel dimension of size 1 included -- (1, h, w) for a radiograph, (1, r, c, s) for a volume, (1, f) for the clinical
    vector -- or None to skip that input (its map is None).  strides: per input as the window, or None = the window itself, i.e.
    windows that do not overlap.  THIS DEVIATES FROM CAPTUM, whose default stride is 1: on a 160 x 384 x 384 volume that default
    asks for millions of forwards.  baselines: resolve_baselines (None = zeros, a number, a tensor like the input).
    chunk: windows per model pass, folded into the batch dimension (exact in eval() mode, refused in training mode).
    sparse (default): keep the trunk outputs of the forward of the intact inputs and per window encode only the slice images it
    touches -- sum_k |touched_k| slice encodes for a volume instead of K * S, and none of the other inputs'.  Kept features are
    valid only where samples do not interact, so sparse=True needs model.eval() whatever the chunk.  sparse=False builds every
    occluded copy in full and calls the model plainly: the yardstick.  return_deltas: also the per-input (K_m, B) device tensors
    delta_m (None for a skipped input).  No parameter and no p.grad is touched; nothing is read back to the host."""
    xs_in = tuple(xs)
    M = len(xs_in)
    if sliding_window_shapes is None or len(sliding_window_shapes) != M:
        raise ValueError(f"occlusion: sliding_window_shapes has one entry per input ({M}), each a window or None")
    strides = (None,) * M if strides is None else tuple(strides)
    if len(strides) != M:
        raise ValueError(f"occlusion: strides is None or has one entry per input ({M})")
    boxes = [None if w is None else _box(x.shape, w, s)[1:] for x, w, s in zip(xs_in, sliding_window_shapes, strides)]
    Ks = [0 if bx is None else occlusion_windows(x.shape, *bx)[1] for x, bx in zip(xs_in, boxes)]
    chunk = _check_chunk(model, chunk, max(Ks + [1]))
    if sparse and model.training:
        raise ValueError("occlusion: sparse=True keeps encoder features across model passes, which is valid only where samples do not "
                         "interact: put the model in eval() mode, or use sparse=False with chunk=1")
    xs = _inputs(xs_in)
    bases = resolve_baselines(xs, baselines)
    B, dev = int(xs[0].shape[0]), xs[0].device
    tgt = _targets(target, xs)
    trunks = _trunks(model) if sparse else {}
    for i in trunks:
        if i >= M or xs[i].dim() not in (4, 5):
            raise ValueError(f"occlusion: trunk `_fe{i}` has no image input among the {M} inputs")
    views = {i: _view_of(model, xs[i]) for i in trunks}
    kimg = {i: slice_dims(views[i], xs[i].shape)[0] for i in trunks}
    cache, st, handles = {}, {"m": None}, []

    def images_of(i, mod):
        def pre(_, args, kwargs):
            """what the trunk encodes in a window pass: the touched slice images of the occluded volume, nothing of another input"""
            m = st["m"]
            if m is None or (i == m and kimg[i] == 1):
                return None                                    # the intact inputs / the dense copies of a radiograph: as given
            if i != m:
                return (args[0].new_empty((0,) + tuple(args[0].shape[1:])),) + tuple(args[1:]), kwargs
            pl, (w, s) = st["plan"], boxes[m]
            r0, r1 = pl.off[st["k0"]], pl.off[st["k0"] + st["J"]]
            imgs = ops.occl_slices(xs[m], pl.rows[r0:r1], w, s, pl.K_img, pl.H, pl.W, pl.strides4, base=bases[m])
            return (imgs,) + tuple(args[1:]), kwargs

        def forward(x, lane=None):
            return None if x.shape[0] == 0 else type(mod).forward(mod, x, lane=lane)          # no images: no encoder work at all

        def post(_, args, out):
            m = st["m"]
            if m is None:
                if i in cache:
                    raise RuntimeError("occlusion: a trunk ran twice in one forward")
                cache[i] = _feature_rows(out.detach())
                return None
            if i == m and kimg[i] == 1:
                return None
            J = st["J"]
            if i != m:
                rows = ops.occl_rows(cache[i], None, st["keep"][i][:J])
            else:
                rows = ops.occl_rows(cache[i], _feature_rows(out), st["plan"].src[st["k0"]:st["k0"] + J])
            return rows.reshape((J * rows.shape[1],) + tuple(rows.shape[2:])).permute(0, 3, 1, 2)
        return pre, forward, post

    maps, deltas = [None] * M, [None] * M
    try:
        for i, mod in trunks.items():
            pre, forward, post = images_of(i, mod)
            handles.append(mod.register_forward_pre_hook(pre, with_kwargs=True))
            handles.append(mod.register_forward_hook(post))
            mod.forward = forward
        with torch.no_grad():
            f0 = _forward_main(model, xs).float().gather(1, tgt)
            for i in trunks:
                if i not in cache:
                    raise RuntimeError(f"occlusion: trunk `_fe{i}` did not run in the forward")
            st["keep"] = {i: torch.full((chunk, c.shape[0]), -1, dtype=torch.int32, device=dev) for i, c in cache.items()}
            for m, x in enumerate(xs):
                if boxes[m] is None:
                    continue
                w, s = boxes[m]
                K = Ks[m]
                gathered = m in trunks and kimg[m] > 1           # this input's copies are never built: its slices are gathered
                if gathered:
                    st["plan"] = _Plan(views[m], x.shape, w, s, K, chunk, dev)
                delta = torch.empty((K, B), device=dev, dtype=torch.float32)
                for k0 in range(0, K, chunk):
                    J = min(chunk, K - k0)
                    st.update(m=m if sparse else None, k0=k0, J=J)
                    pts = []
                    for i, xi in enumerate(xs):
                        if i in trunks and (i != m or gathered):
                            # a trunk input the pass does not read: an element expanded to the batch of J * B the model expects
                            pts.append(xi.new_empty(1).expand((J * B,) + tuple(xi.shape[1:])))
                        elif i == m:
                            pts.append(ops.occl_points(xi, w, s, k0, J, base=bases[m]).reshape((J * B,) + tuple(xi.shape[1:])))
                        else:
                            pts.append(xi if J == 1 else xi.repeat((J,) + (1,) * (xi.dim() - 1)))
                    Fp = _forward_main(model, tuple(pts)).float().gather(1, tgt.repeat(J, 1))
                    del pts
                    delta[k0:k0 + J] = f0.reshape(1, B) - Fp.reshape(J, B)
                st["m"] = None
                deltas[m] = delta
                maps[m] = ops.occl_fold(delta, x.shape[1:], w, s)
    finally:
        for h in handles:
            h.remove()
        for mod in trunks.values():
            mod.__dict__.pop("forward", None)
    return (tuple(maps), tuple(deltas)) if return_deltas else tuple(maps)


def occlusion_totals(maps, xs):
    """(B, M) fp32 device tensor of the per-sample sums of the occlusion maps (attribution_totals); a skipped input counts 0"""
    B, dev = int(xs[0].shape[0]), xs[0].device
    cols = [torch.zeros(B, dtype=torch.float32, device=dev) if mp is None
            else ops.rowdot(mp.contiguous(), torch.ones_like(mp)) for mp in maps]
    return torch.stack(cols, dim=1)
