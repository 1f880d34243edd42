"""numpy restatement of the occlusion maps (run/_occlusion.py, koaf_occl.hip), by brute force: a boolean mask per window, the
occluded copies by np.where, the touched slice images by folding the mask as the models fold a volume, the map by a loop over the
windows in order in fp32.  Nothing here uses a closed form the code under test uses."""
import itertools

import numpy as np

# the cases of the issue: (name, input shape with its batch, window, strides, views to fold it under)
CASES = (
    ("vol27", (2, 1, 10, 7, 5), (1, 4, 3, 2), (1, 3, 2, 2), ("rc", "cs", "rs", "src")),
    ("vol1", (1, 1, 6, 5, 4), (1, 6, 5, 4), (1, 6, 5, 4), ("rc", "cs", "rs", "src")),
    ("src", (2, 1, 4, 6, 9), (1, 2, 4, 4), (1, 1, 3, 3), ("src",)),          # overlap along all three: up to 8 windows an element
    ("xr", (2, 1, 9, 7), (1, 4, 4), (1, 3, 4), (None,)),
    ("clin", (2, 1, 9), (1, 4), (1, 3), ()),
)


def starts(d, w, s):
    """the window starts along one dimension: step s until a window reaches the end"""
    out, lo = [], 0
    while True:
        out.append(lo)
        if lo + w >= d:
            return out
        lo += s


def masks(shape, window, strides):
    """[K, *shape[1:]] booleans: mask k is True where window k covers (row-major over the dimensions, the last one fastest)"""
    dims = tuple(shape[1:])
    per_dim = [starts(d, w, s) for d, w, s in zip(dims, window, strides)]
    out = []
    for los in itertools.product(*per_dim):
        m = np.zeros(dims, dtype=bool)
        m[tuple(slice(lo, lo + w) for lo, w in zip(los, window))] = True       # (numpy clips the slice at the end)
        out.append(m)
    return np.stack(out)


def points(x, msk, base=None):
    """[J, *x.shape]: x with the elements under mask j replaced by the baseline (None = 0, a number, or an array like x)"""
    b = np.zeros_like(x) if base is None else np.broadcast_to(np.asarray(base, dtype=x.dtype), x.shape)
    return np.stack([np.where(m[None], b, x) for m in msk])


def fold(x, view):
    """the image batch [B * K, H, W] the models' fold_slices makes of x (view None: a radiograph (B, 1, H, W))"""
    if view is None:
        return x.reshape((x.shape[0],) + x.shape[2:])
    v = x[:, 0]
    if view == "rc":                     # (B, R, C, S) -> (B, S, R, C)
        v = v.transpose(0, 3, 1, 2)
    elif view == "rs":                   # (B, R, C, S) -> (B, C, R, S)
        v = v.transpose(0, 2, 1, 3)
    elif view not in ("cs", "src"):      # (B, R, C, S) / (B, S, R, C) as they lie
        raise ValueError(view)
    return np.ascontiguousarray(v).reshape((-1,) + v.shape[2:])


def touched(msk_k, view):
    """the slice images window mask msk_k [*shape[1:]] intersects, ascending"""
    return np.flatnonzero(fold(msk_k[None], view).any(axis=(1, 2))).tolist()


def fold_map(delta, msk):
    """map [B, *dims] from delta [K, B] (fp32): the covering windows' deltas added in ascending k in fp32, one fp32 division"""
    delta = np.asarray(delta, dtype=np.float32)
    K, B = delta.shape
    s = np.zeros((B,) + msk.shape[1:], dtype=np.float32)
    cnt = np.zeros(msk.shape[1:], dtype=np.int32)
    for k in range(K):
        for b in range(B):
            s[b][msk[k]] = s[b][msk[k]] + delta[k, b]
        cnt += msk[k]
    assert cnt.min() >= 1
    return s / cnt.astype(np.float32)[None]
