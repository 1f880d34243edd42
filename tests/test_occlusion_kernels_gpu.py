"""GPU: the four kernels of koaf_occl.hip against the brute force of occl_twin.py, every check with torch.equal -- the kernels
copy, select and add in a pinned order, so nothing is merely close.  Shapes are occl_twin.CASES: rows of 350, 63 and 9 elements
(no 16-byte path), 216 and 120 (the 16-byte path); clipped last windows, overlapping windows, one window that is the whole input."""
import numpy as np
import pytest
import torch

import occl_twin as T

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = {c[0]: c[1:] for c in T.CASES}


def _x(shape, salt=0):
    r = np.random.default_rng(17 + salt + sum(shape))
    return r.standard_normal(shape).astype(F32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bases(x, dev):
    """(what the op takes, what the twin takes): zeros, a constant, a tensor like x"""
    t = _x(x.shape, salt=5)
    return ((None, None), (-0.75, F32(-0.75)), (_dev(t, dev), t))


@pytest.mark.parametrize("name", list(CASES))
def test_occl_points(dev, name):
    """J = 1 and 4 (or all K windows where there are fewer), the chunk that ends at the last window and chunks with k0 > 0"""
    from oaprogressionmmf_amd import ops
    shape, window, strides, _ = CASES[name]
    x = _x(shape)
    msk = T.masks(shape, window, strides)
    K = len(msk)
    chunks = {(0, 1), (K - 1, 1), (max(K - 4, 0), min(4, K)), (K // 2, min(4, K - K // 2))}
    assert any(k0 > 0 and k0 + J == K for k0, J in chunks) or K == 1
    xd = _dev(x, dev)
    for bd, bn in _bases(x, dev):
        for k0, J in sorted(chunks):
            got = ops.occl_points(xd, window, strides, k0, J, base=bd)
            assert got.shape == (J,) + shape and got.dtype == torch.float32
            assert torch.equal(got.cpu(), torch.from_numpy(T.points(x, msk[k0:k0 + J], bn))), (name, k0, J)
    # an offset view: rows of 216 / 120 elements that are no longer 16-byte aligned take the one-element path, with the same bits
    if x[0].size % 4 == 0:
        buf = torch.empty(x.size + 1, device=dev)
        off = buf[1:].view(shape).copy_(xd)
        assert off.data_ptr() % 16 != 0
        assert torch.equal(ops.occl_points(off, window, strides, 0, 1), ops.occl_points(xd, window, strides, 0, 1))


@pytest.mark.parametrize("name,view", [(c[0], v) for c in T.CASES for v in c[4]])
def test_occl_slices(dev, name, view):
    """every image under every window (so each image repeats under several windows, touched or not), then a shuffled part of that
    table whose length is no multiple of the staged kernel's 16 rows and which ends in the middle of a sample"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.run import cam_strides
    shape, window, strides, _ = CASES[name]
    x = _x(shape, salt=1)
    msk = T.masks(shape, window, strides)
    K_img, sb, sk, si, sj = cam_strides(view, shape)
    xd = _dev(x, dev)
    for bd, bn in _bases(x, dev):
        folded = [T.fold(T.points(x, msk[k:k + 1], bn)[0], view) for k in range(len(msk))]
        H, W = folded[0].shape[1:]
        full = np.array([(k, n) for k in range(len(msk)) for n in range(shape[0] * K_img)], dtype=np.int32)
        part = np.random.default_rng(3).permutation(full)[:max(1, (len(full) * 2 // 3) | 1)]
        if K_img > 1:
            mid = K_img // 2 + (K_img if shape[0] > 1 else 0)               # the table ends half-way through a sample
            part = np.concatenate([part, [(len(msk) - 1, n) for n in range(mid)]]).astype(np.int32)
        for rows in (full, part):
            got = ops.occl_slices(xd, _dev(rows, dev), window, strides, K_img, H, W, (sb, sk, si, sj), base=bd)
            assert got.shape == (len(rows), 1, H, W)
            want = np.stack([folded[k][n] for k, n in rows])[:, None]
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (name, view)


def test_occl_slices_equal_the_models_fold(dev):
    """the same rows through models' fold_slices of the dense occluded copy: what the trunk would have received"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.models._common import fold_slices
    from oaprogressionmmf_amd.run import cam_strides, touched_images
    shape, window, strides, views = CASES["vol27"]
    xd = _dev(_x(shape, salt=2), dev)
    for view in views:
        K_img, sb, sk, si, sj = cam_strides(view, shape)
        for k in (0, 13, 26):
            imgs = fold_slices(ops.occl_points(xd, window, strides, k, 1, base=0.5)[0], view)
            n = [b * K_img + kk for b in range(shape[0]) for kk in touched_images(view, shape, window, strides, k)]
            rows = _dev(np.array([(k, i) for i in n], dtype=np.int32), dev)
            got = ops.occl_slices(xd, rows, window, strides, K_img, imgs.shape[2], imgs.shape[3], (sb, sk, si, sj), base=0.5)
            assert torch.equal(got, imgs[n]), (view, k)


@pytest.mark.parametrize("elems,dtype", [(1, torch.float32), (9, torch.float32), (2048, torch.float32), (18, torch.bfloat16)])
def test_occl_rows(dev, elems, dtype):
    """rows of 4, 36 and 8192 bytes (36: no 16-byte path; bf16 rows of 36 bytes), src all cached, all fresh, and mixed"""
    from oaprogressionmmf_amd import ops
    J, N, Fr = 3, 5, 7
    g = torch.Generator().manual_seed(elems)
    cache = torch.randn(N, 1, elems, generator=g).to(dtype)
    fresh = torch.randn(Fr, 1, elems, generator=g).to(dtype)
    r = np.random.default_rng(elems)
    mixed = r.integers(-1, Fr, size=(J, N)).astype(np.int32)
    mixed[0, 0], mixed[J - 1, N - 1] = -1, Fr - 1
    for src in (np.full((J, N), -1, dtype=np.int32), r.integers(0, Fr, size=(J, N)).astype(np.int32), mixed):
        got = ops.occl_rows(cache.to(dev), fresh.to(dev), _dev(src, dev))
        want = torch.stack([torch.stack([cache[n] if src[j, n] < 0 else fresh[src[j, n]] for n in range(N)]) for j in range(J)])
        assert got.shape == (J, N, 1, elems) and got.dtype == dtype
        assert torch.equal(got.cpu(), want)
    keep = ops.occl_rows(cache.to(dev), None, _dev(np.full((2, N), -1, dtype=np.int32), dev))
    assert torch.equal(keep.cpu(), torch.stack([cache, cache])), "no fresh rows at all: the cache replicated"


@pytest.mark.parametrize("name,counts", [("vol27", 4), ("clin", 2), ("src", 8), ("vol1", 1)])
def test_occl_fold(dev, name, counts):
    """deltas eight decades apart, so that another summation order gives other bits; an element lies under 1 ... `counts` windows
    (the 27-window volume's last dimension has window = stride, so it reaches 4; the src case overlaps along all three: 8)"""
    from oaprogressionmmf_amd import ops
    shape, window, strides, _ = CASES[name]
    msk = T.masks(shape, window, strides)
    K, B = len(msk), shape[0]
    cover = msk.sum(0)
    assert cover.min() == 1 and cover.max() == counts
    r = np.random.default_rng(K)
    delta = (r.standard_normal((K, B)) * 10.0 ** r.uniform(-4, 4, (K, B))).astype(F32)
    want = T.fold_map(delta, msk)
    got = ops.occl_fold(_dev(delta, dev), shape[1:], window, strides)
    assert got.shape == shape and torch.equal(got.cpu(), torch.from_numpy(want))
    if counts >= 4:
        back = T.fold_map(delta[::-1], msk[::-1])
        assert not np.array_equal(back, want), "the data tells summation orders apart"
