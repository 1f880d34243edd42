"""CPU: the host side of the occlusion maps (run.occlusion, run/_occlusion.py).  The window arithmetic and the touched slice images
against the brute force of occl_twin.py; the refusals that need no device; the four entry points as koaf.h declares them, bound
by the library at the unchanged ABI version; and the Python route -- chunking through the batch dimension, the deltas, the fold,
the explain_epoch plumbing -- on a stub model with the two dense ops replaced by the twin."""
import ctypes

import numpy as np
import pytest
import torch

import occl_twin as T


@pytest.mark.parametrize("name,shape,window,strides,views", T.CASES, ids=[c[0] for c in T.CASES])
def test_windows_and_touched_images_equal_the_brute_force(name, shape, window, strides, views):
    from oaprogressionmmf_amd.run import cam_strides, occlusion_windows, touched_images
    from oaprogressionmmf_amd.run._occlusion import _window
    msk = T.masks(shape, window, strides)
    counts, K = occlusion_windows(shape, window, strides)
    assert counts == tuple(len(T.starts(d, w, s)) for d, w, s in zip(shape[1:], window, strides))
    assert K == len(msk) == int(np.prod(counts))
    for k in range(K):                                    # the closed-form box of window k is the mask, in the same order
        m = np.zeros(shape[1:], dtype=bool)
        m[tuple(slice(lo, hi) for lo, hi in _window(shape, window, strides, k))] = True
        assert np.array_equal(m, msk[k]), (name, k)
    for view in views:
        K_img = cam_strides(view, shape)[0]
        for k in range(K):
            got = touched_images(view, shape, window, strides, k)
            assert got == T.touched(msk[k], view), (name, view, k)
            assert all(0 <= kk < K_img for kk in got)
    for view in views:
        with pytest.raises(ValueError, match=f"window {K} of {K}"):
            touched_images(view, shape, window, strides, K)


def test_known_window_counts():
    from oaprogressionmmf_amd.run import occlusion_windows
    assert occlusion_windows((2, 1, 10, 7, 5), (1, 4, 3, 2), (1, 3, 2, 2)) == ((1, 3, 3, 3), 27)
    assert occlusion_windows((1, 1, 6, 5, 4), (1, 6, 5, 4), (1, 6, 5, 4)) == ((1, 1, 1, 1), 1)
    assert occlusion_windows((2, 1, 9), (1, 4), (1, 3)) == ((1, 3), 3)
    assert [T.starts(9, 4, 3)[j] for j in range(3)] == [0, 3, 6]                    # windows [0,4) [3,7) [6,9)
    assert occlusion_windows((2, 1, 9), (1, 4)) == ((1, 3), 3), "strides None: the window itself -- [0,4) [4,8) [8,9)"
    # the product shapes of the issue: 160 x 384 x 384 under 16 x 32 x 32 windows
    assert occlusion_windows((1, 1, 160, 384, 384), (1, 16, 32, 32))[1] == 1440


def test_refusals():
    from oaprogressionmmf_amd.run import occlusion, occlusion_windows, touched_images
    shape = (2, 1, 10, 7, 5)
    with pytest.raises(ValueError, match="strides <= window"):
        occlusion_windows(shape, (1, 4, 3, 2), (1, 5, 2, 2))                       # s > w
    with pytest.raises(ValueError, match="window <= extents"):
        occlusion_windows(shape, (1, 4, 8, 2), (1, 3, 2, 2))                       # w > d
    with pytest.raises(ValueError, match="1 <= strides"):
        occlusion_windows(shape, (1, 4, 3, 2), (1, 0, 2, 2))
    for bad in ((4, 3, 2), (1, 1, 4, 3, 2), 4):                                    # wrong rank
        with pytest.raises(ValueError, match="entr"):
            occlusion_windows(shape, bad, None)
    with pytest.raises(ValueError, match="entries"):
        occlusion_windows(shape, (1, 4, 3, 2), (3, 2, 2))
    with pytest.raises(ValueError, match="Unknown view"):
        touched_images("sr", shape, (1, 4, 3, 2), None, 0)
    m, (xs, y) = _stub(), _inputs()
    m.train()
    with pytest.raises(ValueError, match="eval\\(\\)"):
        occlusion(m, xs, y, [(1, 2, 2), (1, 4)], sparse=True)                      # whatever the chunk
    with pytest.raises(ValueError, match="eval\\(\\)"):
        occlusion(m, xs, y, [(1, 2, 2), (1, 4)], sparse=False, chunk=2)
    m.eval()
    with pytest.raises(ValueError, match="encoder trunk"):
        occlusion(m, xs, y, [(1, 2, 2), (1, 4)])                                   # sparse needs trunks to cache, as gradcam finds them
    with pytest.raises(ValueError, match="one entry per input"):
        occlusion(m, xs, y, [(1, 2, 2)], sparse=False)
    with pytest.raises(ValueError, match="chunk"):
        occlusion(m, xs, y, [(1, 2, 2), (1, 4)], sparse=False, chunk=65)
    with pytest.raises(ValueError, match="window <= extents"):
        occlusion(m, xs, y, [(1, 5, 2), None], sparse=False)
    assert m.calls == [], "every refusal comes ahead of the first model pass"


def test_occl_entry_points_are_declared_and_built():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    P, I, L, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    # koaf_occl_points(x, base, base_value, out, J, B, dims, win, str, k0, stream)
    assert protos["koaf_occl_points"] == (ctypes.c_int, [P, P, F, P, I, I, P, P, P, I, P])
    # koaf_occl_slices(x, base, base_value, out, rows, nrows, B, dims, win, str, K_img, H, W, sb, sk, si, sj, stream)
    assert protos["koaf_occl_slices"] == (ctypes.c_int, [P, P, F, P, P, I, I, P, P, P, I, I, I, L, L, L, L, P])
    # koaf_occl_rows(cache, fresh, src, out, J, N, F, row_bytes, stream)
    assert protos["koaf_occl_rows"] == (ctypes.c_int, [P, P, P, P, I, I, I, L, P])
    # koaf_occl_fold(delta, out, K, B, dims, win, str, stream)
    assert protos["koaf_occl_fold"] == (ctypes.c_int, [P, P, I, I, P, P, P, P])
    assert _lib.defines()["KOAF_VERSION"] == 200
    handle = _lib.lib()                            # (binds every declared symbol: a library without the four fails here)
    for name in ("koaf_occl_points", "koaf_occl_slices", "koaf_occl_rows", "koaf_occl_fold"):
        assert getattr(handle, name).argtypes == protos[name][1]
    mk = (_lib.LIB_PATH.parent / "Makefile").read_text()
    rest = [ln for ln in mk.splitlines() if ln.startswith("REST_SRCS")]
    assert len(rest) == 1 and "koaf_occl.hip" in rest[0].split()


def test_occl_kernels_refuse_bad_arguments_without_a_device():
    """the argument checks run ahead of any launch: a box that breaks 1 <= str <= win <= dims, windows outside the box, images
    that do not tile the sample, rows that are no multiple of four bytes, a window count that is not the box's"""
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    EINVAL = _lib.defines()["KOAF_EINVAL"]
    p = ctypes.c_void_p(256)                       # (never dereferenced: every call below is refused first)
    A = ctypes.c_int32 * 4
    dims, win, st = A(1, 10, 7, 5), A(1, 4, 3, 2), A(1, 3, 2, 2)
    assert L.koaf_occl_points(p, None, 0.0, p, 1, 1, dims, A(1, 4, 3, 6), st, 0, None) == EINVAL
    assert b"koaf_occl_points" in L.koaf_last_error()
    assert L.koaf_occl_points(p, None, 0.0, p, 1, 1, dims, win, A(1, 5, 2, 2), 0, None) == EINVAL
    assert L.koaf_occl_points(p, None, 0.0, p, 2, 1, dims, win, st, 26, None) == EINVAL       # windows 26, 27 of 27
    assert L.koaf_occl_points(p, None, 0.0, p, 65, 1, dims, win, st, 0, None) == EINVAL
    assert L.koaf_occl_points(p, None, 0.0, None, 1, 1, dims, win, st, 0, None) == EINVAL
    assert L.koaf_occl_points(p, None, 0.0, p, 1, 1, None, win, st, 0, None) == EINVAL
    # 5 images of 10 x 7 with the rc strides tile the sample; 4 images do not, nor do strides that leave it
    assert L.koaf_occl_slices(p, None, 0.0, p, p, 1, 1, dims, win, st, 4, 10, 7, 350, 1, 35, 5, None) == EINVAL
    assert b"koaf_occl_slices" in L.koaf_last_error()
    assert L.koaf_occl_slices(p, None, 0.0, p, p, 1, 1, dims, win, st, 5, 10, 7, 350, 2, 35, 5, None) == EINVAL
    assert L.koaf_occl_slices(p, None, 0.0, p, None, 1, 1, dims, win, st, 5, 10, 7, 350, 1, 35, 5, None) == EINVAL
    for row_bytes in (0, 6, -4):
        assert L.koaf_occl_rows(p, p, p, p, 1, 1, 1, row_bytes, None) == EINVAL
        assert b"koaf_occl_rows" in L.koaf_last_error()
    assert L.koaf_occl_rows(p, None, p, p, 1, 1, 1, 4, None) == EINVAL                        # fresh rows without a fresh tensor
    assert L.koaf_occl_fold(p, p, 26, 1, dims, win, st, None) == EINVAL
    assert b"27" in L.koaf_last_error()
    assert L.koaf_occl_fold(p, None, 27, 1, dims, win, st, None) == EINVAL


# ---- the Python route on a stub ------------------------------------------------------------------------------------------------
def _stub():
    """a smooth two-input stub with the product models' calling convention: (B, 2) logits"""
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 16).reshape(1, 1, 4, 4))
            self.c = torch.nn.Parameter(torch.linspace(0.5, -0.25, 9).reshape(1, 9))
            self.calls = []

        def forward(self, img, clin):
            self.calls.append(int(img.shape[0]))
            u = (img * self.a).flatten(1).sum(1) + (clin.flatten(1) * self.c).sum(1)
            v = (img.flatten(1) ** 2).sum(1) * 0.1 - clin.flatten(1).sum(1)
            return torch.stack([torch.tanh(u) + 0.05 * u * u, v], dim=1)
    return Stub().eval()


def _inputs(B=3):
    g = torch.Generator().manual_seed(11)
    return (torch.randn(B, 1, 4, 4, generator=g), torch.randn(B, 1, 9, generator=g)), torch.tensor([[1], [0], [0]][:B])


def _occl_points_t(x, window, strides, k0, J, base=None):
    b = None if base is None else base.numpy() if torch.is_tensor(base) else base
    msk = T.masks(tuple(x.shape), window, strides)[k0:k0 + J]
    return torch.from_numpy(T.points(x.numpy(), msk, b))


def _occl_fold_t(delta, shape, window, strides):
    return torch.from_numpy(T.fold_map(delta.numpy(), T.masks((1,) + tuple(shape), window, strides)))


@pytest.fixture
def twin_ops(monkeypatch):
    from oaprogressionmmf_amd import ops
    monkeypatch.setattr(ops, "occl_points", _occl_points_t)
    monkeypatch.setattr(ops, "occl_fold", _occl_fold_t)
    monkeypatch.setattr(ops, "rowdot", lambda a, b: (a * b).flatten(1).sum(1))
    return ops


def test_dense_route_on_a_stub(twin_ops):
    """sparse=False: one forward of the intact inputs, then ceil(K / chunk) passes per input at batch J * B; the deltas are the
    score differences of a plain loop over the windows, the maps their fold; a skipped input gives None and costs no pass"""
    from oaprogressionmmf_amd.run import occlusion
    m, (xs, y) = _stub(), _inputs()
    wins, strs = [(1, 3, 2), (1, 4)], [(1, 1, 2), (1, 3)]           # 2 x 2 = 4 windows of the image, 3 of the vector
    bases = (-0.5, torch.full((3, 1, 9), 0.25))
    maps, deltas = occlusion(m, xs, y, wins, strs, baselines=bases, chunk=3, sparse=False, return_deltas=True)
    assert m.calls == [3, 9, 3, 9], "F(x), then 4 windows as 3 + 1 and 3 windows as 3, at B = 3"
    with torch.no_grad():
        F = m(*xs).gather(1, y)[:, 0]
        for i, (x, b) in enumerate(zip(xs, (-0.5, 0.25))):
            msk = T.masks(tuple(x.shape), wins[i], strs[i])
            assert deltas[i].shape == (len(msk), 3)
            for k in range(len(msk)):
                pt = torch.from_numpy(T.points(x.numpy(), msk[k:k + 1], b)[0])
                Fk = m(*[pt if j == i else xs[j] for j in range(2)]).gather(1, y)[:, 0]
                assert torch.allclose(deltas[i][k], F - Fk, rtol=1e-5, atol=1e-6)
            assert maps[i].shape == x.shape and maps[i].dtype == torch.float32
            assert np.array_equal(maps[i].numpy(), T.fold_map(deltas[i].numpy(), msk))
    one = occlusion(m, xs, y, wins, strs, baselines=bases, chunk=1, sparse=False)
    for a, b in zip(maps, one):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    m.calls.clear()
    skipped, d = occlusion(m, xs, y, [None, (1, 4)], sparse=False, return_deltas=True)
    assert skipped[0] is None and d[0] is None and skipped[1].shape == xs[1].shape and m.calls == [3, 3, 3, 3]
    assert all(p.requires_grad and p.grad is None for p in m.parameters())


def test_explain_epoch_plumbing_on_a_stub(twin_ops):
    from oaprogressionmmf_amd.run import ensemble_explain_foldw, explain_epoch, occlusion
    from oaprogressionmmf_amd.run._explain import EXPLAIN_FNS
    assert EXPLAIN_FNS[-1] == "occlusion"
    m, (xs, y) = _stub(), _inputs()
    modals = ("xr_pa", "clin")
    loader = [{"image__xr_pa": xs[0][lo:hi], "image__clin": xs[1][lo:hi], "target": y[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in ((0, 2), (2, 3))]
    seen = []

    def sink(ids, mods, maps):
        assert list(mods) == list(modals)
        seen.append((list(ids), maps))
    kw = dict(sliding_window_shapes=[(1, 2, 2), None], strides=None, baselines=0.5, chunk=2, sparse=False)
    acc = explain_epoch(m, loader, modals, device="cpu", explain_fn="occlusion", sink=sink, explain_kwargs=kw)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "occl_attrs", "occl_percent"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    assert m.calls == [2, 4, 4, 1, 2, 2], "per batch F(x) and 4 windows in chunks of 2 (B = 2, then 1)"
    want = occlusion(m, xs, y, **kw)
    assert want[1] is None and all(maps[1] is None for _, maps in seen)
    assert torch.allclose(torch.cat([maps[0] for _, maps in seen]), want[0], rtol=1e-5, atol=1e-6)
    attrs = np.asarray(acc["occl_attrs"])
    assert attrs.shape == (3, 2) and (attrs[:, 1] == 0).all(), "a skipped input counts 0"
    np.testing.assert_allclose(attrs[:, 0], want[0].flatten(1).sum(1).numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(np.asarray(acc["occl_percent"]).sum(1), 100.0, atol=2e-3)
    assert not any(torch.is_tensor(v) for vals in acc.values() for v in vals), "the returned lists hold no maps"
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="occl")
    np.testing.assert_allclose(np.asarray(ens["occl_percent"]) * 100.0, acc["occl_percent"], atol=2e-3)
    assert explain_epoch(None, [], modals, explain_fn="occlusion") == {}
