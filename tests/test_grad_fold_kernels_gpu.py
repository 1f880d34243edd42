"""GPU: the gradient fold / norm / clip-coefficient / scale kernels on flat tensors, against numpy restatements of their pinned
arithmetic.  Sizes cover the scalar tails against the 16-byte vector width, one block versus many, and a last short block; each
is also tried on a buffer offset by 64 elements (a 256-byte arena slot) between NaN sentinels that must survive."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 257, 4097, 1_000_003)
PAD = 64
F32 = np.float32


def _rng(n, salt=0):
    return np.random.default_rng(7919 * salt + n)


class _Slot(object):
    """an n-element device range that starts `off` elements into a buffer, NaN on both sides of it"""

    def __init__(self, dev, values, off):
        n = values.size
        host = np.full(off + n + PAD, np.nan, dtype=F32)
        host[off:off + n] = values
        self.buf, self.off, self.n = torch.from_numpy(host).to(dev), off, n
        self.t = self.buf[off:off + n]

    def values(self):
        host = self.buf.cpu().numpy()
        assert np.isnan(host[:self.off]).all() and np.isnan(host[self.off + self.n:]).all(), "wrote outside its range"
        return host[self.off:self.off + self.n]


def _bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def _ws(dev, sizes):
    from oaprogressionmmf_amd import ops
    ws, cuts = ops.grad_norm_ws(sizes, dev)
    ws.fill_(float("nan"))                                     # every slot must be written, none accumulated into
    return ws, cuts


def _norm(dev, tensors, max_norm, norm_type):
    from oaprogressionmmf_amd import ops
    ws, cuts = _ws(dev, [t.numel() for t in tensors])
    for t, cut in zip(tensors, cuts):
        ops.grad_norm_part(t, cut, norm_type)
    norm, coef = ops.grad_norm_final(ws, max_norm, norm_type)
    return norm.cpu().numpy(), coef.cpu().numpy()


def _coef_np(max_norm, norm):
    with np.errstate(all="ignore"):
        c = F32(max_norm) / (F32(norm) + F32(1e-6))
    return c if not (c > F32(1.0)) else F32(1.0)               # (a NaN stays a NaN)


@pytest.mark.parametrize("off", [0, PAD])
@pytest.mark.parametrize("n", SIZES)
def test_fold_modes_are_the_numpy_fp32_expression(dev, n, off):
    """three rounds (micro-batches) with w = 1, 0.5, 0.375: mode 0, mode 1, then mode 2 writes acc + w g over g and leaves acc;
    product rounded, then the sum -- np.float32(w) * g, then + -- bit for bit"""
    from oaprogressionmmf_amd import ops
    r = _rng(n)
    gs = [(r.standard_normal(n) * 10.0 ** r.uniform(-3, 3, n)).astype(F32) for _ in range(3)]
    acc = _Slot(dev, np.full(n, 7.0, dtype=F32), off)          # (mode 0 must overwrite, not add)
    g = [_Slot(dev, v, off) for v in gs]
    ops.grad_fold(acc.t, g[0].t, 1.0, 0)
    want = F32(1.0) * gs[0]
    assert np.array_equal(_bits(acc.values()), _bits(want))
    ops.grad_fold(acc.t, g[1].t, 0.5, 1)
    want = want + F32(0.5) * gs[1]
    assert np.array_equal(_bits(acc.values()), _bits(want))
    for k in (0, 1):
        assert np.array_equal(_bits(g[k].values()), _bits(gs[k]))      # g is only read in modes 0 and 1
    ws, cuts = _ws(dev, [n])
    ops.grad_fold(acc.t, g[2].t, 0.375, 2, ws=cuts[0], norm_type=2.0)
    final = want + F32(0.375) * gs[2]
    assert np.array_equal(_bits(g[2].values()), _bits(final))
    assert np.array_equal(_bits(acc.values()), _bits(want))            # acc unchanged by mode 2
    # the partials the fold emitted are those of a norm pass over what it wrote
    norm, _ = ops.grad_norm_final(ws, 1.0, 2.0)
    norm2, _ = _norm(dev, [g[2].t], 1.0, 2.0)
    assert _bits(norm.cpu().numpy()) == _bits(norm2)
    n64 = np.sqrt(np.sum(final.astype(np.float64) ** 2))
    assert abs(float(norm) - n64) <= 2.0 ** -23 * n64


def test_fold_mode2_without_workspace_and_inf_partials(dev):
    from oaprogressionmmf_amd import ops
    n = 4097
    r = _rng(n, 5)
    a, b = r.standard_normal(n).astype(F32), r.standard_normal(n).astype(F32)
    acc, g = _Slot(dev, a, PAD), _Slot(dev, b, PAD)
    ops.grad_fold(acc.t, g.t, 0.375, 2)
    want = a + F32(0.375) * b
    assert np.array_equal(_bits(g.values()), _bits(want))
    g2 = _Slot(dev, b, PAD)
    ws, cuts = _ws(dev, [n])
    ops.grad_fold(acc.t, g2.t, 0.375, 2, ws=cuts[0], norm_type=float("inf"))
    norm, _ = ops.grad_norm_final(ws, 1.0, float("inf"))
    assert _bits(norm.cpu().numpy()) == _bits(np.abs(want).max())


@pytest.mark.parametrize("off", [0, PAD])
@pytest.mark.parametrize("n", SIZES)
def test_two_norm_is_the_float64_norm_rounded_once(dev, n, off):
    """values spanning 1e-20 ... 1e15 in one tensor; squares and sums are fp64, so the only rounding that shows is the final
    cast: |norm - norm64| <= 2^-23 norm64.  Twice, from a NaN-filled workspace: the same bits."""
    r = _rng(n, 1)
    v = (r.standard_normal(n) * 10.0 ** r.uniform(-20, 15, n)).astype(F32)
    s = _Slot(dev, v, off)
    n64 = np.sqrt(np.sum(v.astype(np.float64) ** 2))
    got = [_norm(dev, [s.t], 1.0, 2.0)[0] for _ in range(2)]
    assert abs(float(got[0]) - n64) <= 2.0 ** -23 * n64, (float(got[0]), n64)
    assert _bits(got[0]) == _bits(got[1])
    assert np.array_equal(_bits(s.values()), _bits(v))


def test_two_norm_does_not_overflow_and_combines_ranges(dev):
    two = torch.tensor([3e25, 3e25], device=dev)               # an fp32 square would be +Inf
    norm, coef = _norm(dev, [two], 1.0, 2.0)
    n64 = np.sqrt(2.0) * np.float64(F32(3e25))
    assert np.isfinite(norm) and abs(float(norm) - n64) <= 2.0 ** -23 * n64
    assert _bits(coef) == _bits(_coef_np(1.0, norm))
    r = _rng(0, 2)
    a, b = r.standard_normal(100_003).astype(F32), (1e3 * r.standard_normal(4097)).astype(F32)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    norm, _ = _norm(dev, [ta, tb], 1.0, 2.0)                   # partials of two ranges, one finalize
    n64 = np.sqrt(np.sum(a.astype(np.float64) ** 2) + np.sum(b.astype(np.float64) ** 2))
    assert abs(float(norm) - n64) <= 2.0 ** -23 * n64
    assert _bits(norm) == _bits(_norm(dev, [ta, tb], 1.0, 2.0)[0])


@pytest.mark.parametrize("off", [0, PAD])
@pytest.mark.parametrize("n", SIZES)
def test_inf_norm_is_exact_and_propagates_nonfinite(dev, n, off):
    r = _rng(n, 3)
    v = (r.standard_normal(n) * 10.0 ** r.uniform(-20, 15, n)).astype(F32)
    s = _Slot(dev, v, off)
    norm, coef = _norm(dev, [s.t], 2.5, float("inf"))
    assert _bits(norm) == _bits(np.abs(v).max())
    assert _bits(coef) == _bits(_coef_np(2.5, norm))
    for pos in sorted({0, n // 2, n - 1}):                     # first lane, the middle, the scalar tail
        for bad in (np.nan, -np.inf):
            w = v.copy()
            w[pos] = bad
            got, c = _norm(dev, [_Slot(dev, w, off).t], 2.5, float("inf"))
            if np.isnan(bad):
                assert np.isnan(got) and np.isnan(c), (pos, got, c)
            else:
                assert np.isposinf(got) and float(c) == 0.0, (pos, got, c)


@pytest.mark.parametrize("off", [0, PAD])
@pytest.mark.parametrize("n", SIZES)
def test_coefficient_and_scale(dev, n, off):
    """coef is the fp32 expression min(1, max_norm / (norm + 1e-6f)) of the returned norm, bit for bit; the scale is numpy's
    fp32 g * coef, bit for bit; a max_norm above the norm gives exactly 1 and leaves g's bits alone"""
    from oaprogressionmmf_amd import ops
    r = _rng(n, 4)
    v = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 3, n)).astype(F32)
    s = _Slot(dev, v, off)
    ws, cuts = _ws(dev, [n])
    ops.grad_norm_part(s.t, cuts[0], 2.0)
    max_norm = float(F32(0.37 * float(ops.grad_norm_final(ws, 1.0, 2.0)[0])))
    norm, coef = ops.grad_norm_final(ws, max_norm, 2.0)
    c = coef.cpu().numpy()
    assert _bits(c) == _bits(_coef_np(max_norm, norm.cpu().numpy())) and 0.0 < float(c) < 1.0
    ops.grad_scale(s.t, coef)
    assert np.array_equal(_bits(s.values()), _bits(v * F32(c)))
    s = _Slot(dev, v, off)
    norm, coef = ops.grad_norm_final(ws, 2.0 * float(norm) + 1.0, 2.0)
    assert _bits(coef.cpu().numpy()) == _bits(F32(1.0))
    ops.grad_scale(s.t, coef)
    assert np.array_equal(_bits(s.values()), _bits(v))


def test_nonfinite_norms_reach_the_gradient_as_torch_has_it(dev):
    from oaprogressionmmf_amd import ops
    n = 4097
    v = _rng(n, 6).standard_normal(n).astype(F32)
    for bad, kind in ((np.nan, 2.0), (np.inf, 2.0), (np.nan, float("inf"))):
        w = v.copy()
        w[1234] = bad
        s = _Slot(dev, w, PAD)
        ws, cuts = _ws(dev, [n])
        ops.grad_norm_part(s.t, cuts[0], kind)
        norm, coef = ops.grad_norm_final(ws, 1.0, kind)
        ops.grad_scale(s.t, coef)
        out = s.values()
        if np.isnan(bad):
            assert np.isnan(norm.item()) and np.isnan(coef.item()) and np.isnan(out).all()
        else:                                                  # clip_grad_norm_: inf norm -> coef 0 -> 0 * g (inf * 0 = NaN)
            assert np.isposinf(norm.item()) and coef.item() == 0.0
            keep = np.arange(n) != 1234
            assert (out[keep] == 0.0).all() and np.isnan(out[1234])
