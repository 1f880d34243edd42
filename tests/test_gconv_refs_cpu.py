"""The references of test_gconv_gpu.py, proven against each other on any machine (gconv_refs.py): a GPU failure there then
points at the kernel, not at the slab layout the test assumed."""
import pytest
import torch

import gconv_refs as R

# (C, groups): every group width the ABI admits, Cg = C / groups in {1, 2, 4, 8, 16, 32, 64}; more than one slab where it is cheap
PAIRS = [(64, 64), (128, 128), (64, 32), (128, 32), (128, 16), (64, 4), (128, 4), (64, 1), (128, 2)]


def _operands(C, groups, seed):
    g = torch.Generator().manual_seed(seed)
    Cg = C // groups
    a = torch.randn(2, 7, 5, C, generator=g, dtype=torch.float64)
    w = torch.randn(C, 3, 3, Cg, generator=g, dtype=torch.float64) * (9 * Cg) ** -0.5
    return a, w


def test_pairs_cover_every_group_width():
    assert {C // g for C, g in PAIRS} == {1, 2, 4, 8, 16, 32, 64}


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,groups", PAIRS)
def test_slab_convolution_is_the_grouped_convolution(C, groups, stride):
    """per slab, the dense 64 -> 64 convolution with expand(w) == the grouped convolution, in float64"""
    a, w = _operands(C, groups, 100 + C + groups)
    y = R.gconv64(a, w, stride, groups)
    ys = R.slab_conv64(a, R.expand(w, C, groups), stride)
    assert y.shape == ys.shape == (2, (7 - 1) // stride + 1, (5 - 1) // stride + 1, C)
    assert float((y - ys).abs().max()) <= 1e-12


@pytest.mark.parametrize("C,groups", PAIRS)
def test_expand_compress(C, groups):
    Cg = C // groups
    _, w = _operands(C, groups, 200 + C + groups)
    w = w.float()
    wexp = R.expand(w, C, groups)
    assert wexp.shape == (C // 64, 64, 9, 64) and wexp.dtype == w.dtype
    assert torch.equal(R.compress(wexp, C, groups), w)                       # exact: elements are only moved
    assert torch.equal(R.expand(w.reshape(C, 9, Cg), C, groups), wexp)
    assert int((wexp != 0).sum()) == int((w != 0).sum())                     # nothing beside the blocks
    # the block of output channel co = 64 z + col holds the slab-local input channels of col's group, in order
    for co in (0, Cg - 1, C // 2 + 1, C - 1):
        z, col = divmod(co, 64)
        g0 = (col // Cg) * Cg
        assert torch.equal(wexp[z, col, :, g0:g0 + Cg], w[co].reshape(9, Cg))
    # compress ignores whatever lies off the blocks
    noisy = torch.where(wexp != 0, wexp, torch.full_like(wexp, 7.0))
    assert torch.equal(R.compress(noisy, C, groups), w)
    on = R.expand(torch.ones_like(w), C, groups) != 0
    assert torch.equal(R.compress(torch.where(on, wexp, torch.full_like(wexp, float("nan"))), C, groups), w)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,groups", [(64, 32), (128, 4), (64, 1)])
def test_gradient_twins_are_autograd(C, groups, stride):
    a, w = _operands(C, groups, 300 + C + groups)
    a.requires_grad_(True)
    w.requires_grad_(True)
    y = R.gconv64(a, w, stride, groups)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    y.backward(dy)
    assert float((R.dgrad64(dy, w.detach(), a.shape, stride, groups) - a.grad).abs().max()) <= 1e-12
    assert float((R.wgrad64(dy, a.detach(), stride, groups) - w.grad).abs().max()) <= 1e-12
    # and through the slabs: the weight gradient of the dense slab convolution, compressed, is the grouped one
    wexp = R.expand(w.detach(), C, groups).requires_grad_(True)
    R.slab_conv64(a.detach(), wexp, stride).backward(dy)
    assert float((R.compress(wexp.grad, C, groups) - w.grad).abs().max()) <= 1e-12


def test_unsupported_group_widths_are_refused():
    for C, groups in ((96, 32), (128, 3), (192, 2)):
        with pytest.raises(AssertionError):
            R.expand(torch.zeros(C, 3, 3, max(C // groups, 1)), C, groups)
