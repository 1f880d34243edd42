"""GPU: the two kernels of koaf_coal.hip against the brute force of coal_twin.py.  koaf_coal_tokens copies, so it is held to
torch.equal, into a NaN-filled output with a guard region behind it; koaf_shapley_fold sums in fp64 and is held to the rounding
bound of its own sums."""
import numpy as np
import pytest
import torch

import coal_twin as T

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
SEG7 = [0, 1, 3, 4, 6, 7]            # M = 5, L = 7: segments of length 1 at the front, in the middle and at the end
SEG8 = [0, 1, 3, 4, 7, 8]            # L = 8: L * D is a multiple of 4 for every D, so 16-byte units straddle tokens where D % 4 != 0
MASKS5 = [0, 31, 1, 16, 4, 10, 21, 27, 14]


def _rand(shape, salt=0):
    return np.random.default_rng(23 + salt + sum(shape)).standard_normal(shape).astype(F32)


def _run(dev, tx, t0, seg_off, masks, misalign=False):
    """ops.coal_tokens into a NaN-filled view with a guard behind it; misalign: tx, t0 and out are views that start 4 bytes past a
    16-byte boundary"""
    from oaprogressionmmf_amd import ops

    def put(a):
        if not misalign:
            return torch.from_numpy(a).to(dev)
        buf = torch.empty(a.size + 1, device=dev)
        v = buf[1:].view(a.shape).copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    J, (B, L, D) = len(masks), tx.shape
    n = J * B * L * D
    lead = 1 if misalign else 0
    buf = torch.full((lead + n + GUARD,), float("nan"), device=dev)
    buf[lead + n:] = -777.0
    out = buf[lead:lead + n].view(J, B, L, D)
    got = ops.coal_tokens(put(tx), put(t0), seg_off, masks, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (J, B, L, D)
    assert bool((buf[lead + n:] == -777.0).all()), "the guard behind the output is intact"
    want = T.tokens(tx, t0, seg_off, masks)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), "bit equality (and no NaN left: every element is written)"


@pytest.mark.parametrize("D", [1, 3, 4, 36, 260])
@pytest.mark.parametrize("B,B0", [(1, 1), (3, 1), (3, 3)])
def test_coal_tokens_rows(dev, D, B, B0):
    """D = 1, 3: rows of 4 and 12 bytes; 4, 36: one and nine 16-byte units a row; 260: 65 units, more than one wave a row.  L = 7:
    L * D % 4 != 0 for odd D (one element per lane); L = 8: the 16-byte path for every D, units straddling tokens for D = 1, 3.
    A mask of 0, the full mask, single inputs and mixed ones; J = 9 and J = 1."""
    for seg in (SEG7, SEG8):
        L = seg[-1]
        tx, t0 = _rand((B, L, D)), _rand((B0, L, D), salt=1)
        _run(dev, tx, t0, seg, MASKS5)
        _run(dev, tx, t0, seg, [21])


@pytest.mark.parametrize("D", [3, 4, 36])
def test_coal_tokens_unaligned_views(dev, D):
    """views whose pointers are 4-byte aligned only take the one-element path, with the same bits"""
    tx, t0 = _rand((3, 8, D), salt=2), _rand((1, 8, D), salt=3)
    _run(dev, tx, t0, SEG8, MASKS5, misalign=True)


def test_coal_tokens_one_token_one_input(dev):
    for D in (1, 4):
        _run(dev, _rand((2, 1, D)), _rand((1, 1, D), salt=1), [0, 1], [0, 1])
        _run(dev, _rand((2, 1, D)), _rand((2, 1, D), salt=1), [0, 1], [1])


def test_coal_tokens_all_256_coalitions_of_eight(dev):
    """M = 8, J = 256: four launches of 64 masks; segments of lengths 1, 2, 1, 3, 1, 1, 2, 1"""
    seg = [0, 1, 3, 4, 7, 8, 9, 11, 12]
    for D, B0 in ((4, 1), (3, 2)):
        _run(dev, _rand((2, 12, D)), _rand((B0, 12, D), salt=1), seg, list(range(256)))
    _run(dev, _rand((2, 12, 4)), _rand((1, 12, 4), salt=1), seg, list(range(255, -1, -1))[:65])


def test_coal_tokens_more_than_one_block_a_sample(dev):
    """L * D = 4420 and 4419 elements: a second, partial block of 4096 per sample, on either path"""
    seg = [0, 1, 9, 16, 17]
    for D in (260, 259):
        _run(dev, _rand((2, 17, D)), _rand((1, 17, D), salt=1), seg, [0, 15, 6, 9, 1])


def _bars(v, M):
    """(n + 4) * 2^-53 * c * max|v|: a sum of n products weight x difference whose absolute weights sum to 1, every difference at
    most c * max|v|; (n - 1) additions, one product and one weight rounding per term, and the twin's own three roundings"""
    vmax = float(np.abs(v).max())
    u = 2.0 ** -53
    return (2 ** (M - 1) + 4) * u * 2 * vmax, (2 ** max(M - 2, 0) + 4) * u * 4 * vmax


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_shapley_fold(dev, M, B):
    from oaprogressionmmf_amd import ops
    S = 1 << M
    r = np.random.default_rng(1000 * M + B)
    v = r.uniform(-1.0, 1.0, size=(S, B)).astype(F32)
    phi, inter, loo, solo = ops.shapley_fold(torch.from_numpy(v).to(dev), M)
    assert phi.shape == loo.shape == solo.shape == (B, M) and inter.shape == (B, M, M)
    assert all(t.dtype == torch.float64 and t.is_cuda for t in (phi, inter, loo, solo))
    wp, wi, wl, ws = T.shapley(v)
    bar, ibar = _bars(v, M)
    err = [float(np.abs(g.cpu().numpy() - w).max()) for g, w in ((phi, wp), (inter, wi), (loo, wl), (solo, ws))]
    print(f"\n[shapley_fold M {M} B {B}] |phi| {err[0]:.2e} (bar {bar:.2e}), |inter| {err[1]:.2e} (bar {ibar:.2e}), loo {err[2]:.2e}, solo {err[3]:.2e}")
    assert err[0] <= bar and err[2] <= bar and err[3] <= bar and err[1] <= ibar
    assert float(inter.diagonal(dim1=1, dim2=2).abs().max()) == 0.0
    if M == 1:
        assert float(inter.abs().max()) == 0.0
    v64 = v.astype(np.float64)
    eff = np.abs(phi.sum(1).cpu().numpy() - (v64[S - 1] - v64[0])).max()
    assert eff <= M * bar, "efficiency"
    # an additive game: phi = loo = solo = a, no interaction
    # (multiples of 2^-10: every coalition's sum is exact in fp32, so the fp32 game is additive itself)
    a = r.integers(-1024, 1025, size=(B, M)) / 1024.0
    add = np.stack([sum((a[:, i] for i in range(M) if s >> i & 1), np.full(B, 0.25)) for s in range(S)])
    assert np.array_equal(add.astype(F32).astype(np.float64), add)
    pa, ia, la, sa = (t.cpu().numpy() for t in ops.shapley_fold(torch.from_numpy(add.astype(F32)).to(dev), M))
    abar, aibar = _bars(add, M)
    assert max(np.abs(pa - a).max(), np.abs(la - a).max(), np.abs(sa - a).max()) <= abar
    assert np.abs(ia).max() <= aibar
