"""Per-element parity of the softmax losses (koaf_loss.hip: focal loss and cross-entropy, one-block and grid form) at their edges:
the one-block / grid switch, a last chunk of one element, the second slot of the second stage's lanes, a batch boundary inside a
chunk, C = 1, zero class weights, ignored and bad labels, every target ignored -- and invariance under a common offset of the
logits, which a norm over a mixed batch cannot see.

test_kernels_gpu.py compares whole tensors by a ratio of norms.  Here the logits are multiples of 2^-10 with |x| < 16 (adding 64
or 1024 is exact) and every element has a confidence grade: its target logit is the best other logit +- a margin of 0, 1, 4, 8, 12
or 16.  The elements of one grade form a group, and within each group
  * the gradient holds the 4 x yardstick rule of test_elem_edges_gpu.py: worst |d - d64| <= max(4 x the worst error of torch's fp32
    CPU result in the same group, gamma(k) * max|d64| of the group), k counted from the kernel source (loss_optim_refs.k_grad:
    K_P + 4 for the cross-entropy, K_P = max_j (2 (m - x_j) + 2 C + 6) |d_j| / max|d| over the group, the target's own factor counted
    apart; the focal factor adds (2.65 g + |g - 1| + 1)(3 C + 11) + 15; a weighted mean adds the chain of its denominator's sum);
  * the loss scalar holds the same rule with the floor gamma(m) * sum|l_i| * wgt, m = loss_optim_refs.sum_chain(n), the longest
    addition chain of the form that ran and nothing else: ceil(n / 256) + 8 in one block (lane stride, LDS tree), 16 + 8 +
    ceil(chunks / 256) + 8 on the grid (printed per row);
  * loss and gradient of x + c are bit-equal to those of x for c in {64, 1024, -1024}; each grid-form row run twice is bit-equal.
The references are the float64 formulas of loss_optim_refs.py on the same fp32 inputs (held against autograd by
test_loss_optim_refs_cpu.py, where the bars are also checked from both sides).

Measured on an MI355X (they document; every bar is computed in the test).  Worst kernel error / torch-fp32 error per group over all
rows -- cross-entropy: 1.0 .. 1.3 at margins -16 .. +1, 0.11 at +4, <= 0.01 at +8 .. +16; focal: 1.3 .. 2.6 at margins -16 .. +1 (17 once
at -4, at 0.12 of its floor), 0.09 at +4, < 0.01 at +8 .. +16: in the confident groups log1p / expm1 keep the digits that torch's
1 - exp() loses.  Measured k = worst error / (u max|d64|): <= 6.9 (cross-entropy, counted 12 .. 60), <= 11.9 (focal, counted 68 .. 298);
at most 0.27 of the counted k in any group.
Loss scalar: at most 0.17 of its bar (1 x 3 x 1, m = 9).  Offsets: 0 of up to 24579 gradient elements differ.
On the kernel as it was before the maximum was subtracted first (lse = m + logf(s), x - lse, 1 - pt): the offset rows fail from
c = +64 on (82 of 111 elements at 37 x 3, 11913 of 16386 at 8193 x 2, worst 8.1e-8), and so do the confident focal groups at offset 0:
margin +8 at 15 x torch's error (3.7 x the bar), +16 at 5.3 x (1.3 x the bar); measured k 3.0e4 at +8, 2.7e7 at +16."""
import numpy as np
import pytest
import torch

import loss_optim_refs as R
from elem_refs import U

pytestmark = pytest.mark.gpu

GROUPS = R.loss_groups()
NG = len(GROUPS)
CW5 = [0.5, 2.0, 0.0, 1.25, 0.75]          # class weights, one of them 0


def _ws(B, S):
    from oaprogressionmmf_amd._lib import lib
    return lib().koaf_loss_ws(B, S)


def _run(dev, x, tg, gamma_, mean, focal, cw):
    from oaprogressionmmf_amd import ops
    loss, dl = ops.focal_loss(x.to(dev), tg.to(dev), gamma_, mean=mean, focal=focal, class_weight=None if cw is None else cw.to(dev))
    return loss.cpu(), dl.cpu()


def _case(tg):
    """targets: -100 at the first and the last element and at both sides of the first chunk boundary"""
    tg = tg.clone()
    n = tg.numel()
    for i in (0, R.LOSS_CHUNK - 1, R.LOSS_CHUNK, n - 1):
        if i < n and n > 2:
            tg.view(-1)[i] = -100
    return tg


def _hold(dev, x, tg, grp, gamma_, mean, focal, cw, what, ngroups=NG):
    """one call held per group and as a scalar; returns (loss, dl)"""
    B, C = x.shape[0], x.shape[1]
    n = tg.numel()
    ref = R.softmax_loss_ref(x, tg, cw, gamma_, focal, mean)
    ly, dy = R.torch_loss_fp32(x, tg, cw, gamma_, focal, mean)
    loss, dl = _run(dev, x, tg, gamma_, mean, focal, cw)
    wm = (not focal) and cw is not None
    zero = ~(ref["valid"] & (ref["d"].abs().sum(1) > 0))
    assert float(dl.movedim(1, -1)[zero].abs().max() if zero.any() else 0.0) == 0.0, what + ": an ignored or zero-weight element has a gradient"
    rep = R.loss_group_report(dl, ref, dy, grp, ngroups, n, C, gamma_, focal, wm)
    for r in rep:
        a, s = GROUPS[r["group"]]
        print(f"GROUP {what} margin {a * s:+d}: kernel {r['err']:.3e} yardstick {r['yard']:.3e} ratio {r['err'] / max(r['yard'], 1e-300):.2f} "
              f"bar {r['bar']:.3e} k {r['k']} measured k {r['err'] / (U * r['dmax']):.1f}")
    bad = [r for r in rep if not r["ok"]]
    # k (loss_optim_refs.k_grad): the softmax factor's K_P = max_j (2 (m - x_j) + 2 C + 6) |d_j| / max|d| (expf 2, the argument's two
    # subtractions, log1p(s1)'s 2 C + 4), + 4 for w, wgt, its reciprocal and the last product; focal: + dl's
    # (2.65 g + |g - 1| + 1)(3 C + 11) + 15; weighted mean: + the denominator's chain
    assert not bad, f"{what}: groups beyond max(4 x yardstick, gamma(k) max|d64|): " + "; ".join(
        f"margin {GROUPS[r['group']][0] * GROUPS[r['group']][1]:+d} err {r['err']:.3e} torch fp32 {r['yard']:.3e} bar {r['bar']:.3e}" for r in bad)
    s = R.loss_scalar_report(loss, ref, ly, n, C, gamma_, focal, wm)
    print(f"LOSS {what} ({R.loss_form(n)} form, m {s['m']}): kernel {s['err']:.3e} yardstick {s['yard']:.3e} bar {s['bar']:.3e}")
    # m = the longest addition chain of the form that ran (loss_optim_refs.sum_chain)
    assert s["ok"], f"{what}: loss off by {s['err']:.3e}; torch fp32 is off by {s['yard']:.3e}, bar {s['bar']:.3e} (m {s['m']})"
    return loss, dl


# (B, C, S, grid form?): B * S in {1, 255, 256, 257, 8192, 8193, 12288, 12289}, S = 1 and S > 1, C in {1, 2, 3, 5}
GEOMETRY = [
    (1, 3, 1, False),           # one element: one lane, the rest of the tree adds zeros
    (5, 2, 51, False),          # 255: one short pass, S > 1
    (256, 5, 1, False),         # 256: every lane once
    (1, 3, 257, False),         # 257: lane 0 twice, S > 1
    (8192, 2, 1, False),        # the one-block form's last size: 32 per lane
    (2, 3, 4096, False),        # the same size with S > 1
    (8193, 2, 1, True),         # the grid form's first size: three chunks, the last of ONE element
    (3, 3, 2731, True),         # 8193 with S > 1: batch boundaries at 2731 and 5462, inside chunks 0 and 1
    (12288, 5, 1, True),        # three full chunks
    (3, 2, 4096, True),         # the same size with S > 1: batch boundaries on the chunk boundaries
    (12289, 3, 1, True),        # four chunks, the last of one element
    (1, 5, 12289, True),        # the same size as one image
]


@pytest.mark.parametrize("B,C,S,grid", GEOMETRY, ids=[f"{b}x{c}x{s}" for b, c, s, _ in GEOMETRY])
def test_loss_geometry(dev, B, C, S, grid):
    assert (_ws(B, S) > 0) == grid and (grid or _ws(B, S) == 0), "the row does not run the form its comment names"
    x, tg, grp = R.loss_inputs(B, C, S, 100 + B + S)
    tg = _case(tg)
    for focal in (True, False):
        what = f"{B}x{C}x{S} {'focal g2 mean' if focal else 'cross-entropy'}"
        loss, dl = _hold(dev, x, tg, grp, 2.0, True, focal, None, what)
        if grid:
            loss2, dl2 = _run(dev, x, tg, 2.0, True, focal, None)
            assert loss2.item() == loss.item() and torch.equal(dl2, dl), what + ": the grid form is not deterministic"


@pytest.mark.parametrize("B,S,grid", [(257, 1, False), (3, 2731, True)])
def test_loss_single_class_is_exactly_zero(dev, B, S, grid):
    """C = 1: log_softmax is 0 whatever the logit; loss and gradient are exactly 0 (gamma 0 included: 0^0 = 1 times log 1)"""
    assert (_ws(B, S) > 0) == grid
    x, tg, _ = R.loss_inputs(B, 1, S, 7)
    for focal, gamma_ in ((True, 2.0), (True, 0.0), (True, 1.0), (False, 0.0)):
        for c in (0.0, 1024.0):
            loss, dl = _run(dev, x + c, tg, gamma_, True, focal, None)
            assert loss.item() == 0.0 and float(dl.abs().max()) == 0.0, (focal, gamma_, c)


def test_loss_million_elements(dev):
    """256 * 4096 + 1 elements: 257 partials, so lane 0 of loss_grid_sum_kernel takes a second slot; the last chunk holds one element.
    Once: focal, mean, C = 2.  m = 16 + 8 (a chunk) + 2 + 8 (second stage) = 34"""
    B, C, S = 1, 2, 256 * 4096 + 1
    assert _ws(B, S) == 2 * 257 + 4
    x, tg, grp = R.loss_inputs(B, C, S, 9)
    tg = _case(tg)
    _hold(dev, x, tg, grp, 2.0, True, True, None, f"{B}x{C}x{S} focal g2 mean")


OPT_SHAPES = [(2, 3, 1000, False), (3, 3, 2731, True)]


@pytest.mark.parametrize("gamma_", [0.0, 1.0, 2.0, 3.5])
@pytest.mark.parametrize("B,C,S,grid", OPT_SHAPES, ids=["one-block", "grid"])
def test_loss_options(dev, B, C, S, grid, gamma_):
    """every gamma with mean and sum, with and without class weights (one of them 0); -100 at the first and last element and at both
    sides of the chunk boundary"""
    assert (_ws(B, S) > 0) == grid
    x, tg, grp = R.loss_inputs(B, C, S, 200 + S)
    tg = _case(tg)
    for cw in (None, torch.tensor(CW5[:C])):
        for mean in (True, False):
            _hold(dev, x, tg, grp, gamma_, mean, True, cw, f"{B}x{C}x{S} focal g{gamma_} {'mean' if mean else 'sum'} cw {cw is not None}")
    if gamma_ == 0.0:
        _hold(dev, x, tg, grp, 0.0, True, False, torch.tensor(CW5[:C]), f"{B}x{C}x{S} cross-entropy cw True")


@pytest.mark.parametrize("B,C,S,grid", OPT_SHAPES, ids=["one-block", "grid"])
def test_loss_gamma_half(dev, B, C, S, grid):
    """gamma 0.5: (1 - pt)^-0.5 in the gradient -- only at margins <= 12, where 1 - pt is far from 0 in fp32 for reference and kernel
    alike; class weights without the zero one (0^-0.5 * 0 is NaN in torch too)"""
    assert (_ws(B, S) > 0) == grid
    margins = tuple(a for a in R.MARGINS if a <= 12)
    groups = R.loss_groups(margins)
    assert groups == GROUPS[:len(groups)]
    x, tg, grp = R.loss_inputs(B, C, S, 300 + S, margins=margins)
    tg = _case(tg)
    for cw in (None, torch.tensor([0.5, 2.0, 1.25])):
        for mean in (True, False):
            _hold(dev, x, tg, grp, 0.5, mean, True, cw, f"{B}x{C}x{S} focal g0.5 {'mean' if mean else 'sum'} cw {cw is not None}", ngroups=len(groups))


@pytest.mark.parametrize("B,C,S,grid", [(37, 3, 1, False), (2, 5, 1000, False), (3, 3, 2731, True), (8193, 2, 1, True)],
                         ids=["37x3x1", "2x5x1000", "3x3x2731", "8193x2x1"])
def test_loss_shift_invariance(dev, B, C, S, grid):
    """the softmax losses do not depend on a common offset of the logits, and on these inputs (x + c is exact) neither does
    torch's fp32 CPU result: loss and gradient of x + c are bit-equal to those of x"""
    assert (_ws(B, S) > 0) == grid
    x, tg, grp = R.loss_inputs(B, C, S, 400 + S)
    tg = _case(tg)
    for focal in (True, False):
        for cw in (None, torch.tensor(CW5[:C])):
            loss0, dl0 = _run(dev, x, tg, 2.0, True, focal, cw)
            for c in (64.0, 1024.0, -1024.0):
                xc = x + c
                assert torch.equal(xc - c, x)
                loss, dl = _run(dev, xc, tg, 2.0, True, focal, cw)
                ne = int((dl != dl0).sum())
                worst = float((dl.double() - dl0.double()).abs().max())
                print(f"SHIFT {B}x{C}x{S} focal {focal} cw {cw is not None} c {c:+.0f}: {ne} of {dl.numel()} gradient elements differ, "
                      f"worst {worst:.3e}; loss {loss.item()!r} vs {loss0.item()!r}")
                assert ne == 0 and loss.item() == loss0.item(), \
                    f"{B}x{C}x{S} focal {focal} cw {cw is not None}: offset {c:+.0f} changes {ne} gradient elements (worst {worst:.3e}), " \
                    f"loss {loss.item()!r} vs {loss0.item()!r}"


@pytest.mark.parametrize("B,C,S,grid", OPT_SHAPES, ids=["one-block", "grid"])
def test_cross_entropy_with_every_target_ignored(dev, B, C, S, grid):
    """torch: the mean over no element is NaN, the gradient all 0"""
    assert (_ws(B, S) > 0) == grid
    x, tg, _ = R.loss_inputs(B, C, S, 500)
    tg = torch.full_like(tg, -100)
    ly, dy = R.torch_loss_fp32(x, tg, None, 0.0, False, True)
    assert np.isnan(ly.item()) and float(dy.abs().max()) == 0.0
    for cw in (None, torch.tensor(CW5[:C])):
        loss, dl = _run(dev, x, tg, 0.0, True, False, cw)
        assert np.isnan(loss.item()) and float(dl.abs().max()) == 0.0 and torch.isfinite(dl).all()


@pytest.mark.parametrize("B,C,S,grid", OPT_SHAPES, ids=["one-block", "grid"])
def test_loss_bad_label_is_counted(dev, B, C, S, grid):
    from oaprogressionmmf_amd import ops
    assert (_ws(B, S) > 0) == grid
    x, tg, grp = R.loss_inputs(B, C, S, 600)
    tg = _case(tg)
    n = tg.numel()
    bad = [5, n // 2, n - 2]
    tg.view(-1)[bad] = torch.tensor([C, 7, -1])
    ops.numerics_status(reset=True)
    for focal in (True, False):
        _, dl = _hold(dev, x, tg, grp, 2.0, True, focal, None, f"{B}x{C}x{S} bad labels focal {focal}")
        assert float(dl.movedim(1, -1).reshape(n, C)[bad].abs().max()) == 0.0
        assert ops.numerics_status(reset=True)["nonfinite"] == len(bad)


@pytest.mark.parametrize("B,C,S,grid", [(1, 3, 1, False), (2, 3, 1000, False), (3, 3, 2731, True), (8193, 5, 1, True)],
                         ids=["1x3x1", "2x3x1000", "3x3x2731", "8193x5x1"])
def test_loss_writes_every_gradient_element(dev, B, C, S, grid):
    """dlogits goes in as NaN (and the loss too): an element nobody writes shows"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import check, lib
    assert (_ws(B, S) > 0) == grid
    x, tg, grp = R.loss_inputs(B, C, S, 700)
    tg = _case(tg)
    ops.numerics_status()                       # (registers the status words the launches may bump)
    xd, td = x.to(dev), tg.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for focal in (True, False):
        dl = torch.full_like(xd, float("nan"))
        loss = torch.full((), float("nan"), device=dev)
        nws = _ws(B, S)
        ws = torch.full((max(nws, 1),), float("nan"), device=dev)
        wsp = ws.data_ptr() if nws > 0 else None
        if focal:
            check(lib().koaf_focal_loss(xd.data_ptr(), td.data_ptr(), None, loss.data_ptr(), dl.data_ptr(), B, C, S, 2.0, 1, wsp, st), "focal_loss")
        else:
            check(lib().koaf_ce_loss(xd.data_ptr(), td.data_ptr(), None, loss.data_ptr(), dl.data_ptr(), B, C, S, wsp, st), "ce_loss")
        loss2, dl2 = ops.focal_loss(xd, td, 2.0, focal=focal)
        assert torch.isfinite(dl).all() and torch.isfinite(loss).item(), f"focal {focal}: an element was not written"
        assert torch.equal(dl, dl2) and loss.item() == loss2.item()
