"""Element-wise parity of the HBM-bound kernels (koaf_bn.hip, koaf_rows.hip, koaf_preproc.hip, the fused attention forward) at their edges: scalar tails,
the second trip of the grid-stride loops, the row growth and the width extremes of the column reductions, the one- / two-stage
thresholds of the finalisations, max-pool borders and ties, softmax with large logits, both vector widths of the augmenter.

test_kernels_gpu.py compares whole tensors by a ratio of norms; here every element (every channel of a reduction) is held to
  * bit equality where the kernel does no arithmetic (moves, widen, fill, min / max, ReLU, masks, arg-max),
  * k * u * sum|terms| for a fixed chain of k roundings (k counted from the kernel source, beside each assert),
  * gamma(m) * sum|terms| for an fp32 sum whose longest chain of additions is m (elem_refs.col_chain),
  * 4 x the worst per-element error of torch's own fp32 CPU implementation of the same op on the same input (the yardstick)
    for results through erff / expf / powf / rsqrt, where no bound can be derived; never below the bar test_kernels_gpu.py
    already holds the kernel to (its norm-ratio bar times max|ref| as a per-element figure).  The figures beside those
    asserts -- kernel error / yardstick error -- were measured on an MI355X; they document, the bar is computed.
The references are float64 torch / numpy on the CPU fed the same fp32 inputs (elem_refs.py).
The case helpers of koaf_bn.hip's kernels take store=: torch.float32 here; test_elem_edges_bf16_gpu.py runs them again with the
activations stored as bf16, and holds the activation plane images (koaf_planes.hip) per element in both storages."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elem_refs as R
from elem_refs import U, gamma

pytestmark = pytest.mark.gpu

CAP = 256 * 32 * 256        # work items of a capped element-wise grid (ew_grid with KOAF_EW_BLOCKS_PER_CU = 32)
needs_default_cap = pytest.mark.skipif("KOAF_EW_BLOCKS_PER_CU" in os.environ,
                                       reason="KOAF_EW_BLOCKS_PER_CU is set: the grid cap is not the 2^21 work items these shapes are sized for")
BWD = 4e-6                  # test_kernels_gpu.py's bar of the gradient contractions


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def within(got, ref, bound, what):
    """every element: |got - ref| <= bound (float64 on the CPU)"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    over = err > bound
    if over.any():
        i = int((err - bound).argmax())
        idx = np.unravel_index(i, err.shape)
        raise AssertionError(f"{what}: {int(over.sum())}/{err.numel()} elements beyond the bound; worst at {idx}: got "
                             f"{got.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r} err {err.flatten()[i].item():.3e} "
                             f"bound {bound.flatten()[i].item():.3e}")


def yardstick(got, ref, yard, what, floor=0.0):
    """the 4x-yardstick rule: worst |got - ref| <= max(4 * worst |yard - ref|, floor); prints both figures"""
    got, yard = got.detach().double().cpu(), yard.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e, y = float((got - ref).abs().max()), float((yard - ref).abs().max())
    bar = max(4.0 * y, floor)
    print(f"YARD {what}: kernel {e:.3e} yardstick {y:.3e} bar {bar:.3e}")
    assert e <= bar, f"{what}: worst element off by {e:.3e}; torch fp32 is off by {y:.3e}, bar {bar:.3e}"
    return bar


def saved_of(mean, invstd, sc, sh, dev):
    return torch.stack([mean, invstd, sc, sh]).to(dev)


# =================================================================================================
# A. column-reduction geometry
# =================================================================================================
WIDTHS = [4, 8, 128, 512, 1024, 2048, 3072]


def _colstats_case(ops, dev, rows, C, seed, store=torch.float32):
    """store: the storage of the activation x (elem_refs.stored: rounded on the CPU, the reference takes the widened values); the
    partial sums are fp32 in either storage and owe the same bound"""
    g = gen(seed)
    x = R.stored(torch.randn(rows, C, generator=g) * 2.0 + torch.randn(C, generator=g)[None, :], store)
    for shift in (None, torch.randn(C, generator=g)):
        lib_rows = ops.lib().koaf_colpart_rows(rows, C)
        assert lib_rows == R.col_geom(rows, C)["nblk"], (rows, C)
        part = ops.colstats(x.to(store).to(dev), rows, C, shift=None if shift is None else shift.to(dev))
        assert part.shape == (lib_rows, 2, C)
        got = part.double().sum(0).cpu()            # (the second stage is fp64: exact to the last fp32 bit or so; allowed for in m)
        v = x.double() - (0.0 if shift is None else shift.double()[None, :])
        # terms: x - k is one rounding with a shift, none without; its square carries that error twice plus its own rounding
        within(got[0], v.sum(0), R.col_bound(rows, C, 1024, 1 if shift is not None else 0, v.abs()), f"colstats sum {rows}x{C}")
        within(got[1], (v * v).sum(0), R.col_bound(rows, C, 1024, 3 if shift is not None else 1, v * v), f"colstats sumsq {rows}x{C}")


@pytest.mark.parametrize("C", WIDTHS)
def test_colstats_geometry(dev, C):
    from oaprogressionmmf_amd import ops
    for i, rows in enumerate(R.case_a_rows(C)):
        _colstats_case(ops, dev, rows, C, 100 + i)


def _bn_bwd_case(ops, dev, rows, C, seed, modes=(0, 1, 2), store=torch.float32):
    """store: the storage of the activations c and ymask; gradients, dz, dc and the per-channel vectors are fp32 in either"""
    g = gen(seed)
    sc, sh = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3
    mean, invstd = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    c = R.draw_preact(g, (rows, C), sc, sh, store=store)
    y = R.stored(torch.randn(rows, C, generator=g), store)      # mask_mode 1 reads the sign of y itself: no arithmetic, nothing borderline
    if store == torch.bfloat16:
        # the sign test on the widened bf16 value: +0 and -0 are not positive, the smallest positive subnormal (0x0001) is
        y.view(-1)[:3] = torch.tensor([0.0, -0.0, 2.0 ** -133])
        assert torch.equal(R.bf16_bits(y.view(-1)[:3].bfloat16()), torch.tensor([0x0000, 0x8000, 0x0001]))
    grad = torch.randn(rows, C, generator=g)
    saved = saved_of(mean, invstd, sc, sh, dev)
    cd = c.to(store).to(dev)
    for mode in modes:
        mask = {0: torch.ones(rows, C, dtype=torch.bool), 1: y > 0, 2: (c.double() * sc.double() + sh.double()) > 0}[mode]
        dz_ref = torch.where(mask, grad, torch.zeros(()))
        s1, s2, a1, a2 = R.bn_sums_ref(dz_ref, c, mean, invstd)
        for separate in (False, True):
            gd = grad.to(dev)
            dz_out = torch.full((rows, C), float("nan"), device=dev) if separate else None
            dgm, dbt = torch.empty(C, device=dev), torch.empty(C, device=dev)
            dc = ops.bn_bwd(gd, cd, saved, rows, C, rows, dgm, dbt, mode, ymask=y.to(store).to(dev) if mode == 1 else None, dz_out=dz_out)
            what = f"bn_bwd {rows}x{C} mode {mode} {'separate' if separate else 'in place'}"
            dz = dz_out if separate else gd
            if mode == 0 and not separate:
                assert torch.equal(gd.cpu(), grad)          # (no mask, no dz_out: g is left as it is)
            else:
                assert torch.equal(dz.cpu(), dz_ref), what + ": dz is not where(mask, g, 0) bit for bit"
            if separate:
                assert torch.equal(gd.cpu(), grad), what + ": g was written although dz_out was given"
            # sum dz: the terms are exact (0 roundings); sum dz * ((c - mean) * invstd): subtract, multiply, multiply = 3
            b1, b2 = R.col_bound(rows, C, 1024, 0, a1), R.col_bound(rows, C, 1024, 3, a2)
            within(dbt, s1, b1, what + " dbeta")
            within(dgm, s2, b2, what + " dgamma")
            # dc = k0 (dz - k1) - k2 (c - mean): each product is a subtraction and a multiplication, then the final subtraction: 3
            # roundings per product; k1 and k2 carry the sums' bounds and their own rounding to fp32 (the rest of their chain is fp64)
            dc_ref, A, B = R.bn_dc_ref(dz_ref, c, mean, invstd, sc, s1, s2, rows)
            k1, k2 = s1 / rows, sc.double() * invstd.double() * s2 / rows
            dk1 = b1 / rows + U * k1.abs()
            dk2 = (sc.double() * invstd.double()).abs() * b2 / rows + U * k2.abs()
            bound = 3 * U * (A.abs() + B.abs()) + sc.double().abs() * dk1 + (c.double() - mean.double()).abs() * dk2
            within(dc, dc_ref, bound * (1 + 8 * U), what + " dc")


@pytest.mark.parametrize("C", WIDTHS)
def test_bn_bwd_reduce_geometry(dev, C):
    from oaprogressionmmf_amd import ops
    for i, rows in enumerate(R.case_a_rows(C)):
        _bn_bwd_case(ops, dev, rows, C, 200 + i)


def _ln_param_case(ops, dev, rows, D, seed):
    g = gen(seed)
    x = torch.randn(rows, D, generator=g) * 3 + 1
    gam, bet = torch.randn(D, generator=g) * 0.5 + 1, torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    xd, gd = x.to(dev), gam.to(dev)
    _, mean, rstd = ops.layernorm_fwd(xd, gd, bet.to(dev), rows, D, 1e-5)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dx = ops.layernorm_bwd(dy.to(dev), xd, gd, mean, rstd, dg, db, rows, D)
    # the parameter-gradient kernel reads the fp32 mean / rstd it is given: the reference widens exactly those
    xh = (x.double() - mean.double().cpu()[:, None]) * rstd.double().cpu()[:, None]
    t = dy.double() * xh
    # dgamma terms dy * ((x - mean) * rstd): 3 roundings; dbeta terms: none.  Geometry: col_geom(rows, D, 256)
    within(dg, t.sum(0), R.col_bound(rows, D, 256, 3, t.abs()), f"layernorm_bwd dgamma {rows}x{D}")
    within(db, dy.double().sum(0), R.col_bound(rows, D, 256, 0, dy.double().abs()), f"layernorm_bwd dbeta {rows}x{D}")
    return x, gam, bet, dy, mean, rstd, dx


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_bwd_param_geometry(dev, D):
    from oaprogressionmmf_amd import ops
    for i, rows in enumerate(R.case_a_rows(D)):
        _ln_param_case(ops, dev, rows, D, 300 + i)


def test_column_reductions_rows_per_block_grow(dev):
    """rows / max_blk beyond 4 * RP: the blocks take more rows each (rpb 80 instead of 64 at C = 64; 6 instead of 4 at D = 2048)"""
    from oaprogressionmmf_amd import ops
    assert R.col_geom(70001, 64)["rpb"] == 80 and R.col_geom(1500, 2048, 256)["rpb"] == 6 and R.col_geom(16500, 64, 256)["rpb"] == 80
    _colstats_case(ops, dev, 70001, 64, 401)
    _bn_bwd_case(ops, dev, 70001, 64, 402, modes=(2,))
    _ln_param_case(ops, dev, 1500, 2048, 403)
    _ln_param_case(ops, dev, 16500, 64, 404)


@pytest.mark.parametrize("C", [6, 12, 20, 1536])
def test_column_reductions_refuse_unsupported_widths(dev, C):
    """col_geom is host code: it returns false -- and the entry points KOAF_EINVAL -- before anything is launched"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    rows = 8
    x = torch.zeros(rows, C, device=dev)
    v = torch.ones(C, device=dev)
    assert R.col_geom(rows, C) is None and ops.lib().koaf_colpart_rows(rows, C) == -1
    with pytest.raises(KoafError):
        ops.colstats(x, rows, C)
    with pytest.raises(KoafError):
        ops.bn_bwd(x.clone(), x, torch.stack([v, v, v, v]), rows, C, rows, v.clone(), v.clone(), 2)
    with pytest.raises(KoafError):
        ops.layernorm_bwd(x, x, v, torch.zeros(rows, device=dev), torch.ones(rows, device=dev), v.clone(), v.clone(), rows, C)
    # the entry points themselves refuse too (the wrappers above stop at the geometry query)
    part = torch.zeros(2 * rows * C + 16, device=dev)
    import ctypes
    r = ctypes.c_int32(0)
    assert ops.lib().koaf_colstats(x.data_ptr(), rows, C, part.data_ptr(), ctypes.addressof(r), None, 0, None) != 0
    torch.cuda.synchronize()


# =================================================================================================
# B. finalisation thresholds: one stage up to 128 partial rows, ceil(rows / 64) slices beyond, 64 slices from 4096
# =================================================================================================
PART_ROWS = [1, 16, 17, 128, 129, 191, 4095, 4096, 4100]


@pytest.mark.parametrize("C", [64, 200])
@pytest.mark.parametrize("rows", PART_ROWS)
def test_bn_finalize_thresholds(dev, rows, C):
    from oaprogressionmmf_amd import ops
    g = gen(500 + rows + C)
    count = 37 * rows
    for shifted in (False, True):
        # partial sums of `count` samples of variance about 1 around a mean of about 0.3 (about the shift when there is one)
        part = torch.empty(rows, 2, C)
        part[:, 0] = torch.randn(rows, C, generator=g) * 6 + 37 * 0.3
        part[:, 1] = (torch.rand(rows, C, generator=g) + 0.6) * 37 * 1.1
        gam, bet = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.2
        rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        shift = torch.randn(C, generator=g) if shifted else None
        rmd, rvd = rm.to(dev), rv.to(dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        mom, eps = 0.1, 1e-5
        saved = ops.bn_finalize(part.to(dev), C, count, gam.to(dev), bet.to(dev), rmd, rvd, nbt, mom, eps, True,
                                shift=None if shift is None else shift.to(dev))
        assert int(nbt) == 1
        s1, s2 = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
        acc = rows * 2.0 ** -52 * (part[:, 0].double().abs().sum(0) + s2) / count       # the fp64 accumulation's own error
        dm = s1 / count
        var = (s2 / count - dm * dm).clamp_min(0)
        m = dm + (shift.double() if shifted else 0.0)
        is_ = (var + eps).rsqrt()
        what = f"bn_finalize rows {rows} C {C} shift {shifted}"
        # mean: the fp64 result rounded once
        within(saved[0], m, U * m.abs() + acc, what + " mean")
        # invstd = 1 / sqrtf(fl(var) + eps): var's rounding (half of it reaches the root), the addition (half), sqrtf and the
        # division within an ulp (2u) each: <= 5 u relative; 6 for the second order
        within(saved[1], is_, 6 * U * is_ + acc * is_ ** 3, what + " invstd")
        # sc = gamma * invstd: one more rounding
        sc = gam.double() * is_
        within(saved[2], sc, 7 * U * sc.abs() + acc * (gam.double() * is_ ** 3).abs(), what + " sc")
        # sh = beta - (m * gamma) * invstd: m, two products, invstd's 6, the subtraction: 10 over the two magnitudes
        sh = bet.double() - m * sc
        within(saved[3], sh, 10 * U * (bet.double().abs() + (m * sc).abs()) + acc * (1 + (m * gam.double() * is_ ** 3).abs()), what + " sh")
        # running = (1 - f) * running + f * new: 1 - f, two products, the sum, and the new value's own rounding: 5
        rm_ref = (1 - mom) * rm.double() + mom * m
        within(rmd, rm_ref, 5 * U * (((1 - mom) * rm.double()).abs() + (mom * m).abs()) + acc, what + " running_mean")
        unb = var * (count / (count - 1))
        rv_ref = (1 - mom) * rv.double() + mom * unb
        within(rvd, rv_ref, 5 * U * (((1 - mom) * rv.double()).abs() + (mom * unb).abs()) + acc, what + " running_var")


@pytest.mark.parametrize("C", [64, 200])
@pytest.mark.parametrize("rows", PART_ROWS)
def test_bn_bwd_from_part_thresholds(dev, rows, C):
    from oaprogressionmmf_amd import ops
    g = gen(600 + rows + C)
    count, trows = 37 * rows, 8
    sc, sh = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.2
    mean, invstd = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    saved = saved_of(mean, invstd, sc, sh, dev)
    dz, c = torch.randn(trows, C, generator=g), torch.randn(trows, C, generator=g)
    dzmax = dz.abs().max().reshape(1).to(dev)
    for nsum, i1 in ((2, 1), (3, 1), (3, 2)):
        part = torch.randn(rows, nsum, C, generator=g) * 3
        s1, s2 = part[:, 0].double().sum(0), part[:, i1].double().sum(0)
        acc1 = rows * 2.0 ** -52 * part[:, 0].double().abs().sum(0)
        acc2 = rows * 2.0 ** -52 * part[:, i1].double().abs().sum(0)
        for train in (True, False):
            dgm, dbt = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
            ap = ops.bn_bwd_from_part(part.to(dev), nsum, i1, dz.to(dev), c.to(dev), saved, trows, C, count, dgm, dbt, fused=True,
                                      dzmax=dzmax, train=train)
            what = f"bn_bwd_from_part rows {rows} C {C} ({nsum},{i1}) train {train}"
            # dbeta / dgamma: the fp64 sums rounded once
            within(dbt, s1, U * s1.abs() + acc1, what + " dbeta")
            within(dgm, s2, U * s2.abs() + acc2, what + " dgamma")
            coef = ap.coef.cpu()
            assert coef.shape == (4, C)
            assert torch.equal(coef[0], sc), what + " coef[0] is sc itself"
            if not train:
                assert torch.equal(coef[1:], torch.zeros(3, C)), what + " eval: dc = sc * dz"
                continue
            k1 = s1 / count
            k2 = sc.double() * invstd.double() * s2 / count
            # k1, k2: fp64 expressions rounded once
            within(coef[1], k1, U * k1.abs() + acc1 / count, what + " coef[1]")
            within(coef[2], k2, U * k2.abs() + acc2 / count * (sc.double() * invstd.double()).abs(), what + " coef[2]")
            # coef[3] = k2 * mean - k0 * k1 in fp32 from the rounded k1, k2: their rounding, a product each, the subtraction: 3
            k3 = k2 * mean.double() - sc.double() * k1
            within(coef[3], k3, 3 * U * ((k2 * mean.double()).abs() + (sc.double() * k1).abs()) * (1 + 8 * U) +
                   (acc1 + acc2) / count * 4, what + " coef[3]")


# =================================================================================================
# C. tails and the grid cap
# =================================================================================================
def _pointwise_case(ops, dev, n, seed):
    g = gen(seed)
    x, dy = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)
    xd, dyd = x.to(dev), dy.to(dev)
    # no arithmetic: bit-equal
    assert torch.equal(ops.relu_fwd(xd).cpu(), torch.relu(x)), f"relu_fwd n={n}"
    assert torch.equal(ops.relu_bwd(dyd, xd).cpu(), torch.where(x > 0, dy, torch.zeros(()))), f"relu_bwd n={n}"
    # one rounding (k = 1): the fp32 sum of two fp32 values
    s = x.double() + dy.double()
    within(ops.add(xd, dyd), s, U * s.abs(), f"add n={n}")
    assert torch.equal(ops.add(xd, dyd).cpu(), x + dy), f"add n={n}"       # (and correctly rounded: the same bits as torch's)
    # erff / expf: the yardstick rule; floors = test_pointwise_loss_adam's 1e-6 / 1e-5 norm ratios times max|ref|
    x64 = x.double()
    ref = R.gelu_ref(x64)
    # measured: kernel 4.5e-07 / torch fp32 1.2e-06 at n = 8388615, 4.2e-07 / 8.0e-07 at n = 1023, <= 8.3e-08 / 5.6e-07 at n <= 7
    yardstick(ops.gelu_fwd(xd), ref, F.gelu(x), f"gelu_fwd n={n}", floor=1e-6 * float(ref.abs().max()))
    xg = x.clone().requires_grad_(True)
    F.gelu(xg).backward(dy)
    refb = dy.double() * R.gelu_grad_ref(x64)
    # measured: kernel 6.4e-07 / torch fp32 9.0e-07 at n = 8388615, 2.3e-07 / 3.7e-07 at n = 1023, <= 1.4e-07 / 1.4e-07 at n <= 7
    yardstick(ops.gelu_bwd(dyd, xd), refb, xg.grad, f"gelu_bwd n={n}", floor=1e-5 * float(refb.abs().max()))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 1023])
def test_pointwise_tails(dev, n):
    from oaprogressionmmf_amd import ops
    _pointwise_case(ops, dev, n, 700 + n)


@needs_default_cap
def test_pointwise_past_the_grid_cap(dev):
    from oaprogressionmmf_amd import ops
    _pointwise_case(ops, dev, 4 * (CAP + 1) + 3, 799)


@needs_default_cap
@pytest.mark.parametrize("dtype,lo,hi", [(torch.uint8, 0, 256), (torch.uint16, 0, 65536), (torch.int16, -32768, 32768)])
def test_widen_tails_and_cap(dev, dtype, lo, hi):
    from oaprogressionmmf_amd import ops
    g = gen(800)
    for n in (1, 3, 5, 4 * (CAP + 1) + 2):
        raw = torch.randint(lo, hi, (n,), generator=g, dtype=torch.int32)
        raw[0], raw[-1] = lo, hi - 1
        x = raw.to(dtype)
        assert torch.equal(ops.widen(x.to(dev)).cpu(), raw.float()), (dtype, n)


@needs_default_cap
def test_fill_dropout_past_the_grid_cap(dev):
    from oaprogressionmmf_amd import ops
    n = CAP + 5
    buf = torch.zeros(n + 3, device=dev)
    ops.check(ops.lib().koaf_fill(buf.data_ptr(), 1.5, n, None), "fill")
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.cat([torch.full((n,), 1.5), torch.zeros(3)]))
    p, seed = 0.25, 4242                     # (exact in fp32, so that 1 / (1 - p) is one rounding)
    x = (torch.rand(n, generator=gen(801)) + 0.5)
    xd = x.to(dev)
    d1 = ops.dropout(xd, p, seed)
    assert torch.equal(d1, ops.dropout(xd, p, seed)) and not torch.equal(d1, ops.dropout(xd, p, seed + 1))
    d1c = d1.cpu()
    kept = d1c != 0
    # keep rate: binomial(n, 1 - p), 4 standard deviations
    assert abs(float(kept.double().mean()) - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n)
    # kept values: x * fl(1 / (1 - p)): the factor's rounding and the product's (k = 2)
    within(d1c[kept], x[kept].double() / (1 - p), 2 * U * x[kept].double() / (1 - p), "dropout scaling")
    # the generator is counter-based: element i draws the same number whatever n is
    assert torch.equal(d1c[:1000], ops.dropout(xd[:1000].clone(), p, seed).cpu())
    assert torch.equal(d1c[-5:] != 0, (ops.dropout(torch.ones(n, device=dev), p, seed)[-5:] != 0).cpu())
    # dropout2d: (image, channel) planes, index n * C + c -- the draw the element-wise kernel makes on the pooled (N, C) tensor
    N, HW, C = 2, 16385, 64
    assert N * HW * C > CAP
    x2 = (torch.rand(N, HW, C, generator=gen(802)) + 0.5)
    y2 = ops.dropout2d(x2.to(dev), N, HW, C, p, seed)
    assert torch.equal(y2, ops.dropout2d(x2.to(dev), N, HW, C, p, seed))
    keep_nc = (ops.dropout(torch.ones(N, C, device=dev), p, seed) != 0).cpu()
    y2c = y2.cpu()
    assert torch.equal(y2c != 0, keep_nc[:, None, :].expand(N, HW, C))
    k2 = y2c != 0
    within(y2c[k2], x2[k2].double() / (1 - p), 2 * U * x2[k2].double() / (1 - p), "dropout2d scaling")


def _tail_case(ops, dev, rows, C, seed, store=torch.float32):
    """bn_add_relu (plain, + identity, + identity through its own BatchNorm) and bn_bwd_apply, per element.  store: the storage of
    c, idt and y; y stored as bf16 owes the fp32 bound B plus the rounding of the store, elem_refs.stored16_bound(ref, B)"""
    g = gen(seed)
    c, idt = R.stored(torch.randn(rows, C, generator=g), store), R.stored(torch.randn(rows, C, generator=g), store)
    out_bound = (lambda ref, B: B) if store == torch.float32 else R.stored16_bound
    s3 = torch.stack([torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5 + 1,
                      torch.randn(C, generator=g) * 0.1])
    sd = torch.stack([torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5 + 1,
                      torch.randn(C, generator=g) * 0.1])
    cd, idd, s3d, sdd = c.to(store).to(dev), idt.to(store).to(dev), s3.to(dev), sd.to(dev)
    c64, i64 = c.double(), idt.double()
    p1, h1 = c64 * s3[2].double(), s3[3].double()
    p2, h2 = i64 * sd[2].double(), sd[3].double()
    # relu is 1-Lipschitz: the bound of its argument holds for its result
    # fmaf(c, sc, sh): one rounding (k = 1)
    ref = torch.relu(p1 + h1)
    yk = ops.bn_add_relu(cd, s3d, rows, C)
    assert yk.dtype == store
    within(yk, ref, out_bound(ref, U * (p1.abs() + h1.abs())), f"bn_add_relu {rows}x{C}")
    # fmaf(c, sc, sh) + idt: k = 2
    ref = torch.relu(p1 + h1 + i64)
    within(ops.bn_add_relu(cd, s3d, rows, C, idt=idd), ref, out_bound(ref, 2 * U * (p1.abs() + h1.abs() + i64.abs())),
           f"bn_add_relu + idt {rows}x{C}")
    # fmaf(c, sc, sh) + fmaf(idt, idsc, idsh): k = 2 along either branch (its fma, the sum)
    ref = torch.relu(p1 + h1 + p2 + h2)
    within(ops.bn_add_relu(cd, s3d, rows, C, idt=idd, idsaved=sdd), ref,
           out_bound(ref, 2 * U * (p1.abs() + h1.abs() + p2.abs() + h2.abs())), f"bn_add_relu + idt + idsaved {rows}x{C}")
    # bn_bwd_apply from hand-made coefficients: k0 * (dz - k1) - k2 * (c - mean): subtraction, product, final subtraction: k = 3
    dz = torch.randn(rows, C, generator=g)
    coef = torch.stack([s3[2], torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1])
    A = coef[0].double() * (dz.double() - coef[1].double())
    B = coef[2].double() * (c64 - s3[0].double())
    dc = ops.BnApply(dz.to(dev), cd, coef.to(dev), None, s3d[0], rows, C).materialize()
    within(dc, A - B, 3 * U * (A.abs() + B.abs()) * (1 + 8 * U), f"bn_bwd_apply {rows}x{C}")


@needs_default_cap
@pytest.mark.parametrize("rows,C", [(CAP // 16 + 1, 64), (CAP + 3, 4), (7, 64)])
def test_bottleneck_tail_and_bn_apply_past_the_grid_cap(dev, rows, C):
    """rows * C / 4 vectors: cap + 16 at C = 64 (a whole number of rows: cap + 3 is not one), cap + 3 at C = 4; and a small one"""
    from oaprogressionmmf_amd import ops
    _tail_case(ops, dev, rows, C, 810 + C)


def _maxpool_case(ops, dev, N, H, W, C, seed, exact=True, loop_ref=True, store=torch.float32):
    """store: the storage of the pool's input c and of its output y (the arg-max bytes and the gradients do not depend on it)"""
    g = gen(seed)
    OH, OW = R.pool_out(H), R.pool_out(W)
    if exact:
        # sc in {0.5, 1, 2}, sh and c multiples of 1/16: sc * c + sh is exact in fp32, ties are true ties
        sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
        sh = torch.randint(-8, 9, (C,), generator=g).float() / 16
        c = R.stored(R.draw_grid(g, (N, H, W, C)), store)        # (grid values are bf16 values: test_elem_edges_cpu.py)
    else:
        sc, sh = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3
        c = R.stored(torch.randn(N, H, W, C, generator=g), store)
    a = torch.relu(c.double() * sc.double() + sh.double())
    y_ref, am_ref = R.maxpool_ref(a)
    saved = saved_of(sc, sc, sc, sh, dev)
    y, am = ops.maxpool_fwd(c.to(store).to(dev), saved, N, H, W, C)
    what = f"maxpool {N}x{H}x{W}x{C} {'exact' if exact else 'random'}"
    assert y.shape == (N, OH, OW, C) and y.dtype == store
    if exact:
        assert torch.equal(y.double().cpu(), y_ref), what + ": y"
        assert torch.equal(am.cpu(), am_ref), what + ": arg-max is not the first maximum in row-major window order"
    else:
        # fmaxf(c * sc + sh, 0): a product and a sum, or one fused rounding: k = 2 over the window's largest |terms|; the maximum of
        # values each within e of the reference's is within e of the reference's maximum
        e = 2 * U * float(((c.double() * sc.double()).abs() + sh.double().abs()).max())
        within(y, y_ref, e if store == torch.float32 else R.stored16_bound(y_ref, e), what + ": y")
        if store == torch.bfloat16:
            # the storage contract of test_bf16_gpu.py: the fp32 instantiation's y on the widened input, rounded once by torch
            y32, am32 = ops.maxpool_fwd(c.to(dev), saved, N, H, W, C)
            assert torch.equal(y, y32.bfloat16()) and torch.equal(am, am32), what + ": not the fp32 mode's result rounded once"
    dy = torch.randn(N, OH, OW, C, generator=g)
    # the gradient lands where the kernel's own arg-max says (checked above against the reference's where the data allow it)
    da_ref, ab = (R.maxpool_bwd_ref if loop_ref else R.maxpool_bwd_gather_ref)(dy, am.cpu(), H, W)
    da = ops.maxpool_bwd(dy.to(dev), am, N, H, W, C)
    # at most four windows meet in a pixel: three additions (k = 3)
    within(da, da_ref, 3 * U * ab, what + ": maxpool_bwd")
    return c, sc, sh, y, am, dy, da


@needs_default_cap
def test_maxpool_past_the_grid_cap(dev):
    from oaprogressionmmf_amd import ops
    N, H, W, C = 2, 514, 514, 64
    assert N * R.pool_out(H) * R.pool_out(W) * C // 4 == 2113568 > CAP
    _maxpool_case(ops, dev, N, H, W, C, 820, exact=True, loop_ref=False)


@needs_default_cap
def test_gap_bwd_past_the_grid_cap(dev):
    from oaprogressionmmf_amd import ops
    N, HW, C = 1311, 100, 64
    assert N * HW * C // 4 > CAP
    d = torch.randn(N, C, generator=gen(830))
    got = ops.gap_bwd(d.to(dev), N, HW, C).cpu()
    ref = (d.double() / HW)[:, None, :].expand(N, HW, C)
    # dout * fl(1 / HW): the factor's rounding and the product's -- within 2 ulp of dout / HW
    within(got, ref, 2 * torch.from_numpy(np.spacing(ref.float().abs().numpy())).double(), "gap_bwd past the cap")


# =================================================================================================
# D. max-pool borders and ties
# =================================================================================================
POOL_SHAPES = [(1, 1, 1), (2, 1, 7), (2, 7, 1), (1, 2, 2), (3, 5, 8), (2, 9, 6)]


def _pool_bn_bwd(ops, dev, c, sc, sh, am, dy, da, N, H, W, C, seed, store=torch.float32):
    """bn_bwd(pool=...): the pool's input gradient gathered inside the BatchNorm reduction -- dz bit-equal to maxpool_bwd followed
    by the mask, sums inside the case A bound.  store: the storage of c (given widened, as _maxpool_case returns it)"""
    g = gen(seed)
    rows = N * H * W
    mean, invstd = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    saved = saved_of(mean, invstd, sc, sh, dev)
    cd = c.to(store).to(dev)
    dgm, dbt = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ap = ops.bn_bwd(None, cd, saved, rows, C, rows, dgm, dbt, 2, fused=True, pool=(dy.to(dev), am, N, H, W))
    mask = ((c.double() * sc.double() + sh.double()) > 0).reshape(rows, C)
    dz_ref = torch.where(mask, da.cpu().reshape(rows, C), torch.zeros(()))
    what = f"bn_bwd(pool) {N}x{H}x{W}x{C}"
    assert torch.equal(ap.dz.reshape(rows, C).cpu(), dz_ref), what + ": dz"
    s1, s2, a1, a2 = R.bn_sums_ref(dz_ref, c.reshape(rows, C), mean, invstd)
    # each dz term is itself a sum of up to four gradients (k = 3) before it enters the column sum; the reference sums the
    # kernel's own fp32 dz, so those roundings are on both sides: 0 and 3 term roundings as in case A
    within(dbt, s1, R.col_bound(rows, C, 1024, 0, a1), what + " dbeta")
    within(dgm, s2, R.col_bound(rows, C, 1024, 3, a2), what + " dgamma")


@pytest.mark.parametrize("C", [4, 64, 128])
@pytest.mark.parametrize("N,H,W", POOL_SHAPES)
def test_maxpool_borders(dev, N, H, W, C):
    from oaprogressionmmf_amd import ops
    for exact in (True, False):
        c, sc, sh, y, am, dy, da = _maxpool_case(ops, dev, N, H, W, C, 900 + H * 16 + W + C, exact=exact)
        if exact:       # (exact pre-activations: the mask's sign needs no margin; zeros are masked on both sides alike)
            _pool_bn_bwd(ops, dev, c, sc, sh, am, dy, da, N, H, W, C, 950 + C)


def _maxpool_ties_case(ops, dev, C, store=torch.float32):
    """windows that are all zero after the ReLU, and windows with the same positive value at two or more positions (copied
    pre-activations, the same sc / sh in every channel): the first position in row-major window order is recorded, as
    F.max_pool2d does (test_elem_edges_cpu.py holds the reference to that), and the gradient goes there alone.
    store: the storage of c and y (every value here is a bf16 value)"""
    N, H, W = 2, 9, 10
    g = gen(960)
    sc, sh = torch.full((C,), 0.5), torch.full((C,), 0.25)
    c = R.draw_grid(g, (N, H, W, C))
    c[0, :4] = -3.0                                  # relu(0.5 * -3 + 0.25) = 0: all-zero windows, arg-max = first valid position
    c[0, 5:8, 2:7] = c[0, 5:6, 2:3] .abs() + 1.0     # a 3 x 5 patch of one positive value: ties inside and across windows
    c[1, :, 1::2] = c[1, :, 0:-1:2]                  # every column equals its left neighbour
    assert torch.equal(R.stored(c, store), c)
    a = torch.relu(c.double() * 0.5 + 0.25)
    y_ref, am_ref = R.maxpool_ref(a)
    assert int((y_ref == 0).sum()) > 0
    y, am = ops.maxpool_fwd(c.to(store).to(dev), saved_of(sc, sc, sc, sh, dev), N, H, W, C)
    assert y.dtype == store and torch.equal(y.double().cpu(), y_ref)
    assert torch.equal(am.cpu(), am_ref), "a tie is not resolved to the first maximum in row-major window order"
    dy = torch.randn(N, R.pool_out(H), R.pool_out(W), C, generator=g)
    da_ref, ab = R.maxpool_bwd_ref(dy, am_ref, H, W)
    da = ops.maxpool_bwd(dy.to(dev), am, N, H, W, C)
    within(da, da_ref, 3 * U * ab, "maxpool_bwd on ties")         # (k = 3: at most four windows meet in a pixel)
    a_leaf = a.clone().permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(a_leaf, 3, 2, 1).backward(dy.double().permute(0, 3, 1, 2))
    within(da, a_leaf.grad.permute(0, 2, 3, 1), 3 * U * ab, "maxpool_bwd on ties vs float64 autograd")
    _pool_bn_bwd(ops, dev, c, sc, sh, am, dy, da, N, H, W, C, 961, store=store)


@pytest.mark.parametrize("C", [4, 64])
def test_maxpool_ties(dev, C):
    from oaprogressionmmf_amd import ops
    _maxpool_ties_case(ops, dev, C)


@pytest.mark.parametrize("W", [1, 5, 7, 15, 16, 17])
def test_pool_gather_walk_around_rp(dev, W):
    """the gather carries (ix, iy, n) from pass to pass by ix += RP and wrapping: W below, at and above RP = 16 (C = 64); several
    passes per thread, several images"""
    from oaprogressionmmf_amd import ops
    N, H, C = 3, 11, 64
    assert R.col_rp(C) == 16
    c, sc, sh, y, am, dy, da = _maxpool_case(ops, dev, N, H, W, C, 970 + W, exact=True)
    _pool_bn_bwd(ops, dev, c, sc, sh, am, dy, da, N, H, W, C, 980 + W)


# =================================================================================================
# E. global average pooling
# =================================================================================================
@pytest.mark.parametrize("C", [4, 64, 2048])
@pytest.mark.parametrize("HW", [1, 2, 49, 100])
def test_gap(dev, HW, C):
    from oaprogressionmmf_amd import ops
    for N in (1, 3):
        g = gen(1000 + HW + C + N)
        y = torch.randn(N, HW, C, generator=g) + 0.5
        # HW additions in order, then * fl(1 / HW): m = HW + 2
        within(ops.gap_fwd(y.to(dev), N, HW, C), y.double().mean(1), gamma(HW + 2) * y.double().abs().sum(1) / HW, f"gap_fwd {N}x{HW}x{C}")
        d = torch.randn(N, C, generator=g)
        ref = (d.double() / HW)[:, None, :].expand(N, HW, C)
        # dout * fl(1 / HW): two roundings -- within 2 ulp of dout / HW
        within(ops.gap_bwd(d.to(dev), N, HW, C), ref, 2 * torch.from_numpy(np.spacing(ref.float().abs().numpy())).double(),
               f"gap_bwd {N}x{HW}x{C}")


# =================================================================================================
# F. LayerNorm
# =================================================================================================
def _ln_case(ops, dev, rows, D, seed, x=None, tag=""):
    g = gen(seed)
    if x is None:
        x = torch.randn(rows, D, generator=g) * 3 + 1
    gam, bet = torch.randn(D, generator=g) * 0.5 + 1, torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    eps = 1e-5
    xd, gd = x.to(dev), gam.to(dev)
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bet.to(dev), rows, D, eps)
    y_ref, m_ref, rs_ref = R.layernorm_ref(x, gam, bet, eps)
    what = f"layernorm {rows}x{D}{tag}"
    # mean: per lane ceil(D / 256) steps of four additions, six wave-shuffle additions, the division: m = 4 ceil(D / 256) + 7
    within(mean, m_ref, gamma(4 * R.cdiv(D, 256) + 7) * x.double().abs().sum(1) / D, what + " mean")
    # rsqrt / division: the yardstick rule, floors = test_layernorm's 2e-6 (y) and 1e-5 (dx) norm ratios times max|ref|
    xl = x.clone().requires_grad_(True)
    y32 = F.layer_norm(xl, (D,), gam, bet, eps)
    y32.backward(dy)
    rs32 = (x.var(1, unbiased=False) + eps).rsqrt()
    yardstick(rstd, rs_ref, rs32, what + " rstd", floor=2e-6 * float(rs_ref.abs().max()))
    yardstick(y, y_ref, y32, what + " y", floor=2e-6 * float(y_ref.abs().max()))
    x64 = x.double().requires_grad_(True)
    F.layer_norm(x64, (D,), gam.double(), bet.double(), eps).backward(dy.double())
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dx = ops.layernorm_bwd(dy.to(dev), xd, gd, mean, rstd, dg, db, rows, D)
    yardstick(dx, x64.grad, xl.grad, what + " dx", floor=1e-5 * float(x64.grad.abs().max()))
    return y, mean, rstd


# measured (kernel / torch fp32), worst over every D and row count: rstd 3.5e-08 / 4.6e-08, y 9.6e-07 / 9.6e-07 (5 x 4096), dx 3.1e-07 /
# 4.8e-07; the floors (2e-6 and 1e-5 of max|ref|) are what binds at these sizes
@pytest.mark.parametrize("D", [4, 8, 128, 256, 1024, 2048, 4096])
def test_layernorm_shapes(dev, D):
    from oaprogressionmmf_amd import ops
    for rows in (1, 3, 4, 5):       # four rows to a block: a partial last block, and a second block of one row
        _ln_case(ops, dev, rows, D, 1100 + D + rows)
        _ln_param_case(ops, dev, rows, D, 1150 + D + rows)


def test_layernorm_offset_mean_and_constant_row(dev):
    from oaprogressionmmf_amd import ops
    rows, D = 5, 1024
    # a mean a hundred standard deviations from zero: E[x^2] - E[x]^2 in fp32 would lose the variance's leading digits
    # measured (kernel / torch fp32): rstd 1.1e-06 / 7.0e-07, y 1.8e-05 / 1.7e-05, dx 1.0e-05 / 6.7e-05
    x = 10 + 0.1 * torch.randn(rows, D, generator=gen(1190))
    _ln_case(ops, dev, rows, D, 1191, x=x, tag=" offset mean")
    # a constant row: every output finite, y within D u |c| rstd |gamma| of beta (the mean of D equal fp32 values is off by at
    # most D u |c|; nothing else separates x - mean from zero)
    D, cval = 256, 3.0
    g = gen(1192)
    x = torch.randn(3, D, generator=g)
    x[1] = cval
    gam, bet = torch.randn(D, generator=g) * 0.5 + 1, torch.randn(D, generator=g)
    y, mean, rstd = ops.layernorm_fwd(x.to(dev), gam.to(dev), bet.to(dev), 3, D, 1e-5)
    assert torch.isfinite(y).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    within(y[1], bet.double(), D * U * cval * float(rstd[1]) * gam.double().abs(), "layernorm constant row")
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dx = ops.layernorm_bwd(torch.randn(3, D, generator=g).to(dev), x.to(dev), gam.to(dev), mean, rstd, dg, db, 3, D)
    assert torch.isfinite(dx).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()


# =================================================================================================
# G. softmax and attention
# =================================================================================================
def _softmax_case(ops, dev, x, what):
    rows, n = x.shape
    ref = x.double().softmax(-1)
    got = ops.softmax_rows_(x.clone().to(dev)).cpu()
    assert torch.isfinite(got).all(), what + ": non-finite"
    # floor: test_attention's 2e-6 norm ratio times max|ref|
    bar = yardstick(got, ref, x.softmax(-1), what, floor=2e-6 * float(ref.abs().max()))
    # a row of n values each within the bar, added in float64 here: n u for the kernel's own normalisation sum
    assert float((got.double().sum(-1) - 1).abs().max()) <= n * U + bar, what + ": rows do not sum to 1"


# measured (kernel / torch fp32), worst over the shapes: O(1) logits 1.4e-08 / 1.4e-08 (5 x 65), +-200 logits 1.0e-07 / 1.0e-07 (4 x 65);
# n = 1: 0 / 0
@pytest.mark.parametrize("rows", [1, 4, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_softmax_rows(dev, n, rows):
    from oaprogressionmmf_amd import ops
    g = gen(1200 + n + rows)
    _softmax_case(ops, dev, torch.randn(rows, n, generator=g), f"softmax {rows}x{n} O(1)")
    x = (torch.rand(rows, n, generator=g) - 0.5) * 400
    x[rows - 1] = 173.25                     # an all-equal row: 1 / n everywhere
    _softmax_case(ops, dev, x, f"softmax {rows}x{n} +-200")


def _attention_case(ops, dev, B, n, h, d, seed):
    g = gen(seed)
    dim = h * d
    scale = dim ** -0.5
    qkv = torch.randn(B, n, 3 * dim, generator=g).double().requires_grad_(True)
    q, k, v = qkv.reshape(B, n, 3, h, d).permute(2, 0, 3, 1, 4)
    attn_ref = (torch.einsum("bhid,bhjd->bhij", q, k) * scale).softmax(-1)
    out_ref = torch.einsum("bhij,bhjd->bhid", attn_ref, v).permute(0, 2, 1, 3).reshape(B, n, dim)
    dout = torch.randn(B, n, dim, generator=g)
    out_ref.backward(dout.double())
    qd = qkv.detach().float().to(dev)
    out, attn = ops.attention_fwd(qd, B, n, h, d, scale)
    # test_attention's bars
    assert rel_err(attn, attn_ref) < 2e-6, (n, h, d)
    assert rel_err(out, out_ref) < 2e-6, (n, h, d)
    assert rel_err(ops.attention_bwd(dout.to(dev), qd, attn, B, n, h, d, scale), qkv.grad) < 2 * BWD, (n, h, d)
    # and no row of attn may be off where the norm does not look: every row sums to 1 (n u for the sum, 2e-6 the bar above)
    assert float((attn.double().sum(-1) - 1).abs().max()) <= n * U + 2e-6


@pytest.mark.parametrize("n", [1, 2, 63, 65, 129, 300, 384])
def test_attention_key_chunks(dev, n):
    """one, two and three 128-key chunks (three are padded to four: both wave groups run the same barriers)"""
    from oaprogressionmmf_amd import ops
    _attention_case(ops, dev, 2, n, 2, 32, 1300 + n)


@pytest.mark.parametrize("d", [4, 132, 384, 6])
def test_attention_head_widths(dev, d):
    """d = 132 / 384: two and three 128-column chunks of P V (three padded to four); d = 6: d & 3 != 0, which the fused kernel
    declines on the host -- the three-launch path takes it on the GEMM's unaligned loaders"""
    from oaprogressionmmf_amd import ops
    _attention_case(ops, dev, 2, 40, 2, d, 1350 + d)


# measured (kernel / torch fp32): n = 100 fused 1.5e-07 / 1.5e-07, n = 520 three launches 2.7e-07 / 2.7e-07
@pytest.mark.parametrize("n", [100, 520])
def test_attention_large_exact_logits(dev, n):
    """scores that are exact in fp32 and reach +-256: q in {0, +-1, +-2, +-4}, k multiples of 0.5 up to 8, h = 4, d = 16.  With
    the model's scale (h d)^-0.5 = 1 / 8 such operands cannot pass |score| = 4 * 8 * 16 / 8 = 64, below expf's overflow at 88.7, so
    the scale handed to the entry point is 1 / 2 (a power of two: the scores stay exact) and rows 0..3 reach +-256.  A softmax
    without the row maximum returns Inf / NaN there.  n = 100: the fused kernel; n = 520: three launches (koaf_softmax_rows)"""
    from oaprogressionmmf_amd import ops
    B, h, d, scale = 1, 4, 16, 0.5
    q, k, v = R.exact_attention_qk(gen(1400 + n), n, h, d)
    qkv = torch.stack([q, k, v], 0).permute(1, 0, 2, 3).reshape(1, n, 3 * h * d).contiguous()
    s64 = torch.einsum("ihd,jhd->hij", q.double(), k.double()) * scale
    s32 = torch.einsum("ihd,jhd->hij", q, k) * scale
    assert torch.equal(s32.double(), s64) and float(s64.abs().max()) >= 150        # exact, and large
    ref = s64.softmax(-1)[None]
    out, attn = ops.attention_fwd(qkv.to(dev), B, n, h, d, scale)
    assert torch.isfinite(attn).all() and torch.isfinite(out).all()
    yardstick(attn, ref, s32.softmax(-1)[None], f"attention exact logits n={n}", floor=2e-6 * float(ref.abs().max()))
    out_ref = torch.einsum("hij,jhd->ihd", ref[0], v.double()).reshape(1, n, h * d)
    assert rel_err(out, out_ref) < 2e-6


# =================================================================================================
# H. input pipeline and layout moves
# =================================================================================================
def _aug_states(which):
    """(cos, sin, exponent or 0, rotated) rows in PTBatchAugment's layout"""
    rot = lambda deg: (math.cos(math.radians(deg)), math.sin(math.radians(deg)), 1.0)      # noqa: E731
    none = (1.0, 0.0, 0.0)
    table = {"a": [(none, 0.0), (rot(0.0), 2.0), (rot(7.0), 0.5)],
             "b": [(rot(90.0), 2.0), (rot(45.0), 0.5), (none, 0.5)],
             "c": [(rot(-11.0), 0.0), (rot(45.0), 2.0), (rot(90.0), 0.0)]}
    return torch.tensor([[r[0], r[1], ex, r[2]] for r, ex in table[which]], dtype=torch.float32)


# measured, exponent 0.5 (kernel / torch fp32): 7 degrees 4.4e-05 / 2.2e-05 (24 x 20, S = 3; the square root steepens next to the
# sample's minimum), 45 degrees 1.2e-05 / 1.1e-05, not rotated 5.3e-07 / 5.0e-07
@pytest.mark.parametrize("Rr,Cc", [(5, 7), (24, 20)])
@pytest.mark.parametrize("S", [1, 3, 4, 8])
def test_augment_both_vector_widths(dev, S, Rr, Cc):
    """koaf_augment against float64 affine_grid + grid_sample around the unit-range, gamma and normalise steps; S % 4 == 0 takes
    the four-slices-per-thread instantiation, whose result must be, bit for bit, that of each slice run on its own (S = 1)"""
    from oaprogressionmmf_amd import ops
    B, mean, std = 3, 0.4, 0.2
    g = gen(1500 + S + Rr)
    for which in ("a", "b", "c"):
        raw = (torch.rand(B, Rr, Cc, S, generator=g) * 0.7 + 0.3) * 300.0
        raw[:, 0, 0, 0], raw[:, Rr - 1, Cc - 1, 0] = 5.0, 310.0       # the extremes: corner pixels of slice 0
        prm = _aug_states(which)
        xd = raw.to(dev)
        mm = ops.minmax(xd, B)
        assert torch.equal(mm.cpu(), torch.tensor([[5.0, 310.0]] * B))
        y = ops.augment(xd, mm, prm.to(dev), B, Rr, Cc, S, mean, std).cpu()
        ref = R.augment_ref(raw, prm, mean, std)
        y32 = R.augment_ref(raw, prm, mean, std, dtype=torch.float32)
        for b in range(B):
            ex = float(prm[b, 2])
            what = f"augment {which}{b} S={S} {Rr}x{Cc} ex={ex}"
            if ex == 0.5:
                yardstick(y[b], ref[b], y32[b], what, floor=2e-5)
            else:
                # test_batch_augment_vs_reference's bar (fixture F12): 2e-5 absolute on values of order 1
                e = float((y[b].double() - ref[b]).abs().max())
                assert e < 2e-5, f"{what}: off by {e:.3e}"
        if S > 1:
            for s in range(S):
                one = raw[..., s:s + 1].contiguous().to(dev)
                ys = ops.augment(one, mm, prm.to(dev), B, Rr, Cc, 1, mean, std).cpu()
                assert torch.equal(ys[..., 0], y[..., s]), f"augment {which} S={S}: slice {s} differs from its own S = 1 run"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 4096 + 1, 300 * 4096 + 1])
def test_minmax_edges(dev, n, B):
    """one block covers 4096 elements up to 256 blocks, which then stride: the last two sizes are several blocks + 1 and past that"""
    from oaprogressionmmf_amd import ops
    g = gen(1600 + B)
    x = torch.randn(B, n, generator=g)
    x[B - 1] = 2.5                               # a constant sample
    if n > 1:
        x[0, n // 2] = -0.0
        x[0, n - 1] = x[0].max() + 1             # the maximum in the last element, the part a dropped tail would lose
    mm = ops.minmax(x.to(dev), B).cpu()
    assert torch.equal(mm[:, 0], x.amin(1)) and torch.equal(mm[:, 1], x.amax(1))
    z = torch.zeros(1, n)
    z[0, n - 1] = -0.0
    mz = ops.minmax(z.to(dev), 1).cpu()
    assert torch.equal(mz, torch.zeros(1, 2))    # (-0.0 == 0.0)


@pytest.mark.parametrize("shape,mode", [((2, 3, 13), "linear"), ((2, 2, 7, 9), "bilinear"), ((1, 2, 5, 7, 6), "trilinear")])
def test_resize_edges(dev, shape, mode):
    """identity, output size 1, x2.5 and x0.37 against float64 F.interpolate at test_interpolate_any_scale_vs_reference's bar, 2e-6
    of the largest magnitude per element.  The shapes are small on purpose: the kernel forms the source coordinate in fp32 as
    torch's fp32 op does (fixture F8 pins it to that op's values), so the coordinate carries a few of its own ulps, times the
    slope between neighbours.  Below 16 that is under the bar; at 41 -> 102 it is not, for the kernel (8.7e-06) as for torch's
    own fp32 op (8.8e-06, bar 5.6e-06), and a kernel that placed the samples exactly would leave fixture F8's bar instead (7.0e-06
    of 5.2e-06 on xr_075).  Torch's fp32 op on the same input is held to the same bar beside it."""
    from oaprogressionmmf_amd import ops
    x = torch.randn(*shape, generator=gen(1700 + len(shape)))
    xd = x.to(dev)
    sp = shape[2:]
    assert torch.equal(ops.resize(xd, list(sp)).cpu(), x), "identity size is not the identity"
    for what, size in (("size 1", [1] * len(sp)), ("x2.5", [int(math.floor(v * 2.5)) for v in sp]),
                       ("x0.37", [max(1, int(math.floor(v * 0.37))) for v in sp])):
        ref = F.interpolate(x.double(), size=size, mode=mode, align_corners=False)
        ref32 = F.interpolate(x, size=size, mode=mode, align_corners=False)
        got = ops.resize(xd, size).cpu()
        assert got.shape == ref.shape
        bar = 2e-6 * float(ref.abs().max())
        e, e32 = float((got.double() - ref).abs().max()), float((got - ref32).abs().max())
        print(f"RESIZE {mode} {what}: vs float64 {e:.3e}, vs torch fp32 {e32:.3e}, bar {bar:.3e}")
        assert e < bar, f"resize {mode} {what}: off the float64 op by {e:.3e} (bar {bar:.3e})"
        assert e32 < bar, f"resize {mode} {what}: off torch's fp32 op by {e32:.3e} (bar {bar:.3e})"


@pytest.mark.parametrize("Rr,Cc,S", [(1, 1, 1), (5, 7, 33), (32, 1, 32), (3, 11, 31)])
def test_fold_unfold_downscale_edges(dev, Rr, Cc, S):
    from oaprogressionmmf_amd import ops
    B = 2
    g = gen(1800 + Rr + S)
    x = torch.randn(B, Rr, Cc, S, generator=g)
    f = ops.slice_fold(x.to(dev), B, Rr, Cc, S)
    assert torch.equal(f.cpu(), x.permute(0, 3, 1, 2).reshape(B * S, Rr, Cc))
    assert torch.equal(ops.slice_unfold(f, B, Rr, Cc, S).cpu(), x)
    gsl = torch.randn(B * S, Rr, Cc, generator=g)
    assert torch.equal(ops.slice_unfold(gsl.to(dev), B, Rr, Cc, S).cpu(), gsl.reshape(B, S, Rr, Cc).permute(0, 2, 3, 1))
    # downscale2 needs even R and C: the same shapes rounded up to even
    R2, C2 = Rr + Rr % 2, Cc + Cc % 2
    x = torch.randn(B, R2, C2, S, generator=g)
    for fs in (1, 2) if S % 2 == 0 else (1,):
        x64 = x.double().reshape(B, R2 // 2, 2, C2 // 2, 2, S // fs, fs)
        ref = x64.mean((2, 4, 6))
        mag = x64.abs().sum((2, 4, 6)) / (4 * fs)
        # 4 fs - 1 additions and the product with 1 / (4 fs) (exact: a power of two, counted all the same): k = 4 fs
        within(ops.downscale2(x.to(dev), B, R2, C2, S, fs), ref, 4 * fs * U * mag, f"downscale2 {R2}x{C2}x{S} fs={fs}")
