"""Element-wise parity of the bf16-STORAGE instantiations of the HBM-bound kernels (koaf_bn.hip, koaf_planes.hip) at their edges:
the cases of test_elem_edges_gpu.py run again with the activations stored as bf16, the store's rounding on a table of every
rounding decision, the activation plane images per element in both storages, and the wrappers' refusal of mixed storage.

In the storage mode a kernel addresses its activations differently (two-byte elements, 8-byte vectors: load4<true>, load4_nt<true>,
store4<true>, store4_nt<true> of koaf_common.h) and computes exactly what the fp32 mode computes on the widened values.  So:
  * activations (c, idt, ymask, y, the pool input) are drawn in fp32 and rounded to bf16 on the CPU (elem_refs.stored); the float64
    reference is computed from the widened values; gradients (g, dz, dy) and all per-channel vectors stay fp32;
  * every fp32-typed output -- part, dgamma, dbeta, dz, dc, gap_fwd's result, the arg-max bytes -- is held to EXACTLY the bound the
    fp32 case holds it to (the asserts are those of test_elem_edges_gpu.py's case helpers, called with store=torch.bfloat16):
    bit equality for dz = where(mask, g, 0) and the arg-max, k * u * sum|terms| for dc and bn_bwd_apply (k = 3), gamma(m) * sum|terms|
    for part / dgamma / dbeta (m = elem_refs.col_chain) and gap_fwd (m = HW + 2);
  * every bf16-typed output -- bn_add_relu's y, maxpool_fwd's y -- is held to elem_refs.stored16_bound(ref, B), B the fp32 case's
    k * u * sum|terms| (k = 1 / 2 / 2 for the three tails, k = 2 for the pool): the storage term u16 (|ref| + B), u16 = 2^-8, or
    2^-134 below the normal range.  Where the values are bf16 values (the exact pool cases, the ties) y is bit-equal to the
    reference; in the random pool cases y is in addition torch.equal to the fp32 instantiation's y rounded by torch;
  * the store itself (case C) is held bit for bit (int16 view, NaN as NaN) to torch's CPU conversion on elem_refs.bf16_round_cases():
    to nearest even at every binade, ties, subnormal results kept, overflow to Inf, ReLU's +0, NaN;
  * the plane images (case I, both storages): |hi + lo - ref| <= k u sum|terms| fsc + 2^-22 |ref| + 2^-25 with k = 0 / 1 / 2 for
    tf 0 / 1 / 2, hi bit-equal to fp16(ref) wherever the k roundings cannot move it across an fp16 rounding boundary.

Which test launches which A16 = true instantiation, at which grid / block geometry:
  colstats_kernel<true>                A: 7 widths x 5 row counts (1, 2, 4 blocks; RP 256 .. 1; 1 - 3 column chunks), 70001 x 64 (rpb 80)
  bn_bwd_reduce_kernel<true, false>    A: the same shapes, modes 0 / 1 / 2, in place and dz_out; 70001 x 64 mode 2
  bn_bwd_reduce_kernel<true, true>     D: six border shapes x C in {4, 64, 128} (RP 256 / 16 / 8), the ties, W around RP at C = 64
  bn_bwd_apply_kernel<true>            A (every bn_bwd ends in it); B: past the ew_grid cap at C = 64 and C = 4, and 7 x 64
  bn_add_relu_kernel<true>             B: the same three shapes, plain / + idt / + idt through its BatchNorm; C: the rounding table
  maxpool_fwd_kernel<true>             B: 2 x 514 x 514 x 64 (past the cap); C: 1 x 1 images; D: borders, ties, gather walk
  gap_fwd_kernel<true>                 E: HW in {1, 2, 49, 100} x C in {4, 64, 2048} x N in {1, 3} (one block; 2 and 6 at C = 2048)
  act_planes_kernel<0 / 1 / 2, true>   I: n8 in {1, 255, 256, 257, 260, 264, 65} (one block, one + a ragged second), tf 1 past its
                                       own cap of 16384 blocks; the <.., false> twins by the same tests
gap_fwd past the ew_grid cap is not built: its grid-stride loop runs over N * C / 4 work items, which takes a 33M-channel tensor
to pass the cap of 2^21 -- no product shape does --, and the loop is the one the kernels of case B share.
"""
import pytest
import torch

import elem_refs as R
from elem_refs import gamma
from test_elem_edges_gpu import (CAP, POOL_SHAPES, WIDTHS, _bn_bwd_case, _colstats_case, _maxpool_case, _maxpool_ties_case, _pool_bn_bwd,
                                 _tail_case, gen, needs_default_cap, saved_of, within)
from test_tiles_gpu import Record

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
STORES = pytest.mark.parametrize("store", [torch.float32, BF], ids=["fp32", "bf16"])


# =================================================================================================
# A. column-reduction geometry
# =================================================================================================
@pytest.mark.parametrize("C", WIDTHS)
def test_colstats_geometry_bf16(dev, C):
    from oaprogressionmmf_amd import ops
    for i, rows in enumerate(R.case_a_rows(C)):
        _colstats_case(ops, dev, rows, C, 2100 + i, store=BF)


@pytest.mark.parametrize("C", WIDTHS)
def test_bn_bwd_reduce_geometry_bf16(dev, C):
    """mode 1 takes the sign of the bf16 ymask: +0, -0 and the smallest positive subnormal are planted (_bn_bwd_case), the
    reference is ymask.float() > 0"""
    from oaprogressionmmf_amd import ops
    for i, rows in enumerate(R.case_a_rows(C)):
        _bn_bwd_case(ops, dev, rows, C, 2200 + i, store=BF)


def test_column_reductions_rows_per_block_grow_bf16(dev):
    from oaprogressionmmf_amd import ops
    assert R.col_geom(70001, 64)["rpb"] == 80
    _colstats_case(ops, dev, 70001, 64, 2401, store=BF)
    _bn_bwd_case(ops, dev, 70001, 64, 2402, modes=(2,), store=BF)


# =================================================================================================
# B. tails and the ew_grid cap
# =================================================================================================
@needs_default_cap
@pytest.mark.parametrize("rows,C", [(CAP // 16 + 1, 64), (CAP + 3, 4), (7, 64)])
def test_bottleneck_tail_and_bn_apply_past_the_grid_cap_bf16(dev, rows, C):
    from oaprogressionmmf_amd import ops
    _tail_case(ops, dev, rows, C, 2810 + C, store=BF)


@needs_default_cap
def test_maxpool_past_the_grid_cap_bf16(dev):
    from oaprogressionmmf_amd import ops
    N, H, W, C = 2, 514, 514, 64
    assert N * R.pool_out(H) * R.pool_out(W) * C // 4 > CAP
    _maxpool_case(ops, dev, N, H, W, C, 2820, exact=True, loop_ref=False, store=BF)


# =================================================================================================
# C. the store's rounding
# =================================================================================================
def _check_store_bits(got, exp, what):
    """bit equality of a bf16 result with the table's expectation, NaN compared as NaN"""
    gb, eb = R.bf16_bits(got.cpu().reshape(-1)), R.bf16_bits(exp.reshape(-1))
    bad = gb != eb
    if bad.any():
        ef = exp.reshape(-1).float()
        sub = bad & (ef != 0) & (ef.abs() < R.BF16_MIN_NORMAL)
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} stored values differ from torch's round-to-nearest-even conversion, "
                             f"{int(sub.sum())} of them where the expectation is subnormal; first at {i}: got {int(gb[i]):#06x} want {int(eb[i]):#06x}")


def test_store_rounding_nontemporal(dev):
    """store4_nt<true> through bn_add_relu with sc = 1, sh = 0: fmaf(c, 1, 0) + idt is the table's exact sum, the ReLU and the store's
    rounding are all that happens to it.  The device conversion (round_bf16x4) keeps subnormal results, as torch's does: the table
    is asserted whole, subnormals included"""
    from oaprogressionmmf_amd import ops
    c, idt = R.bf16_round_cases()
    rows = c.numel() // 4
    one, zero = torch.ones(4), torch.zeros(4)
    try:
        y = ops.bn_add_relu(c.reshape(rows, 4).to(dev), saved_of(zero, one, one, zero, dev), rows, 4, idt=idt.reshape(rows, 4).to(dev))
        assert y.dtype == BF
        _check_store_bits(y, R.bf16_round_expect(c, idt), "bn_add_relu store")
    finally:
        ops.numerics_status(reset=True)      # (the table's large values and NaNs are counted as saturated: leave the words clean)


def test_store_cached_one_pixel_pool(dev):
    """store4<true> through maxpool_fwd on 1 x 1 images (sc = 1, sh = 0, the table's c alone): relu(c) = c is a bf16 value, the pool
    is a move -- this proves that the cached store writes both dwords and keeps every pattern, NaN and +Inf included; the
    rounding of store4<true> is exercised by the random pool cases below"""
    from oaprogressionmmf_amd import ops
    c, _ = R.bf16_round_cases()
    N = c.numel() // 4
    one, zero = torch.ones(4), torch.zeros(4)
    try:
        y, am = ops.maxpool_fwd(c.reshape(N, 1, 1, 4).to(dev), saved_of(zero, one, one, zero, dev), N, 1, 1, 4)
        assert y.dtype == BF and y.shape == (N, 1, 1, 4)
        _check_store_bits(y, R.bf16_round_expect(c, torch.zeros_like(c)), "maxpool_fwd store")
        assert torch.equal(am.cpu(), torch.full((N, 1, 1, 4), 4, dtype=torch.uint8)), "the centre is the only position inside a 1 x 1 image"
    finally:
        ops.numerics_status(reset=True)


# =================================================================================================
# D. pool borders, ties, gather walk
# =================================================================================================
@pytest.mark.parametrize("C", [4, 64, 128])
@pytest.mark.parametrize("N,H,W", POOL_SHAPES)
def test_maxpool_borders_bf16(dev, N, H, W, C):
    from oaprogressionmmf_amd import ops
    for exact in (True, False):
        c, sc, sh, y, am, dy, da = _maxpool_case(ops, dev, N, H, W, C, 2900 + H * 16 + W + C, exact=exact, store=BF)
        if exact:
            _pool_bn_bwd(ops, dev, c, sc, sh, am, dy, da, N, H, W, C, 2950 + C, store=BF)


@pytest.mark.parametrize("C", [4, 64])
def test_maxpool_ties_bf16(dev, C):
    from oaprogressionmmf_amd import ops
    _maxpool_ties_case(ops, dev, C, store=BF)


@pytest.mark.parametrize("W", [1, 5, 7, 15, 16, 17])
def test_pool_gather_walk_around_rp_bf16(dev, W):
    from oaprogressionmmf_amd import ops
    N, H, C = 3, 11, 64
    assert R.col_rp(C) == 16
    c, sc, sh, y, am, dy, da = _maxpool_case(ops, dev, N, H, W, C, 2970 + W, exact=True, store=BF)
    _pool_bn_bwd(ops, dev, c, sc, sh, am, dy, da, N, H, W, C, 2980 + W, store=BF)


# =================================================================================================
# E. global average pooling
# =================================================================================================
@pytest.mark.parametrize("C", [4, 64, 2048])
@pytest.mark.parametrize("HW", [1, 2, 49, 100])
def test_gap_bf16(dev, HW, C):
    from oaprogressionmmf_amd import ops
    for N in (1, 3):
        y = R.stored(torch.randn(N, HW, C, generator=gen(3000 + HW + C + N)) + 0.5, BF)
        out = ops.gap_fwd(y.to(BF).to(dev), N, HW, C)
        assert out.dtype == torch.float32
        # HW additions in order, then * fl(1 / HW): m = HW + 2 -- the fp32 case's bound
        within(out, y.double().mean(1), gamma(HW + 2) * y.double().abs().sum(1) / HW, f"gap_fwd bf16 {N}x{HW}x{C}")


# =================================================================================================
# I. activation plane images, per element, both storages
# =================================================================================================
def _act_planes_run(ops, dev, tf, cs, store, **over):
    """the wrapper call of one elem_refs.act_case -> (hi, lo) fp16 [npix][C]; the zero chunk behind the planes is checked here"""
    npix, C = cs["x"].shape
    up = lambda t: None if t is None else t.to(dev)          # noqa: E731
    x = cs["x"].to(store if tf != 2 else torch.float32).to(dev)
    x2 = None if cs["x2"] is None else cs["x2"].to(store).to(dev)
    kw = dict(sc=up(cs["sc"]), sh=up(cs["sh"]), x2=x2, sc2=up(cs["sc2"]), amax=up(cs["amax"]), fscale=cs["fscale"])
    kw.update(over)
    planes = ops.act_planes(x, npix, C, tf, **kw)
    hi, lo, tail = R.act_planes_unpack(planes, npix, C)
    assert torch.equal(tail, torch.zeros(8, dtype=torch.int16)), "the 8-element chunk behind the planes is not zero"
    return hi, lo


@STORES
@pytest.mark.parametrize("tf", [0, 1, 2])
def test_act_planes_per_element(dev, tf, store):
    """k = tf roundings on the way to x' (elem_refs.act_planes_ref); tf 2: x is the fp32 gradient, x2 the activation in `store`"""
    from oaprogressionmmf_amd import ops
    for C, n8 in R.ACT_SHAPES:
        cs = R.act_case(C, n8, tf, store)
        hi, lo = _act_planes_run(ops, dev, tf, cs, store)
        share = R.act_planes_check(hi, lo, tf, cs, f"act_planes tf {tf} C {C} n8 {n8}")
        assert share <= 1e-3, (tf, C, n8, share)


@STORES
def test_act_planes_past_its_own_grid_cap(dev, store):
    """16384 blocks of 256 work items, then the grid strides: one work item past that (C = 8), tf 1 -- k = 1"""
    from oaprogressionmmf_amd import ops
    cs = R.act_case(8, R.ACT_CAP_N8, 1, store)
    assert cs["npix"] == 16384 * 256 + 1
    hi, lo = _act_planes_run(ops, dev, 1, cs, store)
    share = R.act_planes_check(hi, lo, 1, cs, "act_planes past the cap")
    assert share <= 1e-3, share


@STORES
@pytest.mark.parametrize("top", [1e-9, 1.0, 3e4, 0.0])
def test_act_planes_amax_scales(dev, top, store):
    """tf 0 (k = 0: x * 2^(15 - e) is exact) with the scale taken from the device scalar amax = max|x| = m 2^e: tiny, unit and near
    the fp16 range's end; amax = 0 (an all-zero tensor: scale 1)"""
    from oaprogressionmmf_amd import ops
    C, npix = 64, 33
    x = torch.randn(npix, C, generator=gen(3100))
    x = R.stored(x / x.abs().max() * top, store) if top else torch.zeros(npix, C)
    amax = x.abs().max().reshape(1)
    assert top == 0.0 or abs(float(amax) / top - 1) < 2 * R.U16
    cs = dict(npix=npix, x=x, x2=None, sc=None, sh=None, sc2=None, amax=amax, fscale=0.0)
    hi, lo = _act_planes_run(ops, dev, 0, cs, store)
    assert R.act_planes_check(hi, lo, 0, cs, f"act_planes tf 0 amax {top}") == 0.0
    if top:
        assert 2.0 ** 14 <= float(hi.abs().max()) <= 2.0 ** 15       # amax * scale lies in [2^14, 2^15): a binade below the fp16 range's end


@STORES
def test_act_planes_clamp_and_status_word(dev, store):
    """elements beyond 65504 / fsc clamp to +-65504 with lo == 0, and status word 0 grows by exactly their number (read as
    test_numerics_status_words_saturation_and_nonfinite reads it); tf 0 at the fixed scale 16, k = 0"""
    from oaprogressionmmf_amd import ops
    C, npix = 64, 33
    x = torch.randn(npix, C, generator=gen(3200))
    over = torch.randperm(npix * C, generator=gen(3201))[:37]
    x.view(-1)[over] = torch.where(torch.arange(37) % 2 == 0, 1.0, -1.0) * (5000.0 + 100.0 * torch.arange(37))      # * 16 > 65504
    x = R.stored(x, store)
    cs = dict(npix=npix, x=x, x2=None, sc=None, sh=None, sc2=None, amax=None, fscale=16.0)
    ref, e, raw, k = R.act_planes_ref(0, x, 16.0)
    beyond = raw.abs() > R.H16_MAX
    assert int(beyond.sum()) == 37 and k == 0
    ops.numerics_status(reset=True)
    hi, lo = _act_planes_run(ops, dev, 0, cs, store)
    st = ops.numerics_status(reset=True)
    assert st == {"saturated": 37, "nonfinite": 0}, st
    assert R.act_planes_check(hi, lo, 0, cs, "act_planes clamp") == 0.0
    assert torch.equal(hi[beyond].double(), torch.sign(raw[beyond]) * R.H16_MAX) and torch.equal(lo[beyond], torch.zeros(37, dtype=torch.float16))


# =================================================================================================
# the wrappers refuse mixed storage
# =================================================================================================
def _refused(call, match, outputs=()):
    """the call raises KoafError naming the call and the argument, launches nothing that the launch record sees, and leaves the
    NaN-filled outputs as they were"""
    from oaprogressionmmf_amd._lib import KoafError
    with Record() as rec:
        with pytest.raises(KoafError, match=match):
            call()
    assert rec.launches == [], rec.launches
    torch.cuda.synchronize()
    for t in outputs:
        assert torch.isnan(t.float()).all(), f"{match}: an output was written"


def test_wrappers_refuse_mixed_storage(dev):
    """the entry points take float* and one act16 flag: a call whose activations are not all fp32 or all bf16 would read a two-byte
    tensor at four bytes per element, past its end.  Only the wrapper can see it (ops/_base.py _act16, _grads32); nothing mismatched
    is handed to the C entry points here"""
    from oaprogressionmmf_amd import ops
    rows, C = 8, 64
    N, H, W = 2, 2, 2
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=dev, dtype=dtype)       # noqa: E731
    c32 = torch.randn(rows, C, generator=gen(3300)).to(dev)
    c16, c64 = c32.bfloat16(), c32.double()
    v = torch.ones(C, device=dev)
    saved = torch.stack([v, v, v, v])
    # bn_add_relu: c, idt, out
    _refused(lambda: ops.bn_add_relu(c32, saved, rows, C, idt=c16), "bn_add_relu: idt")
    _refused(lambda: ops.bn_add_relu(c16, saved, rows, C, idt=c32), "bn_add_relu: idt")
    for c, out in ((c32, nan(rows, C, dtype=BF)), (c16, nan(rows, C))):
        _refused(lambda: ops.bn_add_relu(c, saved, rows, C, out=out), "bn_add_relu: out", [out])
    _refused(lambda: ops.bn_add_relu(c64, saved, rows, C), "bn_add_relu: c")
    # bn_bwd: c, ymask share a storage; g, dz_out, dc_out, pool[0] are fp32
    dg, db = nan(C), nan(C)
    for c, ym in ((c32, c16), (c16, c32)):
        g = nan(rows, C)
        _refused(lambda: ops.bn_bwd(g, c, saved, rows, C, rows, dg, db, 1, ymask=ym), "bn_bwd: ymask", [g, dg, db])
    g16 = nan(rows, C, dtype=BF)
    _refused(lambda: ops.bn_bwd(g16, c32, saved, rows, C, rows, dg, db, 2), "bn_bwd: g", [g16, dg, db])
    for kw in ("dz_out", "dc_out"):
        g, o = nan(rows, C), nan(rows, C, dtype=BF)
        _refused(lambda: ops.bn_bwd(g, c16, saved, rows, C, rows, dg, db, 2, **{kw: o}), "bn_bwd: " + kw, [g, o, dg, db])
    pg, am = nan(N, 1, 1, C, dtype=BF), torch.zeros(N, 1, 1, C, dtype=torch.uint8, device=dev)
    _refused(lambda: ops.bn_bwd(None, c16, saved, rows, C, rows, dg, db, 2, fused=True, pool=(pg, am, N, H, W)), r"bn_bwd: pool\[0\]", [dg, db])
    # single-activation calls: fp32 or bf16, nothing else
    _refused(lambda: ops.maxpool_fwd(c64.reshape(N, H, W, C), saved, N, H, W, C), "maxpool_fwd: c")
    _refused(lambda: ops.gap_fwd(c64.reshape(N, H * W, C), N, H * W, C), "gap_fwd: y")
    _refused(lambda: ops.colstats(c64, rows, C), "colstats: x")
    # BnApply.materialize: c either, dz and out fp32
    coef = torch.stack([v, v, v])
    out16 = nan(rows, C, dtype=BF)
    _refused(lambda: ops.BnApply(c32, c16, coef, None, v, rows, C).materialize(out=out16), "bn_bwd_apply: out", [out16])
    _refused(lambda: ops.BnApply(c16, c16, coef, None, v, rows, C).materialize(), "bn_bwd_apply: dz")
    _refused(lambda: ops.BnApply(c32, c64, coef, None, v, rows, C).materialize(), "bn_bwd_apply: c")
    # act_planes: tf 2 takes an fp32 x and x2 in either storage; tf 0 / 1 take x in either and no x2
    _refused(lambda: ops.act_planes(c16, rows, C, 2, v, v, x2=c16, sc2=v, fscale=16.0), "act_planes: x ")
    _refused(lambda: ops.act_planes(c32, rows, C, 2, v, v, x2=c64, sc2=v, fscale=16.0), "act_planes: x2")
    _refused(lambda: ops.act_planes(c32, rows, C, 1, v, v, x2=c16, fscale=16.0), "act_planes: x2")
    _refused(lambda: ops.act_planes(c64, rows, C, 0, fscale=16.0), "act_planes: x ")
    # and the matched calls of either storage go through
    for c in (c32, c16):
        y = ops.bn_add_relu(c, saved, rows, C, idt=c, out=torch.empty_like(c))
        assert y.dtype == c.dtype and torch.isfinite(y.float()).all()
        ops.bn_bwd(torch.ones(rows, C, device=dev), c, saved, rows, C, rows, dg, db, 1, ymask=c)
        ops.act_planes(c32, rows, C, 2, v, v, x2=c, sc2=v, fscale=16.0)
    assert torch.isfinite(dg).all() and torch.isfinite(db).all()
