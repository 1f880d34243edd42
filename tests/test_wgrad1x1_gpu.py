"""The 256-wide-tile kernel of the 1x1 / stride-1 weight gradients (koaf_wgrad1.hip) against the generic path it replaces.

koaf_conv2d_wgrad hands a 1x1 / stride-1 weight gradient to koaf_wgrad1 when the call runs the fp16 scheme on fp32 tensors, both
channel counts are whole multiples of 128 with at least one of them >= 256, and the split-K plan (wgrad_plan, unchanged) leaves
k-ranges of at least 1024 pixels (koaf_conv.hip wgrad1_tile).  Every row of CASES is the smallest shape of its kind that the rule
engages; it goes through ops.conv2d_wgrad as the model calls it and ASSERTS FROM THE LAUNCH RECORD the variant, tile, tile count
and split count.  dw and the slab workspace are pre-filled with NaN.

Held per case:
  * dw is torch.equal to the generic path on the same inputs: ops.gemm with the descriptor koaf_conv2d_wgrad builds for
    koaf_gemm_kernel (128 x 128 tiles, the same splitk, slabs) followed by koaf_slab_reduce.  The kernel keeps koaf_gemm_kernel's
    arithmetic, pieces and order of piece products per accumulator, so nothing may move.
  * against float64 on the CPU for eight sampled 64 x 64 blocks of dw (corners and interior, both halves of every tile along both
    dimensions): relative L2 < BWD per block and the componentwise bar of test_wgrad_gpu.py (8 x torch's fp32 product of the same
    operands); BWD and the bar's function are imported from test_tiles_gpu, not restated.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: the generic kernel at 128-wide tiles keeps the bf16 scheme, bf16 storage, k-ranges
under 1024 pixels and channel counts that are no multiple of 128.

Inputs are drawn on the device (one set per shape, shared by its calls); only the sampled columns travel to the CPU."""
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

from test_tiles_gpu import BWD, Record, componentwise, rel_err

pytestmark = pytest.mark.gpu

W1K, GEN = "koaf_wgrad1", "koaf_gemm"
Case = namedtuple("Case", "name shape call bm bn splitk empty last")
# shape (N, H, W, Cin, Cout); call: plain (dy + its amax) | apply_prologue (dy an ops.BnApply -- tf 2 on A --, x behind its BatchNorm
# prologue -- tf 1 on B: the production combination); splitk / empty trailing splits / rows of the last live split: wgrad_plan's,
# as koaf_conv2d_wgrad_ws reports them (test_the_table_against_the_library_plan)
S1 = (17, 62, 63, 256, 1024)      # P = 66 402 = 2 mod 32: 64 splits of 1056 rows, the last live one 930, one empty; 4 tiles 256 x 256
S2 = (5, 57, 61, 512, 2048)       # P = 17 385 = 9 mod 32: 16 splits of 1088 rows, 16 tiles per split
S3 = (65, 63, 65, 256, 256)       # P = 266 175 = 31 mod 32: 256 splits of one tile, the last live one 63 rows, 3 empty; two-level slab reduce
S4 = (65, 63, 65, 128, 512)       # the same 256 splits on 256 x 128 tiles (two per split)
S5 = (65, 63, 65, 512, 128)       # 128 x 256 tiles
S6 = (9, 61, 62, 1024, 512)       # P = 34 038 = 22 mod 32: 32 splits, 8 tiles per split
SHAPES = [S1, S2, S3, S4, S5, S6]
CASES = [
    Case("256to1024-plain", S1, "plain", 256, 256, 64, 1, 930),
    Case("256to1024-apply_prologue", S1, "apply_prologue", 256, 256, 64, 1, 930),
    Case("512to2048-apply_prologue", S2, "apply_prologue", 256, 256, 16, 0, 1065),
    Case("256to256-apply_prologue", S3, "apply_prologue", 256, 256, 256, 3, 63),
    Case("128to512-apply_prologue", S4, "apply_prologue", 256, 128, 256, 3, 63),
    Case("512to128-apply_prologue", S5, "apply_prologue", 128, 256, 256, 3, 63),
    Case("1024to512-plain", S6, "plain", 256, 256, 32, 0, 310),
]
Refusal = namedtuple("Refusal", "name shape call store")
R1 = (9, 20, 20, 512, 2048)       # P = 3600: k-ranges of 480 pixels
R2 = (17, 62, 63, 256, 192)       # Cout no multiple of 128
REFUSALS = [
    Refusal("bf16scheme", S1, "bf16scheme", "fp32"),      # dy_amax withheld
    Refusal("bf16storage", S1, "apply_prologue", "bf16"),      # x and the apply's c stored as bf16 (act16 3)
    Refusal("kchunk480", R1, "plain", "fp32"),
    Refusal("cout192", R2, "plain", "fp32"),
]


def plan_of(shape):
    """(P, splitk, kchunk, empty trailing splits, rows of the last live split) from the library's workspace size:
    koaf_conv2d_wgrad_ws = (splitk + 16) * Cout * Cin"""
    from oaprogressionmmf_amd import _lib
    N, H, W, Cin, Cout = shape
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, 1, 1, 1, 0)
    P = N * H * W
    assert ws > 0 and ws % (Cout * Cin) == 0
    splitk = ws // (Cout * Cin) - 16
    kchunk = (-(-P // splitk) + 31) // 32 * 32
    live = -(-P // kchunk)
    return P, splitk, kchunk, splitk - live, P - (live - 1) * kchunk


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_table_against_the_library_plan(case):
    P, splitk, kchunk, empty, last = plan_of(case.shape)
    assert (splitk, empty, last) == (case.splitk, case.empty, case.last), (case.name, P, splitk, kchunk, empty, last)
    assert kchunk >= 1024, (case.name, kchunk)


@lru_cache(maxsize=1)
def inputs(shape, dev, store16=False):
    """device operands of a shape: x [P, Cin], its prologue (sc, sh), the gradient dy [P, Cout] with its amax, and the BatchNorm-backward
    recipe (ops.BnApply) of an apply row; store16: x and the apply's conv output c stored as bf16 (activation storage mode)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout = shape
    P = N * H * W
    g_ = torch.Generator(device=dev).manual_seed(9100 + (SHAPES + [R1, R2]).index(shape))

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    t = dict(x=rnd(P, Cin) * 1.5 + 0.3, sc=rnd(Cin) * 0.2 + 1.0, sh=rnd(Cin) * 0.1, dy=rnd(P, Cout) * 1e-3)
    if store16:
        t["x"] = t["x"].bfloat16()
    t["amax"] = t["dy"].abs().max().reshape(1).float()
    if any(c.shape == shape and c.call == "apply_prologue" for c in CASES):
        c, g = rnd(P, Cout) * 1.5 + 0.3, rnd(P, Cout) * 1e-3
        if store16:
            c = c.bfloat16()
        gam, bet = rnd(Cout) * 0.2 + 1.0, rnd(Cout) * 0.1
        sv = ops.bn_finalize(ops.colstats(c, P, Cout), Cout, P, gam, bet, torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev),
                             torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)
        dgm, dbt = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
        t["apply"] = ops.bn_bwd(g, c, sv, P, Cout, P, dgm, dbt, 2, fused=True)
    torch.cuda.synchronize()
    return t


def nan_like(n, dev):
    return torch.full((n,), float("nan"), device=dev)


def call_model(dev, shape, t, call):
    """ops.conv2d_wgrad as the model calls it -> (dw [Cout, Cin], the launch records)"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout = shape
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, 1, 1, 1, 0)
    dw, slabs = nan_like(Cout * Cin, dev).reshape(Cout, 1, 1, Cin), nan_like(ws, dev)
    prol = call == "apply_prologue"
    arg = t["apply"] if prol else t["dy"]
    am = t["amax"] if call == "plain" else None
    with Record() as rec:
        ops.conv2d_wgrad(arg, t["x"], dw, N, H, W, Cin, Cout, 1, 1, 1, 0, t["sc"] if prol else None,
                         t["sh"] if prol else None, dy_amax=am, aplanes=False, slabs=slabs)
    torch.cuda.synchronize()
    return dw.reshape(Cout, Cin), rec.launches


def call_generic(dev, shape, t, call, splitk):
    """the generic path: koaf_gemm on the descriptor koaf_conv2d_wgrad builds (K-major fp32 operands, 128 x 128 tiles, the same splitk,
    slabs), then koaf_slab_reduce"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout = shape
    P = N * H * W
    L = _lib.lib()
    dw, slabs = nan_like(Cout * Cin, dev), nan_like((splitk + 16) * Cout * Cin, dev)
    g = _lib.KoafGemm()
    g.alpha, g.nb0, g.nb1, g.prec, g.fmt = 1.0, 1, 1, 1, 1
    g.A.kind, g.A.ld, g.B.kind, g.B.ld, g.B.ptr, g.B.fscale = 1, Cout, 1, Cin, t["x"].data_ptr(), ops.ACT_SCALE
    if call == "apply_prologue":
        ap = t["apply"]
        g.A.ptr, g.A.ptr2, g.A.tf, g.A.amax = ap.dz.data_ptr(), ap.c.data_ptr(), 2, ap.amax.data_ptr()
        g.A.sc, g.A.sc2, g.A.sh = ap.coef.data_ptr(), ap.coef.data_ptr() + 4 * 2 * Cout, ap.coef.data_ptr() + 4 * 3 * Cout
        g.B.tf, g.B.sc, g.B.sh = 1, t["sc"].data_ptr(), t["sh"].data_ptr()
    else:
        g.A.ptr, g.A.amax = t["dy"].data_ptr(), t["amax"].data_ptr()
    g.M, g.N, g.K, g.bm, g.bn, g.splitk = Cout, Cin, P, 128, 128, splitk
    g.C, g.ldc = (slabs if splitk > 1 else dw).data_ptr(), Cin
    with Record() as rec:
        ops.gemm(g)
    if splitk > 1:
        ops.check(L.koaf_slab_reduce(slabs.data_ptr(), splitk, Cout * Cin, dw.data_ptr(), ops._stream()), "slab_reduce")
    torch.cuda.synchronize()
    return dw.reshape(Cout, Cin), rec.launches


def sampled_blocks(Cout, Cin):
    """eight 64 x 64 blocks of dw as (row block, column block): the four corners and four interior ones, chosen so that both halves of
    a 256-wide (or 128-wide) tile are met along both dimensions"""
    rb, cb = Cout // 64, Cin // 64
    picks = [(0, 0), (rb - 1, cb - 1), (0, cb - 1), (rb - 1, 0), (rb // 2, cb // 2), (rb // 2 - 1, (cb // 2 + 1) % cb), (1 % rb, 2 % cb),
             (2 % rb, 1 % cb), (3 % rb, 3 % cb), ((rb // 2 + 1) % rb, 0), (0, (cb // 2 + 1) % cb)]
    out = []
    for p in picks:
        if p not in out:
            out.append(p)
    assert len(out) >= 8 or len(out) == rb * cb
    return out[:8]


def hold_blocks(case, t, dw):
    """the float64 bars of the sampled blocks; the operands of a block are formed on the CPU from its columns of the device tensors"""
    N, H, W, Cin, Cout = case.shape
    prol = case.call == "apply_prologue"
    worst, worst_cw = 0.0, (0.0, 0.0)
    for bi, bj in sampled_blocks(Cout, Cin):
        rs, cs = slice(64 * bi, 64 * bi + 64), slice(64 * bj, 64 * bj + 64)
        x = t["x"][:, cs].cpu()
        if prol:
            ap = t["apply"]
            coef = ap.coef.reshape(4, Cout)[:, rs].cpu()
            dz, c = ap.dz.reshape(-1, Cout)[:, rs].cpu(), ap.c.reshape(-1, Cout)[:, rs].cpu()
            d32 = coef[0] * dz + coef[3] - coef[2] * c
            d64 = coef[0].double() * dz.double() + coef[3].double() - coef[2].double() * c.double()
            sc, sh = t["sc"][cs].cpu(), t["sh"][cs].cpu()
            a32, a64 = torch.relu(x * sc + sh), torch.relu(x.double() * sc.double() + sh.double())
        else:
            d32 = t["dy"][:, rs].cpu()
            d64, a32, a64 = d32.double(), x, x.double()
        ref64, ref32, den = d64.t() @ a64, d32.t() @ a32, d32.abs().double().t() @ a32.abs().double() + 1e-300
        got = dw[rs, cs]
        e = rel_err(got, ref64)
        cw, bar = componentwise(got, ref64, ref32, den)
        print(f"[wgrad1x1] {case.name:28s} block ({bi:2d},{bj:2d}) rel L2 {e:.2e} (bar {BWD:.0e}) componentwise {cw:.2e} (bar {bar:.2e})")
        assert e < BWD, (case.name, bi, bj, e)
        assert cw <= bar, (case.name, bi, bj, cw, bar)
        worst = max(worst, e)
        worst_cw = max(worst_cw, (cw, bar))
    return worst, worst_cw


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_wide_tile_kernel_equals_the_generic_path(dev, case):
    N, H, W, Cin, Cout = case.shape
    try:
        t = inputs(case.shape, dev)
        dw, launches = call_model(dev, case.shape, t, case.call)
        gemms = [r for r in launches if r["variant"] in (W1K, GEN)]
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        tiles = (Cout // case.bm) * (Cin // case.bn)
        prol = case.call == "apply_prologue"
        want = dict(variant=W1K, bm=case.bm, bn=case.bn, tiles=tiles, grid_x=tiles, splitk=case.splitk, M=Cout, N=Cin, K=N * H * W, fmt=1,
                    a_tf=2 if prol else 0, b_tf=1 if prol else 0, act16=0)
        assert {f: r[f] for f in want} == want, (case.name, r, want)
        bad = ~torch.isfinite(dw)
        assert not bool(bad.any()), (case.name, f"{int(bad.sum())} elements of dw: a tile or a split's slab was not written")
        assert torch.equal(call_model(dev, case.shape, t, case.call)[0], dw), (case.name, "the same call twice")
        ref, lg = call_generic(dev, case.shape, t, case.call, case.splitk)
        assert len(lg) == 1 and (lg[0]["variant"], lg[0]["bm"], lg[0]["bn"], lg[0]["splitk"]) == (GEN, 128, 128, case.splitk), (case.name, lg)
        ndiff = int((ref != dw).sum())
        print(f"\n[wgrad1x1] {case.name:28s} {r['variant']} {r['bm']}x{r['bn']} tiles {r['tiles']} splitk {r['splitk']} empty {case.empty} "
              f"last split {case.last} rows | elements that differ from the generic path: {ndiff}")
        assert torch.equal(ref, dw), (case.name, ndiff, "bit-identical to koaf_gemm_kernel on 128 x 128 tiles")
        hold_blocks(case, t, dw)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernel(dev, case):
    N, H, W, Cin, Cout = case.shape
    try:
        t = inputs(case.shape, dev, case.store == "bf16")
        dw, launches = call_model(dev, case.shape, t, case.call)
        gemms = [r for r in launches if r["variant"] in (W1K, GEN)]
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        assert (r["variant"], r["bm"], r["bn"]) == (GEN, 128, 128), (case.name, r)
        assert r["fmt"] == (0 if case.call == "bf16scheme" else 1) and r["act16"] == (3 if case.store == "bf16" else 0), (case.name, r)
        assert bool(torch.isfinite(dw).all()), case.name
    finally:
        torch.cuda.empty_cache()
