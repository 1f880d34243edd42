"""Band-wise parity of the three stem kernels (koaf_stem.hip) at their band, tile and walk edges.

stem_fwd_mma_kernel walks units of image x 4 output rows in 192-column bands of 32-pixel tiles with persistent blocks (512 at the
most), prefetches the next band -- or the next unit's first band -- into registers and folds its statistics once a unit is
complete; stem_wgrad_mma_kernel walks the same units in 96-column bands of 16-pixel tiles, one slab per block (1024 at the most),
koaf_slab_reduce finishes in one or two levels; stem_dgrad_kernel covers the dc grid in 16 x 16 tiles with a 13 x 13 interior.
test_stem / test_stem_dgrad (test_kernels_gpu.py, test_input_grads_kernels_gpu.py) run at most 8 units and hold one whole-tensor
norm; here every shape sits on one of those edges and every band is held on its own.  The walking rows ASSERT their unit and block
counts from koaf_stem_stats_rows and koaf_stem_wgrad_ws, so each provably does what its comment says.

Bars (owned by the module docstrings of test_kernels_gpu.py, test_tiles_gpu.py and test_elem_edges_gpu.py; nothing new is invented):
  * relative L2 against the float64 CPU result over the whole tensor and PER BAND: 2e-6 forward, BWD = 4e-6 gradients.  Bands:
    y per output row (n, oy) and per output column ox (over n, oy, co); dw per filter tap (49, all channels); dx per input row
    (n, iy) and per input column ix.  A fault confined to one band column, or to the first unit after a walk, moves a
    whole-tensor norm by 1 / sqrt(bands).
  * componentwise: max |y - y64| / (|a| * |b| summed over the contraction) <= max(8 x the same ratio of torch's fp32 CPU result on
    the same operands, the norm bar of that result).  The floor is there because at one- or few-term sums torch's fp32 error can
    be zero; the faults this is for (a dropped piece 2^-16, a stale band, one wrong row) are >= 1e-4 .. 1e-5.
  * statistics partials, PER UNIT ROW (not summed over units): |part - ref| <= gamma(m + k) * sum|terms|, m = 4 OW terms per channel
    in a unit, ref the float64 sums of the y the device wrote, k the roundings of a term as _colstats_case counts them (sum: 0, with
    a shift 1; sum of squares: 1, with a shift 3).
  * bf16 storage: y bit-equal to the fp32 y rounded once, the statistics those of the rounded values.
  * a dy that is a BatchNorm-backward apply (ops.BnApply) is held to the float64 product of dy64 = coef0 * dz + coef3 - coef2 * c.
dw and the slab workspace (ops.stem_wgrad `slabs=`) go in as NaN: a block that does not deliver its slab, or an idle block that
does not deliver zeros, shows as NaN in dw.

Each case prints one table line: geometry (units, blocks / slabs, bands), worst band, componentwise ratio and bar, worst
statistics partial as a fraction of its bound.

Measured on an MI355X (they document; every bar is computed in the test), worst over the cases:
  forward   row band 1.65e-07 (171 x 24 x 8), column band 1.35e-07 (1 x 5 x 385), componentwise 3.2e-07 against bars of 2.0e-06 ..
            2.7e-06, statistics partials <= 0.42 of their bound (1 x 1 x 1; <= 0.20 elsewhere); the 25 MB case takes 0.6 s
  dw        tap 4.23e-07 (1025 x 2 x 18, 1024 slabs), 2.3e-07 elsewhere; componentwise 3.1e-07 (bar 4.0e-06)
  dx        row band 2.83e-07, column band 1.37e-06 (2 x 1 x 70: a one-row image, few terms per pixel), componentwise 6.5e-08
  BnApply   dw tap 2.25e-07, dx band 2.86e-07 (c in fp32 and in bf16 alike)."""
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F

from elem_refs import gamma
from test_elem_edges_gpu import within
from test_tiles_gpu import BWD, FWD, band_errors, componentwise, rel_err

pytestmark = pytest.mark.gpu

TH, FWD_BAND, FWD_TILE, WG_BAND, WG_TILE, DG_I = 4, 192, 32, 96, 16, 13      # koaf_stem.hip: SM_TH, SM_BAND, 32-pixel tiles, SW_BAND, SW_TILE_W, SD_I
FWD_GRID, WG_GRID = 512, 1024                                                # persistent blocks of the forward, slab cap of the weight gradient


def out_dim(h):
    return (h + 6 - 7) // 2 + 1


# (N, H, W); OH = ceil(H / 2), OW = ceil(W / 2)
DEGENERATE = [(1, 1, 1), (1, 2, 7)]                         # fewer rows and columns than the filter; OH = 1
FWD_TILE_EDGE = [(2, 9, 62), (2, 9, 63), (2, 9, 65)]        # OW = 31, 32, 33; OH = 5: the second unit has one live wave
FWD_BAND_EDGE = [(1, 5, 382), (1, 5, 383), (1, 5, 385)]     # OW = 191, 192, 193
WG_BAND_EDGE = [(1, 3, 190), (1, 3, 191), (1, 3, 193)]      # OW = 95, 96, 97: the last gives a second band of one pixel
ROWS_PER_UNIT = [(2, 1, 70), (2, 3, 70), (2, 5, 70), (2, 7, 70)]     # OH mod 4 = 1, 2, 3, 0
FWD_WALKS = [(513, 2, 386), (171, 24, 8)]                   # 513 units over 512 blocks: two bands each (block 0 prefetches across a unit
#                                                             boundary and resets its statistics; y is 25 MB) | 513 units, three per image
WG_WALKS = [(1025, 2, 18)]                                  # 1025 units over the 1024-slab cap
SLAB_LEVELS = [(7, 2, 270), (8, 2, 250)]                    # 63 slabs (one reduce level) and 64 slabs (two levels)
DG_TILE_EDGE = [(1, 26, 26), (1, 27, 27), (1, 25, 53), (2, 52, 27)]   # OH, OW = 13 / 14 / 13 x 27 / 26 x 14: one tile, 2 x 2, 1 x 3, exact end of a second

FWD_SHAPES = DEGENERATE + FWD_TILE_EDGE + FWD_BAND_EDGE + ROWS_PER_UNIT + FWD_WALKS
FWD_BF16 = {g[-1] for g in (DEGENERATE, FWD_TILE_EDGE, FWD_BAND_EDGE, ROWS_PER_UNIT, FWD_WALKS)}      # one case per group
WG_SHAPES = DEGENERATE + FWD_TILE_EDGE + WG_BAND_EDGE + ROWS_PER_UNIT + WG_WALKS + SLAB_LEVELS
DG_SHAPES = DEGENERATE + DG_TILE_EDGE + ROWS_PER_UNIT
WG_MODES_SHAPE, DG_MODES_SHAPE = (1, 3, 193), (1, 27, 27)     # the ragged case of the three dy modes
ALL_SHAPES = sorted(set(FWD_SHAPES + WG_SHAPES + DG_SHAPES))


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def geometry(ops, shape):
    """(OH, OW, units, slabs) -- the unit and slab counts as the LIBRARY states them"""
    N, H, W = shape
    L = ops.lib()
    ws = L.koaf_stem_wgrad_ws(N, H, W)
    assert ws % (49 * 64) == 0
    return out_dim(H), out_dim(W), L.koaf_stem_stats_rows(N, H), ws // (49 * 64) - 16


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and float64 references: one set per shape, shared by its tests and left unchanged
# ---------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(shape):
    N, H, W = shape
    g = torch.Generator().manual_seed(9100 + ALL_SHAPES.index(shape))
    OH, OW = out_dim(H), out_dim(W)

    def rnd(*s):
        return torch.randn(*s, generator=g)
    return dict(x=rnd(N, H, W) * 1.5 + 0.3, w1t=rnd(49, 64) * 49 ** -0.5, shift=rnd(64) * 0.1, dy=rnd(N, OH, OW, 64),
                c=rnd(N, OH, OW, 64) * 1.5 + 0.3, coef=torch.stack([rnd(64) * 0.2 + 1.0, rnd(64), rnd(64) * 0.1, rnd(64) * 0.1]))


def filt(w1t):
    """w1t [49][64] -> [64][1][7][7]"""
    return w1t.t().reshape(64, 1, 7, 7)


def fwd_cpu(x, w1t):
    """x [N,H,W], w1t [49,64] -> y [N,OH,OW,64] in the operands' type"""
    return F.conv2d(x[:, None], filt(w1t), stride=2, padding=3).permute(0, 2, 3, 1).contiguous()


def wgrad_cpu(dy, x):
    """-> dw1t [49][64]"""
    dw = torch.nn.grad.conv2d_weight(x[:, None], (64, 1, 7, 7), dy.permute(0, 3, 1, 2), stride=2, padding=3)
    return dw.reshape(64, 49).t().contiguous()


def dgrad_cpu(dy, w1t, shape):
    """-> dx [N,H,W]"""
    N, H, W = shape
    return torch.nn.grad.conv2d_input((N, 1, H, W), filt(w1t), dy.permute(0, 3, 1, 2), stride=2, padding=3)[:, 0].contiguous()


@lru_cache(maxsize=2)
def fwd_refs(shape):
    t = inputs(shape)
    x, w = t["x"], t["w1t"]
    return fwd_cpu(x.double(), w.double()), fwd_cpu(x, w), fwd_cpu(x.abs(), w.abs()).double() + 1e-300


def dy_forms(shape, mode):
    """(dy64, dy32) of a gradient mode: the tensor itself, or the apply's recipe evaluated in float64 / fp32 (c widened from its storage)"""
    t = inputs(shape)
    if mode == "plain":
        return t["dy"].double(), t["dy"]
    c = t["c"].bfloat16().float() if mode == "apply_bf16" else t["c"]
    k = t["coef"]
    k64 = k.double()
    return k64[0] * t["dy"].double() + k64[3] - k64[2] * c.double(), k[0] * t["dy"] + k[3] - k[2] * c


def dy_device(ops, dev, shape, mode):
    """the dy argument of ops.stem_wgrad / ops.stem_dgrad: a tensor, or an ops.BnApply over (dz, c, coef) with c in fp32 / bf16"""
    t = inputs(shape)
    if mode == "plain":
        return t["dy"].to(dev)
    N, H, W = shape
    c = t["c"].to(dev)
    return ops.BnApply(t["dy"].to(dev), c.bfloat16() if mode == "apply_bf16" else c, t["coef"].to(dev), None, None,
                       N * out_dim(H) * out_dim(W), 64)


def bar_of(cw_bar, norm_bar):
    return max(cw_bar, norm_bar)


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def check_stats(part, y, shift, shape, units, what):
    """every unit row of part [units][2][64] against the float64 sums of the y the device wrote -> worst |err| / bound"""
    N, H, W = shape
    OH, OW = out_dim(H), out_dim(W)
    ty = -(-OH // TH)
    assert part.shape == (units, 2, 64) and units == N * ty, (what, part.shape)
    d = y.double().cpu() - (0.0 if shift is None else shift.double())
    d = F.pad(d, (0, 0, 0, 0, 0, ty * TH - OH)).reshape(N, ty, TH, OW, 64)             # (rows past OH: no terms)
    m = TH * OW
    k1, k2 = (1, 3) if shift is not None else (0, 1)
    s1, a1 = d.sum((2, 3)).reshape(units, 64), d.abs().sum((2, 3)).reshape(units, 64)
    s2 = (d * d).sum((2, 3)).reshape(units, 64)
    b1, b2 = gamma(m + k1) * a1, gamma(m + k2) * s2
    within(part[:, 0], s1, b1, what + " statistics sum")
    within(part[:, 1], s2, b2, what + " statistics sum of squares")
    p = part.double().cpu()
    return max(float(((p[:, 0] - s1).abs() / (b1 + 1e-300)).max()), float(((p[:, 1] - s2).abs() / (b2 + 1e-300)).max()))


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=ids(FWD_SHAPES))
def test_stem_fwd_edges(dev, shape):
    from oaprogressionmmf_amd import ops
    N, H, W = shape
    OH, OW, units, _ = geometry(ops, shape)
    assert units == N * -(-OH // TH)
    if shape in FWD_WALKS:
        assert units == 513 > FWD_GRID, (shape, units)                  # the grid walks: block 0 takes units 0 and 512
    if shape == FWD_WALKS[0]:
        assert -(-OW // FWD_BAND) == 2                                 # ... and prefetches unit 512 under the second band of unit 0
    t = inputs(shape)
    xd, wd, shd = t["x"].to(dev), t["w1t"].to(dev), t["shift"].to(dev)
    y64, y32, den = fwd_refs(shape)
    y = ops.stem_fwd(xd, wd, N, H, W)
    assert y.shape == (N, OH, OW, 64)
    rows = band_errors(y.reshape(N * OH, OW * 64), y64.reshape(N * OH, OW * 64), band=1)
    cols = band_errors(y.permute(2, 0, 1, 3).reshape(OW, -1), y64.permute(2, 0, 1, 3).reshape(OW, -1), band=1)
    assert rows.numel() == N * OH and cols.numel() == OW
    whole = rel_err(y, y64)
    cw, cbar = componentwise(y, y64, y32, den)
    cbar = bar_of(cbar, FWD)
    # statistics and shift: the same y, bit for bit (test_stem's property); every unit row of the partials on its own
    worst_part = 0.0
    for shift in (None, shd):
        y2, part = ops.stem_fwd(xd, wd, N, H, W, stats=True, shift=shift)
        assert torch.equal(y2, y), (shape, "the statistics epilogue changed y")
        worst_part = max(worst_part, check_stats(part, y2, None if shift is None else t["shift"], shape, units,
                                                 f"stem_fwd {shape} shift {shift is not None}"))
    extra = ""
    if shape in FWD_BF16:
        y16 = ops.stem_fwd(xd, wd, N, H, W, dtype=torch.bfloat16)
        assert y16.dtype == torch.bfloat16 and torch.equal(y16, y.bfloat16()), (shape, "bf16 y is not the fp32 y rounded once")
        for shift in (None, shd):
            y16s, part = ops.stem_fwd(xd, wd, N, H, W, dtype=torch.bfloat16, stats=True, shift=shift)
            assert torch.equal(y16s, y16), shape
            worst_part = max(worst_part, check_stats(part, y16s, None if shift is None else t["shift"], shape, units,
                                                     f"stem_fwd bf16 {shape} shift {shift is not None}"))
        extra = " | bf16: bit-equal, rounded once"
    print(f"\n[stem] fwd   {str(shape):16s} OH {OH:3d} OW {OW:3d} units {units:4d} grid.x {min(units, FWD_GRID):3d} bands {-(-OW // FWD_BAND)} "
          f"tiles {-(-OW // FWD_TILE):2d} | worst row {rows.max().item():.2e} worst column {cols.max().item():.2e} whole {whole:.2e} | "
          f"componentwise {cw:.2e} (bar {cbar:.2e}) | partials {worst_part:.2f} of the bound{extra}")
    assert cols.max().item() < FWD, (shape, "output column ox", int(cols.argmax()), cols.max().item())
    assert rows.max().item() < FWD, (shape, "output row (n * OH + oy)", int(rows.argmax()), rows.max().item())
    assert whole < FWD, (shape, whole)
    assert cw <= cbar, (shape, cw, cbar)


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def run_wgrad(ops, dev, shape, mode):
    N, H, W = shape
    OH, OW, units, slabs_n = geometry(ops, shape)
    assert slabs_n == min(WG_GRID, units * -(-OW // WG_TILE)), (shape, slabs_n)
    t = inputs(shape)
    xd = t["x"].to(dev)
    arg = dy_device(ops, dev, shape, mode)

    def call():
        dw = torch.full((64, 7, 7, 3), float("nan"), device=dev)
        slabs = torch.full(((slabs_n + 16) * 49 * 64,), float("nan"), device=dev)
        ops.stem_wgrad(arg, xd, dw, N, H, W, slabs=slabs)
        torch.cuda.synchronize()
        return dw
    dw = call()
    bad = ~torch.isfinite(dw)
    assert not bool(bad.any()), (shape, mode, f"{int(bad.sum())} of {dw.numel()} elements: a block did not deliver its slab")
    assert torch.equal(call(), dw), (shape, mode, "the slab sum is deterministic")
    assert torch.equal(dw[..., 0], dw[..., 1]) and torch.equal(dw[..., 0], dw[..., 2]), (shape, mode)      # the three folded channels
    got = dw[..., 0].reshape(64, 49).t()                                                                  # -> [49][64]
    dy64, dy32 = dy_forms(shape, mode)
    x = t["x"]
    r64, r32, den = wgrad_cpu(dy64, x.double()), wgrad_cpu(dy32, x), wgrad_cpu(dy32.abs(), x.abs()).double() + 1e-300
    taps = band_errors(got, r64, band=1)
    assert taps.numel() == 49
    whole = rel_err(got, r64)
    cw, cbar = componentwise(got, r64, r32, den)
    cbar = bar_of(cbar, BWD)
    print(f"\n[stem] wgrad {str(shape):16s} {mode:10s} OH {OH:3d} OW {OW:3d} units {units:4d} slabs {slabs_n:4d} bands {-(-OW // WG_BAND)} "
          f"reduce levels {2 if slabs_n >= 64 else 1} | worst tap {taps.max().item():.2e} whole {whole:.2e} | componentwise {cw:.2e} (bar {cbar:.2e})")
    assert taps.max().item() < BWD, (shape, mode, "tap kh * 7 + kw", int(taps.argmax()), taps.max().item())
    assert whole < BWD, (shape, mode, whole)
    assert cw <= cbar, (shape, mode, cw, cbar)
    return units, slabs_n


@pytest.mark.parametrize("shape", WG_SHAPES, ids=ids(WG_SHAPES))
def test_stem_wgrad_edges(dev, shape):
    from oaprogressionmmf_amd import ops
    units, slabs_n = run_wgrad(ops, dev, shape, "plain")
    if shape in WG_WALKS:
        assert units == 1025 and slabs_n == WG_GRID < units          # block 0 takes units 0 and 1024
    if shape in SLAB_LEVELS:
        assert slabs_n == (63, 64)[SLAB_LEVELS.index(shape)]         # koaf_slab_reduce: two levels from 64 slabs on
        assert slabs_n > units                                       # ... and idle blocks that must deliver zero slabs


@pytest.mark.parametrize("mode", ["plain", "apply", "apply_bf16"])
def test_stem_wgrad_dy_modes(dev, mode):
    from oaprogressionmmf_amd import ops
    run_wgrad(ops, dev, WG_MODES_SHAPE, mode)


# ---------------------------------------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def run_dgrad(ops, dev, shape, mode):
    N, H, W = shape
    OH, OW = out_dim(H), out_dim(W)
    t = inputs(shape)
    arg = dy_device(ops, dev, shape, mode)
    wd = t["w1t"].to(dev)
    dx = ops.stem_dgrad(arg, wd, N, H, W)
    torch.cuda.synchronize()
    assert dx.shape == (N, H, W) and bool(torch.isfinite(dx).all()), (shape, mode)
    assert torch.equal(ops.stem_dgrad(arg, wd, N, H, W), dx), (shape, mode)
    dy64, dy32 = dy_forms(shape, mode)
    w = t["w1t"]
    r64, r32 = dgrad_cpu(dy64, w.double(), shape), dgrad_cpu(dy32, w, shape)
    den = dgrad_cpu(dy32.abs(), w.abs(), shape).double() + 1e-300
    rows = band_errors(dx.reshape(N * H, W), r64.reshape(N * H, W), band=1)
    cols = band_errors(dx.permute(2, 0, 1).reshape(W, N * H), r64.permute(2, 0, 1).reshape(W, N * H), band=1)
    assert rows.numel() == N * H and cols.numel() == W
    whole = rel_err(dx, r64)
    cw, cbar = componentwise(dx, r64, r32, den)
    cbar = bar_of(cbar, BWD)
    print(f"\n[stem] dgrad {str(shape):16s} {mode:10s} OH {OH:3d} OW {OW:3d} tiles {-(-OH // DG_I)}x{-(-OW // DG_I)} | worst row {rows.max().item():.2e} "
          f"worst column {cols.max().item():.2e} whole {whole:.2e} | componentwise {cw:.2e} (bar {cbar:.2e})")
    assert rows.max().item() < BWD, (shape, mode, "input row (n * H + iy)", int(rows.argmax()), rows.max().item())
    assert cols.max().item() < BWD, (shape, mode, "input column ix", int(cols.argmax()), cols.max().item())
    assert whole < BWD, (shape, mode, whole)
    assert cw <= cbar, (shape, mode, cw, cbar)


@pytest.mark.parametrize("shape", DG_SHAPES, ids=ids(DG_SHAPES))
def test_stem_dgrad_edges(dev, shape):
    from oaprogressionmmf_amd import ops
    run_dgrad(ops, dev, shape, "plain")


@pytest.mark.parametrize("mode", ["plain", "apply", "apply_bf16"])
def test_stem_dgrad_dy_modes(dev, mode):
    from oaprogressionmmf_amd import ops
    run_dgrad(ops, dev, DG_MODES_SHAPE, mode)
