"""The 3x3 / stride-1 / pad-1 convolutions over activation plane images, forward and data gradient, per band and per tile of the kernel
that ran: the rectangle-tile kernel (koaf_gemm/t2d, 8 x 16 pixels, 128 x 64), the 128-row halo kernel (koaf_gemm/halo128, 128 x 64 |
128 x 128) and the 256-row halo kernel (koaf_gemm/halo, 256 x 64 | 256 x 128), at the edges plan_tiles (koaf_gemm.hip) and halo_max_w
(koaf_gemm_kernel.h) draw between them, and the refusals that fall back to the per-tap gather kernel.

Every row of ROWS goes through ops.conv2d_fwd / ops.conv2d_dgrad as the model calls them (weight plane images, aplanes at its default,
the halo mode at its default unless the row says otherwise) and ASSERTS FROM THE LAUNCH RECORD variant, bm, bn, tiles, grid_x == tiles,
fmt 1, act16 and M / N / K: a row that lands on another kernel fails.  tests/test_conv3_plan_cpu.py asks the planner the same on any
machine.  shape = (N, H, W, Cin, Cout) in forward orientation; the data gradient of a row is the same convolution, so its plan reads
A.C = Cout and its GEMM N = Cin.  Outputs, statistics, partial sums and max |dz| go in as NaN (ops.conv._empty patched); every fp32 call
runs twice and must reproduce itself bit for bit.

Calls.  Forward: prologue (BatchNorm + ReLU folded into the plane cut, statistics about a generic shift -- the production call) | plain
(statistics about zero).  Data gradient: bnb2 (dy a BnApply, residual, fused BatchNorm-backward epilogue mode 2, max |dz| -- the
production call) | plain (dy + amax) | apply | apply_res | bnb1 (dy, residual, epilogue mode 1 with two BatchNorms).  "-bf16": the
call in bf16 activation storage (forward act16 1, data gradient act16 2), held by the existing property only: bit-equal to the fp32 mode
on widened inputs, the forward output rounded once, gradients fp32.
REFUSED by the library: no combination of the three kernels (every call of the table has its instantiation in all three storage roles).
One refusal sits in front of them: the BatchNorm column reductions (ops.colstats / ops.bn_bwd, koaf_colpart_rows) do not take C = 96 |
160 | 192 (C / 4 does not divide 256), so no BnApply of that width can come out of the library's own BatchNorm.  The data gradients with
Cout = 96 | 160 | 192 (the odd chunk counts) assert that error and take the same recipe -- dz, c, coef, koaf_bn_bwd_finalize's bound --
formed by torch on the device; the GEMM and its plane cut, not the reduction, are under test here.

Held per fp32 call (the bars are test_tiles_gpu.py's and test_gconv_gpu.py's; nothing new is invented):
  * relative L2 against float64 on the CPU per 128 rows OF THE TILE ORDER and over the whole tensor: FWD forward, BWD gradients.  The halo
    kernels' tiles are raster bands; for t2d tile_order() reorders the rows into the 8 x 16 rectangles of one image (tile = image, tile
    row, tile column; row = (y, x) inside it) and asserts that every pixel is covered exactly once.
  * componentwise max |y - y64| / (|a| @ |b|) <= 8 x the same ratio of torch's fp32 product of the same operands.
  * forward statistics PER PARTIAL ROW: part[t] against the float64 sums of (y64 - shift) and (y64 - shift)^2 over exactly the pixels of
    tile t (a rectangle for t2d, a raster band of bm rows otherwise, the ragged last one included), relative L2 over the columns, 1e-4
    on sums and 1e-5 on squares; part.shape[0] and the column totals as well.
  * fused BatchNorm-backward partial sums PER PARTIAL ROW against float64 over the tile's pixels, relative L2 over the columns at
    run_dgrad's 1e-4.  The same per-tile sums formed by torch in fp32 on the CPU are printed beside it ("ref32").  That
    reference stayed under a tenth of the bar on every row (MEASURED below), so no row takes the fallback the test carries: a sum
    whose fp32 reference is NOT under 1e-5 (cancelling sums) is normalised by the tile's sum of |terms| instead, and says so in its line.
  * mode-2 masks: run_dgrad's construction, inputs more than 1e-5 from the mask boundary, asserted; max |dz| as there.
Each call prints one line: variant / tile / tiles, worst band, componentwise ratio and bar, worst per-tile statistic.

MEASURED (MI355X), worst over the rows of a kernel -- band | componentwise (its bar) | per-tile statistics:
  t2d      forward        2.8e-7 | 2.6e-7 (1.7e-6) | sums 1.7e-7 (bar 1e-4) squares 1.1e-7 (bar 1e-5)
           data gradient  2.7e-7 | 2.8e-7 (2.3e-6) | partials 2.7e-7 (bar 1e-4; torch's fp32 per-tile sums from float64: 3.8e-7)
  halo128  forward        2.8e-7 | 3.0e-7 (2.1e-6) | sums 2.0e-7 squares 1.7e-7
           data gradient  2.8e-7 | 1.5e-7 (1.4e-6) | partials 2.9e-7 (fp32 reference 5.3e-7; 2.2e-6 on the three-pixel row 3x1x1)
  halo     forward        7.5e-7 | 1.3e-7 (5.7e-7) | sums 2.8e-7 squares 3.0e-7
           data gradient  3.8e-7 | 1.7e-7 (4.1e-7) | partials 6.2e-7 (fp32 reference 5.4e-7)
  gather   forward        3.8e-7 | 1.9e-7 (1.7e-6) | sums 1.3e-7 squares 1.6e-7"""
import zlib
from collections import namedtuple
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from test_tiles_gpu import BWD, FWD, G, H128, H256, Record, _conv64, _dgrad64, band_errors, componentwise, rel_err

pytestmark = pytest.mark.gpu

T2D = "koaf_gemm/t2d"
Row = namedtuple("Row", "name shape op variant bm bn calls halo")
PROD = {"fwd": ("prologue",), "dgrad": ("bnb2",)}
FULL = {"fwd": ("prologue", "plain", "prologue-bf16"), "dgrad": ("bnb2", "plain", "apply", "apply_res", "bnb1", "bnb2-bf16")}


def R(shape, op, variant, bm, bn, full=False, halo=1):
    N, H, W, Cin, Cout = shape
    name = f"{N}x{H}x{W}-{Cin}to{Cout}-{op}" + (f"-halo{halo}" if halo != 1 else "")
    return Row(name, shape, op, variant, bm, bn, (FULL if full else PROD)[op], halo)


ROWS = [
    # ---- the rectangle kernel: A.C = 64, 64 | 128 output columns, H % 8 == 0, W % 16 == 0, W inside the halo kernels' limit
    R((5, 8, 16, 64, 64), "fwd", T2D, 128, 64, full=True),           # one tile per image: all four borders in every tile
    R((2, 16, 32, 64, 128), "fwd", T2D, 128, 64, full=True),         # 2 x 2 tiles per image, two column tiles
    R((1, 24, 48, 64, 64), "fwd", T2D, 128, 64),                     # 3 x 3 tiles: the centre tile touches no border
    R((1, 8, 96, 64, 64), "fwd", T2D, 128, 64),                      # the widest row, six tiles across (production width)
    R((3, 16, 64, 64, 128), "fwd", T2D, 128, 64),                    # 128 columns at their widest W
    R((5, 8, 16, 64, 64), "dgrad", T2D, 128, 64, full=True),         # (the flipped filter)
    R((2, 16, 32, 128, 64), "dgrad", T2D, 128, 64, full=True),
    R((1, 24, 48, 64, 64), "dgrad", T2D, 128, 64),
    R((1, 8, 96, 64, 64), "dgrad", T2D, 128, 64),
    # ---- what must NOT take the rectangle kernel
    R((2, 12, 16, 64, 64), "fwd", H128, 128, 64),                    # H % 8
    R((2, 8, 24, 64, 64), "fwd", H128, 128, 64),                     # W % 16
    R((2, 8, 16, 32, 64), "fwd", H128, 128, 64),                     # 32 channels: one chunk
    R((2, 8, 16, 64, 256), "fwd", H128, 128, 128),                   # 256 columns
    R((2, 8, 16, 128, 64), "fwd", H256, 256, 64),                    # 128 channels
    R((1, 8, 112, 64, 64), "fwd", G, 64, 64),                        # W past 96: per-tap gather on the picker's tile
    R((1, 8, 80, 64, 128), "fwd", G, 64, 64),                        # W past 64 at 128 columns
    R((2, 16, 32, 64, 128), "fwd", H256, 256, 128, halo=2),          # ops.set_conv3x3_halo(2)
    R((2, 16, 32, 64, 128), "fwd", H128, 128, 128, halo=3),          # ops.set_conv3x3_halo(3)
    # ---- the 128-row halo kernel: A.C <= 64 and W <= 96 (64 columns) | 48 (128 columns)
    R((2, 77, 78, 64, 64), "dgrad", H128, 128, 64),                  # (its forward row is test_tiles_gpu.py's w78-halo128)
    R((1, 7, 96, 64, 64), "fwd", H128, 128, 64, full=True),          # W at the limit, last tile of 32 rows
    R((1, 7, 97, 64, 64), "fwd", G, 64, 64),                         # ... and past it
    R((3, 9, 48, 64, 128), "fwd", H128, 128, 128, full=True),        # 128 x 128, W at fits128
    R((3, 9, 49, 64, 128), "fwd", H256, 256, 128),                   # ... and past it: 256 rows
    R((7, 5, 5, 32, 64), "fwd", H128, 128, 64, full=True),           # 25-pixel images, five to a tile, one chunk, ragged
    R((40, 3, 3, 64, 64), "fwd", H128, 128, 64),                     # 9-pixel images
    R((1, 1, 50, 64, 64), "fwd", H128, 128, 64),                     # one image row
    R((6, 20, 1, 64, 64), "fwd", H128, 128, 64),                     # one image column: the raster neighbours are other rows
    R((3, 1, 1, 64, 64), "fwd", H128, 128, 64),                      # only the centre tap
    R((2, 12, 16, 64, 64), "dgrad", H128, 128, 64, full=True),
    R((7, 5, 5, 32, 64), "dgrad", H128, 128, 64, full=True),         # N = 32: half of a 64-column tile
    R((3, 9, 48, 128, 64), "dgrad", H128, 128, 128, full=True),      # 128 x 128 as a data gradient
    R((2, 16, 16, 160, 64), "dgrad", H128, 128, 128),                # (the twin of a 256-row row: A.C = 64), column tiles 128 + 32
    R((40, 3, 3, 64, 64), "dgrad", H128, 128, 64),
    R((6, 20, 1, 64, 64), "dgrad", H128, 128, 64),
    R((3, 1, 1, 64, 64), "dgrad", H128, 128, 64),
    # ---- the 256-row halo kernel: A.C > 64, or W past fits128; the halo double-buffered across 32-channel chunks
    R((1, 48, 48, 128, 128), "fwd", H256, 256, 128),
    R((3, 24, 24, 256, 256), "fwd", H256, 256, 128),                 # 6.75 row tiles, two column tiles, eight chunks
    R((5, 12, 12, 512, 512), "fwd", H256, 256, 128),                 # a tile straddles three images, 16 chunks, four column tiles
    R((2, 39, 39, 128, 128), "fwd", H256, 256, 128),                 # radiograph sizes
    R((7, 10, 10, 512, 512), "fwd", H256, 256, 128),
    R((1, 5, 96, 128, 64), "fwd", H256, 256, 64, full=True),         # the widest row at 64 columns
    R((1, 5, 97, 128, 64), "fwd", G, 64, 64),                        # ... and past it
    R((2, 9, 56, 64, 128), "fwd", H256, 256, 128),                   # A.C <= 64 but past fits128
    R((2, 16, 16, 96, 128), "fwd", H256, 256, 128, full=True),       # three chunks
    R((2, 16, 16, 160, 64), "fwd", H256, 256, 64),                   # five chunks
    R((2, 16, 16, 128, 192), "fwd", H256, 256, 128),                 # half-filled column tile (bn 128)
    R((2, 16, 16, 128, 96), "fwd", H256, 256, 64),                   # half-filled column tile (bn 64)
    R((1, 4, 4, 128, 128), "fwd", H256, 256, 128, full=True),        # 16 rows in a 256-row tile
    R((2, 1, 64, 128, 128), "fwd", H256, 256, 128),                  # one image row
    R((2, 64, 1, 128, 64), "fwd", H256, 256, 64),                    # one image column
    R((1, 48, 48, 128, 128), "dgrad", H256, 256, 128),
    R((3, 24, 24, 256, 256), "dgrad", H256, 256, 128),
    R((5, 12, 12, 512, 512), "dgrad", H256, 256, 128),
    R((2, 39, 39, 128, 128), "dgrad", H256, 256, 128),
    R((2, 16, 16, 128, 96), "dgrad", H256, 256, 128, full=True),     # A.C = 96: three chunks
    R((2, 16, 16, 64, 160), "dgrad", H256, 256, 64),                 # A.C = 160: five chunks
    R((2, 16, 16, 96, 128), "dgrad", H256, 256, 64, full=True),      # N = 96: half-filled column tile (bn 64)
    R((2, 16, 16, 192, 128), "dgrad", H256, 256, 128),               # N = 192: half-filled column tile (bn 128)
    R((2, 16, 16, 128, 192), "dgrad", H256, 256, 128),               # A.C = 192: six chunks
    R((1, 4, 4, 128, 128), "dgrad", H256, 256, 128, full=True),
]


def gemm_dims(row):
    """(M, N, K) of the koaf_gemm call behind a row"""
    N, H, W, Cin, Cout = row.shape
    return (N * H * W, Cout, 9 * Cin) if row.op == "fwd" else (N * H * W, Cin, 9 * Cout)


def n_tiles(row):
    M, Ng, _ = gemm_dims(row)
    return -(-M // row.bm) * -(-Ng // row.bn)


def tile_order(row):
    """the output rows in the order of the tiles that wrote them: raster order for the halo and gather kernels; for t2d the 8 x 16
    rectangles of one image, tile (image, tile row, tile column), row (y, x) inside it -- every pixel exactly once"""
    N, H, W = row.shape[:3]
    M = N * H * W
    if row.variant != T2D:
        return torch.arange(M)
    assert H % 8 == 0 and W % 16 == 0
    order = torch.arange(M).reshape(N, H // 8, 8, W // 16, 16).permute(0, 1, 3, 2, 4).reshape(-1)
    assert order.numel() == M and torch.equal(order.sort().values, torch.arange(M))
    return order


def tile_sums(v, order, bm):
    """[tiles, C] float64 sums of v [M, C] over the rows of every tile (the ragged last one included)"""
    v = v.reshape(order.numel(), -1)[order]
    v = F.pad(v, (0, 0, 0, (-v.shape[0]) % bm))
    return v.reshape(-1, bm, v.shape[1]).sum(1)


def rows_err(got, ref, den=None):
    """relative L2 over the columns of every row of got [T, C] against ref; den: the norm it is relative to (default: ref's)"""
    got, ref = got.detach().double().cpu(), ref.double()
    den = ref if den is None else den.double()
    return (got - ref).norm(dim=1) / (den.norm(dim=1) + 1e-300)


@contextmanager
def nan_outputs(ops):
    """every tensor ops.conv allocates for a call comes back filled with NaN"""
    real = ops.conv._empty

    def nan_empty(*a, **k):
        out = real(*a, **k)
        return out.fill_(float("nan")) if out.is_floating_point() else out
    ops.conv._empty = nan_empty
    try:
        yield
    finally:
        ops.conv._empty = real


def check_record(row, launches, act16):
    M, Ng, K = gemm_dims(row)
    assert len(launches) == 1, (row.name, launches)
    r = launches[0]
    tiles = n_tiles(row)
    want = dict(variant=row.variant, bm=row.bm, bn=row.bn, tiles=tiles, grid_x=tiles, splitk=1, nbatch=1, fmt=1, act16=act16, M=M, N=Ng, K=K,
                emit=0)
    assert {f: r[f] for f in want} == want, (row.name, r, want)
    return r


def line(row, call, r, text):
    print(f"\n[conv3] {row.name:30s} {call:13s} {r['variant']:17s} {r['bm']:3d}x{r['bn']:<3d} tiles {r['tiles']:3d} act16 {r['act16']} | {text}")


def generator(row):
    g_ = torch.Generator().manual_seed(zlib.crc32(row.name.encode()))

    def rnd(*shape):
        return torch.randn(*shape, generator=g_)
    return g_, rnd


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def run_forward(dev, row):
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout = row.shape
    M = N * H * W
    _, rnd = generator(row)
    x = rnd(N, H, W, Cin) * 1.5 + 0.3
    w = rnd(Cout, 3, 3, Cin) * (9 * Cin) ** -0.5
    sc, sh, shift = rnd(Cin) * 0.2 + 1.0, rnd(Cin) * 0.1, rnd(Cout) * 0.3 + 0.2
    wd, scd, shd, shiftd = w.to(dev), sc.to(dev), sh.to(dev), shift.to(dev)
    img = ops.build_weight_planes(wd, Cout, 9, Cin)
    order = tile_order(row)
    nt = -(-M // row.bm)

    def call_(xd, prologue):
        with nan_outputs(ops), Record() as rec:
            y, part = ops.conv2d_fwd(xd, wd, N, H, W, Cin, Cout, 3, 3, 1, 1, scd if prologue else None, shd if prologue else None,
                                     stats=True, shift=shiftd if prologue else None, wimg=img)
        torch.cuda.synchronize()
        return y, part, rec.launches

    for call in row.calls:
        prologue = call.startswith("prologue")
        if call.endswith("-bf16"):
            xb = x.bfloat16().float().to(dev)
            y32, p32, _ = call_(xb, prologue)
            y, part, launches = call_(xb.bfloat16(), prologue)
            r = check_record(row, launches, 1)
            assert y.dtype == torch.bfloat16 and part.dtype == torch.float32 and part.shape[0] == nt, row.name
            assert bool(torch.isfinite(y32).all()), row.name
            assert torch.equal(y, y32.bfloat16()), (row.name, call, "the fp32 mode's output on widened inputs, rounded once")
            assert torch.equal(part, p32), (row.name, call, "statistics from the fp32 accumulators")
            line(row, call, r, "bit-equal to the fp32 mode on widened inputs, rounded once")
            continue
        xd = x.to(dev)
        y, part, launches = call_(xd, prologue)
        r = check_record(row, launches, 0)
        assert y.dtype == torch.float32 and bool(torch.isfinite(y).all()), (row.name, call, "a tile of y was not written")
        assert part.shape[0] == nt and bool(torch.isfinite(part).all()), (row.name, call, part.shape)
        y2, part2, _ = call_(xd, prologue)
        assert torch.equal(y2, y) and torch.equal(part2, part), (row.name, call, "the same call twice")
        x64, w64 = x.double(), w.double()
        a64, a32 = (torch.relu(x64 * sc.double() + sh.double()), torch.relu(x * sc + sh)) if prologue else (x64, x)
        y64 = _conv64(a64, w64, 3, 1, 1).reshape(M, Cout)
        y32 = _conv64(a32, w, 3, 1, 1).reshape(M, Cout)
        den = _conv64(a32.abs(), w.abs(), 3, 1, 1).double().reshape(M, Cout) + 1e-300
        yc = y.cpu().reshape(M, Cout)
        be = band_errors(yc[order], y64[order])
        whole = rel_err(yc, y64)
        cw, bar = componentwise(yc, y64, y32, den)
        d = y64 - (shift.double() if prologue else 0.0)
        e1, e2 = rows_err(part[:, 0], tile_sums(d, order, row.bm)), rows_err(part[:, 1], tile_sums(d * d, order, row.bm))
        t1, t2 = rel_err(part[:, 0].double().sum(0), d.sum(0)), rel_err(part[:, 1].double().sum(0), (d * d).sum(0))
        line(row, call, r, f"worst band {be.max().item():.2e} whole {whole:.2e} | componentwise {cw:.2e} (bar {bar:.2e}) | per-tile sums "
                           f"{e1.max().item():.1e} squares {e2.max().item():.1e} totals {t1:.1e} {t2:.1e}")
        assert be.max().item() < FWD, (row.name, call, int(be.argmax()), be.max().item())
        assert whole < FWD, (row.name, call, whole)
        assert cw <= bar, (row.name, call, cw, bar)
        assert e1.max().item() < 1e-4, (row.name, call, "sums of tile", int(e1.argmax()), e1.max().item())
        assert e2.max().item() < 1e-5, (row.name, call, "squares of tile", int(e2.argmax()), e2.max().item())
        assert t1 < 1e-4 and t2 < 1e-5, (row.name, call, t1, t2)


# ------------------------------------------------------------------------------------------------
# data gradient
# ------------------------------------------------------------------------------------------------
def run_dgrad(dev, row):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    from oaprogressionmmf_amd.ops.bn import BnApply
    N, H, W, Cin, Cout = row.shape
    M = N * H * W
    shape8 = row.shape + (3, 1, 1)
    g_, rnd = generator(row)
    w = rnd(Cout, 3, 3, Cin) * (9 * Cin) ** -0.5
    wd = w.to(dev)
    img = ops.build_weight_planes(wd, Cout, 9, Cin)
    res = rnd(N, H, W, Cin) * 1e-3
    dy = rnd(N, H, W, Cout) * 1e-3
    c = rnd(N, H, W, Cout) * 1.5 + 0.3                      # the conv output whose BatchNorm is back-propagated (BnApply)
    gup = rnd(N, H, W, Cout) * 1e-3
    cx = rnd(N, H, W, Cin) * 1.5 + 0.3                      # the producer's conv output and its BatchNorm record
    sv = torch.stack([rnd(Cin) * 0.3, torch.rand(Cin, generator=g_) + 0.5, (rnd(Cin) * 0.5 + 1).abs().clamp(min=0.25), rnd(Cin) * 0.2])
    # mode 2 masks by the sign of sc * c + sh: the inputs keep that value out of rounding's reach (|.| > 1e-5 on values of order 1)
    cx = torch.where((cx * sv[2] + sv[3]).abs() < 1e-3, cx + 0.1, cx)
    yk, c2 = rnd(N, H, W, Cin), rnd(N, H, W, Cin)           # mode 1 masks by y > 0
    sv2 = torch.stack([rnd(Cin) * 0.3, torch.rand(Cin, generator=g_) + 0.5, rnd(Cin), rnd(Cin)])
    gam, bet = (rnd(Cout) * 0.2 + 1).to(dev), (rnd(Cout) * 0.1).to(dev)
    resd, dyd, gupd, svd, sv2d = res.to(dev), dy.to(dev), gup.to(dev), sv.to(dev), sv2.to(dev)
    am = dyd.abs().max().reshape(1).float()
    order = tile_order(row)
    nt = -(-M // row.bm)

    def bn_apply(cc):
        """the BnApply of the BatchNorm behind the convolution, from its input in one storage mode"""
        if (256 * 4) % Cout:
            # the library's column reductions do not take this width (koaf_colpart_rows: C / 4 divides 256): the same recipe from torch
            with pytest.raises(KoafError, match="unsupported C"):
                ops.colstats(cc, M, Cout)
            cf = cc.float().reshape(M, Cout)
            mean, invstd = cf.mean(0), (cf.var(0, unbiased=False) + 1e-5).rsqrt()
            k0 = gam * invstd
            dz = gupd.reshape(M, Cout) * ((cf - mean) * k0 + bet > 0)
            k1, s2 = dz.sum(0) / M, (dz * ((cf - mean) * invstd)).sum(0) / M
            k2 = k0 * invstd * s2
            coef = torch.stack([k0, k1, k2, k2 * mean - k0 * k1]).contiguous()
            amax = (k0.abs() * (dz.abs().max() + k1.abs()) + k2.abs() * (M - 1) ** 0.5 / invstd).max().reshape(1)   # koaf_bn_bwd_finalize's bound
            return BnApply(dz.reshape(N, H, W, Cout).contiguous(), cc, coef, amax, mean.contiguous(), M, Cout)
        svc = ops.bn_finalize(ops.colstats(cc, M, Cout), Cout, M, gam, bet, torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev),
                              torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)
        dgm, dbt = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
        return ops.bn_bwd(gupd.clone(), cc, svc, M, Cout, M, dgm, dbt, 2, fused=True)

    def call_(call, arg, t):
        """t: the BatchNorm-backward operands (cx, y, c2) in the storage mode of the call"""
        kw = dict(wimg=img)
        if call in ("plain", "bnb1"):
            kw["dy_amax"] = am
        if call not in ("plain", "apply"):
            kw["residual"] = resd
        if call == "bnb1":
            kw["bnb"] = dict(mode=1, c=t["cx"], y=t["y"], saved=svd, c2=t["c2"], saved2=sv2d)
        elif call == "bnb2":
            kw["bnb"] = dict(mode=2, c=t["cx"], saved=svd, dz_amax=True)
        with nan_outputs(ops), Record() as rec:
            out = ops.conv2d_dgrad(arg, wd, N, H, W, Cin, Cout, 3, 3, 1, 1, **kw)
        torch.cuda.synchronize()
        return (out if isinstance(out, tuple) else (out,)), rec.launches

    args, refs = {}, {}

    def conv_refs(kind, arg):
        """(g64, g32, den) of the convolution part, shared by the calls of a row with the same dy"""
        if kind not in refs:
            if kind == "apply":
                coef, dz, cc = arg.coef.double().cpu(), arg.dz.double().cpu(), arg.c.double().cpu()
                dy64 = coef[0] * dz + coef[3] - coef[2] * cc
                c32 = arg.coef.cpu()
                dy32 = c32[0] * arg.dz.cpu() + c32[3] - c32[2] * arg.c.float().cpu()
            else:
                dy64, dy32 = dy.double(), dy
            refs[kind] = (_dgrad64(dy64, w.double(), shape8), _dgrad64(dy32, w, shape8), _dgrad64(dy32.abs(), w.abs(), shape8).double())
        return refs[kind]

    for call in row.calls:
        base = call.split("-")[0]
        kind = "apply" if base in ("apply", "apply_res", "bnb2") else "plain"
        if call.endswith("-bf16"):
            assert kind == "apply" and base == "bnb2"
            cb, cxb = c.bfloat16().to(dev), cx.bfloat16()
            assert float((cxb.double() * sv[2].double() + sv[3].double()).abs().min()) > 1e-5
            o32, _ = call_(base, bn_apply(cb.float()), dict(cx=cxb.float().to(dev)))
            o16, launches = call_(base, bn_apply(cb), dict(cx=cxb.to(dev)))
            r = check_record(row, launches, 2)
            assert o16[1].shape[0] == nt and bool(torch.isfinite(o32[0]).all()), row.name
            for a, b in zip(o16, o32):
                assert a.dtype == torch.float32 and torch.equal(a, b), (row.name, call, "gradients are fp32 and equal in both modes")
            line(row, call, r, "bit-equal to the fp32 mode on widened inputs")
            continue
        assert float((cx.double() * sv[2].double() + sv[3].double()).abs().min()) > 1e-5
        if kind == "apply" and kind not in args:
            args[kind] = bn_apply(c.to(dev))
        arg = args[kind] if kind == "apply" else dyd
        t = dict(cx=cx.to(dev), y=yk.to(dev), c2=c2.to(dev))
        out, launches = call_(base, arg, t)
        r = check_record(row, launches, 0)
        assert all(o.dtype == torch.float32 and bool(torch.isfinite(o).all()) for o in out), (row.name, call, "an output was not written")
        out2, _ = call_(base, arg, t)
        assert len(out2) == len(out) and all(torch.equal(a, b) for a, b in zip(out, out2)), (row.name, call, "the same call twice")
        g64, g32, den = conv_refs(kind, arg)
        if base not in ("plain", "apply"):
            g64, g32, den = g64 + res.double(), g32 + res, den + res.double().abs()
        extra = ""
        if base.startswith("bnb"):
            cx64, sv64 = cx.double(), sv.double()
            mask = (yk > 0) if base == "bnb1" else ((cx64 * sv64[2] + sv64[3]) > 0)
            g64, g32 = g64 * mask, g32 * mask
            terms = [(g64, g32), (g64 * ((cx64 - sv64[0]) * sv64[1]), g32 * ((cx - sv[0]) * sv[1]))]
            if base == "bnb1":
                terms.append((g64 * ((c2.double() - sv2[0].double()) * sv2[1].double()), g32 * ((c2 - sv2[0]) * sv2[1])))
            part = out[1]
            assert part.shape[:2] == (nt, len(terms)), (row.name, call, part.shape)
            worst, worst32, how = [], [], []
            for i, (t64, t32) in enumerate(terms):
                s64 = tile_sums(t64, order, row.bm)
                ref32 = rows_err(tile_sums(t32, order, row.bm).float(), s64).max().item()       # torch's fp32 terms, summed per tile
                dn = None if ref32 < 1e-5 else tile_sums(t64.abs(), order, row.bm)              # cancelling sums: relative to sum |terms|
                e = rows_err(part[:, i], s64, dn)
                tot = rel_err(part[:, i].double().sum(0), t64.reshape(M, Cin).sum(0))
                assert e.max().item() < 1e-4, (row.name, call, "partial sum", i, "tile", int(e.argmax()), e.max().item(), ref32)
                assert tot < 1e-4, (row.name, call, "partial sum", i, tot)
                worst.append(e.max().item()), worst32.append(ref32), how.append("" if dn is None else "*")
            extra = " | per-tile partials " + " ".join(f"{e:.1e}{h}" for e, h in zip(worst, how)) + \
                    " (ref32 " + " ".join(f"{e:.1e}" for e in worst32) + ")"
        dx = out[0].cpu().reshape(M, Cin)
        g64r = g64.reshape(M, Cin)
        be = band_errors(dx[order], g64r[order])
        whole = rel_err(dx, g64r)
        cw, bar = componentwise(dx, g64r, g32.reshape(M, Cin), den.reshape(M, Cin) + 1e-300)
        line(row, call, r, f"worst band {be.max().item():.2e} whole {whole:.2e} | componentwise {cw:.2e} (bar {bar:.2e}){extra}")
        assert be.max().item() < BWD, (row.name, call, int(be.argmax()), be.max().item())
        assert whole < BWD, (row.name, call, whole)
        assert cw <= bar, (row.name, call, cw, bar)
        if base == "bnb2":
            assert abs(float(out[2]) / float(out[0].abs().max()) - 1) < 1e-6, (row.name, call)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_conv3_edges(dev, row):
    from oaprogressionmmf_amd import ops
    was = ops.set_conv3x3_halo(row.halo)
    try:
        (run_forward if row.op == "fwd" else run_dgrad)(dev, row)
    finally:
        ops.set_conv3x3_halo(was)
        torch.cuda.empty_cache()
