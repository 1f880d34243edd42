"""The dense 1x1 / stride-1 forward convolutions on the 256-row kernel (koaf_fwd1.hip) against the streamed kernel they leave.

koaf_conv2d_fwd hands a pointwise forward convolution to koaf_fwd1 when the call runs the fp16 scheme on fp32 tensors with the weights'
F plane image, without tail or emission, Cin % 32 == 0 with at least two k-tiles, Cout % 128 == 0, the streamed kernels switched on and
M a whole number of 256-row tiles, at least one per CU (M >= 65536) -- koaf_conv.hip fwd1_ok.  koaf_fwd1_form's table names, per
production (Cin, Cout), the form that passed the per-call rule: one tile per block (grid_x = tiles; 512 -> 2048), the persistent walk
(grid_x = min(tiles, 256); 128 -> 512, 256 -> 1024, 256 -> 128, 512 -> 256) or neither (64 -> 256 stays on the streamed kernel: the
first REFUSAL; K = 64 is therefore reached at 64 -> 512); a shape the table does not know runs the walk.  Every row of CASES is the smallest shape of its
kind (all have M >= 65536, none more than 70000 rows); it goes through ops.conv2d_fwd as the model calls it, with y and the statistics
buffer pre-filled with NaN, and ASSERTS FROM THE LAUNCH RECORD the variant, tile, tile count and grid_x.

Held per case:
  * y, the returned row count and part[:rows] are torch.equal to ops.gemm on the descriptor koaf_conv2d_fwd builds, at 128 x 128 tiles
    (ops.gemm bypasses the new rule and runs koaf_gemm/stream), and once more with ops.set_stream(False) around the reference call (the
    block-wide loader).  The new kernel writes two partial rows per 256-row tile where the 128-row tiling puts them.
  * against float64 on the CPU for sampled 64-column blocks of y over ALL rows: relative L2 < FWD per 128-row band and the componentwise
    bar of test_tiles_gpu (8 x torch's fp32 product of the same operands); FWD and the bar's function are imported, not restated.  The
    statistics of the sampled columns are held against the float64 column sums of (y - shift) and (y - shift)^2 at run_forward's bars
    (1e-4 / 1e-5 relative L2 over the columns); the shift is a generic vector, not the mean.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: no koaf_fwd1 record, and the last GEMM record is koaf_gemm or koaf_gemm/stream on 128-row
tiles (stride 2 at the same shape: koaf_fwd_s2).

(K = 64: two k-steps, the next tile's prefetch is issued in the first; 66304 rows = 259 row tiles x 2 = 518 tiles: blocks walk 2 and 3
tiles and a row-tile change falls inside a block's run; 256 -> 768 and 128 -> 384: three column tiles per row tile at either width; Cin = 1024 fills the coefficient table; Cin = 2048
plain runs past it.)"""
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

from test_tiles_gpu import FWD, Record, band_errors, componentwise, rel_err

pytestmark = pytest.mark.gpu

F1, FS2, GEN, STREAM = "koaf_fwd1", "koaf_fwd_s2", "koaf_gemm", "koaf_gemm/stream"
Case = namedtuple("Case", "name shape call stats bn walk")
# shape (N, H, W, Cin, Cout); call: plain | prologue (tf 1); stats: False | True | "shift"; walk: the form koaf_fwd1_form ships the shape in
CASES = [
    Case("64to512-prologue-shift", (64, 32, 32, 64, 512), "prologue", "shift", 256, 1),
    Case("128to512-prologue-259-row-tiles", (37, 32, 56, 128, 512), "prologue", True, 256, 1),
    Case("256to768-prologue-nostats", (64, 32, 32, 256, 768), "prologue", False, 256, 1),
    Case("1024to256-prologue", (64, 32, 32, 1024, 256), "prologue", True, 256, 1),
    Case("2048to256-plain", (64, 32, 32, 2048, 256), "plain", True, 256, 1),
    Case("256to128-plain-shift", (64, 32, 32, 256, 128), "plain", "shift", 128, 1),
    Case("128to384-prologue", (64, 32, 32, 128, 384), "prologue", True, 128, 1),
    Case("512to2048-prologue-one-tile-form", (64, 32, 32, 512, 2048), "prologue", True, 256, 0),
]
Refusal = namedtuple("Refusal", "name shape stride how")
BASE = (64, 32, 32, 128, 256)
REFUSALS = [
    Refusal("64to256-kept-by-the-per-call-rule", (64, 32, 32, 64, 256), 1, "prologue"),
    Refusal("M-65664", (513, 16, 8, 128, 256), 1, "plain"),
    Refusal("M-12288", (48, 16, 16, 256, 512), 1, "plain"),
    Refusal("stream-off", BASE, 1, "nostream"),
    Refusal("tail", BASE, 1, "tail"),
    Refusal("emit", BASE, 1, "emit"),
    Refusal("bf16storage", BASE, 1, "bf16"),
    Refusal("bf16scheme", BASE, 1, "noimg"),
    Refusal("Cout-64", (64, 32, 32, 128, 64), 1, "plain"),
    Refusal("K-32", (64, 32, 32, 32, 256), 1, "plain"),
    Refusal("prologue-Cin-2048", (64, 32, 32, 2048, 128), 1, "prologue"),
    Refusal("stride-2", BASE, 2, "plain"),
]


@lru_cache(maxsize=1)
def inputs(shape, dev):
    """device operands of a shape: x [N, H, W, Cin], its prologue (sc, sh), the packed weight with its plane images, a statistics shift"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout = shape
    g_ = torch.Generator(device=dev).manual_seed(10100 + sum(shape))

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    t = dict(x=rnd(N, H, W, Cin) * 1.5 + 0.3, sc=rnd(Cin) * 0.2 + 1.0, sh=rnd(Cin) * 0.1, w=rnd(Cout, 1, 1, Cin) * Cin ** -0.5,
             shift=rnd(Cout) * 0.3 + 0.2)
    t["img"] = ops.build_weight_planes(t["w"], Cout, 1, Cin)
    torch.cuda.synchronize()
    return t


def call_model(dev, shape, t, call, stats, stride=1, **kw):
    """ops.conv2d_fwd as the model calls it, y and part pre-filled with NaN -> (y [M, Cout], part[:rows] or None, the launch records)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout = shape
    prol = call == "prologue"
    real_empty = ops.conv._empty

    def nan_empty(*a, **k_):
        out = real_empty(*a, **k_)
        return out.fill_(float("nan")) if out.is_floating_point() else out
    ops.conv._empty = nan_empty
    try:
        with Record() as rec:
            out = ops.conv2d_fwd(t["x"], t["w"], N, H, W, Cin, Cout, 1, 1, stride, 0, t["sc"] if prol else None,
                                 t["sh"] if prol else None, stats=bool(stats), shift=t["shift"] if stats == "shift" else None,
                                 wimg=kw.pop("wimg", t["img"]), **kw)
    finally:
        ops.conv._empty = real_empty
    torch.cuda.synchronize()
    return out[0].reshape(-1, Cout), out[1], rec.launches


def call_generic(dev, shape, t, call, stats, stream):
    """koaf_gemm on the descriptor koaf_conv2d_fwd builds, on 128 x 128 tiles -> (y, part [M / 128, 2, Cout] or None, records)"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout = shape
    M = N * H * W
    y = torch.full((M, Cout), float("nan"), device=dev)
    part = torch.full((M // 128, 2, Cout), float("nan"), device=dev) if stats else None
    f, d, amax = t["img"]
    g = _lib.KoafGemm()
    g.alpha, g.nb0, g.nb1, g.splitk, g.fmt = 1.0, 1, 1, 1, 1
    g.A.ptr, g.A.kind, g.A.gather, g.A.ld, g.A.fscale = t["x"].data_ptr(), 0, 0, Cin, ops.ACT_SCALE
    if call == "prologue":
        g.A.tf, g.A.sc, g.A.sh = 1, t["sc"].data_ptr(), t["sh"].data_ptr()
    g.B.ptr, g.B.kind, g.B.gather, g.B.ld = t["w"].data_ptr(), 2, 0, Cin
    g.B.planes, g.B.plane_stride, g.B.amax = f.data_ptr(), Cout * Cin, amax.data_ptr()
    g.M, g.N, g.K, g.bm, g.bn = M, Cout, Cin, 128, 128
    g.C, g.ldc = y.data_ptr(), Cout
    if stats:
        g.stats = part.data_ptr()
        if stats == "shift":
            g.stats_shift = t["shift"].data_ptr()
    was = ops.set_stream(stream)
    try:
        with Record() as rec:
            ops.gemm(g)
    finally:
        ops.set_stream(was)
    torch.cuda.synchronize()
    return y, part, rec.launches


def hold_float64(case, t, y, part):
    """the float64 bars of sampled 64-column blocks over all rows; the A operand is formed ONCE on the CPU"""
    N, H, W, Cin, Cout = case.shape
    M = N * H * W
    x = t["x"].reshape(-1, Cin).cpu()
    if case.call == "prologue":
        sc, sh = t["sc"].cpu(), t["sh"].cpu()
        a32, a64 = torch.relu(x * sc + sh), torch.relu(x.double() * sc.double() + sh.double())
    else:
        a32, a64 = x, x.double()
    a_abs = a32.abs().double()
    nb = Cout // 64
    # both halves of a column tile, the first and the last tile; at K >= 1024 the first and the last block (34 GFLOP in float64)
    blocks = sorted({0, nb - 1} if Cin >= 1024 else {0, nb - 1, nb // 2, (nb // 2 + 1) % nb})
    for bj in blocks:
        cs = slice(64 * bj, 64 * bj + 64)
        w32 = t["w"].reshape(Cout, -1)[cs].cpu()
        y64, y32, den = a64 @ w32.double().t(), a32 @ w32.t(), a_abs @ w32.abs().double().t() + 1e-300
        got = y[:, cs]
        be = band_errors(got, y64)
        cw, bar = componentwise(got, y64, y32, den)
        line = f"[fwd1] {case.name:32s} columns {64 * bj:4d}.. worst band {be.max().item():.2e} (bar {FWD:.0e}) componentwise {cw:.2e} (bar {bar:.2e})"
        assert be.numel() == M // 128
        if part is not None:
            kk = t["shift"][cs].cpu().double() if case.stats == "shift" else torch.zeros(64, dtype=torch.float64)
            d = y64 - kk
            e1 = rel_err(part[:, 0, cs].double().sum(0), d.sum(0))
            e2 = rel_err(part[:, 1, cs].double().sum(0), (d * d).sum(0))
            line += f" | sums {e1:.2e} (bar 1e-4) squares {e2:.2e} (bar 1e-5)"
        print(line)
        assert be.max().item() < FWD, (case.name, bj, int(be.argmax()), be.max().item())
        assert cw <= bar, (case.name, bj, cw, bar)
        if part is not None:
            assert e1 < 1e-4 and e2 < 1e-5, (case.name, bj, e1, e2)


def run_case(dev, case):
    N, H, W, Cin, Cout = case.shape
    M = N * H * W
    assert M % 256 == 0 and 65536 <= M <= 70000
    try:
        t = inputs(case.shape, dev)
        y, part, launches = call_model(dev, case.shape, t, case.call, case.stats)
        gemms = [r for r in launches if r["variant"].startswith("koaf_")]
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        tiles = (M // 256) * (Cout // case.bn)
        want = dict(variant=F1, bm=256, bn=case.bn, tiles=tiles, grid_x=min(tiles, 256) if case.walk else tiles, splitk=1, nbatch=1, M=M,
                    N=Cout, K=Cin, fmt=1, a_tf=1 if case.call == "prologue" else 0, b_tf=0, act16=0, emit=0)
        assert {f: r[f] for f in want} == want, (case.name, r, want)
        assert bool(torch.isfinite(y).all()), (case.name, "a tile of y was not written")
        assert (part is None) == (not case.stats), case.name
        if part is not None:
            assert part.shape[0] == M // 128, (case.name, part.shape)
            assert bool(torch.isfinite(part).all()), (case.name, "a partial row was not written")
        y2, part2, _ = call_model(dev, case.shape, t, case.call, case.stats)
        assert torch.equal(y2, y) and (part is None or torch.equal(part2, part)), (case.name, "the same call twice")
        for stream, variant in ((True, STREAM), (False, GEN)):
            ref, rpart, lg = call_generic(dev, case.shape, t, case.call, case.stats, stream)
            assert len(lg) == 1 and (lg[0]["variant"], lg[0]["bm"], lg[0]["bn"]) == (variant, 128, 128), (case.name, lg)
            ndiff = int((ref != y).sum())
            pdiff = int((rpart != part).sum()) if part is not None else 0
            print(f"\n[fwd1] {case.name:32s} {r['variant']} {r['bm']}x{r['bn']} tiles {r['tiles']} grid.x {r['grid_x']} | elements that differ "
                  f"from {variant}: y {ndiff} part {pdiff}")
            assert torch.equal(ref, y), (case.name, variant, ndiff, "bit-identical to koaf_gemm_kernel on 128 x 128 tiles")
            if part is not None:
                assert torch.equal(rpart, part), (case.name, variant, pdiff, "the statistics rows of the 128-row tiling")
            del ref, rpart
        hold_float64(case, t, y, part)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_256_row_kernel_equals_the_streamed_kernel(dev, case):
    run_case(dev, case)


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernels(dev, case):
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout = case.shape
    was = ops.set_stream(case.how != "nostream")
    try:
        t = dict(inputs(case.shape, dev))
        kw = {}
        call = "prologue" if case.how in ("prologue", "tail") else "plain"
        if case.how == "noimg":
            kw["wimg"] = None
        if case.how == "bf16":
            t["x"] = t["x"].bfloat16()
        if case.how == "tail":
            kw["tail_idt"] = torch.randn(N, H, W, Cin, device=dev)
        if case.how == "emit":
            kw["emit"] = (t["sc"].new_ones(Cout), t["sc"].new_zeros(Cout))
        y, part, launches = call_model(dev, case.shape, t, call, True, stride=case.stride, **kw)
        gemms = [r for r in launches if r["variant"].startswith("koaf_")]
        assert gemms and all(r["variant"] != F1 for r in launches), (case.name, launches)
        last = gemms[-1]
        if case.stride == 2:
            assert (last["variant"], last["bm"]) == (FS2, 256), (case.name, launches)
        else:
            assert last["variant"] in (GEN, STREAM) and last["bm"] == 128, (case.name, launches)
            assert case.how != "nostream" or last["variant"] == GEN, (case.name, launches)
        assert last["fmt"] == (0 if case.how == "noimg" else 1) and last["act16"] == (1 if case.how == "bf16" else 0), (case.name, gemms)
        assert bool(last["emit"]) == (case.how == "emit") and last["a_tf"] == {"tail": 3, "prologue": 1}.get(case.how, 0), (case.name, last)
        assert bool(torch.isfinite(y.float()).all()), case.name
    finally:
        ops.set_stream(was)
        torch.cuda.empty_cache()
