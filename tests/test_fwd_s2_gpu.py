"""The stride-2 forward convolutions on the 256-row gathered kernel (koaf_fwd_s2.hip) against the generic path they leave.

koaf_conv2d_fwd hands a stride-2 forward convolution -- the 1x1 / pad 0 shortcuts and the 3x3 / pad 1 conv2 of a downsampling block -- to
koaf_fwd_s2 when the call runs the fp16 scheme on fp32 tensors with the weights' F plane image, Cin % 32 == 0, Cout % 128 == 0 and
M = N OH OW is a whole number of 256-row tiles (koaf_conv.hip fwd_s2_ok).  Row m = output pixel (n, oy, ox), k = (tap, ci), element
x[n][2 oy - pad + kh][2 ox - pad + kw][ci] behind its transform, 0 outside the image.  Every row of CASES is the smallest shape of its
kind; it goes through ops.conv2d_fwd as the model calls it, with y and the statistics buffer pre-filled with NaN, and ASSERTS FROM THE
LAUNCH RECORD the variant, tile and tile count.

Held per case:
  * y, the returned row count and part[:rows] are torch.equal to the generic path on the same inputs: ops.gemm with the descriptor
    koaf_conv2d_fwd builds for koaf_gemm_kernel on 128 x 128 tiles (the tile the production sizes of these calls run on), which bypasses
    the new rule.  The new kernel writes two partial rows per 256-row tile where the 128-row tiling puts them, so nothing may move.
  * against float64 on the CPU for sampled 64-column blocks of y over ALL rows: relative L2 < FWD per 128-row band and the componentwise
    bar of test_tiles_gpu (8 x torch's fp32 product of the same operands); FWD and the bar's function are imported, not restated.  The
    CPU reference gathers the RAW x, applies the prologue and THEN zeroes the padding.  The statistics of the sampled columns are held
    against the float64 column sums of (y - shift) and (y - shift)^2 at run_forward's bars for the same sums (1e-4 / 1e-5 relative L2
    over the columns); the shift is a generic vector, not the mean, so the first sum is not a cancellation.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: M no multiple of 256, the bf16 scheme (no plane images), bf16 activation storage,
caller-supplied x_planes, an emission request (the library serves none for a gathered call: it must not reach the new kernel either), Cout = 64
and stride 1.

(23 x 31 -> 12 x 16 at 3x3 / pad 1: odd H and W reach all four border taps and the 256-row tiles cross image boundaries; 9 x 10 -> 5 x 5:
a tile spans ten images and each of a thread's four rows, 64 apart, wraps rows and images; Cin = 32: the tap changes every k-step, nine
steps; 1x1 at Cin = 32 is ONE k-tile: the pipeline's prologue meets its drain.)"""
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

from test_tiles_gpu import FWD, Record, band_errors, componentwise, rel_err

pytestmark = pytest.mark.gpu

FS2, GEN = "koaf_fwd_s2", "koaf_gemm"
Case = namedtuple("Case", "name shape call stats bn")
# shape (N, H, W, Cin, Cout, k, pad), stride 2; call: plain | prologue (tf 1); stats: False | True | "shift"
CASES = [
    Case("k3-128to128-prologue-shift", (4, 23, 31, 128, 128, 3, 1), "prologue", "shift", 128),
    Case("k3-256to256-5x5-prologue", (256, 9, 10, 256, 256, 3, 1), "prologue", True, 256),
    Case("k3-32to128-prologue", (4, 23, 31, 32, 128, 3, 1), "prologue", True, 128),
    Case("k1-256to512-plain", (4, 23, 31, 256, 512, 1, 0), "plain", True, 256),
    Case("k1-1024to2048-plain", (2, 31, 31, 1024, 2048, 1, 0), "plain", True, 256),
    Case("k1-32to128-one-ktile", (4, 23, 31, 32, 128, 1, 0), "plain", True, 128),
    Case("k3-128to128-prologue-nostats", (4, 23, 31, 128, 128, 3, 1), "prologue", False, 128),
]
Refusal = namedtuple("Refusal", "name shape stride how")
REFUSALS = [
    Refusal("M-960", (5, 23, 31, 128, 128, 3, 1), 2, "plain"),
    Refusal("bf16scheme", (4, 23, 31, 128, 128, 3, 1), 2, "noimg"),
    Refusal("bf16storage", (4, 23, 31, 128, 128, 3, 1), 2, "bf16"),
    Refusal("x_planes", (4, 23, 31, 128, 128, 3, 1), 2, "xplanes"),
    Refusal("emit", (4, 23, 31, 128, 128, 3, 1), 2, "emit"),
    Refusal("Cout-64", (4, 23, 31, 128, 64, 3, 1), 2, "plain"),
    Refusal("stride-1", (4, 16, 16, 128, 128, 3, 1), 1, "plain"),
]


def out_hw(shape, stride=2):
    N, H, W, Cin, Cout, k, pad = shape
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


@lru_cache(maxsize=1)
def inputs(shape, dev):
    """device operands of a shape: x [N, H, W, Cin], its prologue (sc, sh), the packed weight with its plane images, a statistics shift"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = shape
    g_ = torch.Generator(device=dev).manual_seed(9800 + sum(shape))

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    t = dict(x=rnd(N, H, W, Cin) * 1.5 + 0.3, sc=rnd(Cin) * 0.2 + 1.0, sh=rnd(Cin) * 0.1, w=rnd(Cout, k, k, Cin) * (k * k * Cin) ** -0.5,
             shift=rnd(Cout) * 0.3 + 0.2)
    t["img"] = ops.build_weight_planes(t["w"], Cout, k * k, Cin)
    torch.cuda.synchronize()
    return t


def call_model(dev, shape, t, call, stats, stride=2, **kw):
    """ops.conv2d_fwd as the model calls it, y and part pre-filled with NaN -> (y [M, Cout], part[:rows] or None, the launch records)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = shape
    prol = call == "prologue"
    real_empty = ops.conv._empty

    def nan_empty(*a, **k_):
        out = real_empty(*a, **k_)
        return out.fill_(float("nan")) if out.is_floating_point() else out
    ops.conv._empty = nan_empty
    try:
        with Record() as rec:
            y, part = ops.conv2d_fwd(t["x"], t["w"], N, H, W, Cin, Cout, k, k, stride, pad, t["sc"] if prol else None,
                                     t["sh"] if prol else None, stats=bool(stats), shift=t["shift"] if stats == "shift" else None,
                                     wimg=kw.pop("wimg", t["img"]), **kw)
    finally:
        ops.conv._empty = real_empty
    torch.cuda.synchronize()
    return y.reshape(-1, Cout), part, rec.launches


def call_generic(dev, shape, t, call, stats):
    """the generic path: koaf_gemm on the descriptor koaf_conv2d_fwd builds, on 128 x 128 tiles -> (y, part [M / 128, 2, Cout] or None, records)"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape)
    M, K = N * OH * OW, k * k * Cin
    y = torch.full((M, Cout), float("nan"), device=dev)
    part = torch.full((M // 128, 2, Cout), float("nan"), device=dev) if stats else None
    f, d, amax = t["img"]
    g = _lib.KoafGemm()
    g.alpha, g.nb0, g.nb1, g.splitk, g.fmt = 1.0, 1, 1, 1, 1
    g.A.ptr, g.A.kind, g.A.gather, g.A.fscale = t["x"].data_ptr(), 0, 1, ops.ACT_SCALE
    g.A.H, g.A.W, g.A.C, g.A.CS, g.A.PH, g.A.PW = H, W, Cin, Cin, OH, OW
    g.A.KH, g.A.KW, g.A.stride, g.A.pad, g.A.pad_w = k, k, 2, pad, pad
    if call == "prologue":
        g.A.tf, g.A.sc, g.A.sh = 1, t["sc"].data_ptr(), t["sh"].data_ptr()
    g.B.ptr, g.B.kind, g.B.gather, g.B.ld = t["w"].data_ptr(), 2, 0, K
    g.B.planes, g.B.plane_stride, g.B.amax = f.data_ptr(), Cout * K, amax.data_ptr()
    g.M, g.N, g.K, g.bm, g.bn = M, Cout, K, 128, 128
    g.C, g.ldc = y.data_ptr(), Cout
    if stats:
        g.stats = part.data_ptr()
        if stats == "shift":
            g.stats_shift = t["shift"].data_ptr()
    with Record() as rec:
        ops.gemm(g)
    torch.cuda.synchronize()
    return y, part, rec.launches


def gather_map(shape, tap, dev):
    """source pixel index (clamped into the tensor) and validity of every output pixel for a filter tap"""
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape)
    kh, kw = tap // k, tap % k
    p = torch.arange(N * OH * OW, device=dev)
    n, oy, ox = p // (OH * OW), (p // OW) % OH, p % OW
    sy, sx = 2 * oy - pad + kh, 2 * ox - pad + kw
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return ((n * H + sy.clamp(0, H - 1)) * W + sx.clamp(0, W - 1)), ok


def hold_float64(case, t, y, part):
    """the float64 bars of sampled 64-column blocks over all rows; the A operand is formed ONCE on the CPU from the gathered raw x, the
    padding zeroed AFTER the prologue"""
    N, H, W, Cin, Cout, k, pad = case.shape
    OH, OW = out_hw(case.shape)
    M = N * OH * OW
    xs = t["x"].reshape(-1, Cin)
    a32s, a64s, padded = [], [], 0
    for tap in range(k * k):
        idx, ok = gather_map(case.shape, tap, xs.device)
        x = xs[idx].cpu()
        ok = ok.cpu()[:, None]
        padded += int((~ok).sum())
        if case.call == "prologue":
            sc, sh = t["sc"].cpu(), t["sh"].cpu()
            a32, a64 = torch.relu(x * sc + sh), torch.relu(x.double() * sc.double() + sh.double())
        else:
            a32, a64 = x, x.double()
        a32s.append(a32 * ok)
        a64s.append(a64 * ok)
    assert (padded > 0) == (pad > 0), (case.name, padded)
    a32, a64 = torch.cat(a32s, 1), torch.cat(a64s, 1)
    nb = Cout // 64
    blocks = sorted({0, nb - 1, nb // 2, (nb // 2 + 1) % nb})        # both halves of a column tile, the first and the last tile
    for bj in blocks:
        cs = slice(64 * bj, 64 * bj + 64)
        w32 = t["w"].reshape(Cout, -1)[cs].cpu()
        y64, y32, den = a64 @ w32.double().t(), a32 @ w32.t(), a32.abs().double() @ w32.abs().double().t() + 1e-300
        got = y[:, cs]
        be = band_errors(got, y64)
        cw, bar = componentwise(got, y64, y32, den)
        line = f"[fwd_s2] {case.name:30s} columns {64 * bj:4d}.. worst band {be.max().item():.2e} (bar {FWD:.0e}) componentwise {cw:.2e} (bar {bar:.2e})"
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


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gathered_256_row_kernel_equals_the_generic_path(dev, case):
    N, H, W, Cin, Cout, k, pad = case.shape
    OH, OW = out_hw(case.shape)
    M, K = N * OH * OW, k * k * Cin
    assert M % 256 == 0
    try:
        t = inputs(case.shape, dev)
        y, part, launches = call_model(dev, case.shape, t, case.call, case.stats)
        gemms = [r for r in launches if r["variant"] in (FS2, GEN)]
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        tiles = (M // 256) * (Cout // case.bn)
        want = dict(variant=FS2, bm=256, bn=case.bn, tiles=tiles, grid_x=tiles, splitk=1, nbatch=1, M=M, N=Cout, K=K, fmt=1,
                    a_tf=1 if case.call == "prologue" else 0, b_tf=0, act16=0, emit=0)
        assert {f: r[f] for f in want} == want, (case.name, r, want)
        assert bool(torch.isfinite(y).all()), (case.name, "a tile of y was not written")
        assert (part is None) == (not case.stats), case.name
        if part is not None:
            assert part.shape[0] == M // 128, (case.name, part.shape)
            assert bool(torch.isfinite(part).all()), (case.name, "a partial row was not written")
        y2, part2, _ = call_model(dev, case.shape, t, case.call, case.stats)
        assert torch.equal(y2, y) and (part is None or torch.equal(part2, part)), (case.name, "the same call twice")
        ref, rpart, lg = call_generic(dev, case.shape, t, case.call, case.stats)
        assert len(lg) == 1 and (lg[0]["variant"], lg[0]["bm"], lg[0]["bn"]) == (GEN, 128, 128), (case.name, lg)
        ndiff = int((ref != y).sum())
        pdiff = int((rpart != part).sum()) if part is not None else 0
        print(f"\n[fwd_s2] {case.name:30s} {r['variant']} {r['bm']}x{r['bn']} tiles {r['tiles']} | elements that differ from the generic path: "
              f"y {ndiff} part {pdiff}")
        assert torch.equal(ref, y), (case.name, ndiff, "bit-identical to koaf_gemm_kernel on 128 x 128 tiles")
        if part is not None:
            assert torch.equal(rpart, part), (case.name, pdiff, "the statistics rows of the 128-row tiling")
        hold_float64(case, t, y, part)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernel(dev, case):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    N, H, W, Cin, Cout, k, pad = case.shape
    try:
        t = dict(inputs(case.shape, dev))
        kw = {}
        if case.how == "noimg":
            kw["wimg"] = None
        if case.how == "bf16":
            t["x"] = t["x"].bfloat16()
        if case.how == "xplanes":
            kw["aplanes"] = ops.act_planes(t["x"], N * H * W, Cin, 0, None, None, fscale=ops.ACT_SCALE)
        if case.how == "emit":
            kw["emit"] = (t["sc"].new_ones(Cout), t["sc"].new_zeros(Cout))
        if case.stride == 1:
            kw["aplanes"] = False
        try:
            y, part, launches = call_model(dev, case.shape, t, "plain", case.how != "emit", stride=case.stride, **kw)
        except KoafError:
            # (an emission request on a gathered call: the generic path serves none and says so -- the new kernel must not have taken it)
            assert case.how == "emit", case.name
            ops.launch_log(False)
            return
        gemms = [r for r in launches if r["variant"] in (FS2, GEN) or r["variant"].startswith("koaf_")]
        assert gemms and all(r["variant"] != FS2 for r in launches), (case.name, launches)
        assert gemms[-1]["variant"] == GEN, (case.name, launches)
        assert gemms[-1]["fmt"] == (0 if case.how == "noimg" else 1) and gemms[-1]["act16"] == (1 if case.how == "bf16" else 0), (case.name, gemms)
        assert bool(torch.isfinite(y.float()).all()), case.name
    finally:
        torch.cuda.empty_cache()
