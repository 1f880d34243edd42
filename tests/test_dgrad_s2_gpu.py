"""The stride-2 data gradients on the 256-row kernel (koaf_dgrad_s2.hip) against the generic path they leave.

koaf_conv2d_dgrad_bnb splits a stride-2 data gradient into the four parity classes (y % 2, x % 2) of the input pixels, each a stride-1
transposed gather over its own taps, and hands every class to koaf_dgrad_s2 when the call runs the fp16 scheme with the weights' D plane
image on fp32 tensors, without residual, with no fused reduction or BatchNorm-backward mode 2 with one BatchNorm, 3x3 / pad 1 from dy's
plane images or 1x1 / pad 0 from the fp32 dy (tf 0 | 2), Cout % 32 == 0, Cin % 128 == 0, H and W even and N (H/2) (W/2) a whole number
of 256-row tiles (koaf_dgrad_s2.hip koaf_dgrad_s2_ok).  Every row of CASES is the smallest shape of its kind; it goes through ops.conv2d_dgrad as
the model calls it, with the outputs pre-filled with NaN, and ASSERTS FROM THE LAUNCH RECORD the variant, the tile and the four records
(one per class, class order, K = 0 for a class without a tap).

Held per case:
  * dx / dz, the returned partial rows and max |dz| are torch.equal to the generic path on the same inputs: ops.gemm on the per-class
    descriptors koaf_conv2d_dgrad_bnb builds, on 128 x 128 tiles (the tile the production sizes run on), which bypasses the new rule; the
    partial rows laid out class after class.  The new kernel writes two partial rows per 256-row tile where the 128-row tiling puts them.
  * against float64 on the CPU at the bars test_tiles_gpu.run_dgrad holds: relative L2 < BWD per 128-row band of every class and over
    the whole tensor, the componentwise bar (8 x torch's fp32 product of the same operands), the reduction partials at 1e-4 and max |dz|
    at 1e-6 (BWD and the bar's functions are imported; the last two are run_dgrad's literals).
  * the rows of the classes without a tap (1x1) are exactly 0.0.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: an odd image, classes of 320 rows, a residual, reduction mode 1, bf16 activation storage,
no plane images (the bf16 scheme), Cin = 64, a 3x3 call without dy's plane images, stride 1.

Borders: class row (n, yy, xx) of class (py, px) reads dy[n][yy + offy - kh][xx + offx - kw] with offy = py, kh < 1 + py (3x3 / pad 1).
With even H the LOW border is never out of range, for any shape the kernel accepts (yy + py - kh >= 0); the HIGH border is: the last
class row and column of the classes py = 1 / px = 1 read source row OH = H / 2 at kh = 0 (16 x 16: row / column 8 of an 8 x 8 dy)."""
from collections import namedtuple

import pytest
import torch

import tile256_refs as R
from test_tiles_gpu import BWD, Record, _class_rows, _dgrad64, band_errors, componentwise, rel_err
from tile256_refs import GEN, classes, out_hw

pytestmark = pytest.mark.gpu

DS2 = "koaf_dgrad_s2"
Case = namedtuple("Case", "name shape call bn")
# shape (N, H, W, Cin, Cout, k, pad), stride 2
# call: bnb2_amax / bnb2 (BnApply through plane images, fused reduction mode 2, with / without max |dz|) | planes_plain (dy + amax through
#       plane images) | apply (BnApply on load, tf 2) | plain (dy + amax, tf 0)
CASES = [
    Case("k3-128to128-bnb2-amax", (8, 16, 16, 128, 128, 3, 1), "bnb2_amax", 128),
    Case("k3-256to256-3x4-bnb2", (128, 6, 8, 256, 256, 3, 1), "bnb2", 256),
    Case("k3-256from32-plain", (8, 16, 16, 256, 32, 3, 1), "planes_plain", 256),
    Case("k3-512to512-bnb2", (4, 16, 32, 512, 512, 3, 1), "bnb2", 256),
    Case("k1-256from512-apply", (8, 16, 16, 256, 512, 1, 0), "apply", 256),
    Case("k1-1024from2048-apply", (4, 16, 16, 1024, 2048, 1, 0), "apply", 256),
    Case("k1-128from32-plain", (8, 16, 16, 128, 32, 1, 0), "plain", 128),
    Case("k1-128from64-apply", (8, 16, 16, 128, 64, 1, 0), "apply", 128),      # (the apply on the 128-wide tile: two k-tiles)
]
Refusal = namedtuple("Refusal", "name shape stride how")
REFUSALS = [
    Refusal("odd-image", (4, 23, 31, 128, 128, 3, 1), 2, "plain"),
    Refusal("rows-320", (5, 16, 16, 128, 128, 3, 1), 2, "plain"),
    Refusal("residual", (8, 16, 16, 128, 128, 3, 1), 2, "residual"),
    Refusal("bnb-mode-1", (8, 16, 16, 128, 128, 3, 1), 2, "bnb1"),
    Refusal("bf16storage", (8, 16, 16, 128, 128, 3, 1), 2, "bf16"),
    Refusal("no-images", (8, 16, 16, 128, 128, 3, 1), 2, "noimg"),
    Refusal("Cin-64", (8, 16, 16, 64, 128, 3, 1), 2, "plain"),
    Refusal("no-dy-planes", (8, 16, 16, 128, 128, 3, 1), 2, "noplanes"),
    Refusal("stride-1", (4, 16, 16, 128, 128, 3, 1), 1, "noplanes"),
]


def inputs(shape, dev, stride=2, bf16=False):
    """device operands of a shape: the packed weight with its plane images, a plain dy with its amax, a BnApply of the same size, the
    producer's conv output cx with its BatchNorm record sv (mode 2 masks by the sign of sc * cx + sh: kept out of rounding's reach)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape, stride)
    g_ = torch.Generator(device=dev).manual_seed(9900 + sum(shape))

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    t = dict(w=rnd(Cout, k, k, Cin) * (k * k * Cin) ** -0.5, dy=rnd(N, OH, OW, Cout) * 1e-3)
    t["am"] = t["dy"].abs().max().reshape(1).float()
    t["img"] = ops.build_weight_planes(t["w"], Cout, k * k, Cin)
    t["apply"] = R.bn_apply(dev, N * OH * OW, Cout, c=rnd(N, OH, OW, Cout) * 1.5 + 0.3, gam=rnd(Cout) * 0.2 + 1, bet=rnd(Cout) * 0.1,
                            dz=rnd(N, OH, OW, Cout) * 1e-3, store16=bf16)
    sv = torch.stack([rnd(Cin) * 0.3, torch.rand(Cin, generator=g_, device=dev) + 0.5, (rnd(Cin) * 0.5 + 1).abs().clamp(min=0.25), rnd(Cin) * 0.2])
    cx = rnd(N, H, W, Cin) * 1.5 + 0.3
    cx = torch.where((cx * sv[2] + sv[3]).abs() < 1e-3, cx + 0.1, cx)
    if bf16:
        cx = cx.bfloat16().float()
    assert float((cx.double() * sv[2].double() + sv[3].double()).abs().min()) > 1e-5
    t["cx"], t["sv"], t["y"], t["res"] = (cx.bfloat16() if bf16 else cx), sv, rnd(N, H, W, Cin), rnd(N, H, W, Cin) * 1e-3
    torch.cuda.synchronize()
    return t


def call_model(shape, t, call, stride=2, **kw):
    """ops.conv2d_dgrad as the model calls it, every output pre-filled with NaN -> (the outputs as a tuple, the launch records)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = shape
    use_apply = call in ("bnb2_amax", "bnb2", "apply")
    kw.setdefault("wimg", t["img"])
    if not use_apply:
        kw.setdefault("dy_amax", t["am"])
    if call.startswith("bnb2"):
        kw["bnb"] = dict(mode=2, c=t["cx"], saved=t["sv"], dz_amax=call == "bnb2_amax")
    with R.nan_outputs(), Record() as rec:
        out = ops.conv2d_dgrad(t["apply"] if use_apply else t["dy"], t["w"], N, H, W, Cin, Cout, k, k, stride, pad, **kw)
    torch.cuda.synchronize()
    return (out if isinstance(out, tuple) else (out,)), rec.launches


def call_generic(dev, shape, t, call):
    """the generic path: koaf_gemm on the four class descriptors koaf_conv2d_dgrad_bnb builds, 128 x 128 tiles pinned, the partial rows
    class after class -> ((dx, part, amax) as far as the call has them, the launch records)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape)
    use_apply, bnb = call in ("bnb2_amax", "bnb2", "apply"), call.startswith("bnb2")
    planes = None
    if k == 3:
        planes = ops.conv._dy_planes(t["apply"] if use_apply else t["dy"], None if use_apply else t["am"], N * OH * OW, Cout)
    dx = torch.full((N, H, W, Cin), float("nan"), device=dev)
    nrows = sum(N * c[2] * c[3] // 128 for c in classes(shape))
    part = torch.full((nrows, 2, Cin), float("nan"), device=dev) if bnb else None
    amax = torch.zeros(1, device=dev) if call == "bnb2_amax" else None
    with Record() as rec:
        for g in R.dgrad_class_descriptors(shape, t, call, dx, part, amax, planes):
            ops.gemm(g)
    torch.cuda.synchronize()
    return (dx,) + ((part,) if bnb else ()) + ((amax,) if amax is not None else ()), rec.launches


def hold_float64(case, t, out):
    """run_dgrad's float64 bars: bands of every class, the whole tensor, componentwise; the reduction partials and max |dz|"""
    N, H, W, Cin, Cout, k, pad = case.shape
    shape8 = (N, H, W, Cin, Cout, k, 2, pad)
    w = t["w"].cpu()
    if case.call in ("bnb2_amax", "bnb2", "apply"):
        ap = t["apply"]
        coef, dz, cc = ap.coef.double().cpu(), ap.dz.double().cpu(), ap.c.double().cpu()
        dy64 = coef[0] * dz + coef[3] - coef[2] * cc
        c32 = ap.coef.cpu()
        dy32 = c32[0] * ap.dz.cpu() + c32[3] - c32[2] * ap.c.float().cpu()
    else:
        dy64, dy32 = t["dy"].double().cpu(), t["dy"].cpu()
    g64, g32 = _dgrad64(dy64, w.double(), shape8), _dgrad64(dy32, w, shape8)
    den = _dgrad64(dy32.abs(), w.abs(), shape8).double()
    errs = []
    if case.call.startswith("bnb2"):
        cx, sv = t["cx"].double().cpu(), t["sv"].double().cpu()
        mask = (cx * sv[2] + sv[3]) > 0
        g64, g32 = g64 * mask, g32 * mask
        sums = [g64.sum((0, 1, 2)), (g64 * ((cx - sv[0]) * sv[1])).sum((0, 1, 2))]
        assert out[1].shape[1] == 2, case.name
        errs = [rel_err(out[1][:, i].double().sum(0), ref) for i, ref in enumerate(sums)]
    dx = out[0].cpu()
    bes = [band_errors(a, b) for a, b in zip(_class_rows(dx, shape8), _class_rows(g64, shape8)) if float(b.abs().max()) > 0]
    assert len(bes) == (4 if k == 3 else 1), case.name
    worst = max(be.max().item() for be in bes)
    whole = rel_err(dx, g64)
    cw, bar = componentwise(dx, g64, g32, den + 1e-300)
    print(f"[dgrad_s2] {case.name:24s} worst band {worst:.2e} whole {whole:.2e} (bar {BWD:.0e}) componentwise {cw:.2e} (bar {bar:.2e})"
          + (" partials " + " ".join(f"{e:.1e}" for e in errs) + " (bar 1e-4)" if errs else ""))
    assert worst < BWD and whole < BWD, (case.name, worst, whole)
    assert cw <= bar, (case.name, cw, bar)
    assert all(e < 1e-4 for e in errs), (case.name, errs)
    if case.call == "bnb2_amax":
        assert abs(float(out[2]) / float(out[0].abs().max()) - 1) < 1e-6, case.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_256_row_kernel_equals_the_generic_path(dev, case):
    N, H, W, Cin, Cout, k, pad = case.shape
    cls = classes(case.shape)
    assert H % 2 == 0 and W % 2 == 0 and all(N * c[2] * c[3] % 256 == 0 for c in cls)
    try:
        t = inputs(case.shape, dev)
        out, launches = call_model(case.shape, t, case.call)
        gemms = R.records(launches)
        assert len(gemms) == 4, (case.name, launches)
        a_tf = 2 if case.call == "apply" else 0
        for r, c in zip(gemms, cls):
            M, K = N * c[2] * c[3], c[6] * c[7] * Cout
            tiles = (M // 256) * (Cin // case.bn)
            R.hold_record(case.name, r, dict(variant=DS2, bm=256, bn=case.bn, tiles=tiles, grid_x=tiles, splitk=1, nbatch=1, M=M, N=Cin, K=K, fmt=1,
                                             a_tf=a_tf, b_tf=0, act16=0, emit=0))
        assert [r["K"] > 0 for r in gemms] == ([True] * 4 if k == 3 else [True, False, False, False]), (case.name, gemms)
        for o in out:
            assert bool(torch.isfinite(o).all()), (case.name, "an output element was not written")
        nrows = sum(N * c[2] * c[3] // 128 for c in cls)
        assert len(out) == {"bnb2_amax": 3, "bnb2": 2}.get(case.call, 1) and (len(out) == 1 or out[1].shape[0] == nrows), case.name
        if k == 1:
            dx = out[0]
            assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0, (case.name, "odd pixels are exactly 0.0")
        out2, _ = call_model(case.shape, t, case.call)
        assert all(torch.equal(a, b) for a, b in zip(out, out2)), (case.name, "the same call twice")
        ref, lg = call_generic(dev, case.shape, t, case.call)
        assert len(lg) == 4 and all((r["variant"].startswith(GEN), r["bm"], r["bn"]) == (True, 128, 128) for r in lg if r["K"] > 0), (case.name, lg)
        diffs = [int((a != b).sum()) for a, b in zip(out, ref)]
        print(f"\n[dgrad_s2] {case.name:24s} {gemms[0]['variant']} {gemms[0]['bm']}x{gemms[0]['bn']} tiles "
              f"{[r['tiles'] for r in gemms]} | elements that differ from the generic path (dx, part, amax): {diffs}")
        assert len(ref) == len(out) and all(torch.equal(a, b) for a, b in zip(out, ref)), (case.name, diffs,
                                                                                             "bit-identical to koaf_gemm_kernel on 128 x 128 tiles")
        hold_float64(case, t, out)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernel(dev, case):
    try:
        t = inputs(case.shape, dev, case.stride, bf16=case.how == "bf16")
        kw, call = {}, "planes_plain"
        if case.how == "residual":
            kw["residual"] = t["res"]
        if case.how == "bnb1":
            kw["bnb"] = dict(mode=1, c=t["cx"], y=t["y"], saved=t["sv"])
        if case.how == "bf16":
            call = "bnb2"          # (the BnApply's c and the reduction's c are stored as bf16)
        if case.how == "noimg":
            kw["wimg"] = None
        if case.how == "noplanes":
            kw["aplanes"] = False
        out, launches = call_model(case.shape, t, call, stride=case.stride, **kw)
        R.hold_refusal(case.name, launches, DS2, out, 0 if case.how == "noimg" else 1, 2 if case.how == "bf16" else 0, every=True)
    finally:
        torch.cuda.empty_cache()
