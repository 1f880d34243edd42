"""The stride-2 weight gradients on the 256-wide-tile kernel (koaf_wgrad1.hip, gathered B) against the generic path they leave.

koaf_conv2d_wgrad hands a stride-2 weight gradient -- the 1x1 / pad 0 shortcuts and the 3x3 / pad 1 conv2 of a downsampling block -- to
koaf_wgrad1 when the call runs the fp16 scheme on fp32 tensors without plane images, Cout and KH KW Cin are whole multiples of the tile
(256, or 128 on ONE side), Cin is a whole number of column tiles (a block works on one filter tap) and the split-K plan (wgrad_plan,
unchanged) leaves k-ranges of at least 1024 pixels (koaf_conv.hip wgrad1_tile).  B is then x gathered on the k index: k-row p = output
pixel (n, oy, ox), column (tap, ci), element x[n][2 oy - pad + kh][2 ox - pad + kw][ci] behind its transform, 0 outside the image.
Every row of CASES is the smallest shape of its kind that the rule engages, with P no multiple of 32; it goes through ops.conv2d_wgrad as
the model calls it and ASSERTS FROM THE LAUNCH RECORD the variant, tile, tile count and split count.  dw and the slab workspace are
pre-filled with NaN.

Held per case:
  * dw is torch.equal to the generic path on the same inputs: ops.gemm with the descriptor koaf_conv2d_wgrad builds for
    koaf_gemm_kernel (128 x 128 tiles, the same splitk, the same gather on B, slabs) followed by koaf_slab_reduce.  The zero
    contributions of border taps and of the rows behind a k-range enter the accumulators where the generic kernel's do, so nothing
    may move.
  * against float64 on the CPU for sampled 64 x 64 blocks of dw -- the eight of test_wgrad1x1_gpu.py, and for the 3x3 cases one more
    per filter tap the eight miss, so that all nine taps are met: relative L2 < BWD per block and the componentwise bar of
    test_wgrad_gpu.py (8 x torch's fp32 product of the same operands); BWD and the bar's function are imported from test_tiles_gpu,
    not restated.  The CPU reference gathers the RAW x, applies the prologue and THEN zeroes the padding rows.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: the generic kernel at 128-wide tiles keeps layer2's 3x3 / stride 2 at 128 -> 128 (1152
columns are no whole number of 256-wide tiles beside 128 rows), the bf16 scheme, bf16 storage, k-ranges under 1024 pixels and a 3x3 /
stride-1 call without plane images.

(61 x 61 -> 31 x 31 and 30 x 31 -> 15 x 16 at 1x1; 61 x 62 -> 31 x 31 at 3x3: odd H reaches the bottom border tap, even W does not reach
the right one, top and left are reached in every image; 45 x 47 -> 23 x 24 reaches all four; 9 x 10 -> 5 x 5: a 32-row k-tile crosses
pixel rows and image boundaries several times, and a thread's four units, 8 rows apart, each wrap.)

Inputs are drawn on the device (one set per shape, shared by its calls); only the sampled, gathered columns travel to the CPU."""
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

from test_tiles_gpu import BWD, Record, componentwise, rel_err

pytestmark = pytest.mark.gpu

W1K, GEN = "koaf_wgrad1", "koaf_gemm"
Case = namedtuple("Case", "name shape call bm bn splitk empty last")
# shape (N, H, W, Cin, Cout, k, pad), stride 2; call: plain (dy + its amax) | apply (dy an ops.BnApply -- tf 2 on A --, plain x: the
# shortcuts' production call) | apply_prologue (and x behind its BatchNorm prologue -- tf 1 on B: conv2's); splitk / empty trailing
# splits / rows of the last live split: wgrad_plan's, as koaf_conv2d_wgrad_ws reports them (test_the_table_against_the_library_plan)
S1 = (133, 61, 61, 256, 512, 1, 0)        # P = 127 813: 128 splits of 1024 rows, the last live one 837, 3 empty; 2 tiles 256 x 256
S2 = (529, 61, 61, 128, 256, 1, 0)        # P = 508 369: 512 splits, 15 empty, one 256 x 128 tile
S3 = (529, 61, 61, 256, 128, 1, 0)        # the same plan, one 128 x 256 tile
S4 = (133, 30, 31, 1024, 512, 1, 0)       # P = 31 920: 32 splits; Cin / bn = 4 column tiles in the one tap
S5 = (58, 61, 62, 256, 256, 3, 1)         # P = 55 738: 56 splits, one empty; 9 column tiles = 9 taps
S6 = (13, 45, 47, 512, 512, 3, 1)         # P = 7 176: 7 splits of 1056 rows (no XCD remap); 18 column tiles, two per tap
S7 = (2223, 9, 10, 256, 256, 3, 1)        # P = 55 575: 5 x 5 output pixels per image
SHAPES = [S1, S2, S3, S4, S5, S6, S7]
CASES = [
    Case("k1-256to512-plain", S1, "plain", 256, 256, 128, 3, 837),
    Case("k1-256to512-apply", S1, "apply", 256, 256, 128, 3, 837),
    Case("k1-128to256-apply", S2, "apply", 256, 128, 512, 15, 465),
    Case("k1-256to128-apply", S3, "apply", 128, 256, 512, 15, 465),
    Case("k1-1024to512-plain", S4, "plain", 256, 256, 32, 0, 176),
    Case("k3-256to256-apply_prologue", S5, "apply_prologue", 256, 256, 56, 1, 442),
    Case("k3-512to512-apply_prologue", S6, "apply_prologue", 256, 256, 7, 0, 840),
    Case("k3-256to256-5x5-apply_prologue", S7, "apply_prologue", 256, 256, 56, 1, 279),
]
Refusal = namedtuple("Refusal", "name shape stride call store long_k")
R1 = (241, 61, 62, 128, 128, 3, 1)        # layer2's conv2: M = 128, N = 1152; k-ranges of 2080 pixels
R2 = (3, 40, 40, 512, 1024, 1, 0)         # P = 1200: k-ranges of 416 pixels
R3 = (80, 30, 31, 256, 256, 3, 1)         # 3x3 / stride 1 on the fp32 tensors (aplanes=False)
REFUSALS = [
    Refusal("k3s2-128to128", R1, 2, "apply_prologue", "fp32", True),
    Refusal("bf16scheme", S1, 2, "bf16scheme", "fp32", True),      # dy_amax withheld
    Refusal("bf16storage", S1, 2, "apply", "bf16", True),           # x and the apply's c stored as bf16 (act16 3)
    Refusal("kchunk416", R2, 2, "plain", "fp32", False),
    Refusal("k3s1-no-planes", R3, 1, "apply_prologue", "fp32", True),
]


def out_hw(shape, stride=2):
    N, H, W, Cin, Cout, k, pad = shape
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def plan_of(shape, stride=2):
    """(P, splitk, kchunk, empty trailing splits, rows of the last live split) from the library's workspace size:
    koaf_conv2d_wgrad_ws = (splitk + 16) * Cout * k * k * Cin"""
    from oaprogressionmmf_amd import _lib
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape, stride)
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, k, k, stride, pad)
    P, n = N * OH * OW, Cout * k * k * Cin
    assert ws > 0 and ws % n == 0
    splitk = ws // n - 16
    kchunk = (-(-P // splitk) + 31) // 32 * 32
    live = -(-P // kchunk)
    return P, splitk, kchunk, splitk - live, P - (live - 1) * kchunk


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_table_against_the_library_plan(case):
    P, splitk, kchunk, empty, last = plan_of(case.shape)
    assert (splitk, empty, last) == (case.splitk, case.empty, case.last), (case.name, P, splitk, kchunk, empty, last)
    assert kchunk >= 1024 and P % 32 != 0, (case.name, P, kchunk)


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_the_refusals_against_the_library_plan(case):
    """a refusal that is not about the k-range has k-ranges the rule would take"""
    P, splitk, kchunk, empty, last = plan_of(case.shape, case.stride)
    assert (kchunk >= 1024) == case.long_k, (case.name, P, splitk, kchunk)


@lru_cache(maxsize=1)
def inputs(shape, stride, dev, store16=False):
    """device operands of a shape: x [N H W, Cin], its prologue (sc, sh), the gradient dy [P, Cout] with its amax, and the
    BatchNorm-backward recipe (ops.BnApply); store16: x and the apply's conv output c stored as bf16 (activation storage mode)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape, stride)
    P = N * OH * OW
    g_ = torch.Generator(device=dev).manual_seed(9300 + (SHAPES + [R1, R2, R3]).index(shape))

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    t = dict(x=rnd(N * H * W, Cin) * 1.5 + 0.3, sc=rnd(Cin) * 0.2 + 1.0, sh=rnd(Cin) * 0.1, dy=rnd(P, Cout) * 1e-3)
    if store16:
        t["x"] = t["x"].bfloat16()
    t["amax"] = t["dy"].abs().max().reshape(1).float()
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


def call_model(dev, shape, stride, t, call):
    """ops.conv2d_wgrad as the model calls it -> (dw [Cout, k k Cin], the launch records)"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, pad = shape
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, k, k, stride, pad)
    dw, slabs = nan_like(Cout * k * k * Cin, dev).reshape(Cout, k, k, Cin), nan_like(ws, dev)
    prol = call == "apply_prologue"
    arg = t["apply"] if call in ("apply", "apply_prologue") else t["dy"]
    am = t["amax"] if call == "plain" else None
    with Record() as rec:
        ops.conv2d_wgrad(arg, t["x"], dw, N, H, W, Cin, Cout, k, k, stride, pad, t["sc"] if prol else None,
                         t["sh"] if prol else None, dy_amax=am, aplanes=False, slabs=slabs)
    torch.cuda.synchronize()
    return dw.reshape(Cout, k * k * Cin), rec.launches


def call_generic(dev, shape, t, call, splitk):
    """the generic path: koaf_gemm on the descriptor koaf_conv2d_wgrad builds (A K-major fp32, B the conv gather on the k index, 128 x 128
    tiles, the same splitk, slabs), then koaf_slab_reduce"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape)
    P, Nt = N * OH * OW, k * k * Cin
    L = _lib.lib()
    dw, slabs = nan_like(Cout * Nt, dev), nan_like((splitk + 16) * Cout * Nt, dev)
    g = _lib.KoafGemm()
    g.alpha, g.nb0, g.nb1, g.prec, g.fmt = 1.0, 1, 1, 1, 1
    g.A.kind, g.A.ld, g.B.kind, g.B.ptr, g.B.fscale = 1, Cout, 1, t["x"].data_ptr(), ops.ACT_SCALE
    g.B.gather, g.B.H, g.B.W, g.B.C, g.B.CS, g.B.PH, g.B.PW = 1, H, W, Cin, Cin, OH, OW
    g.B.KH, g.B.KW, g.B.stride, g.B.pad, g.B.pad_w = k, k, 2, pad, pad
    if call == "plain":
        g.A.ptr, g.A.amax = t["dy"].data_ptr(), t["amax"].data_ptr()
    else:
        ap = t["apply"]
        g.A.ptr, g.A.ptr2, g.A.tf, g.A.amax = ap.dz.data_ptr(), ap.c.data_ptr(), 2, ap.amax.data_ptr()
        g.A.sc, g.A.sc2, g.A.sh = ap.coef.data_ptr(), ap.coef.data_ptr() + 4 * 2 * Cout, ap.coef.data_ptr() + 4 * 3 * Cout
    if call == "apply_prologue":
        g.B.tf, g.B.sc, g.B.sh = 1, t["sc"].data_ptr(), t["sh"].data_ptr()
    g.M, g.N, g.K, g.bm, g.bn, g.splitk = Cout, Nt, P, 128, 128, splitk
    g.C, g.ldc = (slabs if splitk > 1 else dw).data_ptr(), Nt
    with Record() as rec:
        ops.gemm(g)
    if splitk > 1:
        ops.check(L.koaf_slab_reduce(slabs.data_ptr(), splitk, Cout * Nt, dw.data_ptr(), ops._stream()), "slab_reduce")
    torch.cuda.synchronize()
    return dw.reshape(Cout, Nt), rec.launches


def sampled_blocks(Cout, Nt, Cin):
    """64 x 64 blocks of dw as (row block, column block): the four corners and four interior ones, chosen so that both halves of a
    256-wide (or 128-wide) tile are met along both dimensions; then one block for every filter tap those eight miss"""
    rb, cb, per_tap = Cout // 64, Nt // 64, Cin // 64
    picks = [(0, 0), (rb - 1, cb - 1), (0, cb - 1), (rb - 1, 0), (rb // 2, cb // 2), (rb // 2 - 1, (cb // 2 + 1) % cb), (1 % rb, 2 % cb),
             (2 % rb, 1 % cb), (3 % rb, 3 % cb), ((rb // 2 + 1) % rb, 0), (0, (cb // 2 + 1) % cb)]
    out = []
    for p in picks:
        if p not in out:
            out.append(p)
    out = out[:8]
    for p in ((i, j) for i in range(rb) for j in range(cb)):      # (a 128-wide side: eight blocks or fewer in all -- take every one)
        if len(out) < 8 and p not in out:
            out.append(p)
    assert len(out) == min(8, rb * cb)
    for tap in range(Nt // Cin):
        if not any(bj // per_tap == tap for _, bj in out):
            out.append(((tap + 1) % rb, tap * per_tap + (tap * 3 + 1) % per_tap))
    assert {bj // per_tap for _, bj in out} == set(range(Nt // Cin))
    return out


def gather_map(shape, tap, dev):
    """source pixel index (clamped into the tensor) and validity of every k-row for a filter tap"""
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = out_hw(shape)
    kh, kw = tap // k, tap % k
    p = torch.arange(N * OH * OW, device=dev)
    n, oy, ox = p // (OH * OW), (p // OW) % OH, p % OW
    sy, sx = 2 * oy - pad + kh, 2 * ox - pad + kw
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return ((n * H + sy.clamp(0, H - 1)) * W + sx.clamp(0, W - 1)), ok


def hold_blocks(case, t, dw):
    """the float64 bars of the sampled blocks; the operands of a block are formed on the CPU from its (gathered) columns of the device
    tensors, the padding rows zeroed AFTER the prologue"""
    N, H, W, Cin, Cout, k, pad = case.shape
    prol = case.call == "apply_prologue"
    taps_hit, padded = set(), 0
    rows, cols = {}, {}          # the operands of a row / column block, formed once and shared by the sampled blocks that meet it

    def row_block(bi):
        rs = slice(64 * bi, 64 * bi + 64)
        if case.call == "plain":
            d32 = t["dy"][:, rs].cpu()
            return d32, d32.double()
        ap = t["apply"]
        coef = ap.coef.reshape(4, Cout)[:, rs].cpu()
        dz, c = ap.dz.reshape(-1, Cout)[:, rs].cpu(), ap.c.reshape(-1, Cout)[:, rs].cpu()
        return coef[0] * dz + coef[3] - coef[2] * c, coef[0].double() * dz.double() + coef[3].double() - coef[2].double() * c.double()

    def col_block(bj):
        tap, c0 = (64 * bj) // Cin, (64 * bj) % Cin
        ci = slice(c0, c0 + 64)
        idx, ok = gather_map(case.shape, tap, t["x"].device)
        x = t["x"][:, ci][idx].cpu()
        ok = ok.cpu()[:, None]
        if prol:
            sc, sh = t["sc"][ci].cpu(), t["sh"][ci].cpu()
            a32, a64 = torch.relu(x * sc + sh), torch.relu(x.double() * sc.double() + sh.double())
        else:
            a32, a64 = x, x.double()
        return tap, int((~ok).sum()), a32 * ok, a64 * ok

    for bi, bj in sampled_blocks(Cout, k * k * Cin, Cin):
        rs, cs = slice(64 * bi, 64 * bi + 64), slice(64 * bj, 64 * bj + 64)
        if bi not in rows:
            rows[bi] = row_block(bi)
        if bj not in cols:
            cols[bj] = col_block(bj)
        (d32, d64), (tap, npad, a32, a64) = rows[bi], cols[bj]
        taps_hit.add(tap)
        padded += npad
        ref64, ref32, den = d64.t() @ a64, d32.t() @ a32, d32.abs().double().t() @ a32.abs().double() + 1e-300
        got = dw[rs, cs]
        e = rel_err(got, ref64)
        cw, bar = componentwise(got, ref64, ref32, den)
        print(f"[wgrad1 gather] {case.name:32s} block ({bi:2d},{bj:2d}) tap {tap} rel L2 {e:.2e} (bar {BWD:.0e}) componentwise {cw:.2e} "
              f"(bar {bar:.2e})")
        assert e < BWD, (case.name, bi, bj, e)
        assert cw <= bar, (case.name, bi, bj, cw, bar)
    assert taps_hit == set(range(k * k)), (case.name, taps_hit)
    assert (padded > 0) == (pad > 0), (case.name, padded)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gathered_wide_tile_kernel_equals_the_generic_path(dev, case):
    N, H, W, Cin, Cout, k, pad = case.shape
    OH, OW = out_hw(case.shape)
    try:
        t = inputs(case.shape, 2, dev)
        dw, launches = call_model(dev, case.shape, 2, t, case.call)
        gemms = [r for r in launches if r["variant"] in (W1K, GEN)]
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        Nt = k * k * Cin
        tiles = (Cout // case.bm) * (Nt // case.bn)
        want = dict(variant=W1K, bm=case.bm, bn=case.bn, tiles=tiles, grid_x=tiles, splitk=case.splitk, M=Cout, N=Nt, K=N * OH * OW, fmt=1,
                    a_tf=0 if case.call == "plain" else 2, b_tf=1 if case.call == "apply_prologue" else 0, act16=0)
        assert {f: r[f] for f in want} == want, (case.name, r, want)
        bad = ~torch.isfinite(dw)
        assert not bool(bad.any()), (case.name, f"{int(bad.sum())} elements of dw: a tile or a split's slab was not written")
        assert torch.equal(call_model(dev, case.shape, 2, t, case.call)[0], dw), (case.name, "the same call twice")
        ref, lg = call_generic(dev, case.shape, t, case.call, case.splitk)
        assert len(lg) == 1 and (lg[0]["variant"], lg[0]["bm"], lg[0]["bn"], lg[0]["splitk"]) == (GEN, 128, 128, case.splitk), (case.name, lg)
        ndiff = int((ref != dw).sum())
        print(f"\n[wgrad1 gather] {case.name:32s} {r['variant']} {r['bm']}x{r['bn']} tiles {r['tiles']} splitk {r['splitk']} empty "
              f"{case.empty} last split {case.last} rows | elements that differ from the generic path: {ndiff}")
        assert torch.equal(ref, dw), (case.name, ndiff, "bit-identical to koaf_gemm_kernel on 128 x 128 tiles")
        hold_blocks(case, t, dw)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernel(dev, case):
    try:
        t = inputs(case.shape, case.stride, dev, case.store == "bf16")
        dw, launches = call_model(dev, case.shape, case.stride, t, case.call)
        gemms = [r for r in launches if r["variant"] in (W1K, GEN)]
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        assert (r["variant"], r["bm"], r["bn"]) == (GEN, 128, 128), (case.name, r)
        assert r["fmt"] == (0 if case.call == "bf16scheme" else 1) and r["act16"] == (3 if case.store == "bf16" else 0), (case.name, r)
        assert bool(torch.isfinite(dw).all()), case.name
    finally:
        torch.cuda.empty_cache()
