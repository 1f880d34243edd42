"""What the tests of the 256-row convolution units share (koaf_fwd1, koaf_fwd_s2, koaf_dgrad_s2, koaf_wgrad1: test_fwd1_gpu.py,
test_fwd_s2_gpu.py, test_dgrad_s2_gpu.py, test_wgrad1x1_gpu.py, test_wgrad1_gather_gpu.py), written once.

A shape is (N, H, W, Cin, Cout, k, pad) with the stride beside it; the dense files write (N, H, W, Cin, Cout) and mean k = 1, pad 0 at
stride 1 (geom).  Four parts:
  * geometry: out_hw, gather_map (row p = output pixel (n, oy, ox), tap (kh, kw): x[n][s oy - pad + kh][s ox - pad + kw], 0 outside the
    image), classes (the parity classes of a stride-2 data gradient), plan_of (the library's split-K plan), sampled_blocks;
  * the float64 operands of the CPU references: a row block of dy (plain, or formed from a BnApply) and a column block of x, dense or
    gathered -- the prologue is applied to the RAW x and the padding zeroed AFTER it (masked).  test_tile256_refs_cpu.py proves them
    against torch's conv2d and its autograd without a GPU, and that shifting the pad, swapping kh / kw or zeroing first is caught;
  * the descriptors koaf_conv.hip builds for a call, for the generic reference path through ops.gemm on 128 x 128 tiles
    (fwd_descriptor, wgrad_descriptor, dgrad_class_descriptors);
  * the checks themselves: the launch record (hold_record), the float64 hold of a forward call (hold_forward64) and of a weight gradient
    (hold_wgrad64), a whole forward / weight-gradient case (check_forward, check_wgrad) and a refusal (hold_refusal).
The bars are test_tiles_gpu's (FWD, BWD, componentwise, band_errors, rel_err), imported, not restated; 1e-4 / 1e-5 are run_forward's
bars of the statistics sums."""
from contextlib import contextmanager
from functools import lru_cache

import torch

from test_tiles_gpu import BWD, FWD, Record, band_errors, componentwise, rel_err

GEN, STREAM = "koaf_gemm", "koaf_gemm/stream"


# ---- geometry ----

def geom(shape):
    """(N, H, W, Cin, Cout, k, pad); a dense file's (N, H, W, Cin, Cout) is k = 1, pad 0"""
    return tuple(shape) + (1, 0) if len(shape) == 5 else tuple(shape)


def out_hw(shape, stride=2):
    N, H, W, Cin, Cout, k, pad = geom(shape)
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def pointwise(shape, stride):
    return geom(shape)[5:] == (1, 0) and stride == 1


def tap_hw(tap, k):
    return tap // k, tap % k


def gather_map(shape, tap, dev, stride=2):
    """source pixel index (clamped into the tensor) and validity of every output pixel (the k-rows of a weight gradient) for a filter tap"""
    N, H, W, Cin, Cout, k, pad = geom(shape)
    OH, OW = out_hw(shape, stride)
    kh, kw = tap_hw(tap, k)
    p = torch.arange(N * OH * OW, device=dev)
    n, oy, ox = p // (OH * OW), (p // OW) % OH, p % OW
    sy, sx = stride * oy - pad + kh, stride * ox - pad + kw
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return ((n * H + sy.clamp(0, H - 1)) * W + sx.clamp(0, W - 1)), ok


def classes(shape):
    """(py, px, Hc, Wc, khs, kws, nkh, nkw, offy, offx) of the four parity classes, as koaf_conv2d_dgrad_bnb forms them"""
    N, H, W, Cin, Cout, k, pad = geom(shape)
    out = []
    for py in range(2):
        for px in range(2):
            khs, kws = (py + pad) & 1, (px + pad) & 1
            nkh, nkw = ((k - khs + 1) // 2 if khs < k else 0), ((k - kws + 1) // 2 if kws < k else 0)
            out.append((py, px, (H - py + 1) // 2, (W - px + 1) // 2, khs, kws, nkh, nkw, (py + pad - khs) // 2, (px + pad - kws) // 2))
    return out


def plan_of(shape, stride=2):
    """(P, splitk, kchunk, empty trailing splits, rows of the last live split) from the library's workspace size:
    koaf_conv2d_wgrad_ws = (splitk + 16) * Cout * k * k * Cin"""
    from oaprogressionmmf_amd import _lib
    N, H, W, Cin, Cout, k, pad = geom(shape)
    OH, OW = out_hw(shape, stride)
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, k, k, stride, pad)
    P, n = N * OH * OW, Cout * k * k * Cin
    assert ws > 0 and ws % n == 0
    splitk = ws // n - 16
    kchunk = (-(-P // splitk) + 31) // 32 * 32
    live = -(-P // kchunk)
    return P, splitk, kchunk, splitk - live, P - (live - 1) * kchunk


def sampled_blocks(Cout, Nt, Cin):
    """64 x 64 blocks of dw [Cout, Nt = taps Cin] as (row block, column block): the four corners and four interior ones, chosen so that both
    halves of a 256-wide (or 128-wide) tile are met along both dimensions; then one block for every filter tap those eight miss.  With one
    tap these are the eight blocks of the dense weight gradient."""
    rb, cb, per_tap = Cout // 64, Nt // 64, Cin // 64
    picks = [(0, 0), (rb - 1, cb - 1), (0, cb - 1), (rb - 1, 0), (rb // 2, cb // 2), (rb // 2 - 1, (cb // 2 + 1) % cb), (1 % rb, 2 % cb),
             (2 % rb, 1 % cb), (3 % rb, 3 % cb), ((rb // 2 + 1) % rb, 0), (0, (cb // 2 + 1) % cb)]
    eight = []
    for p in picks:
        if p not in eight:
            eight.append(p)
    eight = eight[:8]
    out = list(eight)
    for p in ((i, j) for i in range(rb) for j in range(cb)):      # (a 128-wide side: eight blocks or fewer in all -- take every one)
        if len(out) < 8 and p not in out:
            out.append(p)
    assert len(out) == min(8, rb * cb)
    for tap in range(Nt // Cin):
        if not any(bj // per_tap == tap for _, bj in out):
            out.append(((tap + 1) % rb, tap * per_tap + (tap * 3 + 1) % per_tap))
    assert {bj // per_tap for _, bj in out} == set(range(Nt // Cin))
    # (one tap: the dense weight gradient's blocks -- the picks, topped up only beside a 128-wide side, and no block for a missed tap)
    assert Nt != Cin or (out[:len(eight)] == eight and len(out) == min(8, rb * cb))
    return out


def column_blocks(Cout, few=False):
    """sampled 64-column blocks of a forward output: both halves of a column tile, the first and the last tile (few: the first and the last)"""
    nb = Cout // 64
    return sorted({0, nb - 1} if few else {0, nb - 1, nb // 2, (nb // 2 + 1) % nb})


# ---- device fixtures ----

def nan_like(n, dev):
    return torch.full((n,), float("nan"), device=dev)


@contextmanager
def nan_outputs():
    """inside, every floating-point tensor ops.conv allocates is pre-filled with NaN"""
    from oaprogressionmmf_amd import ops
    real_empty = ops.conv._empty

    def nan_empty(*a, **k_):
        out = real_empty(*a, **k_)
        return out.fill_(float("nan")) if out.is_floating_point() else out
    ops.conv._empty = nan_empty
    try:
        yield
    finally:
        ops.conv._empty = real_empty


def bn_apply(dev, rows, C, *, c, dz, gam, bet, store16=False):
    """the BatchNorm-backward recipe (ops.BnApply) of a [rows, C] gradient dz behind the conv output c: colstats -> bn_finalize -> bn_bwd;
    store16: c stored as bf16.  (The caller draws the four tensors, in its own order.)"""
    from oaprogressionmmf_amd import ops
    if store16:
        c = c.bfloat16()
    sv = ops.bn_finalize(ops.colstats(c, rows, C), C, rows, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev),
                         torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)
    dgm, dbt = torch.empty(C, device=dev), torch.empty(C, device=dev)
    return ops.bn_bwd(dz, c, sv, rows, C, rows, dgm, dbt, 2, fused=True)


@lru_cache(maxsize=1)
def forward_inputs(shape, dev, seed):
    """device operands of a forward shape: x [N, H, W, Cin], its prologue (sc, sh), the packed weight with its plane images, a statistics shift"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = geom(shape)
    g_ = torch.Generator(device=dev).manual_seed(seed)

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    t = dict(x=rnd(N, H, W, Cin) * 1.5 + 0.3, sc=rnd(Cin) * 0.2 + 1.0, sh=rnd(Cin) * 0.1, w=rnd(Cout, k, k, Cin) * (k * k * Cin) ** -0.5,
             shift=rnd(Cout) * 0.3 + 0.2)
    t["img"] = ops.build_weight_planes(t["w"], Cout, k * k, Cin)
    torch.cuda.synchronize()
    return t


@lru_cache(maxsize=1)
def wgrad_inputs(shape, stride, dev, seed, store16=False, apply=True):
    """device operands of a weight-gradient shape: x [N H W, Cin], its prologue (sc, sh), the gradient dy [P, Cout] with its amax, and
    (apply; drawn last) the BatchNorm-backward recipe (ops.BnApply); store16: x and the apply's conv output c stored as bf16 (activation
    storage mode)"""
    N, H, W, Cin, Cout, k, pad = geom(shape)
    OH, OW = out_hw(shape, stride)
    P = N * OH * OW
    g_ = torch.Generator(device=dev).manual_seed(seed)

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    t = dict(x=rnd(N * H * W, Cin) * 1.5 + 0.3, sc=rnd(Cin) * 0.2 + 1.0, sh=rnd(Cin) * 0.1, dy=rnd(P, Cout) * 1e-3)
    if store16:
        t["x"] = t["x"].bfloat16()
    t["amax"] = t["dy"].abs().max().reshape(1).float()
    if apply:
        t["apply"] = bn_apply(dev, P, Cout, c=rnd(P, Cout) * 1.5 + 0.3, dz=rnd(P, Cout) * 1e-3, gam=rnd(Cout) * 0.2 + 1.0, bet=rnd(Cout) * 0.1,
                              store16=store16)
    torch.cuda.synchronize()
    return t


# ---- the operands of the CPU references, in fp32 and float64 ----

def transform(x, sc, sh):
    """(fp32, float64) of relu(sc x + sh), of x itself without a prologue (sc None)"""
    if sc is None:
        return x, x.double()
    return torch.relu(x * sc + sh), torch.relu(x.double() * sc.double() + sh.double())


def masked(x, ok, sc, sh):
    """the prologue on the RAW x, and THEN the padding rows zeroed"""
    a32, a64 = transform(x, sc, sh)
    return a32 * ok, a64 * ok


def dense_cols(x, ci, sc, sh):
    """columns ci of the dense operand x [rows, C] (device) behind its prologue -> (tap 0, padded rows 0, fp32, float64) on the CPU"""
    a32, a64 = transform(x[:, ci].cpu(), None if sc is None else sc[ci].cpu(), None if sc is None else sh[ci].cpu())
    return 0, 0, a32, a64


def gathered_cols(shape, stride, x, tap, ci, sc, sh):
    """channels ci of filter tap `tap` of the gathered operand, x [N H W, C] (device) -> (tap, padded rows, fp32, float64) on the CPU"""
    idx, ok = gather_map(shape, tap, x.device, stride)
    ok = ok.cpu()[:, None]
    a32, a64 = masked(x[:, ci][idx].cpu(), ok, None if sc is None else sc[ci].cpu(), None if sc is None else sh[ci].cpu())
    return tap, int((~ok).sum()), a32, a64


def col_block(shape, stride, x, bj, sc, sh):
    """64-column block bj of the [P, taps Cin] operand of a weight gradient: dense for a pointwise call, else gathered"""
    Cin = geom(shape)[3]
    tap, c0 = (64 * bj) // Cin, (64 * bj) % Cin
    ci = slice(c0, c0 + 64)
    return dense_cols(x, ci, sc, sh) if pointwise(shape, stride) else gathered_cols(shape, stride, x, tap, ci, sc, sh)


def all_cols(shape, stride, x, sc, sh):
    """the whole [M, taps Cin] operand of a forward call -> (padded rows, fp32, float64)"""
    if pointwise(shape, stride):
        return dense_cols(x, slice(None), sc, sh)[1:]
    k = geom(shape)[5]
    taps = [gathered_cols(shape, stride, x, tap, slice(None), sc, sh) for tap in range(k * k)]
    return sum(p[1] for p in taps), torch.cat([p[2] for p in taps], 1), torch.cat([p[3] for p in taps], 1)


def apply_rows(ap, C, rs):
    """columns rs of the dy an ops.BnApply stands for: coef0 dz + coef3 - coef2 c -> (fp32, float64)"""
    coef = ap.coef.reshape(4, C)[:, rs].cpu()
    dz, c = ap.dz.reshape(-1, C)[:, rs].cpu(), ap.c.reshape(-1, C)[:, rs].cpu()
    return coef[0] * dz + coef[3] - coef[2] * c, coef[0].double() * dz.double() + coef[3].double() - coef[2].double() * c.double()


def row_block(t, call, Cout, bi):
    """64-column block bi of dy [P, Cout]: the plain dy, or the apply"""
    rs = slice(64 * bi, 64 * bi + 64)
    if call == "plain":
        d32 = t["dy"][:, rs].cpu()
        return d32, d32.double()
    return apply_rows(t["apply"], Cout, rs)


# ---- launch records ----

def records(launches):
    return [r for r in launches if r["variant"].startswith("koaf_")]


def hold_record(name, r, want):
    assert {f: r[f] for f in want} == want, (name, r, want)


def hold_refusal(name, launches, unit, outs, fmt, act16, kept=(GEN,), every=False):
    """a refused call: no record of the unit; the last GEMM record (every: each one with work) is of a kept variant, in the scheme and the
    storage mode asked for; the outputs are finite -> the GEMM records"""
    gemms = records(launches)
    assert gemms and all(r["variant"] != unit for r in launches), (name, launches)
    assert all(r["variant"] in kept for r in ([r for r in gemms if r["K"] > 0] if every else gemms[-1:])), (name, launches)
    assert all((r["fmt"], r["act16"]) == (fmt, act16) for r in (gemms if every else gemms[-1:])), (name, gemms)
    for o in outs:
        assert bool(torch.isfinite(o.float()).all()), name
    return gemms


# ---- forward ----

def conv_fwd(shape, stride, t, call, stats, **kw):
    """ops.conv2d_fwd as the model calls it, y and part pre-filled with NaN -> (y [M, Cout], part[:rows] or None, the launch records)"""
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, pad = geom(shape)
    prol = call == "prologue"
    with nan_outputs(), Record() as rec:
        out = ops.conv2d_fwd(t["x"], t["w"], N, H, W, Cin, Cout, k, k, stride, pad, t["sc"] if prol else None,
                             t["sh"] if prol else None, stats=bool(stats), shift=t["shift"] if stats == "shift" else None,
                             wimg=kw.pop("wimg", t["img"]), **kw)
    torch.cuda.synchronize()
    return out[0].reshape(-1, Cout), out[1], rec.launches


def fwd_descriptor(shape, stride, t, call, stats, y, part):
    """the KoafGemm koaf_conv2d_fwd builds for the call (A dense for a pointwise call, else gathered; B the F plane image), on 128 x 128 tiles"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, pad = geom(shape)
    OH, OW = out_hw(shape, stride)
    M, K = N * OH * OW, k * k * Cin
    f, d, amax = t["img"]
    g = _lib.KoafGemm()
    g.alpha, g.nb0, g.nb1, g.splitk, g.fmt = 1.0, 1, 1, 1, 1
    g.A.ptr, g.A.kind, g.A.fscale = t["x"].data_ptr(), 0, ops.ACT_SCALE
    if pointwise(shape, stride):
        g.A.gather, g.A.ld = 0, Cin
    else:
        g.A.gather, g.A.H, g.A.W, g.A.C, g.A.CS, g.A.PH, g.A.PW = 1, H, W, Cin, Cin, OH, OW
        g.A.KH, g.A.KW, g.A.stride, g.A.pad, g.A.pad_w = k, k, stride, pad, pad
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
    return g


def conv_fwd_generic(dev, shape, stride, t, call, stats, stream=None):
    """the generic path: koaf_gemm on fwd_descriptor (stream: with ops.set_stream(stream) around the call) -> (y, part [M / 128, 2, Cout] or
    None, records)"""
    from oaprogressionmmf_amd import ops
    Cout = geom(shape)[4]
    OH, OW = out_hw(shape, stride)
    M = shape[0] * OH * OW
    y = torch.full((M, Cout), float("nan"), device=dev)
    part = torch.full((M // 128, 2, Cout), float("nan"), device=dev) if stats else None
    g = fwd_descriptor(shape, stride, t, call, stats, y, part)
    was = ops.set_stream(stream) if stream is not None else None
    try:
        with Record() as rec:
            ops.gemm(g)
    finally:
        if stream is not None:
            ops.set_stream(was)
    torch.cuda.synchronize()
    return y, part, rec.launches


def hold_forward64(tag, case, stride, t, y, part, few=False):
    """the float64 bars of sampled 64-column blocks over all rows: relative L2 < FWD per 128-row band, the componentwise bar, the statistics
    sums at 1e-4 / 1e-5; the A operand is formed ONCE on the CPU"""
    N, H, W, Cin, Cout, k, pad = geom(case.shape)
    OH, OW = out_hw(case.shape, stride)
    M = N * OH * OW
    prol = case.call == "prologue"
    padded, a32, a64 = all_cols(case.shape, stride, t["x"].reshape(-1, Cin), t["sc"] if prol else None, t["sh"] if prol else None)
    assert (padded > 0) == (pad > 0), (case.name, padded)
    a_abs = a32.abs().double()
    for bj in column_blocks(Cout, few):
        cs = slice(64 * bj, 64 * bj + 64)
        w32 = t["w"].reshape(Cout, -1)[cs].cpu()
        y64, y32, den = a64 @ w32.double().t(), a32 @ w32.t(), a_abs @ w32.abs().double().t() + 1e-300
        got = y[:, cs]
        be = band_errors(got, y64)
        cw, bar = componentwise(got, y64, y32, den)
        line = f"{tag} columns {64 * bj:4d}.. worst band {be.max().item():.2e} (bar {FWD:.0e}) componentwise {cw:.2e} (bar {bar:.2e})"
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


def check_forward(dev, case, unit, stride, t, tag, grid_x=None, legs=None, few=False):
    """a forward case: the launch record; every tile written; the same call twice; torch.equal to the generic path on 128 x 128 tiles (legs:
    (set_stream, variant) pairs, each asserted from its launch record; default the block-wide koaf_gemm as the library is set); float64"""
    N, H, W, Cin, Cout, k, pad = geom(case.shape)
    OH, OW = out_hw(case.shape, stride)
    M, K = N * OH * OW, k * k * Cin
    assert M % 256 == 0
    try:
        y, part, launches = conv_fwd(case.shape, stride, t, case.call, case.stats)
        gemms = records(launches)
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        tiles = (M // 256) * (Cout // case.bn)
        hold_record(case.name, r, dict(variant=unit, bm=256, bn=case.bn, tiles=tiles, grid_x=tiles if grid_x is None else grid_x(tiles), splitk=1,
                                       nbatch=1, M=M, N=Cout, K=K, fmt=1, a_tf=1 if case.call == "prologue" else 0, b_tf=0, act16=0, emit=0))
        assert bool(torch.isfinite(y).all()), (case.name, "a tile of y was not written")
        assert (part is None) == (not case.stats), case.name
        if part is not None:
            assert part.shape[0] == M // 128, (case.name, part.shape)
            assert bool(torch.isfinite(part).all()), (case.name, "a partial row was not written")
        y2, part2, _ = conv_fwd(case.shape, stride, t, case.call, case.stats)
        assert torch.equal(y2, y) and (part is None or torch.equal(part2, part)), (case.name, "the same call twice")
        for stream, variant in legs or ((None, GEN),):
            ref, rpart, lg = conv_fwd_generic(dev, case.shape, stride, t, case.call, case.stats, stream)
            assert len(lg) == 1 and (lg[0]["variant"], lg[0]["bm"], lg[0]["bn"]) == (variant, 128, 128), (case.name, lg)
            ndiff = int((ref != y).sum())
            pdiff = int((rpart != part).sum()) if part is not None else 0
            print(f"\n{tag} {r['variant']} {r['bm']}x{r['bn']} tiles {r['tiles']}" + (f" grid.x {r['grid_x']}" if legs else "")
                  + f" | elements that differ from {variant if legs else 'the generic path'}: y {ndiff} part {pdiff}")
            assert torch.equal(ref, y), (case.name, variant, ndiff, "bit-identical to koaf_gemm_kernel on 128 x 128 tiles")
            if part is not None:
                assert torch.equal(rpart, part), (case.name, variant, pdiff, "the statistics rows of the 128-row tiling")
            del ref, rpart
        hold_forward64(tag, case, stride, t, y, part, few)
    finally:
        torch.cuda.empty_cache()


# ---- weight gradient ----

def conv_wgrad(dev, shape, stride, t, call):
    """ops.conv2d_wgrad as the model calls it, dw and the slabs pre-filled with NaN -> (dw [Cout, k k Cin], the launch records)"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, pad = geom(shape)
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


def wgrad_descriptor(shape, stride, t, call, splitk, out):
    """the KoafGemm koaf_conv2d_wgrad builds for the call: A = dy K-major (plain, or the apply: tf 2), B = x K-major, dense for a pointwise
    call, else the conv gather on the k index (behind the prologue for apply_prologue: tf 1), 128 x 128 tiles, splitk slabs"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, pad = geom(shape)
    OH, OW = out_hw(shape, stride)
    P, Nt = N * OH * OW, k * k * Cin
    g = _lib.KoafGemm()
    g.alpha, g.nb0, g.nb1, g.prec, g.fmt = 1.0, 1, 1, 1, 1
    g.A.kind, g.A.ld, g.B.kind, g.B.ptr, g.B.fscale = 1, Cout, 1, t["x"].data_ptr(), ops.ACT_SCALE
    if pointwise(shape, stride):
        g.B.ld = Cin
    else:
        g.B.gather, g.B.H, g.B.W, g.B.C, g.B.CS, g.B.PH, g.B.PW = 1, H, W, Cin, Cin, OH, OW
        g.B.KH, g.B.KW, g.B.stride, g.B.pad, g.B.pad_w = k, k, stride, pad, pad
    if call == "plain":
        g.A.ptr, g.A.amax = t["dy"].data_ptr(), t["amax"].data_ptr()
    else:
        ap = t["apply"]
        g.A.ptr, g.A.ptr2, g.A.tf, g.A.amax = ap.dz.data_ptr(), ap.c.data_ptr(), 2, ap.amax.data_ptr()
        g.A.sc, g.A.sc2, g.A.sh = ap.coef.data_ptr(), ap.coef.data_ptr() + 4 * 2 * Cout, ap.coef.data_ptr() + 4 * 3 * Cout
    if call == "apply_prologue":
        g.B.tf, g.B.sc, g.B.sh = 1, t["sc"].data_ptr(), t["sh"].data_ptr()
    g.M, g.N, g.K, g.bm, g.bn, g.splitk = Cout, Nt, P, 128, 128, splitk
    g.C, g.ldc = out.data_ptr(), Nt
    return g


def conv_wgrad_generic(dev, shape, stride, t, call, splitk):
    """the generic path: koaf_gemm on wgrad_descriptor, then koaf_slab_reduce"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, pad = geom(shape)
    n = Cout * k * k * Cin
    dw, slabs = nan_like(n, dev), nan_like((splitk + 16) * n, dev)
    g = wgrad_descriptor(shape, stride, t, call, splitk, slabs if splitk > 1 else dw)
    with Record() as rec:
        ops.gemm(g)
    if splitk > 1:
        ops.check(_lib.lib().koaf_slab_reduce(slabs.data_ptr(), splitk, n, dw.data_ptr(), ops._stream()), "slab_reduce")
    torch.cuda.synchronize()
    return dw.reshape(Cout, k * k * Cin), rec.launches


def hold_wgrad64(tag, case, stride, t, dw, show_tap):
    """the float64 bars of the sampled blocks: relative L2 < BWD and the componentwise bar; the operands of a row / column block are formed
    once on the CPU from its (gathered) columns of the device tensors and shared by the sampled blocks that meet it.  All taps are met,
    and padding exactly where the filter has some."""
    N, H, W, Cin, Cout, k, pad = geom(case.shape)
    prol = case.call == "apply_prologue"
    taps_hit, padded, rows, cols = set(), 0, {}, {}
    for bi, bj in sampled_blocks(Cout, k * k * Cin, Cin):
        rs, cs = slice(64 * bi, 64 * bi + 64), slice(64 * bj, 64 * bj + 64)
        if bi not in rows:
            rows[bi] = row_block(t, case.call, Cout, bi)
        if bj not in cols:
            cols[bj] = col_block(case.shape, stride, t["x"], bj, t["sc"] if prol else None, t["sh"] if prol else None)
        (d32, d64), (tap, npad, a32, a64) = rows[bi], cols[bj]
        taps_hit.add(tap)
        padded += npad
        ref64, ref32, den = d64.t() @ a64, d32.t() @ a32, d32.abs().double().t() @ a32.abs().double() + 1e-300
        got = dw[rs, cs]
        e = rel_err(got, ref64)
        cw, bar = componentwise(got, ref64, ref32, den)
        print(f"{tag} block ({bi:2d},{bj:2d})" + (f" tap {tap}" if show_tap else "")
              + f" rel L2 {e:.2e} (bar {BWD:.0e}) componentwise {cw:.2e} (bar {bar:.2e})")
        assert e < BWD, (case.name, bi, bj, e)
        assert cw <= bar, (case.name, bi, bj, cw, bar)
    assert taps_hit == set(range(k * k)), (case.name, taps_hit)
    assert (padded > 0) == (pad > 0), (case.name, padded)


def check_wgrad(dev, case, unit, stride, t, tag, show_tap):
    """a weight-gradient case: the launch record; every tile and slab written; the same call twice; torch.equal to the generic path on
    128 x 128 tiles at the same splitk; float64"""
    N, H, W, Cin, Cout, k, pad = geom(case.shape)
    OH, OW = out_hw(case.shape, stride)
    try:
        dw, launches = conv_wgrad(dev, case.shape, stride, t, case.call)
        gemms = records(launches)
        assert len(gemms) == 1, (case.name, launches)
        r = gemms[0]
        Nt = k * k * Cin
        tiles = (Cout // case.bm) * (Nt // case.bn)
        hold_record(case.name, r, dict(variant=unit, bm=case.bm, bn=case.bn, tiles=tiles, grid_x=tiles, splitk=case.splitk, M=Cout, N=Nt,
                                       K=N * OH * OW, fmt=1, a_tf=0 if case.call == "plain" else 2,
                                       b_tf=1 if case.call == "apply_prologue" else 0, act16=0))
        bad = ~torch.isfinite(dw)
        assert not bool(bad.any()), (case.name, f"{int(bad.sum())} elements of dw: a tile or a split's slab was not written")
        assert torch.equal(conv_wgrad(dev, case.shape, stride, t, case.call)[0], dw), (case.name, "the same call twice")
        ref, lg = conv_wgrad_generic(dev, case.shape, stride, t, case.call, case.splitk)
        assert len(lg) == 1 and (lg[0]["variant"], lg[0]["bm"], lg[0]["bn"], lg[0]["splitk"]) == (GEN, 128, 128, case.splitk), (case.name, lg)
        ndiff = int((ref != dw).sum())
        print(f"\n{tag} {r['variant']} {r['bm']}x{r['bn']} tiles {r['tiles']} splitk {r['splitk']} empty {case.empty} "
              f"last split {case.last} rows | elements that differ from the generic path: {ndiff}")
        assert torch.equal(ref, dw), (case.name, ndiff, "bit-identical to koaf_gemm_kernel on 128 x 128 tiles")
        hold_wgrad64(tag, case, stride, t, dw, show_tap)
    finally:
        torch.cuda.empty_cache()


def check_wgrad_refusal(dev, case, unit, stride, t):
    """a refused weight gradient: one record, koaf_gemm on 128 x 128 tiles, in the scheme and storage mode of the call; dw finite"""
    try:
        dw, launches = conv_wgrad(dev, case.shape, stride, t, case.call)
        gemms = hold_refusal(case.name, launches, unit, [dw], 0 if case.call == "bf16scheme" else 1, 3 if case.store == "bf16" else 0)
        assert len(gemms) == 1 and (gemms[0]["bm"], gemms[0]["bn"]) == (128, 128), (case.name, gemms)
    finally:
        torch.cuda.empty_cache()


# ---- the stride-2 data gradient ----

def dgrad_class_descriptors(shape, t, call, dx, part, amax, planes):
    """the four KoafGemm koaf_conv2d_dgrad_bnb builds for a stride-2 call, one per parity class, on 128 x 128 tiles: A = dy transposed-gathered
    at stride 1 over the class's taps (from `planes` where the class has a tap and they are given, else fp32: plain, or the apply: tf 2),
    B = the class's taps of the D plane image, the row map, and for bnb2 calls the fused reduction with its partial rows class after class"""
    from oaprogressionmmf_amd import _lib
    N, H, W, Cin, Cout, k, pad = geom(shape)
    OH, OW = out_hw(shape)
    npo = N * OH * OW
    use_apply, bnb = call in ("bnb2_amax", "bnb2", "apply"), call.startswith("bnb2")
    f, d, wamax = t["img"]
    ap = t["apply"]
    out, rows_done = [], 0
    for py, px, Hc, Wc, khs, kws, nkh, nkw, offy, offx in classes(shape):
        g = _lib.KoafGemm()
        g.alpha, g.nb0, g.nb1, g.splitk, g.fmt, g.prec = 1.0, 1, 1, 1, 1, 1
        g.A.amax, g.B.amax = (ap.amax if use_apply else t["am"]).data_ptr(), wamax.data_ptr()
        g.A.kind, g.A.gather = 0, 2
        if use_apply:
            g.A.ptr, g.A.ptr2, g.A.tf = ap.dz.data_ptr(), ap.c.data_ptr(), 2
            g.A.sc, g.A.sc2, g.A.sh = ap.coef.data_ptr(), ap.coef.data_ptr() + 8 * Cout, ap.coef.data_ptr() + 12 * Cout
        else:
            g.A.ptr = t["dy"].data_ptr()
        g.A.H, g.A.W, g.A.C, g.A.CS, g.A.PH, g.A.PW = OH, OW, Cout, Cout, Hc, Wc
        g.A.KH, g.A.KW, g.A.stride, g.A.pad, g.A.pad_w = max(nkh, 1), max(nkw, 1), 1, offy, offx
        g.B.ptr, g.B.kind, g.B.gather, g.B.C, g.B.KW = t["w"].data_ptr() + 4 * (khs * k + kws) * Cin, 2, 0, Cout, g.A.KW
        g.B.planes, g.B.ld, g.B.plane_stride = d.data_ptr() + 2 * (khs * k + kws) * Cout, k * k * Cout, Cin * k * k * Cout
        g.B.tap_stride, g.B.tap_stride_h = 2 * Cout, 2 * k * Cout
        if planes is not None and nkh > 0 and nkw > 0:
            g.A.kind, g.A.planes, g.A.plane_stride, g.A.zeros = 2, planes.data_ptr(), npo * Cout, planes.data_ptr() + 4 * npo * Cout
            g.A.ptr, g.A.ptr2, g.A.tf, g.A.sc, g.A.sh, g.A.sc2 = None, None, 0, None, None, None
        g.M, g.N, g.K, g.bm, g.bn = N * Hc * Wc, Cin, nkh * nkw * Cout, 128, 128
        g.C, g.ldc, g.ldr = dx.data_ptr(), Cin, Cin
        g.cmap, g.cm_PH, g.cm_PW, g.cm_H, g.cm_W, g.cm_py, g.cm_px = 1, Hc, Wc, H, W, py, px
        if bnb:
            sv = t["sv"]
            g.bnb_mode, g.bnb_c, g.bnb_amax = 2, t["cx"].data_ptr(), amax.data_ptr() if amax is not None else None
            g.bnb_mean, g.bnb_invstd, g.bnb_sc, g.bnb_sh = sv[0].data_ptr(), sv[1].data_ptr(), sv[2].data_ptr(), sv[3].data_ptr()
            g.bnb_part = part.data_ptr() + 4 * rows_done * 2 * Cin
            rows_done += g.M // 128
        out.append(g)
    return out
