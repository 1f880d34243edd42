"""Grouped 3x3 convolution (ResNeXt, koaf.h "Grouped 3x3 convolution") per slab, band and element at its edges.

koaf_gconv3x3_fwd / _dgrad / _wgrad take a route through koaf_gemm that no dense convolution takes: the C / 64 block-diagonal
slabs are the batch dimension (grid.z, per-slab offsets A.bs1 / cbs1 / tf_bs / stats_bs), the A operand is a channel slab of a
wider pixel, the tile is forced to 128 x 64 even under 128 rows, the stride-2 data gradient is ONE gathered GEMM, and the fp32
weights are split in the kernel on both contraction schemes.  Every row of SHAPES is the smallest that still reaches its edge
(a tile = 128 rows x one slab, K = 576 = 18 k-steps), goes through ops.gconv_* as the model calls them, and ASSERTS FROM THE
LAUNCH RECORD (koaf.h koaf_launch_log) the tile, batch, scheme and loader transform that served it.  Where a buffer has to be
prepared beforehand -- outputs and statistics inside NaN-filled guard rows -- the same call goes through the C ABI directly.

Bars (owned by the module docstrings of test_kernels_gpu.py and test_tiles_gpu.py; nothing new is invented):
  * relative L2 against the float64 CPU grouped convolution (gconv_refs.py, proven by test_gconv_refs_cpu.py) per slab AND per
    128-row band of the output, and over the whole tensor: FWD = 2e-6 forward, BWD = 4e-6 gradients.  The stride-2 data gradient
    is one GEMM here: its bands are raster bands of dx.
  * componentwise: max |y - y64| / (|a| conv |w|) <= 8 x the same ratio of torch's fp32 CPU grouped convolution of the same
    operands (the prologue evaluated in fp32 as well); the denominator is positive everywhere (data gradient: where it is exactly
    0 no output tap reaches the pixel and dx is exactly 0).
  * statistics: per tile row AND slab, sum (y - k) and sum (y - k)^2 against the float64 sums over that tile's own rows of the
    device's y (the ragged last tile: its real rows only; k = the shift handed in, 0 without one) -- relative L2 over the slab's 64
    channels 1e-4 and 1e-5 (test_conv2d); the totals at the same bars; behind koaf_bn_finalize an offset mean keeps the 1e-6 / 2e-6
    of test_shifted_batchnorm_statistics.
  * guard rows: y / dx are the head of a NaN-filled buffer 128 rows longer, the statistics the head of one a row longer: after the
    call every guard element is still NaN and nothing before them is.
  * bf16 activation storage: the property of test_bf16_gpu.py -- y bit-equal to the fp32 mode on the widened x, rounded once; the
    statistics bit-equal (they come from the fp32 accumulators); the scheme is bf16 whatever rides on the weight.
  * the slab images: gconv_expand_w / gconv_compress_dw bit-equal to gconv_refs.expand / compress at every admitted group width.

Each case prints one table line: the launch record, worst (slab, band) error, whole tensor, componentwise ratio and bar.

Measured (MI355X): forward worst (slab, band) 3.4e-7 (a-g1, one dense slab), componentwise closest 3.3e-7 against its bar 1.1e-6
(g); data gradient 3.4e-7 and 1.5e-7 against 4.7e-7; weight gradient worst slab 2.5e-7; statistics per (tile, slab) 8.9e-7 on sums
and 2.0e-7 on sums of squares.  The per-tile statistics found a fault: koaf_gemm_kernel summed the zero rows of a ragged last
tile about the shift as well and took n k and n k^2 out afterwards, which left 3.2e-4 of the sum (h: 2 real rows of 128) and
3.5e-5 of the sum of squares (b with an offset mean: 4 real rows) -- such a tile now sums its real rows only."""
import ctypes
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

import gconv_refs as R
from test_tiles_gpu import BWD, FWD, Record, band_errors, componentwise, conv_out, rel_err

pytestmark = pytest.mark.gpu

SUM, SUMSQ = 1e-4, 1e-5        # test_kernels_gpu.py test_conv2d: statistics sums / sums of squares

Shape = namedtuple("Shape", "name N H W C stride groups")
SHAPES = [
    Shape("a", 1, 9, 7, 64, 1, 32),         # M = 63 < 64, one slab, Cg = 2
    Shape("a-g1", 1, 9, 7, 64, 1, 1),       # ... Cg = 64: the slab is dense
    Shape("b", 2, 13, 10, 128, 1, 32),      # M = 260: two tiles + 4 rows, two slabs, H != W
    Shape("c", 3, 11, 11, 256, 2, 32),      # odd size at stride 2: OH = 6, M = 108 < 128
    Shape("d", 2, 16, 12, 256, 2, 32),      # even size at stride 2: no bottom / right padding tap
    Shape("e", 2, 12, 12, 512, 1, 32),      # M = 288, 8 slabs
    Shape("f", 2, 6, 5, 1024, 1, 32),       # M = 60, 16 slabs
    Shape("g", 4, 1, 37, 64, 1, 32),        # one image row: two of the three tap rows are always padding
    Shape("h", 2, 2, 2, 128, 2, 32),        # OH = OW = 1
]
BY_NAME = {s.name: s for s in SHAPES}
NAMES = [s.name for s in SHAPES]
SCHEMES = ["f16", "bf16"]       # f16: the operands' amax ride along (KoafGemm.fmt 1); bf16: they are withheld (fmt 0)


def out_hw(s):
    return conv_out(s.H, 3, s.stride, 1), conv_out(s.W, 3, s.stride, 1)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references: one set per shape, computed once, shared by its calls and left unchanged
# ---------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(name):
    """CPU operands of a shape, NHWC: x (mostly positive, so that |a| conv |w| > 0 behind the ReLU of the prologue even where only
    four taps of a two-channel group are inside the image), the packed weight, the prologue (sc, sh), the gradient dy"""
    s = BY_NAME[name]
    g = torch.Generator().manual_seed(9100 + NAMES.index(name))
    Cg = s.C // s.groups
    OH, OW = out_hw(s)

    def rnd(*shape):
        return torch.randn(*shape, generator=g)
    return dict(x=rnd(s.N, s.H, s.W, s.C) * 0.8 + 1.2, w=rnd(s.C, 3, 3, Cg) * (9 * Cg) ** -0.5, sc=rnd(s.C) * 0.2 + 1.0,
                sh=rnd(s.C) * 0.1, dy=rnd(s.N, OH, OW, s.C) * 1e-3)


def prologue(t, dtype):
    return torch.relu(t["x"].to(dtype) * t["sc"].to(dtype) + t["sh"].to(dtype))


@lru_cache(maxsize=None)
def fwd_refs(name, prol):
    """(float64 output, torch's fp32 output of the same operands, |a| conv |w|) [N,OH,OW,C]"""
    s, t = BY_NAME[name], inputs(name)
    a64, a32 = (prologue(t, torch.float64), prologue(t, torch.float32)) if prol else (t["x"].double(), t["x"])
    return (R.gconv64(a64, t["w"], s.stride, s.groups), R.gconv64(a32, t["w"], s.stride, s.groups, dtype=torch.float32),
            R.gconv64(a32.abs(), t["w"].abs(), s.stride, s.groups, dtype=torch.float32).double())


@lru_cache(maxsize=None)
def dgrad_refs(name):
    """(float64 data gradient, torch's fp32 one, |dy| transposed-convolved with |w|) [N,H,W,C]"""
    s, t = BY_NAME[name], inputs(name)
    shape = (s.N, s.H, s.W, s.C)
    return (R.dgrad64(t["dy"], t["w"], shape, s.stride, s.groups), R.dgrad64(t["dy"], t["w"], shape, s.stride, s.groups, dtype=torch.float32),
            R.dgrad64(t["dy"].abs(), t["w"].abs(), shape, s.stride, s.groups, dtype=torch.float32).double())


@lru_cache(maxsize=None)
def wgrad_ref(name):
    s, t = BY_NAME[name], inputs(name)
    return R.wgrad64(t["dy"], prologue(t, torch.float64), s.stride, s.groups)


# ---------------------------------------------------------------------------------------------------------------------------------
# device helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def nan_buf(n, dev):
    return torch.full((n,), float("nan"), device=dev)


def ptr(t):
    return None if t is None else t.data_ptr()


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def slab_weight(dev, w, s, scheme):
    """the expanded weight as the model holds it; bf16: max |w| withheld"""
    from oaprogressionmmf_amd import ops
    wexp = ops.gconv_expand_w(w.to(dev), s.C, s.groups)
    assert float(wexp._koaf_amax) == float(w.abs().max())
    if scheme == "bf16":
        del wexp._koaf_amax
    return wexp


def check_record(tag, launches, M, nz, bm, fmt, act16=0, a_tf=0, b_tf=0, splitk=1, N=64, K=576):
    """the ONE koaf_gemm launch behind a grouped call: block-wide kernel, the forced tile, the slabs as grid.z"""
    assert len(launches) == 1, (tag, launches)
    r = launches[0]
    tiles = cdiv(M, bm) * cdiv(N, 64)
    want = dict(variant="koaf_gemm", bm=bm, bn=64, nbatch=nz, splitk=splitk, M=M, N=N, K=K, tiles=tiles, grid_x=tiles, a_tf=a_tf, b_tf=b_tf,
                fmt=fmt, act16=act16, emit=0)
    assert {f: r[f] for f in want} == want, (tag, r, want)
    return r


def record_line(r):
    return (f"{r['variant']} {r['bm']}x{r['bn']} tiles {r['tiles']} grid.x {r['grid_x']} nbatch {r['nbatch']} splitk {r['splitk']} "
            f"M {r['M']} N {r['N']} K {r['K']} fmt {r['fmt']} tf {r['a_tf']}/{r['b_tf']} act16 {r['act16']}")


def slab_band_errors(out, ref):
    """-> (worst, (slab, band) of the worst, whole tensor): relative L2 per 64-channel slab and 128-row band of out [rows, C] against
    ref (float64)"""
    rows, C = ref.shape
    out = out.detach().double().cpu().reshape(rows, C)
    be = torch.stack([band_errors(out[:, z:z + 64], ref[:, z:z + 64]) for z in range(0, C, 64)])
    assert be.shape == (C // 64, cdiv(rows, 128))            # no slab, no band skipped
    worst, where = be.max().item(), tuple(int(v) for v in torch.unravel_index(be.argmax(), be.shape))
    whole = rel_err(out, ref)
    return worst, where, whole


def hold_guards(tag, buf, n, head):
    """buf went in as NaN: its first n elements are written (and are `head`, the same call through ops), the rest is untouched"""
    assert bool(torch.isnan(buf[n:]).all()), (tag, f"{int((~torch.isnan(buf[n:])).sum())} guard elements written")
    assert not bool(torch.isnan(buf[:n]).any()), (tag, f"{int(torch.isnan(buf[:n]).sum())} of {n} elements not written")
    assert torch.equal(buf[:n], head.reshape(-1)), tag


def tile_statistics(tag, part, y, shift, M, C):
    """part [tiles, 2, C] against the float64 sums of (y - k) and (y - k)^2 over each tile's own rows of the device's y, per slab;
    -> worst (sum, sum of squares) error per (tile, slab) and of the totals"""
    rows = cdiv(M, 128)
    assert tuple(part.shape) == (rows, 2, C), (tag, part.shape)
    p = part.detach().double().cpu()
    assert bool(torch.isfinite(p).all()), tag
    d = y.detach().double().cpu().reshape(M, C)
    if shift is not None:
        d = d - shift.detach().double().cpu()
    worst = [0.0, 0.0]
    for t in range(rows):
        dt = d[128 * t:min(128 * t + 128, M)]
        ref = (dt.sum(0), (dt * dt).sum(0))
        for z in range(0, C, 64):
            for q in range(2):
                e = rel_err(p[t, q, z:z + 64], ref[q][z:z + 64])
                assert e < (SUM, SUMSQ)[q], (tag, f"tile {t} slab {z // 64} {('sum', 'sum of squares')[q]}", e)
                worst[q] = max(worst[q], e)
    tot = (rel_err(p[:, 0].sum(0), d.sum(0)), rel_err(p[:, 1].sum(0), (d * d).sum(0)))
    assert tot[0] < SUM and tot[1] < SUMSQ, (tag, tot)
    return worst, tot


# ---------------------------------------------------------------------------------------------------------------------------------
# the slab images of the weights
# ---------------------------------------------------------------------------------------------------------------------------------
WEIGHT_PAIRS = [(64, 64), (128, 128), (64, 32), (128, 32), (256, 32), (512, 32), (1024, 32), (1024, 16), (64, 1), (192, 3)]


@pytest.mark.parametrize("C,groups", WEIGHT_PAIRS)
def test_gconv_weight_slabs(dev, C, groups):
    """every element of wexp is written and is gconv_refs.expand's (exact zeros off the blocks), amax is max |w|, a NaN in w reaches
    amax; gconv_compress_dw reads the blocks and nothing else"""
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    Cg = C // groups
    g = torch.Generator().manual_seed(7000 + C + groups)
    w = torch.randn(C, 3, 3, Cg, generator=g) * (9 * Cg) ** -0.5
    wd = w.to(dev)
    wexp, amax = nan_buf(C * 9 * 64, dev).reshape(C // 64, 64, 9, 64), torch.zeros(1, device=dev)
    _lib.check(L.koaf_gconv_expand_w(wd.data_ptr(), wexp.data_ptr(), C, groups, amax.data_ptr(), cur_stream()), "gconv_expand_w")
    assert torch.equal(wexp.cpu(), R.expand(w, C, groups)), (C, groups)
    assert float(amax) == float(w.abs().max())
    # without the scalar: the same image
    wexp2 = nan_buf(C * 9 * 64, dev).reshape(C // 64, 64, 9, 64)
    _lib.check(L.koaf_gconv_expand_w(wd.data_ptr(), wexp2.data_ptr(), C, groups, None, cur_stream()), "gconv_expand_w")
    assert torch.equal(wexp2, wexp)
    # gradients come back from the blocks only: the GEMM leaves non-zero products off them
    dwexp = torch.randn(C // 64, 64, 9, 64, generator=g)
    dw = nan_buf(C * 9 * Cg, dev).reshape(C, 3, 3, Cg)
    _lib.check(L.koaf_gconv_compress_dw(dwexp.to(dev).data_ptr(), dw.data_ptr(), C, groups, cur_stream()), "gconv_compress_dw")
    assert torch.equal(dw.cpu(), R.compress(dwexp, C, groups)), (C, groups)
    # a NaN weight is not lost on the way to the scale
    wn = w.clone()
    wn[C // 2, 1, 2, Cg - 1] = float("nan")
    amax.zero_()
    _lib.check(L.koaf_gconv_expand_w(wn.to(dev).data_ptr(), wexp2.data_ptr(), C, groups, amax.data_ptr(), cur_stream()), "gconv_expand_w")
    assert not bool(torch.isfinite(amax).all())
    print(f"\n[gconv] weights C {C:4d} groups {groups:3d} Cg {Cg:2d} | wexp, amax, compressed dw bit-equal to the references")


def test_gconv_weight_slabs_cover_every_group_width():
    assert {C // g for C, g in WEIGHT_PAIRS} == {1, 2, 4, 8, 16, 32, 64}
    assert max(C for C, _ in WEIGHT_PAIRS) == 1024


@pytest.mark.parametrize("C,groups", [(96, 32), (128, 3), (192, 2)])
def test_gconv_weight_slabs_refused(dev, C, groups):
    """C no multiple of 64, groups that do not divide C, a group wider than a slab (Cg = 96)"""
    from oaprogressionmmf_amd import _lib, ops
    Cg = max(C // groups, 1)
    w = torch.zeros(C, 3, 3, Cg, device=dev)
    with pytest.raises(_lib.KoafError):
        ops.gconv_expand_w(w, C, groups)
    with pytest.raises(_lib.KoafError):
        ops.gconv_compress_dw(torch.zeros(cdiv(C, 64), 64, 9, 64, device=dev), torch.empty_like(w), C, groups)


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def direct_fwd(dev, s, xd, wexp, scd, shd, shift, wam, tag, y, part):
    """the same forward through the C ABI into NaN-filled buffers with guard rows behind y and behind the statistics"""
    from oaprogressionmmf_amd import _lib
    OH, OW = out_hw(s)
    M = s.N * OH * OW
    rows = cdiv(M, 128)
    ybuf = nan_buf((M + 128) * s.C, dev) if y.dtype == torch.float32 else nan_buf((M + 128) * s.C, dev).bfloat16()
    pbuf = nan_buf((rows + 1) * 2 * s.C, dev)
    nrow = ctypes.c_int32(-1)
    _lib.check(_lib.lib().koaf_gconv3x3_fwd(xd.data_ptr(), wexp.data_ptr(), ybuf.data_ptr(), s.N, s.H, s.W, s.C, s.stride, ptr(scd), ptr(shd),
                                            pbuf.data_ptr(), ctypes.addressof(nrow), ptr(shift), ptr(wam),
                                            1 if xd.dtype == torch.bfloat16 else 0, cur_stream()), "gconv3x3_fwd")
    torch.cuda.synchronize()
    assert nrow.value == rows, (tag, nrow.value, rows)
    hold_guards(tag + " y", ybuf, M * s.C, y)
    hold_guards(tag + " statistics", pbuf, rows * 2 * s.C, part)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("call", ["plain", "prologue", "prologue+shift"])
@pytest.mark.parametrize("name", NAMES)
def test_gconv_fwd_edges(dev, name, call, scheme):
    """call: plain (in_sc None) | prologue (BatchNorm + ReLU on load, tf 1) | prologue+shift (statistics about 0.98 x the float64
    channel means, as the model passes the running mean); statistics are collected in all three"""
    from oaprogressionmmf_amd import ops
    s, t = BY_NAME[name], inputs(name)
    tag = f"fwd {name} {call} {scheme}"
    OH, OW = out_hw(s)
    M, nz = s.N * OH * OW, s.C // 64
    prol = call != "plain"
    y64, y32, den = fwd_refs(name, prol)
    assert float(den.min()) > 0, tag
    xd, wexp = t["x"].to(dev), slab_weight(dev, t["w"], s, scheme)
    scd, shd = (t["sc"].to(dev), t["sh"].to(dev)) if prol else (None, None)
    shift = (y64.reshape(M, s.C).mean(0) * 0.98).float().to(dev) if call.endswith("shift") else None
    with Record() as rec:
        y, part = ops.gconv3x3_fwd(xd, wexp, s.N, s.H, s.W, s.C, s.stride, scd, shd, stats=True, shift=shift)
    torch.cuda.synchronize()
    r = check_record(tag, rec.launches, M, nz, 128, 1 if scheme == "f16" else 0, a_tf=1 if prol else 0)
    assert r["tiles"] == cdiv(M, 128) == r["grid_x"], (tag, r)
    direct_fwd(dev, s, xd, wexp, scd, shd, shift, getattr(wexp, "_koaf_amax", None), tag, y, part)
    worst, where, whole = slab_band_errors(y, y64.reshape(M, s.C))
    cw, bar = componentwise(y, y64, y32, den)
    print(f"\n[gconv] {tag:30s} {record_line(r)} | worst (slab, band) {worst:.2e} at {where} whole {whole:.2e} | "
          f"componentwise {cw:.2e} (bar {bar:.2e})", end="")
    assert worst < FWD, (tag, where, worst)
    assert whole < FWD, (tag, whole)
    assert cw <= bar, (tag, cw, bar)
    st, tot = tile_statistics(tag, part, y, shift, M, s.C)
    print(f" | tile sums {st[0]:.1e} / squares {st[1]:.1e}, totals {tot[0]:.1e} / {tot[1]:.1e}")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_gconv_fwd_offset_mean(dev, scheme):
    """shape b with channel means several standard deviations from zero (built as test_shifted_batchnorm_statistics builds its
    input): summed about 0.98 x the mean, the ragged last tile (4 of 128 rows) included, the statistics hold per tile and
    koaf_bn_finalize returns mean and invstd at 1e-6 / 2e-6"""
    s = BY_NAME["b"]
    tag = f"fwd b offset-mean {scheme}"
    g = torch.Generator().manual_seed(9200)
    Cg = s.C // s.groups
    x = torch.rand(s.N, s.H, s.W, s.C, generator=g) * 0.02 + 1.0              # nearly constant, positive input
    w = torch.randn(s.C, 3, 3, Cg, generator=g) * 0.01 + 0.05                 # weights with a common positive part
    y64 = R.gconv64(x, w, s.stride, s.groups)
    M = y64.numel() // s.C
    mean_ref, var_ref = y64.reshape(M, s.C).mean(0), y64.reshape(M, s.C).var(0, unbiased=False)
    assert (mean_ref.abs() / var_ref.sqrt()).median() > 3                     # (border pixels keep the std from vanishing)
    from oaprogressionmmf_amd import ops
    xd, wexp = x.to(dev), slab_weight(dev, w, s, scheme)
    shift = (mean_ref * 0.98).float().to(dev)
    with Record() as rec:
        y, part = ops.gconv3x3_fwd(xd, wexp, s.N, s.H, s.W, s.C, s.stride, stats=True, shift=shift)
    torch.cuda.synchronize()
    r = check_record(tag, rec.launches, M, s.C // 64, 128, 1 if scheme == "f16" else 0)
    worst, where, whole = slab_band_errors(y, y64.reshape(M, s.C))
    assert worst < FWD and whole < FWD, (tag, where, worst, whole)
    rm, rv, nbt = shift.clone(), torch.ones(s.C, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    saved = ops.bn_finalize(part, s.C, M, torch.ones(s.C, device=dev), torch.zeros(s.C, device=dev), rm, rv, nbt, 0.1, 1e-5, True, shift=rm)
    em, ei = rel_err(saved[0], mean_ref), rel_err(saved[1], 1.0 / torch.sqrt(var_ref + 1e-5))
    print(f"\n[gconv] {tag:30s} {record_line(r)} | worst (slab, band) {worst:.2e} whole {whole:.2e} | mean {em:.1e} invstd {ei:.1e}", end="")
    assert em < 1e-6 and ei < 2e-6, (tag, em, ei)
    st, tot = tile_statistics(tag, part, y, shift, M, s.C)
    print(f" | tile sums {st[0]:.1e} / squares {st[1]:.1e}, totals {tot[0]:.1e} / {tot[1]:.1e}")


@pytest.mark.parametrize("name", ["b", "c", "f"])
def test_gconv_fwd_bf16_storage(dev, name):
    """x stored as bf16 (act16 1): y is the fp32 mode's on the widened x rounded once, the statistics are the fp32 mode's bits, and
    the call stays on the bf16 scheme whether or not max |w| rides on the weight (koaf.h: "every call with act16 != 0")"""
    from oaprogressionmmf_amd import ops
    s, t = BY_NAME[name], inputs(name)
    tag = f"fwd {name} bf16-storage"
    OH, OW = out_hw(s)
    M, nz = s.N * OH * OW, s.C // 64
    x16 = t["x"].to(dev).bfloat16()
    scd, shd = t["sc"].to(dev), t["sh"].to(dev)
    shift = (fwd_refs(name, True)[0].reshape(M, s.C).mean(0) * 0.98).float().to(dev)
    wexp = slab_weight(dev, t["w"], s, "bf16")
    with Record() as rec32:
        y32, p32 = ops.gconv3x3_fwd(x16.float(), wexp, s.N, s.H, s.W, s.C, s.stride, scd, shd, stats=True, shift=shift)
    with Record() as rec16:
        y16, p16 = ops.gconv3x3_fwd(x16, wexp, s.N, s.H, s.W, s.C, s.stride, scd, shd, stats=True, shift=shift)
    torch.cuda.synchronize()
    check_record(tag + " fp32 mode", rec32.launches, M, nz, 128, 0, act16=0, a_tf=1)
    r = check_record(tag, rec16.launches, M, nz, 128, 0, act16=1, a_tf=1)
    assert y16.dtype == torch.bfloat16 and torch.equal(y16, y32.bfloat16()), tag          # rounded once
    assert torch.equal(p16, p32), tag                                                      # from the fp32 accumulators
    direct_fwd(dev, s, x16, wexp, scd, shd, shift, None, tag, y16, p16)
    # max |w| present: still the bf16 scheme, the same bits
    wam = slab_weight(dev, t["w"], s, "f16")
    with Record() as rec:
        y16a, p16a = ops.gconv3x3_fwd(x16, wam, s.N, s.H, s.W, s.C, s.stride, scd, shd, stats=True, shift=shift)
    torch.cuda.synchronize()
    check_record(tag + " with amax", rec.launches, M, nz, 128, 0, act16=1, a_tf=1)
    assert torch.equal(y16a, y16) and torch.equal(p16a, p16), tag
    print(f"\n[gconv] {tag:30s} {record_line(r)} | bit-equal to the fp32 mode on the widened x, rounded once; statistics bit-equal")


# ---------------------------------------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def run_dgrad(dev, name, scheme, dscale=1.0, wscale=1.0):
    """dscale / wscale: powers of two on dy / w -- the references scale exactly"""
    from oaprogressionmmf_amd import _lib, ops
    s, t = BY_NAME[name], inputs(name)
    tag = f"dgrad {name} {scheme}" + (f" dy x {dscale:g} w x {wscale:g}" if (dscale, wscale) != (1.0, 1.0) else "")
    M, nz = s.N * s.H * s.W, s.C // 64
    g64, g32, den = (v * (dscale * wscale) for v in dgrad_refs(name))
    wexp = slab_weight(dev, t["w"] * wscale, s, scheme)
    dyd = (t["dy"] * dscale).to(dev)
    if scheme == "f16":
        dyd._koaf_amax = dyd.abs().max().reshape(1)
    with Record() as rec:
        dx = ops.gconv3x3_dgrad(dyd, wexp, s.N, s.H, s.W, s.C, s.stride)
    torch.cuda.synchronize()
    r = check_record(tag, rec.launches, M, nz, 128, 1 if scheme == "f16" else 0)         # ONE launch, at stride 2 as well
    # guard rows behind dx
    buf = nan_buf((M + 128) * s.C, dev)
    _lib.check(_lib.lib().koaf_gconv3x3_dgrad(dyd.data_ptr(), wexp.data_ptr(), buf.data_ptr(), s.N, s.H, s.W, s.C, s.stride,
                                              ptr(getattr(wexp, "_koaf_amax", None)), ptr(getattr(dyd, "_koaf_amax", None)), cur_stream()),
               "gconv3x3_dgrad")
    torch.cuda.synchronize()
    hold_guards(tag + " dx", buf, M * s.C, dx)
    if scheme == "bf16":
        # either scalar alone: still the bf16 scheme (ops.gconv3x3_dgrad drops the other), the same bits
        alone_w = slab_weight(dev, t["w"] * wscale, s, "f16")
        alone_dy = dyd.clone()
        alone_dy._koaf_amax = dyd.abs().max().reshape(1)
        for dy_, w_ in ((dyd, alone_w), (alone_dy, wexp)):
            with Record() as rec1:
                dx1 = ops.gconv3x3_dgrad(dy_, w_, s.N, s.H, s.W, s.C, s.stride)
            torch.cuda.synchronize()
            check_record(tag + " one amax", rec1.launches, M, nz, 128, 0)
            assert torch.equal(dx1, dx), tag
    worst, where, whole = slab_band_errors(dx, g64.reshape(M, s.C))
    dxc = dx.cpu()
    unreached = den == 0
    assert bool((dxc[unreached] == 0).all()), (tag, "a pixel no output tap reaches holds a gradient")
    assert bool((g64[unreached] == 0).all()), tag
    cw, bar = componentwise(dx, g64, g32, torch.where(unreached, torch.ones_like(den), den))
    print(f"\n[gconv] {tag:30s} {record_line(r)} | worst (slab, band) {worst:.2e} at {where} whole {whole:.2e} | "
          f"componentwise {cw:.2e} (bar {bar:.2e}) | unreached pixels {int(unreached.sum())}")
    assert worst < BWD, (tag, where, worst)
    assert whole < BWD, (tag, whole)
    assert cw <= bar, (tag, cw, bar)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", NAMES)
def test_gconv_dgrad_edges(dev, name, scheme):
    run_dgrad(dev, name, scheme)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dscale,wscale", [(2.0 ** -20, 2.0 ** 10), (2.0 ** 10, 2.0 ** -20)])
def test_gconv_dgrad_scales(dev, dscale, wscale, scheme):
    """operands far from unit scale (the grouped counterpart of test_fp16_scheme_scales): the scales taken from the two amax
    scalars keep the contraction at the same bars"""
    run_dgrad(dev, "b", scheme, dscale, wscale)


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradient at pixel counts ragged against the k-step (the production plans: test_wgrad_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", ["a", "a-g1", "b", "c", "h"])
def test_gconv_wgrad_small(dev, name, scheme):
    """P = 63, 260, 108 and 2 contracted pixels: slab workspace and dw go in as NaN"""
    from oaprogressionmmf_amd import _lib, ops
    s, t = BY_NAME[name], inputs(name)
    tag = f"wgrad {name} {scheme}"
    OH, OW = out_hw(s)
    P, nz, Cg = s.N * OH * OW, s.C // 64, s.C // s.groups
    ws = _lib.lib().koaf_gconv3x3_wgrad_ws(s.N, s.H, s.W, s.C, s.stride)
    assert ws > 0 and ws % (s.C * 576) == 0, (tag, ws)
    xd, scd, shd = t["x"].to(dev), t["sc"].to(dev), t["sh"].to(dev)
    dyd = t["dy"].to(dev)
    if scheme == "f16":
        dyd._koaf_amax = dyd.abs().max().reshape(1)

    def call():
        slabs = nan_buf(ws, dev)
        with Record() as rec:
            dwexp = ops.gconv3x3_wgrad(dyd, xd, s.N, s.H, s.W, s.C, s.stride, scd, shd, slabs=slabs)
        dw = nan_buf(s.C * 9 * Cg, dev).reshape(s.C, 3, 3, Cg)
        ops.gconv_compress_dw(dwexp, dw, s.C, s.groups)
        torch.cuda.synchronize()
        return dw, dwexp, rec.launches

    dw, dwexp, launches = call()
    r = check_record(tag, launches, 64, nz, 64, 1 if scheme == "f16" else 0, b_tf=1, splitk=ws // (s.C * 576), N=576, K=P)
    assert bool(torch.isfinite(dwexp).all()) and bool(torch.isfinite(dw).all()), (tag, "a block of dw or a split's slab was not written")
    again = call()
    assert torch.equal(again[0], dw) and torch.equal(again[1], dwexp), (tag, "split-K is deterministic")
    dw64 = wgrad_ref(name)
    errs = [rel_err(dw[z:z + 64], dw64[z:z + 64]) for z in range(0, s.C, 64)]
    whole = rel_err(dw, dw64)
    print(f"\n[gconv] {tag:30s} {record_line(r)} | worst slab {max(errs):.2e} at {errs.index(max(errs))} whole {whole:.2e}")
    assert max(errs) < BWD, (tag, errs)
    assert whole < BWD, (tag, whole)
