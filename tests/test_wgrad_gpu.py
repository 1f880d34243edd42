"""Weight-gradient parity at the split-K plans and tiles production reaches.

The weight gradients are the only contractions that run split-K (koaf_conv.hip wgrad_plan: about 1024 blocks, >= 512 k-rows per
split, multiples of 8 past 8 splits).  With gridDim.y % 8 == 0 koaf_gemm_kernel remaps (blockIdx.x, blockIdx.y) to (tile, split)
so that a k-range stays on one XCD; the k-range is kchunk = roundup32(ceil(K / splitk)), so trailing splits can be short or EMPTY
and must still deliver a zero slab; koaf_slab_reduce folds in two levels once there are >= 64 slabs of a small output.  The small
shapes of test_kernels_gpu.py stay at <= 3 splits (one exception: 200 splits of one 64 x 64 tile, K an exact multiple).  Every
row of WGRAD_CASES goes through ops.conv2d_wgrad / ops.gconv3x3_wgrad + ops.gconv_compress_dw as the model calls them and
ASSERTS FROM THE LAUNCH RECORD (koaf.h koaf_launch_log) the variant, tile, split count, batch, scheme, loader transforms and
storage mode that served it: a row that lands elsewhere fails.  tests/test_wgrad_plan_cpu.py asks the library for the same split
counts on any machine and derives each row's remap / empty-split claims from them.

Bars (owned by the module docstrings of test_kernels_gpu.py and test_tiles_gpu.py; nothing new is invented):
  * relative L2 against the float64 CPU weight gradient (torch's convolution backward) over the whole tensor and PER OUTPUT BLOCK
    of dw -- every 64-row band of Cout x every filter tap x every 64-column band of Cin -- and per tap: BWD = 4e-6.  A fault in one
    split of one tile moves a whole-tensor norm by 1 / sqrt(blocks).
  * componentwise: max |dw - dw64| / (|dy|^T |x|) <= 8 x the same ratio of torch's fp32 CPU product of the same operands (the
    loader transforms evaluated in fp32 as well), computed in the test.
  * bf16 activation storage (act16 3): the property of test_bf16_gpu.py -- dw is bit-equal to the fp32-storage call on the widened
    inputs.  Both operands from plane images (kind 3): bit-equal to the fp32-loader call, as
    test_bn_backward_apply_formed_in_the_gemm_loaders states at small size.
  * "deterministic split-K" (koaf.h): the same call twice gives torch.equal results.
dw AND the slab workspace (sized by koaf_conv2d_wgrad_ws / koaf_gconv3x3_wgrad_ws, handed in through `slabs=`) are pre-filled with
NaN: a block that is not written, or an empty split that does not deliver its zero slab, shows as a NaN in dw.
A dy that is a BatchNorm-backward apply (ops.BnApply, KoafOperand.tf 2) is held to the float64 product of
dy64 = coef0 * dz + coef3 - coef2 * c formed from the coefficients the device left, as test_tiles_gpu.py does.

Each case prints one table line: variant / tile / tiles / splitk / empty splits from the record and the plan, worst block error,
componentwise ratio and bar."""
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

from test_tiles_gpu import BWD, Record, componentwise, conv_out, n_tiles, rel_err

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "name kind shape call store variant bm bn splitk remap empty")
# kind   "dense"   ops.conv2d_wgrad(aplanes=False): fp32 K-major loaders -- production for every 1x1 and every stride-2 convolution
#        "planes"  ops.conv2d_wgrad(aplanes=True): both operands from plane images, K-major (KoafOperand.kind 3)
#        "ring"    the same call at 3x3 / stride 1 / pad 1 shapes: the padded-raster ring kernel (koaf_wgrad3.hip) where it takes them
#        "grouped" ops.gconv3x3_wgrad + ops.gconv_compress_dw (32 groups), the C / 64 slabs as the batch dimension
# shape  (N, H, W, Cin, Cout, k, stride, pad); grouped: (N, H, W, C, stride)
# call   plain (dy + its amax: fp16 scheme) | apply_prologue (dy an ops.BnApply -- tf 2 on the K-major A operand --, x behind its
#        BatchNorm prologue -- tf 1 on the K-major B operand: the production combination) | bf16scheme (amax withheld: fmt 0) |
#        prologue (dy + amax, x behind its prologue)
# store  "fp32" (against float64) | "bf16" (x and the apply's c stored as bf16, act16 3: against the fp32 mode on widened inputs)
# variant / bm / bn / splitk: what the launch record must show (splitk = the record's grid.y; ring: its k-range count)
# remap  the kernel's XCD remap of (blockIdx.x, blockIdx.y) runs: splitk > 1 and splitk % 8 == 0
# empty  trailing splits (ring: k-ranges) that start past K and deliver a zero slab
G, RING = "koaf_gemm", "koaf_wgrad3/ring"
GROUPS = 32

W1 = (9, 31, 31, 64, 256, 1, 1, 0)       # P = 8649 = 9 mod 32: 16 splits of 544 rows, the last one 489; 2 tiles 128 x 64
W2 = (9, 31, 31, 256, 64, 1, 1, 0)       # the transposed tile 64 x 128
W3 = (8, 63, 61, 256, 512, 1, 2, 0)      # stride-2 downsample, odd H and W: P = 7936, 8 tiles 128 x 128, 16 splits
W4 = (5, 63, 61, 128, 128, 3, 2, 1)      # P = 4960, 9 tiles: gathered B, one tap per column tile; 8 splits
W5 = (5, 63, 61, 64, 128, 3, 2, 1)       # 5 tiles: a B tile spans two filter taps
W6 = (9, 20, 20, 512, 2048, 1, 1, 0)     # P = 3600, 64 tiles per split under the remap, 8 splits
W7 = (5, 25, 25, 1024, 256, 1, 1, 0)     # P = 3125 = 21 mod 32, 16 tiles, 7 splits: no remap, the `decode` path
W8 = (44, 29, 29, 64, 64, 1, 1, 0)       # P = 37004 = 12 mod 32: 72 splits of 544 rows, split 68 has 12 rows, 69-71 are empty; two-level
#                                          reduce, 72 slabs over 16 groups (5 each, the last group empty)
P1 = (25, 12, 12, 512, 512, 3, 1, 1)     # layer4 of the 384^2 slices: the ring refuses W < 16; P = 3600, 144 tiles, 7 splits
P2 = (36, 10, 10, 512, 512, 3, 1, 1)     # layer4 of the 310^2 radiograph
G1 = (6, 40, 40, 128, 1)                 # P = 9600, 2 slabs, 16 splits
G2 = (8, 61, 63, 256, 2)                 # P = 7936, 4 slabs, 16 splits
G3 = (8, 31, 31, 512, 1)                 # P = 7688 = 8 mod 32, 8 slabs, 16 splits, the last one 8 rows
R1 = (4, 9, 61, 64, 64, 3, 1, 1)         # last width of wgrad3x3_ring_kernel<8>
R2 = (4, 9, 62, 64, 64, 3, 1, 1)         # first width of <16>
R3 = (1, 4, 189, 64, 64, 3, 1, 1)        # last width the ring takes
R4 = (1, 4, 190, 64, 64, 3, 1, 1)        # first width it refuses: the K-major GEMM, 5 tiles 64 x 128, 2 splits
R5 = (40, 24, 24, 128, 64, 3, 1, 1)      # 845 chunks over 512 k-ranges (two (co, ci) tiles): ranges of two chunks, one of one, 89 empty

WGRAD_CASES = [
    # ---- dense, fp32 K-major loaders
    Case("w1-plain", "dense", W1, "plain", "fp32", G, 128, 64, 16, True, 0),
    Case("w1-apply_prologue", "dense", W1, "apply_prologue", "fp32", G, 128, 64, 16, True, 0),
    Case("w1-bf16scheme", "dense", W1, "bf16scheme", "fp32", G, 128, 64, 16, True, 0),
    Case("w1-apply_prologue-bf16", "dense", W1, "apply_prologue", "bf16", G, 128, 64, 16, True, 0),
    Case("w2-plain", "dense", W2, "plain", "fp32", G, 64, 128, 16, True, 0),
    Case("w2-apply_prologue", "dense", W2, "apply_prologue", "fp32", G, 64, 128, 16, True, 0),
    Case("w2-bf16scheme", "dense", W2, "bf16scheme", "fp32", G, 64, 128, 16, True, 0),
    Case("w3-plain", "dense", W3, "plain", "fp32", G, 128, 128, 16, True, 0),
    Case("w3-apply_prologue", "dense", W3, "apply_prologue", "fp32", G, 128, 128, 16, True, 0),
    Case("w3-bf16scheme", "dense", W3, "bf16scheme", "fp32", G, 128, 128, 16, True, 0),
    Case("w3-apply_prologue-bf16", "dense", W3, "apply_prologue", "bf16", G, 128, 128, 16, True, 0),
    Case("w4-plain", "dense", W4, "plain", "fp32", G, 128, 128, 8, True, 0),
    Case("w4-apply_prologue", "dense", W4, "apply_prologue", "fp32", G, 128, 128, 8, True, 0),
    Case("w4-apply_prologue-bf16", "dense", W4, "apply_prologue", "bf16", G, 128, 128, 8, True, 0),
    Case("w5-plain", "dense", W5, "plain", "fp32", G, 128, 128, 8, True, 0),
    Case("w5-apply_prologue", "dense", W5, "apply_prologue", "fp32", G, 128, 128, 8, True, 0),
    Case("w6-plain", "dense", W6, "plain", "fp32", G, 128, 128, 8, True, 0),
    Case("w6-apply_prologue", "dense", W6, "apply_prologue", "fp32", G, 128, 128, 8, True, 0),
    Case("w6-bf16scheme", "dense", W6, "bf16scheme", "fp32", G, 128, 128, 8, True, 0),
    Case("w7-plain", "dense", W7, "plain", "fp32", G, 128, 128, 7, False, 0),
    Case("w7-apply_prologue", "dense", W7, "apply_prologue", "fp32", G, 128, 128, 7, False, 0),
    Case("w7-bf16scheme", "dense", W7, "bf16scheme", "fp32", G, 128, 128, 7, False, 0),
    Case("w8-plain", "dense", W8, "plain", "fp32", G, 64, 64, 72, True, 3),
    Case("w8-apply_prologue", "dense", W8, "apply_prologue", "fp32", G, 64, 64, 72, True, 3),
    Case("w8-bf16scheme", "dense", W8, "bf16scheme", "fp32", G, 64, 64, 72, True, 3),
    # ---- dense, both operands from plane images, K-major (kind 3)
    Case("p1-plain", "planes", P1, "plain", "fp32", G, 128, 128, 7, False, 0),
    Case("p1-apply_prologue", "planes", P1, "apply_prologue", "fp32", G, 128, 128, 7, False, 0),
    Case("p2-plain", "planes", P2, "plain", "fp32", G, 128, 128, 7, False, 0),
    Case("p2-apply_prologue", "planes", P2, "apply_prologue", "fp32", G, 128, 128, 7, False, 0),
    Case("p3-apply_prologue", "planes", W3, "apply_prologue", "fp32", G, 128, 128, 16, True, 0),      # 1x1 / stride 2 as the one-tap gather
    # ---- grouped (ResNeXt), the prologue on x
    Case("g1-f16", "grouped", G1, "prologue", "fp32", G, 64, 64, 16, True, 0),
    Case("g1-bf16scheme", "grouped", G1, "bf16scheme", "fp32", G, 64, 64, 16, True, 0),
    Case("g2-f16", "grouped", G2, "prologue", "fp32", G, 64, 64, 16, True, 0),
    Case("g2-bf16scheme", "grouped", G2, "bf16scheme", "fp32", G, 64, 64, 16, True, 0),
    Case("g2-bf16scheme-bf16", "grouped", G2, "bf16scheme", "bf16", G, 64, 64, 16, True, 0),      # (every grouped act16 call: the bf16 scheme)
    Case("g3-f16", "grouped", G3, "prologue", "fp32", G, 64, 64, 16, True, 0),
    Case("g3-bf16scheme", "grouped", G3, "bf16scheme", "fp32", G, 64, 64, 16, True, 0),
    # ---- the ring kernel and its width edges
    Case("r1-ring8-w61", "ring", R1, "prologue", "fp32", RING, 64, 64, 87, False, 0),
    Case("r2-ring16-w62", "ring", R2, "prologue", "fp32", RING, 64, 64, 88, False, 0),
    Case("r3-ring16-w189", "ring", R3, "prologue", "fp32", RING, 64, 64, 36, False, 0),
    Case("r4-refused-w190", "ring", R4, "prologue", "fp32", G, 64, 128, 2, False, 0),
    Case("r5-ring8-ranges", "ring", R5, "prologue", "fp32", RING, 64, 64, 512, False, 89),
]
SHAPES = [W1, W2, W3, W4, W5, W6, W7, W8, P1, P2, G1, G2, G3, R1, R2, R3, R4, R5]


# ---------------------------------------------------------------------------------------------------------------------------------
# plan arithmetic (no GPU; tests/test_wgrad_plan_cpu.py holds every row's claims against it and against the library)
# ---------------------------------------------------------------------------------------------------------------------------------
def dims(case):
    """(M, N, P) of the weight-gradient GEMM behind a row: M x N output, P = N * OH * OW contracted pixels (grouped: per 64-channel slab)"""
    if case.kind == "grouped":
        N, H, W, C, s = case.shape
        return 64, 576, N * conv_out(H, 3, s, 1) * conv_out(W, 3, s, 1)
    N, H, W, Cin, Cout, k, s, p = case.shape
    return Cout, k * k * Cin, N * conv_out(H, k, s, p) * conv_out(W, k, s, p)


def split_geometry(K, splitk):
    """(kchunk, empty trailing splits, rows of the last live split) of koaf_gemm_kernel's k-ranges: kchunk = roundup32(ceil(K / splitk))"""
    kchunk = (-(-K // splitk) + 31) // 32 * 32
    live = -(-K // kchunk)
    return kchunk, splitk - live, K - (live - 1) * kchunk


def ring_geometry(case):
    """(reach D, chunks, k-ranges nk, (co, ci) tiles, empty k-ranges) of koaf_wgrad3.hip for a 3x3 / stride 1 / pad 1 row: positions
    of the padded raster in 32-position chunks, about 1024 blocks in whole multiples of 8 k-ranges, never more ranges than chunks"""
    N, H, W, Cin, Cout = case.shape[:5]
    D = (W + 2 + 1 + 31) >> 5
    nchunk = -(-N * (H + 2) * (W + 2) // 32)
    ncomb = (Cout // 64) * (Cin // 64)
    nk = min(max(1024 // ncomb, 8) & ~7, nchunk)
    per = -(-nchunk // nk)
    return D, nchunk, nk, ncomb, nk - -(-nchunk // per)


def ring_takes(case):
    """koaf_wgrad3_ring_ok: W >= 16 and the reach of a tap, 2 D + 3 chunks, within the 16-chunk LDS ring"""
    N, H, W, Cin, Cout, k, s, p = case.shape
    D = (W + 2 + 1 + 31) >> 5
    return (k, s, p) == (3, 1, 1) and W >= 16 and 2 * D + 3 <= 16 and D * 32 + 32 < (H + 2) * (W + 2) and (Cout // 64) * (Cin // 64) <= 64


def two_level_reduce(nslab, n):
    """koaf_slab_reduce folds nslab slabs of n floats through 16 partial slabs"""
    return nslab >= 64 and -(-(n // 4) // 64) < 256


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references: one set per shape, shared by its calls
# ---------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=2)
def inputs(shape):
    """CPU operands of a shape, NHWC: x, its prologue (sc, sh), the gradient dy, and the conv output c / upstream gradient g / affine
    parameters of the BatchNorm whose backward an apply row forms on load"""
    g_ = torch.Generator().manual_seed(8000 + SHAPES.index(shape))

    def rnd(*s):
        return torch.randn(*s, generator=g_)
    if len(shape) == 5:
        N, H, W, Cin, s = shape
        Cout, k, p = Cin, 3, 1
    else:
        N, H, W, Cin, Cout, k, s, p = shape
    OH, OW = conv_out(H, k, s, p), conv_out(W, k, s, p)
    return dict(x=rnd(N, H, W, Cin) * 1.5 + 0.3, sc=rnd(Cin) * 0.2 + 1.0, sh=rnd(Cin) * 0.1, dy=rnd(N, OH, OW, Cout) * 1e-3,
                c=rnd(N, OH, OW, Cout) * 1.5 + 0.3, g=rnd(N, OH, OW, Cout) * 1e-3, gam=rnd(Cout) * 0.2 + 1.0, bet=rnd(Cout) * 0.1)


def wgrad_cpu(dy, a, shape):
    """the weight gradient torch's autograd computes for F.conv2d, packed [Cout, k, k, Cin / groups]; dy [N,OH,OW,Cout], a [N,H,W,Cin]"""
    if len(shape) == 5:
        (N, H, W, Cin, s), Cout, k, p, groups = shape, shape[3], 3, 1, GROUPS
    else:
        (N, H, W, Cin, Cout, k, s, p), groups = shape, 1
    dw = torch.nn.grad.conv2d_weight(a.permute(0, 3, 1, 2), (Cout, Cin // groups, k, k), dy.permute(0, 3, 1, 2), stride=s, padding=p,
                                     groups=groups)
    return dw.permute(0, 2, 3, 1).contiguous()


def references(dy32, a32, dy64, a64, shape):
    """(float64 gradient, torch's fp32 gradient of the same operands, |dy|^T |x|)"""
    return wgrad_cpu(dy64, a64, shape), wgrad_cpu(dy32, a32, shape), wgrad_cpu(dy32.abs(), a32.abs(), shape).double() + 1e-300


@lru_cache(maxsize=2)
def tensor_references(shape, prologue):
    """the references of the calls whose dy is the shape's dy tensor: shared by plain / bf16scheme (and prologue / bf16scheme of a
    grouped or ring shape)"""
    t = inputs(shape)
    x, sc, sh = t["x"], t["sc"], t["sh"]
    a32 = torch.relu(x * sc + sh) if prologue else x
    a64 = torch.relu(x.double() * sc.double() + sh.double()) if prologue else x.double()
    return references(t["dy"], a32, t["dy"].double(), a64, shape)


def block_errors(dw, ref):
    """relative L2 error of every output block of dw [Cout, taps, Cin] against ref (float64): 64-row band of Cout x tap x 64-column band
    of Cin (a narrower Cin: one band) -> [bands, taps, column bands]"""
    Cout, taps, Cin = ref.shape
    cb = min(64, Cin)
    assert Cout % 64 == 0 and Cin % cb == 0
    d = dw.detach().double().cpu().reshape(ref.shape)

    def blocks(t):
        return (t ** 2).reshape(Cout // 64, 64, taps, Cin // cb, cb).sum((1, 4))
    e2, r2 = blocks(d - ref), blocks(ref)
    assert e2.shape == (Cout // 64, taps, Cin // cb) and e2.numel() * 64 * cb == ref.numel()        # no block skipped
    return (e2 / (r2 + 1e-300)).sqrt(), (e2.sum((0, 2)) / (r2.sum((0, 2)) + 1e-300)).sqrt()


def check_record(case, launches, act16):
    """the one launch behind the call is on the variant / tile / split count / batch / scheme / transforms the row is there for"""
    assert len(launches) == 1, (case.name, launches)
    r = launches[0]
    M, Ng, P = dims(case)
    apply_, prol = case.call == "apply_prologue", case.call in ("apply_prologue", "prologue") or case.kind == "grouped"
    want = dict(variant=case.variant, bm=case.bm, bn=case.bn, splitk=case.splitk, M=M, N=Ng, fmt=0 if case.call == "bf16scheme" else 1,
                act16=act16, emit=0, nbatch=case.shape[3] // 64 if case.kind == "grouped" else 1)
    if case.variant == RING:
        D, nchunk, nk, ncomb, empty = ring_geometry(case)
        N, H, W = case.shape[:3]
        want.update(tiles=ncomb, grid_x=-(-nk // 8) * 8 * ncomb, K=N * (H + 2) * (W + 2), a_tf=0, b_tf=0)
    else:
        fp32_loaders = case.kind in ("dense", "grouped")          # (plane images: the transforms are in the images)
        want.update(tiles=n_tiles(M, Ng, case.bm, case.bn), grid_x=n_tiles(M, Ng, case.bm, case.bn), K=P,
                    a_tf=2 if apply_ and fp32_loaders else 0, b_tf=1 if prol and fp32_loaders else 0)
    got = {f: r[f] for f in want}
    assert got == want, (case.name, r, want)
    return r


def report(case, r, empty, tail):
    print(f"\n[wgrad] {case.name:24s} {r['variant']:17s} {r['bm']:3d}x{r['bn']:<3d} tiles {r['tiles']:3d} splitk {r['splitk']:3d} empty {empty:2d} "
          f"nbatch {r['nbatch']} fmt {r['fmt']} tf {r['a_tf']}/{r['b_tf']} act16 {r['act16']} | {tail}")


def nan_like(n, dev):
    return torch.full((n,), float("nan"), device=dev)


def all_written(case, dw):
    """dw and the slab workspace went in as NaN: a tile that was never stored, or a split whose slab was not delivered, is still there"""
    bad = ~torch.isfinite(dw)
    assert not bool(bad.any()), (case.name, f"{int(bad.sum())} of {dw.numel()} elements: a block of dw or a split's slab was not written")


def hold(case, r, empty, dw, refs):
    """the float64 bars on a finished gradient dw [Cout, k, k, Cin]"""
    dw64, dw32, den = refs
    flat = dw64.reshape(dw64.shape[0], -1, dw64.shape[-1])
    be, tap = block_errors(dw, flat)
    whole = rel_err(dw, dw64)
    cw, bar = componentwise(dw, dw64, dw32, den)
    where = tuple(int(v) for v in torch.unravel_index(be.argmax(), be.shape))
    report(case, r, empty, f"worst block {be.max().item():.2e} at (band, tap, cin band) {where} whole {whole:.2e} | componentwise {cw:.2e} (bar {bar:.2e})")
    assert whole < BWD, (case.name, whole)
    assert be.max().item() < BWD, (case.name, where, be.max().item())
    assert tap.max().item() < BWD, (case.name, int(tap.argmax()), tap.max().item())       # every tap on its own
    assert cw <= bar, (case.name, cw, bar)


def run_conv(dev, case):
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout, k, s, p = case.shape
    OH, OW = conv_out(H, k, s, p), conv_out(W, k, s, p)
    orow = N * OH * OW
    t = inputs(case.shape)
    b16, use_apply = case.store == "bf16", case.call == "apply_prologue"
    prol = case.call in ("apply_prologue", "prologue")
    aplanes = case.kind != "dense"
    x, c = t["x"], t["c"]
    if b16:
        x, c = x.bfloat16().float(), c.bfloat16().float()
    scd, shd = (t["sc"].to(dev), t["sh"].to(dev)) if prol else (None, None)
    gam, bet = t["gam"].to(dev), t["bet"].to(dev)
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, k, k, s, p)
    assert ws > 0, case.name

    def operands(store16):
        def act(v):
            return v.to(dev).bfloat16() if store16 else v.to(dev)
        if not use_apply:
            dyd = t["dy"].to(dev)
            return act(x), dyd, (dyd.abs().max().reshape(1).float() if case.call != "bf16scheme" else None)
        cc = act(c)
        sv = ops.bn_finalize(ops.colstats(cc, orow, Cout), Cout, orow, gam, bet, torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev),
                             torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)
        dgm, dbt = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
        return act(x), ops.bn_bwd(t["g"].to(dev), cc, sv, orow, Cout, orow, dgm, dbt, 2, fused=True), None

    def call(xd, arg, am, ap):
        dw, slabs = nan_like(Cout * k * k * Cin, dev).reshape(Cout, k, k, Cin), nan_like(ws, dev)
        with Record() as rec:
            ops.conv2d_wgrad(arg, xd, dw, N, H, W, Cin, Cout, k, k, s, p, scd, shd, dy_amax=am, aplanes=ap, slabs=slabs)
        torch.cuda.synchronize()
        return dw, rec.launches

    xd, arg, am = operands(b16)
    dw, launches = call(xd, arg, am, aplanes)
    r = check_record(case, launches, 3 if b16 else 0)
    empty = ring_geometry(case)[4] if case.variant == RING else split_geometry(orow, r["splitk"])[1]
    assert empty == case.empty, (case.name, empty)
    all_written(case, dw)
    assert torch.equal(call(xd, arg, am, aplanes)[0], dw), (case.name, "split-K is deterministic")
    if case.kind == "planes":
        assert torch.equal(call(xd, arg, am, False)[0], dw), (case.name, "the fp32 K-major loaders form the same bits")
    if b16:
        x32, arg32, am32 = operands(False)
        dw32, l32 = call(x32, arg32, am32, aplanes)
        assert l32[0]["act16"] == 0 and torch.equal(dw, dw32), case.name
        report(case, r, empty, "bit-equal to the fp32 mode on widened inputs")
        return
    if use_apply:
        coef, c32 = arg.coef.double().cpu(), arg.coef.cpu()
        dy64 = coef[0] * arg.dz.double().cpu() + coef[3] - coef[2] * arg.c.double().cpu()
        dy32 = c32[0] * arg.dz.cpu() + c32[3] - c32[2] * arg.c.float().cpu()
        a32 = torch.relu(x * t["sc"] + t["sh"])
        a64 = torch.relu(x.double() * t["sc"].double() + t["sh"].double())
        refs = references(dy32.reshape(N, OH, OW, Cout), a32, dy64.reshape(N, OH, OW, Cout), a64, case.shape)
    else:
        refs = tensor_references(case.shape, prol)
    hold(case, r, empty, dw, refs)


def run_grouped(dev, case):
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, C, s = case.shape
    Cg = C // GROUPS
    t = inputs(case.shape)
    b16 = case.store == "bf16"
    x = t["x"].bfloat16().float() if b16 else t["x"]
    scd, shd = t["sc"].to(dev), t["sh"].to(dev)
    ws = _lib.lib().koaf_gconv3x3_wgrad_ws(N, H, W, C, s)

    def call(store16):
        xd, dyd = (x.to(dev).bfloat16() if store16 else x.to(dev)), t["dy"].to(dev)
        if case.call != "bf16scheme":
            dyd._koaf_amax = dyd.abs().max().reshape(1)
        slabs = nan_like(ws, dev)
        with Record() as rec:
            dwexp = ops.gconv3x3_wgrad(dyd, xd, N, H, W, C, s, scd, shd, slabs=slabs)
        dw = nan_like(C * 9 * Cg, dev).reshape(C, 3, 3, Cg)
        ops.gconv_compress_dw(dwexp, dw, C, GROUPS)
        torch.cuda.synchronize()
        return dw, dwexp, rec.launches

    dw, dwexp, launches = call(b16)
    r = check_record(case, launches, 3 if b16 else 0)
    empty = split_geometry(dims(case)[2], r["splitk"])[1]
    assert empty == case.empty, (case.name, empty)
    all_written(case, dwexp)
    all_written(case, dw)
    again = call(b16)
    assert torch.equal(again[0], dw) and torch.equal(again[1], dwexp), (case.name, "split-K is deterministic")
    if b16:
        dw32, dwexp32, l32 = call(False)
        assert l32[0]["act16"] == 0 and l32[0]["fmt"] == 0 and torch.equal(dw, dw32) and torch.equal(dwexp, dwexp32), case.name
        report(case, r, empty, "bit-equal to the fp32 mode of the bf16 scheme on widened inputs")
        return
    hold(case, r, empty, dw, tensor_references(case.shape, True))


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c.name for c in WGRAD_CASES])
def test_weight_gradient_split_plans(dev, case):
    try:
        (run_grouped if case.kind == "grouped" else run_conv)(dev, case)
    finally:
        torch.cuda.empty_cache()


def test_slab_workspace_too_small_raises(dev):
    """ops.conv2d_wgrad / ops.gconv3x3_wgrad / ops.stem_wgrad refuse a `slabs=` workspace under koaf_conv2d_wgrad_ws /
    koaf_gconv3x3_wgrad_ws / koaf_stem_wgrad_ws floats"""
    from oaprogressionmmf_amd import _lib, ops
    N, H, W, Cin, Cout = 4, 16, 16, 64, 64
    x, dy = torch.zeros(N, H, W, Cin, device=dev), torch.zeros(N, H, W, Cout, device=dev)
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, 1, 1, 1, 0)
    assert ws > 0
    with pytest.raises(_lib.KoafError):
        ops.conv2d_wgrad(dy, x, torch.empty(Cout, 1, 1, Cin, device=dev), N, H, W, Cin, Cout, 1, 1, 1, 0, slabs=torch.empty(ws - 1, device=dev))
    wg = _lib.lib().koaf_gconv3x3_wgrad_ws(N, H, W, Cin, 1)
    with pytest.raises(_lib.KoafError):
        ops.gconv3x3_wgrad(dy, x, N, H, W, Cin, 1, slabs=torch.empty(wg - 1, device=dev))
    wst = _lib.lib().koaf_stem_wgrad_ws(N, H, W)
    assert wst > 0
    with pytest.raises(_lib.KoafError):
        ops.stem_wgrad(torch.zeros(N, H // 2, W // 2, 64, device=dev), torch.zeros(N, H, W, device=dev), torch.empty(64, 7, 7, 3, device=dev),
                       N, H, W, slabs=torch.empty(wst - 1, device=dev))
