"""Band-wise parity of the transformer-side contractions: the plans of koaf_linear.hip and the GEMM chains of koaf_attention.hip.

These calls run koaf_gemm instantiations no convolution touches -- the K-contiguous x K-contiguous and K-major x K-major pairs
on the bf16 x 3 scheme, batch strides, alpha, the bias / residual epilogue, the whole scalar kernel set (VEC = false) -- behind
plan logic of their own: linear_tile, linear_splitk (1 to 8 splits, the XCD remap when the count is a multiple of 8),
koaf_slab_reduce_epilogue, the three narrow-head kernels and their N <= 8 && M * N <= 4096 && K >= 64 boundary.  test_linear /
test_attention (test_kernels_gpu.py) hold one whole-tensor norm per result.  Every row of LINEAR_ROWS states, for the forward
and for the data gradient, the narrow head or the GEMM's tile and split count, and ASSERTS it from the launch record
(koaf.h koaf_launch_log; a narrow head leaves no record): a row that lands elsewhere fails.  tests/test_linear_plan_cpu.py asks the
library for the same split counts on any machine.

Bars (owned by the module docstrings of test_kernels_gpu.py, test_tiles_gpu.py and test_elem_edges_gpu.py; nothing new is invented):
  * relative L2 against the float64 CPU result over the whole tensor and PER BAND: 2e-6 forward, BWD = 4e-6 gradients, 2 BWD the
    attention backward.  Bands: 64 output rows x 128 columns (Linear forward and data gradient), 64 x 64 blocks of dw, the
    (batch, head, 32-query tile) of attn / out, the (batch, head, 64-row band) of each of dq, dk, dv on its own.
  * componentwise (Linear): max |y - y64| / (|a| @ |b| (+ |bias| + |residual|)) <= max(8 x the same ratio of torch's fp32 CPU
    result on the same operands, the norm bar of that result).
  * results through expf (attention): the 4 x yardstick rule of test_elem_edges_gpu.py per element, floor = the norm bar times
    max |ref|.
The Linear outputs AND the split-K workspace go in as NaN (the entry points are called as ops.linear_* call them, with buffers of
the test's own): a tile that is not stored, or a split whose slab is not delivered, shows as NaN.

koaf_attention_bwd is four koaf_gemm launches (dV, dP, dQ, dK; the softmax backward between them is a row kernel of its own): the
record must show four, each batched over B * h.  At n = 483 all four run on the scalar loaders (a leading dimension of 483).

Each case prints one table line with the geometry from the record and the achieved figures.

Measured on an MI355X (they document; every bar is computed in the test), worst over the cases:
  Linear     forward block 7.74e-07 (966 x 6144 x 2048, unsplit), data gradient 7.43e-07 (8 x 2048 x 514, scalar kernels, one 2048-long
             k-loop), dw block 9.05e-07 (3000 x 2048 x 512); the split rows stay at 1.3e-07 .. 3.9e-07, the scalar-kernel split-K rows
             (8 x 2048 x 514 forward, 8 x 514 x 2048 data gradient) at 2.6e-07 / 2.8e-07; componentwise <= 3.4e-07 (bars 2e-06 / 4e-06)
  attention  attn tile 1.58e-07, out tile 4.75e-07 (1 x 513 x 2 x 32), dq / dk / dv band 4.62e-07 / 4.58e-07 / 4.17e-07 (bar 8e-06);
             per element the kernels are within 0.6 .. 2.2 x torch's fp32 error (the rule allows 4 x)."""
from collections import namedtuple
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F

from test_elem_edges_gpu import yardstick
from test_tiles_gpu import BWD, FWD, Record, componentwise, rel_err

pytestmark = pytest.mark.gpu

HEAD = "head"
Row = namedtuple("Row", "M N K fwd dgrad")
# fwd / dgrad: HEAD (the direct narrow-head kernel: no koaf_gemm launch) or (bm, bn, splitk) of the one koaf_gemm launch.  The data
# gradient's GEMM is M x K over N.  An unaligned call (N % 4 or K % 4) runs the scalar kernels: always 64 x 64.
LINEAR_ROWS = [
    Row(8, 2048, 2048, (64, 128, 8), (64, 128, 8)),         # few rows: 64 x 128 tile, 8 splits -- the XCD remap runs
    Row(8, 2048, 1024, (64, 128, 4), (64, 128, 8)),         # K / splits >= 256: 4 splits
    Row(8, 2048, 600, (64, 128, 2), (64, 64, 8)),           # 2 splits, 320 + 280
    Row(200, 512, 1500, (64, 64, 5), (64, 128, 2)),         # 64 x 64 tile, 5 splits, the last 220
    Row(966, 2048, 2048, (128, 128, 4), (128, 128, 4)),     # two volumes of 483 tokens: 128 x 128 tile, 4 splits, ragged last row tile
    Row(966, 6144, 2048, (128, 128, 1), (128, 128, 4)),     # the qkv projection: forward unsplit
    Row(3000, 2048, 512, (128, 128, 1), (128, 128, 5)),     # dgrad 5 splits of 416, the last 384
    Row(8, 2048, 514, (64, 64, 2), (64, 64, 1)),            # K % 4 != 0: SPLIT-K ON THE SCALAR KERNELS, 288 + 226
    Row(8, 514, 2048, (64, 64, 1), (64, 64, 2)),            # ... and in the data gradient
    Row(129, 130, 36, (64, 64, 1), (64, 64, 1)),            # scalar kernels, unsplit, ragged tiles both ways
    Row(8, 2, 64, HEAD, HEAD), Row(8, 2, 65, HEAD, HEAD), Row(512, 8, 128, HEAD, HEAD),                  # the head boundary: inside
    Row(8, 2, 63, (64, 64, 1), (64, 64, 1)), Row(513, 8, 128, (64, 64, 1), (64, 64, 1)), Row(8, 9, 128, (64, 64, 1), (64, 64, 1)),     # outside
]


def row_id(r):
    return f"{r.M}x{r.N}x{r.K}"


def vector_path(r):
    """gemm_vec_ok for the three Linear calls: 16-byte rows of every operand and of the output"""
    return r.N % 4 == 0 and r.K % 4 == 0


def blocks2d(t, ref, bm, bn):
    """relative L2 error of every bm x bn block of t [R, C] against ref (float64), ragged edges included -> [ceil(R / bm), ceil(C / bn)]"""
    t = t.detach().double().cpu().reshape(ref.shape)
    R, C = ref.shape
    pr, pc = (-R) % bm, (-C) % bn

    def blocks(v):
        return F.pad(v ** 2, (0, pc, 0, pr)).reshape((R + pr) // bm, bm, (C + pc) // bn, bn).sum((1, 3))
    e2, r2 = blocks(t - ref), blocks(ref)
    assert e2.shape == (-(-R // bm), -(-C // bn))                 # no block skipped
    return (e2 / (r2 + 1e-300)).sqrt()


def worst(be):
    return be.max().item(), tuple(int(v) for v in torch.unravel_index(be.argmax(), be.shape))


@lru_cache(maxsize=1)
def linear_inputs(r):
    g = torch.Generator().manual_seed(7000 + LINEAR_ROWS.index(r))

    def rnd(*s, scale=1.0):
        return torch.randn(*s, generator=g) * scale
    M, N, K = r.M, r.N, r.K
    return dict(x=rnd(M, K), w=rnd(N, K, scale=K ** -0.5), b=rnd(N), res=rnd(M, N), dy=rnd(M, N), rdx=rnd(M, K))


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def finite(t, what):
    bad = ~torch.isfinite(t)
    assert not bool(bad.any()), (what, f"{int(bad.sum())} of {t.numel()} elements: a tile was not stored or a split's slab not delivered")


def check_linear_record(r, launches, plan, dims, what):
    if plan == HEAD:
        assert launches == [], (what, launches)
        return "head"
    assert len(launches) == 1, (what, launches)
    rec = launches[0]
    bm, bn, sk = plan
    want = dict(variant="koaf_gemm", M=dims[0], N=dims[1], K=dims[2], bm=bm, bn=bn, splitk=sk, nbatch=1, fmt=0)
    assert {f: rec[f] for f in want} == want, (what, rec, want)
    assert rec["tiles"] == rec["grid_x"] == -(-dims[0] // bm) * -(-dims[1] // bn), (what, rec)
    remap = sk > 1 and sk % 8 == 0            # koaf_gemm_kernel: the XCD remap of (blockIdx.x, blockIdx.y) runs
    return f"{bm:3d}x{bn:<3d} splitk {sk}{' remap' if remap else ''}{'' if vector_path(r) else ' scalar'}"


def hold(what, got, r64, r32, den, bm, bn, bar):
    """the bars on one finished result; -> the table fragment"""
    finite(got, what)
    be, where = worst(blocks2d(got, r64, bm, bn))
    whole = rel_err(got, r64)
    cw, cbar = componentwise(got, r64, r32, den + 1e-300)
    cbar = max(cbar, bar)
    assert be < bar, (what, f"block (row band of {bm}, column band of {bn})", where, be)
    assert whole < bar, (what, whole)
    assert cw <= cbar, (what, cw, cbar)
    return f"worst block {be:.2e} at {where} whole {whole:.2e} cw {cw:.2e} (bar {cbar:.2e})"


@pytest.mark.parametrize("r", LINEAR_ROWS, ids=[row_id(r) for r in LINEAR_ROWS])
def test_linear_plans(dev, r):
    from oaprogressionmmf_amd import ops
    L = ops.lib()
    M, N, K = r.M, r.N, r.K
    t = linear_inputs(r)
    x, w, b, res, dy, rdx = (t[k] for k in ("x", "w", "b", "res", "dy", "rdx"))
    xd, wd, bd, resd, dyd, rdxd = (v.to(dev) for v in (x, w, b, res, dy, rdx))
    ptr, stream = ops._ptr, ops._stream
    try:
        # ---- forward: with bias and residual, and with neither
        p64, p32, pden = x.double() @ w.double().t(), x @ w.t(), (x.abs() @ w.abs().t()).double()
        nws = L.koaf_linear_ws(M, N, K)
        assert nws == (0 if r.fwd == HEAD or r.fwd[2] == 1 else r.fwd[2] * M * N), (row_id(r), nws)
        for full in (True, False):
            y, ws = nan(dev, M, N), (nan(dev, nws) if nws else None)
            with Record() as rec:
                ops.check(L.koaf_linear_fwd(ptr(xd), ptr(wd), ptr(bd) if full else None, ptr(resd) if full else None, ptr(y), ptr(ws),
                                            M, N, K, stream()), "linear_fwd")
            torch.cuda.synchronize()
            what = f"linear_fwd {row_id(r)} {'bias + residual' if full else 'plain'}"
            plan = check_linear_record(r, rec.launches, r.fwd, (M, N, K), what)
            refs = (p64 + b.double() + res.double(), p32 + b + res, pden + b.double().abs() + res.double().abs()) if full else (p64, p32, pden)
            print(f"\n[dense] {what:42s} {plan:30s} | {hold(what, y, *refs, 64, 128, FWD)}")
        del p64, p32, pden
        # ---- data gradient: with residual, and without
        g64, g32, gden = dy.double() @ w.double(), dy @ w, (dy.abs() @ w.abs()).double()
        nws = L.koaf_linear_ws(M, K, N)
        assert nws == (0 if r.dgrad == HEAD or r.dgrad[2] == 1 else r.dgrad[2] * M * K), (row_id(r), nws)
        for full in (True, False):
            dx, ws = nan(dev, M, K), (nan(dev, nws) if nws else None)
            with Record() as rec:
                ops.check(L.koaf_linear_dgrad(ptr(dyd), ptr(wd), ptr(rdxd) if full else None, ptr(dx), ptr(ws), M, N, K, stream()), "linear_dgrad")
            torch.cuda.synchronize()
            what = f"linear_dgrad {row_id(r)} {'residual' if full else 'plain'}"
            plan = check_linear_record(r, rec.launches, r.dgrad, (M, K, N), what)
            refs = (g64 + rdx.double(), g32 + rdx, gden + rdx.double().abs()) if full else (g64, g32, gden)
            print(f"\n[dense] {what:42s} {plan:30s} | {hold(what, dx, *refs, 64, 128, BWD)}")
        del g64, g32, gden
        # ---- weight gradient with db
        dw, db = nan(dev, N, K), nan(dev, N)
        ncs = L.koaf_colsum_ws(M, N)
        cws = nan(dev, ncs) if ncs > 0 else None
        with Record() as rec:
            ops.check(L.koaf_linear_wgrad(ptr(dyd), ptr(xd), ptr(dw), ptr(db), ptr(cws), M, N, K, stream()), "linear_wgrad")
        torch.cuda.synchronize()
        what = f"linear_wgrad {row_id(r)}"
        if r.fwd == HEAD:
            assert rec.launches == [], (what, rec.launches)
            plan = "head"
        else:
            assert len(rec.launches) == 1, (what, rec.launches)
            q = rec.launches[0]
            want = dict(variant="koaf_gemm", M=N, N=K, K=M, splitk=1, nbatch=1, fmt=0)
            assert {f: q[f] for f in want} == want, (what, q, want)
            assert vector_path(r) or (q["bm"], q["bn"]) == (64, 64), (what, q)
            plan = f"{q['bm']:3d}x{q['bn']:<3d} splitk 1{'' if vector_path(r) else ' scalar'}"
        print(f"\n[dense] {what:42s} {plan:30s} | "
              f"{hold(what, dw, dy.double().t() @ x.double(), dy.t() @ x, (dy.abs().t() @ x.abs()).double(), 64, 64, BWD)}")
        finite(db, what + " db")
        assert rel_err(db, dy.double().sum(0)) < 2e-6, what            # (test_linear's bar)
    finally:
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
ATTENTION_SHAPES = [          # (B, n, h, d)
    (2, 483, 8, 256),         # production: the backward on the scalar loaders
    (2, 484, 2, 32),          # the same size on the vector path
    (2, 63, 2, 32), (2, 64, 2, 32), (2, 65, 2, 32),
    (1, 1, 2, 32),
    (2, 40, 2, 6),            # d % 4 != 0: the fused forward declines, everything on the scalar loaders
    (1, 513, 2, 32),          # past the fused kernel's 512 keys: three launches, scalar loaders, a ragged tile
    (1, 520, 2, 32),          # three launches on the vector path
]
BWD_GEMMS = 4                 # koaf_attention_bwd: dV, dP, dQ, dK


def group_bands(t, ref, band):
    """relative L2 error of every `band`-row band of every group: t, ref [G, n, C] -> [G, ceil(n / band)] (no band straddles two groups)"""
    t = t.detach().double().cpu().reshape(ref.shape)
    G, n, C = ref.shape
    pad = (-n) % band

    def bands(v):
        return F.pad((v ** 2).sum(2), (0, pad)).reshape(G, (n + pad) // band, band).sum(2)
    e2, r2 = bands(t - ref), bands(ref)
    assert e2.shape == (G, -(-n // band))                         # no band skipped
    return (e2 / (r2 + 1e-300)).sqrt()


def attention_cpu(qkv, dout, B, n, h, d, scale):
    """(attn [B,h,n,n], out [B,n,h*d], dqkv) in the type of qkv"""
    qkv = qkv.clone().requires_grad_(True)
    q, k, v = qkv.reshape(B, n, 3, h, d).permute(2, 0, 3, 1, 4)
    attn = (torch.einsum("bhid,bhjd->bhij", q, k) * scale).softmax(-1)
    out = torch.einsum("bhij,bhjd->bhid", attn, v).permute(0, 2, 1, 3).reshape(B, n, h * d)
    out.backward(dout.to(qkv.dtype))
    return attn.detach(), out.detach(), qkv.grad


def heads(t, B, n, h, d):
    """[B, n, h * d] -> [B * h, n, d]"""
    return t.reshape(B, n, h, d).permute(0, 2, 1, 3).reshape(B * h, n, d)


@pytest.mark.parametrize("B,n,h,d", ATTENTION_SHAPES, ids=["x".join(map(str, s)) for s in ATTENTION_SHAPES])
def test_attention_bands(dev, B, n, h, d):
    from oaprogressionmmf_amd import ops
    g = torch.Generator().manual_seed(7500 + n * 7 + d)
    dim = h * d
    scale = dim ** -0.5
    qkv, dout = torch.randn(B, n, 3 * dim, generator=g), torch.randn(B, n, dim, generator=g)
    attn64, out64, dqkv64 = attention_cpu(qkv.double(), dout, B, n, h, d, scale)
    attn32, out32, dqkv32 = attention_cpu(qkv, dout, B, n, h, d, scale)
    qd = qkv.to(dev)
    name = f"{B}x{n}x{h}x{d}"
    try:
        with Record() as rf:
            out, attn = ops.attention_fwd(qd, B, n, h, d, scale)
        with Record() as rb:
            dqkv = ops.attention_bwd(dout.to(dev), qd, attn, B, n, h, d, scale)
        torch.cuda.synchronize()
        fused = n <= 512 and d % 4 == 0
        assert len(rf.launches) == (0 if fused else 2), (name, rf.launches)
        assert len(rb.launches) == BWD_GEMMS, (name, rb.launches)
        for q in rf.launches + rb.launches:
            assert q["nbatch"] == B * h and q["splitk"] == 1 and q["fmt"] == 0 and (q["bm"], q["bn"]) == (64, 64), (name, q)
        assert [(q["M"], q["N"], q["K"]) for q in rb.launches] == [(n, d, n), (n, n, d), (n, d, n), (n, d, n)], (name, rb.launches)
        # ---- forward: attn and out per (batch, head, 32-query tile) and per element
        ab, aw = worst(group_bands(attn, attn64.reshape(B * h, n, n), 32))
        ob, ow = worst(group_bands(heads(out, B, n, h, d), heads(out64, B, n, h, d), 32))
        wa, wo, wg = rel_err(attn, attn64), rel_err(out, out64), rel_err(dqkv, dqkv64)
        print(f"\n[dense] attention {name:14s} fwd {'fused' if fused else '3 launches'} bwd gemms {len(rb.launches)} nbatch {B * h} | attn worst tile {ab:.2e} "
              f"whole {wa:.2e} | out worst tile {ob:.2e} whole {wo:.2e}")
        assert wa < 2e-6 and wo < 2e-6, (name, wa, wo)                 # (test_attention's whole-tensor bars)
        assert ab < FWD, (name, "attn (batch * h + head, 32-query tile)", aw, ab)
        assert ob < FWD, (name, "out (batch * h + head, 32-query tile)", ow, ob)
        yardstick(attn, attn64, attn32, f"attention {name} attn", floor=2e-6 * float(attn64.abs().max()))
        yardstick(out, out64, out32, f"attention {name} out", floor=2e-6 * float(out64.abs().max()))
        # ---- backward: dq, dk, dv apart, per (batch, head, 64-row band) and per element
        assert wg < 2 * BWD, (name, wg)                                # (test_attention's whole-tensor bar)
        parts = lambda v: v.reshape(B, n, 3, h, d).permute(2, 0, 3, 1, 4).reshape(3, B * h, n, d)      # noqa: E731
        got, r64, r32 = parts(dqkv.cpu()), parts(dqkv64), parts(dqkv32)
        line = []
        for i, which in enumerate(("dq", "dk", "dv")):
            be, where = worst(group_bands(got[i], r64[i], 64))
            line.append(f"{which} worst band {be:.2e} at {where} whole {rel_err(got[i], r64[i]):.2e}")
            assert be < 2 * BWD, (name, which + " (batch * h + head, 64-row band)", where, be)
            yardstick(got[i], r64[i], r32[i], f"attention {name} {which}", floor=2 * BWD * float(r64[i].abs().max()))
        print(f"[dense] attention {name:14s} bwd whole {wg:.2e} | " + " | ".join(line))
    finally:
        torch.cuda.empty_cache()
