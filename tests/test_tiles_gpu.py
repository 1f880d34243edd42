"""Kernel parity at the shapes that reach the PRODUCTION tile variants of koaf_gemm: 128-row tiles, streamed and block-wide
loaders, persistent blocks that walk several tiles, bf16 activation storage, stride 2 at 128 rows, the halo kernels' width edge.

koaf_gemm_pick_tile shrinks a 128-row / 128-column tile to 64 while the grid is under 384 blocks, so the small shapes of
test_kernels_gpu.py run 64 x 64 tiles almost everywhere.  Every row of TILE_CASES is sized by that rule (>= 384 tiles to keep a
128 tile, > 512 tiles for persistent blocks to walk), goes through ops.conv2d_fwd / ops.conv2d_dgrad as the model calls them
(weight plane images, fp16 scheme) and ASSERTS FROM THE LAUNCH RECORD (koaf.h koaf_launch_log) which variant, tile and grid
served it: a row that lands elsewhere fails.  tests/test_tile_plan_cpu.py asks the picker the same on any machine.

Bars (owned by the module docstring of test_kernels_gpu.py; nothing new is invented):
  * relative L2 against the float64 CPU result PER 128-ROW BAND of the output (every band, the ragged last one included) and
    over the whole tensor: 2e-6 forward, BWD = 4e-6 gradients.  A fault confined to one row band (ragged last tile, the first
    tile after a persistent block crosses a tile boundary, the weight ring's phase) moves a whole-tensor norm by 1 / sqrt(bands).
    Stride-2 data gradients: the bands run over the rows of each parity class (the rows of its GEMM), not over raster rows.
  * componentwise: max |y - y64| / (|a| @ |b|) over all elements.  The bar is 8 x the same ratio of torch's fp32 CPU product of
    the same operands (the loader transform evaluated in fp32 as well), computed in the test: 4 x because each operand is
    carried at 2^-22 instead of 2^-24, 2 x for a different accumulation order.  The faults this is for (a dropped low piece
    2^-11, a stale tile, one wrong row) are >= 1e-4.
  * BatchNorm statistics and the BatchNorm-backward reduction partials: 1e-4 on sums, 1e-5 on sums of squares (test_conv2d).
  * bf16 activation storage: the property of test_bf16_storage_equals_fp32_mode_on_widened_inputs -- bit-equal to the fp32
    mode on widened inputs, the output rounded once.
The data gradients whose dy is a BatchNorm-backward apply (ops.BnApply, KoafOperand.tf 2) are held to the float64 product of
dy64 = coef0 * dz + coef3 - coef2 * c formed from the coefficients the device left (fp32 values taken as exact inputs): the
GEMM and its loader are under test here, the BatchNorm reduction has its own tests.

Each case prints one table line: variant / tile / tiles / grid.x from the record, worst band error, componentwise ratio and bar."""
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FWD, BWD = 2e-6, 4e-6     # test_kernels_gpu.py: forward / gradient contractions against float64
PERSIST = 512             # resident blocks of the persistent kernels (2 per CU x 256 CUs): more tiles than that and they walk

Case = namedtuple("Case", "name op shape call stream store variant bm bn walks")
# op     "fwd" | "dgrad" of the convolution shape = (N, H, W, Cin, Cout, k, stride, pad)
# call   fwd:   plain (tf 0, statistics) | prologue (BatchNorm + ReLU on load, tf 1, statistics) | tail / tail_ds (bottleneck tail,
#               tf 3, without / with the downsample record, statistics) | *_emit (the epilogue cuts the consumer's plane images)
#        dgrad: plain (dy + amax) | apply (BnApply on load, tf 2) | apply_res (+ residual) | bnb1 (dy, residual, fused BatchNorm-
#               backward epilogue mode 1, two BatchNorms) | bnb2 (BnApply, residual, epilogue mode 2, max |dz|)
# stream ops.set_stream: True = the default (streamed kernel where it serves), False = block-wide loader
# store  "fp32" (against float64) | "bf16" (activation_storage: bf16 -- against the fp32 mode on widened inputs)
# variant / bm / bn / walks: what the launch record must show (walks: grid.x < tiles, persistent blocks walk several tiles)
S, E, G, H128, H256 = "koaf_gemm/stream", "koaf_gemm/emit", "koaf_gemm", "koaf_gemm/halo128", "koaf_gemm/halo"

F1 = (43, 24, 24, 64, 256, 1, 1, 0)        # 24 768 rows (last tile 64 rows), 388 tiles 128 x 128, K = 64: two k-steps
F2 = (152, 17, 19, 128, 64, 1, 1, 0)       # 49 096 rows = 72 mod 128 = 8 mod 32, 384 tiles 128 x 64, K = 128: four k-steps (not a multiple of the ring's three)
F3 = (48, 16, 16, 256, 512, 1, 1, 0)       # 12 288 rows, exactly 384 tiles, four column tiles, K = 256: eight k-steps
F4 = (245, 10, 10, 1024, 256, 1, 1, 0)     # 24 500 rows = 52 mod 128 = 20 mod 32, 384 tiles, K = 1024 = STREAM_TAB_K: tf 1 still streams
F5 = (130, 10, 10, 2048, 512, 1, 1, 0)     # 13 000 rows, 408 tiles, K = 2048: tf 1 past the table -> block-wide; tf 0 streams
F6 = (114, 24, 24, 256, 128, 1, 1, 0)      # 65 664 rows, 513 tiles > 512 resident blocks: the persistent kernels walk, K = 256
# data gradients: the GEMM's N is Cin, its K is Cout
D1 = (43, 24, 24, 256, 64, 1, 1, 0)        # N = 256, K = 64: 388 tiles 128 x 128
D2 = (152, 17, 19, 64, 128, 1, 1, 0)       # N = 64, K = 128: 384 tiles 128 x 64, ragged against 128 and 32
D3 = (48, 16, 16, 512, 256, 1, 1, 0)       # N = 512, K = 256: exactly 384
D4 = (114, 24, 24, 128, 256, 1, 1, 0)      # N = 128, K = 256: 513 tiles, walks
D5 = (245, 10, 10, 256, 1024, 1, 1, 0)     # N = 256, K = 1024: 384 tiles, rows 20 mod 32
# stride 2 at 128-row tiles, odd H and W: 3x3 128 -> 128 (forward 411 tiles; the four parity classes of the data gradient 386 ..
# 411 tiles each) and the 1x1 downsample 256 -> 512 (forward 776 tiles: walks; data gradient: one class has the tap, 388 tiles)
S3 = (53, 63, 61, 128, 128, 3, 2, 1)
S1 = (25, 63, 61, 256, 512, 1, 2, 0)
# 3x3 / stride 1 beside test_activation_plane_images (the family's own table, both orientations, per tile: test_conv3_edges_gpu.py):
# W = 78 with odd H (layer1 of the 310^2 radiograph: the 128-row halo kernel, not the rectangle one) and the halo kernels' width limit at 128 output columns, W = 64 (halo, 256 rows) | 65 (per-tap gather)
W78 = (2, 77, 78, 64, 64, 3, 1, 1)
W64 = (2, 33, 64, 128, 128, 3, 1, 1)
W65 = (2, 33, 65, 128, 128, 3, 1, 1)

TILE_CASES = [
    # ---- dense 1x1 / stride 1 forward, streamed
    Case("f1-plain", "fwd", F1, "plain", True, "fp32", S, 128, 128, False),
    Case("f1-prologue", "fwd", F1, "prologue", True, "fp32", S, 128, 128, False),
    Case("f1-tail", "fwd", F1, "tail", True, "fp32", S, 128, 128, False),
    Case("f1-tail_ds", "fwd", F1, "tail_ds", True, "fp32", S, 128, 128, False),
    Case("f1-prologue_emit", "fwd", F1, "prologue_emit", True, "fp32", S, 128, 128, False),
    Case("f2-plain", "fwd", F2, "plain", True, "fp32", S, 128, 64, False),
    Case("f2-prologue", "fwd", F2, "prologue", True, "fp32", S, 128, 64, False),
    Case("f2-tail", "fwd", F2, "tail", True, "fp32", S, 128, 64, False),
    Case("f2-tail_emit", "fwd", F2, "tail_emit", True, "fp32", S, 128, 64, False),
    Case("f3-plain", "fwd", F3, "plain", True, "fp32", S, 128, 128, False),
    Case("f3-prologue", "fwd", F3, "prologue", True, "fp32", S, 128, 128, False),
    Case("f4-prologue", "fwd", F4, "prologue", True, "fp32", S, 128, 128, False),
    Case("f4-tail_ds", "fwd", F4, "tail_ds", True, "fp32", S, 128, 128, False),
    Case("f5-plain", "fwd", F5, "plain", True, "fp32", S, 128, 128, False),
    Case("f5-prologue", "fwd", F5, "prologue", True, "fp32", G, 128, 128, False),      # K > STREAM_TAB_K: must fall back
    Case("f6-plain", "fwd", F6, "plain", True, "fp32", S, 128, 128, True),
    Case("f6-prologue", "fwd", F6, "prologue", True, "fp32", S, 128, 128, True),
    Case("f6-prologue_emit", "fwd", F6, "prologue_emit", True, "fp32", S, 128, 128, True),
    Case("f6-tail", "fwd", F6, "tail", True, "fp32", S, 128, 128, False),              # (the two-source loaders: one tile per block)
    # ---- ... block-wide (ops.set_stream(False)): the production path of the bf16 storage mode
    Case("f1-plain-bw", "fwd", F1, "plain", False, "fp32", G, 128, 128, False),
    Case("f1-prologue-bw", "fwd", F1, "prologue", False, "fp32", G, 128, 128, False),
    Case("f1-tail_ds-bw", "fwd", F1, "tail_ds", False, "fp32", G, 128, 128, False),
    Case("f1-prologue_emit-bw", "fwd", F1, "prologue_emit", False, "fp32", E, 128, 128, False),
    Case("f2-prologue-bw", "fwd", F2, "prologue", False, "fp32", G, 128, 64, False),
    Case("f2-tail_emit-bw", "fwd", F2, "tail_emit", False, "fp32", E, 128, 64, False),
    Case("f3-tail-bw", "fwd", F3, "tail", False, "fp32", G, 128, 128, False),
    Case("f4-prologue-bw", "fwd", F4, "prologue", False, "fp32", G, 128, 128, False),
    Case("f6-plain-bw", "fwd", F6, "plain", False, "fp32", G, 128, 128, True),
    Case("f6-prologue-bw", "fwd", F6, "prologue", False, "fp32", G, 128, 128, True),
    Case("f6-prologue_emit-bw", "fwd", F6, "prologue_emit", False, "fp32", E, 128, 128, True),
    # ---- data gradients of dense 1x1 / stride 1, streamed
    Case("d1-plain", "dgrad", D1, "plain", True, "fp32", S, 128, 128, False),
    Case("d1-apply", "dgrad", D1, "apply", True, "fp32", S, 128, 128, False),
    Case("d1-apply_res", "dgrad", D1, "apply_res", True, "fp32", S, 128, 128, False),
    Case("d1-bnb1", "dgrad", D1, "bnb1", True, "fp32", S, 128, 128, False),
    Case("d1-bnb2", "dgrad", D1, "bnb2", True, "fp32", S, 128, 128, False),
    Case("d2-plain", "dgrad", D2, "plain", True, "fp32", S, 128, 64, False),
    Case("d2-apply", "dgrad", D2, "apply", True, "fp32", S, 128, 64, False),           # the 128 x 64 tf 2 instantiation
    Case("d2-bnb2", "dgrad", D2, "bnb2", True, "fp32", S, 128, 64, False),
    Case("d3-plain", "dgrad", D3, "plain", True, "fp32", S, 128, 128, False),
    Case("d3-bnb2", "dgrad", D3, "bnb2", True, "fp32", S, 128, 128, False),
    Case("d4-plain", "dgrad", D4, "plain", True, "fp32", S, 128, 128, True),
    Case("d4-bnb1", "dgrad", D4, "bnb1", True, "fp32", S, 128, 128, True),
    Case("d4-apply_res", "dgrad", D4, "apply_res", True, "fp32", S, 128, 128, False),
    Case("d5-plain", "dgrad", D5, "plain", True, "fp32", S, 128, 128, False),
    Case("d5-apply", "dgrad", D5, "apply", True, "fp32", S, 128, 128, False),
    # ---- ... block-wide
    Case("d1-plain-bw", "dgrad", D1, "plain", False, "fp32", G, 128, 128, False),
    Case("d1-bnb2-bw", "dgrad", D1, "bnb2", False, "fp32", G, 128, 128, False),
    Case("d2-apply-bw", "dgrad", D2, "apply", False, "fp32", G, 128, 64, False),
    Case("d3-bnb1-bw", "dgrad", D3, "bnb1", False, "fp32", G, 128, 128, False),
    Case("d4-plain-bw", "dgrad", D4, "plain", False, "fp32", G, 128, 128, True),
    # ---- stride 2 at 128-row tiles
    Case("s3-fwd-plain", "fwd", S3, "plain", True, "fp32", G, 128, 128, False),
    Case("s3-fwd-prologue", "fwd", S3, "prologue", True, "fp32", G, 128, 128, False),
    Case("s3-dgrad-plain", "dgrad", S3, "plain", True, "fp32", G, 128, 128, False),
    Case("s3-dgrad-bnb2", "dgrad", S3, "bnb2", True, "fp32", G, 128, 128, False),
    Case("s1-fwd-plain", "fwd", S1, "plain", True, "fp32", G, 128, 128, True),
    Case("s1-fwd-prologue", "fwd", S1, "prologue", True, "fp32", G, 128, 128, True),
    Case("s1-dgrad-plain", "dgrad", S1, "plain", True, "fp32", G, 128, 128, False),
    Case("s1-dgrad-apply_res", "dgrad", S1, "apply_res", True, "fp32", G, 128, 128, False),
    # ---- activation_storage: bf16 (act16 1 forward / 2 data gradient): the block-wide 128-row kernels are the production path
    Case("f1-prologue-bf16", "fwd", F1, "prologue", True, "bf16", G, 128, 128, False),
    Case("f1-tail-bf16", "fwd", F1, "tail", True, "bf16", G, 128, 128, False),
    Case("f2-prologue-bf16", "fwd", F2, "prologue", True, "bf16", G, 128, 64, False),
    Case("f6-prologue-bf16", "fwd", F6, "prologue", True, "bf16", G, 128, 128, True),
    Case("f6-prologue_emit-bf16", "fwd", F6, "prologue_emit", True, "bf16", E, 128, 128, True),
    Case("d1-bnb2-bf16", "dgrad", D1, "bnb2", True, "bf16", G, 128, 128, False),
    Case("d2-apply-bf16", "dgrad", D2, "apply", True, "bf16", G, 128, 64, False),
    Case("s3-fwd-prologue-bf16", "fwd", S3, "prologue", True, "bf16", G, 128, 128, False),
    Case("s3-dgrad-bnb2-bf16", "dgrad", S3, "bnb2", True, "bf16", G, 128, 128, False),
    Case("s1-fwd-prologue-bf16", "fwd", S1, "prologue", True, "bf16", G, 128, 128, True),
    Case("s1-dgrad-apply_res-bf16", "dgrad", S1, "apply_res", True, "bf16", G, 128, 128, False),
    # ---- 3x3 / stride 1: what test_activation_plane_images lacks (the halo kernels set their tile themselves)
    Case("w78-halo128", "fwd", W78, "prologue", True, "fp32", H128, 128, 64, False),
    Case("w64-halo", "fwd", W64, "prologue", True, "fp32", H256, 256, 128, False),
    Case("w65-gather", "fwd", W65, "prologue", True, "fp32", G, 64, 64, False),
]


def conv_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def gemm_dims(case):
    """[(M, N, K)] of the koaf_gemm calls behind a case, as koaf_conv2d_fwd / koaf_conv2d_dgrad_bnb form them (a stride-2 data
    gradient: one GEMM per parity class of the input pixels, K = its taps x Cout; classes without a tap have K = 0)"""
    N, H, W, Cin, Cout, k, s, p = case.shape
    if case.op == "fwd":
        return [(N * conv_out(H, k, s, p) * conv_out(W, k, s, p), Cout, k * k * Cin)]
    if s == 1:
        return [(N * H * W, Cin, k * k * Cout)]
    out = []
    for py in range(2):
        for px in range(2):
            khs, kws = (py + p) & 1, (px + p) & 1
            nkh, nkw = ((k - khs + 1) // 2 if khs < k else 0), ((k - kws + 1) // 2 if kws < k else 0)
            out.append((N * ((H - py + 1) // 2) * ((W - px + 1) // 2), Cin, nkh * nkw * Cout))
    return out


def n_tiles(M, N, bm, bn):
    return -(-M // bm) * -(-N // bn)


G_ = torch.Generator().manual_seed(4321)


def rnd(*shape, scale=1.0):
    return torch.randn(*shape, generator=G_) * scale


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def band_errors(y, ref, band=128):
    """relative L2 error of every `band`-row band of y [rows, C] against ref (float64), the ragged last band included"""
    y, ref = y.detach().double().cpu().reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    e2, r2 = ((y - ref) ** 2).sum(1), (ref ** 2).sum(1)
    pad = (-e2.numel()) % band
    e2, r2 = F.pad(e2, (0, pad)).reshape(-1, band).sum(1), F.pad(r2, (0, pad)).reshape(-1, band).sum(1)
    assert e2.numel() == -(-y.shape[0] // band)           # no band skipped
    return (e2 / (r2 + 1e-300)).sqrt()


class Record:
    """the koaf_gemm launches of the calls inside the with block"""

    def __enter__(self):
        from oaprogressionmmf_amd import ops
        ops.launch_log(True)
        return self

    def __exit__(self, *exc):
        from oaprogressionmmf_amd import ops
        self.launches = ops.launch_log_read()
        ops.launch_log(False)
        return False


def check_record(case, launches, act16):
    """the launches with work (K > 0) are the GEMMs gemm_dims() predicts, each on the variant / tile / grid the case is there for"""
    dims = gemm_dims(case)
    assert len(launches) == len(dims), (case.name, launches)         # (a stride-2 data gradient: all four classes are recorded)
    worked = []
    for r, (M, N, K) in zip(launches, dims):
        assert (r["M"], r["N"], r["K"]) == (M, N, K), (case.name, r)
        assert r["fmt"] == 1 and r["splitk"] == 1 and r["nbatch"] == 1, (case.name, r)
        if K == 0:
            continue
        tiles = n_tiles(M, N, case.bm, case.bn)
        assert r["variant"] == case.variant, (case.name, r)
        assert (r["bm"], r["bn"]) == (case.bm, case.bn), (case.name, r)
        assert r["tiles"] == tiles, (case.name, r, tiles)
        if case.walks:
            assert r["tiles"] > PERSIST and r["grid_x"] == PERSIST, (case.name, r)
        else:
            assert r["grid_x"] == r["tiles"], (case.name, r)
        assert r["act16"] == act16, (case.name, r)
        assert bool(r["emit"]) == case.call.endswith("_emit"), (case.name, r)
        want_tf = {"plain": 0, "prologue": 1, "prologue_emit": 1, "tail": 3, "tail_ds": 3, "tail_emit": 3, "apply": 2, "apply_res": 2,
                   "bnb1": 0, "bnb2": 2}[case.call]
        if not (case.shape[5] == 3 and (case.op == "dgrad" or case.shape[6] == 1)):     # (plane images: the transform is in the pre-pass)
            assert r["a_tf"] == want_tf, (case.name, r)
        worked.append(r)
    assert worked
    return worked[0]


def componentwise(y, y64, y32, den):
    """(max |y - y64| / den, 8 x max |y32 - y64| / den): the kernel's componentwise error and its bar from torch's fp32 product"""
    got = ((y.detach().double().cpu().reshape(y64.shape) - y64).abs() / den).max().item()
    ref = ((y32.double() - y64).abs() / den).max().item()
    return got, 8.0 * ref


def report(case, rec, worst, whole, cw, bar, extra=""):
    print(f"\n[tiles] {case.name:24s} {rec['variant']:17s} {rec['bm']:3d}x{rec['bn']:<3d} tiles {rec['tiles']:4d} grid.x {rec['grid_x']:4d} "
          f"tf {rec['a_tf']} act16 {rec['act16']} | worst band {worst:.2e} whole {whole:.2e} | componentwise {cw:.2e} (bar {bar:.2e}){extra}")


def _conv64(a, w, k, s, p):
    """float64 / float32 NHWC convolution on the CPU; a [N,H,W,Cin], w packed [Cout,k,k,Cin] -> [N,OH,OW,Cout]"""
    if k == 1 and s == 1:
        return (a.reshape(-1, a.shape[-1]) @ w.reshape(w.shape[0], -1).t()).reshape(*a.shape[:3], w.shape[0])
    return F.conv2d(a.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=s, padding=p).permute(0, 2, 3, 1).contiguous()


def _dgrad64(dy, w, shape):
    """data gradient of the same convolution: dy [N,OH,OW,Cout], w packed [Cout,k,k,Cin] -> [N,H,W,Cin]"""
    N, H, W, Cin, Cout, k, s, p = shape
    if k == 1 and s == 1:
        return (dy.reshape(-1, Cout) @ w.reshape(Cout, Cin)).reshape(N, H, W, Cin)
    return torch.nn.grad.conv2d_input((N, Cin, H, W), w.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), stride=s,
                                      padding=p).permute(0, 2, 3, 1).contiguous()


def _class_rows(t, shape):
    """[rows, C] views of a [N,H,W,C] gradient in the row order of the GEMMs that wrote it (stride 2: one per parity class)"""
    if shape[6] == 1:
        return [t.reshape(-1, t.shape[-1])]
    return [t[:, py::2, px::2, :].reshape(-1, t.shape[-1]) for py in range(2) for px in range(2)]


def _forward(ops, dev, case, x, w, img, sc, sh, idt, ids, em):
    N, H, W, Cin, Cout, k, s, p = case.shape
    kw = dict(wimg=img)
    call = case.call
    if call.endswith("_emit"):
        kw["emit"] = em
    else:
        kw["stats"] = True
    if call.startswith("tail"):
        kw["tail_idt"] = idt
        if call == "tail_ds":
            kw["tail_idsaved"] = ids
    tf = call != "plain"
    return ops.conv2d_fwd(x, w, N, H, W, Cin, Cout, k, k, s, p, sc if tf else None, sh if tf else None, **kw)


def run_forward(dev, case):
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, s, p = case.shape
    rows = N * H * W
    call = case.call
    x = rnd(N, H, W, Cin) * 1.5 + 0.3
    w = rnd(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5)
    sc, sh = rnd(Cin) * 0.2 + 1.0, rnd(Cin) * 0.1
    idt = rnd(N, H, W, Cin) if call.startswith("tail") else None
    ids = torch.stack([rnd(Cin) * 0.1, 1.0 + 0.1 * rnd(Cin), 1.0 + 0.3 * rnd(Cin), 0.2 * rnd(Cin)]) if call == "tail_ds" else None
    em = (torch.rand(Cout, generator=G_) + 0.5, rnd(Cout) * 0.1)
    if case.store == "bf16":
        x = x.bfloat16().float()
        idt = idt.bfloat16().float() if idt is not None else None
    xd, wd, scd, shd = x.to(dev), w.to(dev), sc.to(dev), sh.to(dev)
    idtd, idsd, emd = (idt.to(dev) if idt is not None else None), (ids.to(dev) if ids is not None else None), (em[0].to(dev), em[1].to(dev))
    img = ops.build_weight_planes(wd, Cout, k * k, Cin)
    was = ops.set_stream(case.stream)
    try:
        if case.store == "bf16" and call == "tail":
            # the stored tail y is rounded BEFORE it is multiplied (test_bottleneck_tail_formed_in_the_conv1_loader): the same bits as
            # the element-wise tail pass followed by the plain convolution, both in the storage mode
            saved = torch.stack([scd, scd, scd, shd])
            y_t = ops.bn_add_relu(xd.bfloat16(), saved, rows, Cin, idt=idtd.bfloat16())
            o_t, p_t = ops.conv2d_fwd(y_t, wd, N, H, W, Cin, Cout, k, k, s, p, None, None, stats=True, wimg=img)
            out32 = None
            with Record() as rec:
                out = _forward(ops, dev, case, xd.bfloat16(), wd, img, scd, shd, idtd.bfloat16(), idsd, emd)
        elif case.store == "bf16":
            # the fp32 mode on the widened inputs first (streams where it can), then the storage mode under the record
            out32 = _forward(ops, dev, case, xd, wd, img, scd, shd, idtd, idsd, emd)
            with Record() as rec:
                out = _forward(ops, dev, case, xd.bfloat16(), wd, img, scd, shd, idtd.bfloat16() if idtd is not None else None, idsd, emd)
        else:
            with Record() as rec:
                out = _forward(ops, dev, case, xd, wd, img, scd, shd, idtd, idsd, emd)
    finally:
        ops.set_stream(was)
    torch.cuda.synchronize()
    r = check_record(case, rec.launches, 1 if case.store == "bf16" else 0)
    y = out[0]
    if case.store == "bf16" and call == "tail":
        assert y.dtype == out[2].dtype == torch.bfloat16, case.name
        assert torch.equal(out[2], y_t) and torch.equal(y, o_t) and torch.equal(out[1], p_t), case.name
        y64 = torch.relu(x.double() * sc.double() + sh.double() + idt.double()).float().bfloat16().double()
        assert rel_err(y.float(), _conv64(y64, w.double(), k, s, p)) < 4e-3, case.name      # (8 significand bits of the output)
        print(f"\n[tiles] {case.name:24s} {r['variant']:17s} {r['bm']:3d}x{r['bn']:<3d} tiles {r['tiles']:4d} grid.x {r['grid_x']:4d} "
              f"tf {r['a_tf']} act16 {r['act16']} | bit-equal to the tail pass + plain convolution in the storage mode")
        return
    if case.store == "bf16":
        assert y.dtype == torch.bfloat16 and torch.equal(y, out32[0].bfloat16()), case.name       # rounded once
        if out[1] is not None:
            assert torch.equal(out[1], out32[1]), case.name                                       # statistics: from the fp32 accumulators
        if call.endswith("_emit"):
            orow = y.numel() // Cout                                  # (the images of the STORED output, as a pass of its own would cut them)
            assert torch.equal(y._koaf_eplanes[0], ops.act_planes(y, orow, Cout, 1, emd[0], emd[1], fscale=ops.ACT_SCALE)), case.name
        print(f"\n[tiles] {case.name:24s} {r['variant']:17s} {r['bm']:3d}x{r['bn']:<3d} tiles {r['tiles']:4d} grid.x {r['grid_x']:4d} "
              f"tf {r['a_tf']} act16 {r['act16']} | bit-equal to the fp32 mode on widened inputs, rounded once")
        return
    # float64 reference of the operand the loader forms, and torch's fp32 product of the same operands for the componentwise bar
    x64, w64 = x.double(), w.double()
    if call == "plain":
        a64, a32 = x64, x
    else:
        a64, a32 = x64 * sc.double() + sh.double(), x * sc + sh
        if call.startswith("tail"):
            i64, i32 = idt.double(), idt
            if ids is not None:
                i64, i32 = i64 * ids[2].double() + ids[3].double(), idt * ids[2] + ids[3]
            a64, a32 = a64 + i64, a32 + i32
        a64, a32 = torch.relu(a64), torch.relu(a32)
    y64 = _conv64(a64, w64, k, s, p)
    y32 = _conv64(a32, w, k, s, p)
    den = _conv64(a32.abs(), w.abs(), k, s, p).double() + 1e-300         # (|a| @ |b|: fp32 is plenty for a denominator)
    be = band_errors(y, y64.reshape(-1, Cout))
    whole = rel_err(y, y64)
    cw, bar = componentwise(y, y64, y32, den)
    report(case, r, be.max().item(), whole, cw, bar)
    assert be.max().item() < FWD, (case.name, int(be.argmax()), be.max().item())
    assert whole < FWD, case.name
    assert cw <= bar, (case.name, cw, bar)
    if call.startswith("tail"):
        assert rel_err(out[2], a64) < 1e-6, case.name          # the side-stored tail (test_bottleneck_tail's bar)
    if call.endswith("_emit"):
        orow = y64.numel() // Cout
        assert torch.equal(y._koaf_eplanes[0], ops.act_planes(y, orow, Cout, 1, emd[0], emd[1], fscale=ops.ACT_SCALE)), case.name
    else:
        yr = y64.reshape(-1, Cout)
        assert rel_err(out[1][:, 0].double().sum(0), yr.sum(0)) < 1e-4, case.name
        assert rel_err(out[1][:, 1].double().sum(0), (yr * yr).sum(0)) < 1e-5, case.name


def run_dgrad(dev, case):
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout, k, s, p = case.shape
    OH, OW = conv_out(H, k, s, p), conv_out(W, k, s, p)
    orow, rows = N * OH * OW, N * H * W
    call, b16 = case.call, case.store == "bf16"
    w = rnd(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5)
    wd = w.to(dev)
    img = ops.build_weight_planes(wd, Cout, k * k, Cin)
    res = rnd(N, H, W, Cin) * 1e-3 if call != "plain" and call != "apply" else None
    resd = res.to(dev) if res is not None else None
    use_apply = call in ("apply", "apply_res", "bnb2")

    def stored(t):      # an ACTIVATION of the call in the storage mode under test: bf16 values, kept as bf16 or widened
        return t.bfloat16() if b16 else t

    if use_apply:
        c = stored((rnd(N, OH, OW, Cout) * 1.5 + 0.3).to(dev))         # the conv output whose BatchNorm is back-propagated
        g = (rnd(N, OH, OW, Cout) * 1e-3).to(dev)
    else:
        dy = rnd(N, OH, OW, Cout) * 1e-3
        dyd = dy.to(dev)
        am = dyd.abs().max().reshape(1).float()
    bnb_t = None
    if call.startswith("bnb"):
        cx = rnd(N, H, W, Cin) * 1.5 + 0.3                              # the producer's conv output and its BatchNorm record
        sv = torch.stack([rnd(Cin) * 0.3, torch.rand(Cin, generator=G_) + 0.5, (rnd(Cin) * 0.5 + 1).abs().clamp(min=0.25), rnd(Cin) * 0.2])
        # mode 2 masks by the sign of sc * c + sh: the inputs keep that value out of rounding's reach (|.| > 1e-5 on values of order 1)
        cx = torch.where((cx * sv[2] + sv[3]).abs() < 1e-3, cx + 0.1, cx)
        if b16:
            cx = cx.bfloat16().float()
        assert float((cx.double() * sv[2].double() + sv[3].double()).abs().min()) > 1e-5
        yk = rnd(N, H, W, Cin)                                          # mode 1 masks by y > 0
        c2 = rnd(N, H, W, Cin)
        sv2 = torch.stack([rnd(Cin) * 0.3, torch.rand(Cin, generator=G_) + 0.5, rnd(Cin), rnd(Cin)])
        if b16:
            yk, c2 = yk.bfloat16().float(), c2.bfloat16().float()
        bnb_t = dict(cx=cx, sv=sv, y=yk, c2=c2, sv2=sv2)

    gam, bet = (rnd(Cout) * 0.2 + 1).to(dev), (rnd(Cout) * 0.1).to(dev)

    def bn_record(x, rows_, C):     # (the same affine parameters in both storage modes)
        return ops.bn_finalize(ops.colstats(x, rows_, C), C, rows_, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev),
                               torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)

    def one(store16):
        """the call in one storage mode (False: every activation widened to fp32)"""
        def act(t):
            return t.to(dev).bfloat16() if store16 else t.to(dev).float()
        kw = dict(wimg=img)
        if use_apply:
            cc = act(c)
            svc = bn_record(cc, orow, Cout)
            dgm, dbt = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
            arg = ops.bn_bwd(g.clone(), cc, svc, orow, Cout, orow, dgm, dbt, 2, fused=True)
        else:
            arg = dyd
            kw["dy_amax"] = am
        if resd is not None:
            kw["residual"] = resd
        if call == "bnb1":
            kw["bnb"] = dict(mode=1, c=act(bnb_t["cx"]), y=act(bnb_t["y"]), saved=bnb_t["sv"].to(dev), c2=act(bnb_t["c2"]),
                             saved2=bnb_t["sv2"].to(dev))
        elif call == "bnb2":
            kw["bnb"] = dict(mode=2, c=act(bnb_t["cx"]), saved=bnb_t["sv"].to(dev), dz_amax=True)
        with Record() as rec:
            out = ops.conv2d_dgrad(arg, wd, N, H, W, Cin, Cout, k, k, s, p, **kw)
        torch.cuda.synchronize()
        return (out if isinstance(out, tuple) else (out,)), rec.launches, arg

    was = ops.set_stream(case.stream)
    try:
        if b16:
            out32, _, _ = one(False)
        out, launches, arg = one(b16)
    finally:
        ops.set_stream(was)
    r = check_record(case, launches, 2 if b16 else 0)
    if b16:
        for a, b in zip(out, out32):
            assert a.dtype == torch.float32 and torch.equal(a, b), case.name          # gradients are never stored as bf16
        print(f"\n[tiles] {case.name:24s} {r['variant']:17s} {r['bm']:3d}x{r['bn']:<3d} tiles {r['tiles']:4d} grid.x {r['grid_x']:4d} "
              f"tf {r['a_tf']} act16 {r['act16']} | bit-equal to the fp32 mode on widened inputs")
        return
    w64 = w.double()
    if use_apply:
        coef, dz, cc = arg.coef.double().cpu(), arg.dz.double().cpu(), arg.c.double().cpu()
        dy64 = coef[0] * dz + coef[3] - coef[2] * cc
        c32 = arg.coef.cpu()
        dy32 = c32[0] * arg.dz.cpu() + c32[3] - c32[2] * arg.c.float().cpu()
    else:
        dy64, dy32 = dy.double(), dy
    g64 = _dgrad64(dy64, w64, case.shape)
    g32 = _dgrad64(dy32, w, case.shape)
    den = _dgrad64(dy32.abs(), w.abs(), case.shape).double()
    if res is not None:
        g64, g32, den = g64 + res.double(), g32 + res, den + res.double().abs()
    extra = ""
    if call.startswith("bnb"):
        cx, sv = bnb_t["cx"].double(), bnb_t["sv"].double()
        mask = (bnb_t["y"] > 0) if call == "bnb1" else ((cx * sv[2] + sv[3]) > 0)
        g64, g32 = g64 * mask, g32 * mask
        sums = [g64.sum((0, 1, 2)), (g64 * ((cx - sv[0]) * sv[1])).sum((0, 1, 2))]
        if call == "bnb1":
            sv2 = bnb_t["sv2"].double()
            sums.append((g64 * ((bnb_t["c2"].double() - sv2[0]) * sv2[1])).sum((0, 1, 2)))
        part = out[1]
        assert part.shape[1] == len(sums), case.name
        errs = [rel_err(part[:, i].double().sum(0), ref) for i, ref in enumerate(sums)]
        extra = " | partials " + " ".join(f"{e:.1e}" for e in errs)
    dx = out[0].cpu()
    bes = [band_errors(a, b) for a, b in zip(_class_rows(dx, case.shape), _class_rows(g64, case.shape))]
    worst, where = max((be.max().item(), (i, int(be.argmax()))) for i, be in enumerate(bes))       # (class, band) of the worst band
    whole = rel_err(dx, g64)
    cw, bar = componentwise(dx, g64, g32, den + 1e-300)
    report(case, r, worst, whole, cw, bar, extra)
    assert worst < BWD, (case.name, where, worst)
    assert whole < BWD, case.name
    assert cw <= bar, (case.name, cw, bar)
    if call.startswith("bnb"):
        assert all(e < 1e-4 for e in errs), (case.name, errs)
        if call == "bnb2":
            assert abs(float(out[2]) / float(out[0].abs().max()) - 1) < 1e-6, case.name


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.name for c in TILE_CASES])
def test_production_tile_variants(dev, case):
    try:
        (run_forward if case.op == "fwd" else run_dgrad)(dev, case)
    finally:
        torch.cuda.empty_cache()
