"""CPU guard of tests/test_conv3_edges_gpu.py: every row of its shape table still gets the kernel tile it claims.

plan_tiles (koaf_gemm.hip; host code, the library loads without a GPU) sends a 3x3 / stride-1 / pad-1 convolution over activation plane
images to the rectangle kernel, to one of the two halo shapes or back to the per-tap gather kernel on the picker's tile.  Each row is
asked through koaf_gemm_part_rows on the descriptor koaf_conv2d_fwd / koaf_conv2d_dgrad_bnb form for it (placeholder addresses: the
planning code reads no memory): the forward with gather 1 and the F image at the fixed activation scale, the data gradient with gather
2, A.amax set and the D image as B.  A later change to the rule, to halo_max_w or to the shapes fails here, on any machine; the variant
itself is asserted from the launch record on the GPU."""
import ctypes

import pytest
import torch

from test_conv3_edges_gpu import FULL, G, H128, H256, ROWS, T2D, gemm_dims, tile_order
from test_tiles_gpu import TILE_CASES


def _descriptor(row):
    from oaprogressionmmf_amd import _lib
    N, H, W, Cin, Cout = row.shape
    M, Ng, K = gemm_dims(row)
    fwd = row.op == "fwd"
    Ca = Cin if fwd else Cout                # the channels of the gathered operand: x forward, dy in the data gradient
    fake = 0x10000
    g = _lib.KoafGemm()
    g.M, g.N, g.K = M, Ng, K
    g.nb0 = g.nb1 = g.splitk = 1
    g.A.kind, g.A.gather, g.A.planes, g.A.zeros, g.A.plane_stride = 2, 1 if fwd else 2, fake, fake, M * Ca
    g.A.H, g.A.W, g.A.C, g.A.CS, g.A.PH, g.A.PW = H, W, Ca, Ca, H, W
    g.A.KH, g.A.KW, g.A.stride, g.A.pad, g.A.pad_w = 3, 3, 1, 1, 1
    if fwd:
        g.A.fscale = 16.0
    else:
        g.A.amax = fake
    g.B.kind, g.B.planes, g.B.amax, g.B.ld, g.B.plane_stride = 2, fake, fake, K, Ng * K      # F image [2][Cout][9 Cin] | D image [2][Cin][9 Cout]
    g.fmt, g.C, g.ldc = 1, fake, Ng
    if not fwd:
        g.residual, g.ldr = fake, Ng
    return g


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_rows_get_the_tile_they_claim(row):
    from oaprogressionmmf_amd import _lib, ops
    L = _lib.lib()
    M = gemm_dims(row)[0]
    was = ops.set_conv3x3_halo(row.halo)
    try:
        assert L.koaf_gemm_part_rows(ctypes.byref(_descriptor(row))) == -(-M // row.bm), row.name
    finally:
        ops.set_conv3x3_halo(was)
    if row.variant == G:        # a refusal: the picker's tile
        bm, bn = ctypes.c_int32(), ctypes.c_int32()
        assert L.koaf_gemm_pick_tile(ctypes.byref(_descriptor(row)), ctypes.byref(bm), ctypes.byref(bn)) == 0
        assert (bm.value, bn.value) == (row.bm, row.bn), row.name


def test_table_reaches_every_kernel_tile_and_orientation():
    """the table itself: every (variant, bn) in both orientations, full call sets and bf16 storage on at least two rows of each kernel and
    orientation, both sides of each width limit, both forced halo modes, unique names"""
    have = {(r.variant, r.bn, r.op) for r in ROWS}
    for want in ((T2D, 64, "fwd"), (T2D, 64, "dgrad"), (H128, 64, "fwd"), (H128, 64, "dgrad"), (H128, 128, "fwd"), (H128, 128, "dgrad"),
                 (H256, 64, "fwd"), (H256, 64, "dgrad"), (H256, 128, "fwd"), (H256, 128, "dgrad"), (G, 64, "fwd")):
        assert want in have, want
    for variant in (T2D, H128, H256):
        for op in ("fwd", "dgrad"):
            assert sum(r.variant == variant and r.op == op and r.calls == FULL[op] and r.halo == 1 for r in ROWS) >= 2, (variant, op)
    # the t2d rows: both GEMM widths in both orientations
    assert {(gemm_dims(r)[1], r.op) for r in ROWS if r.variant == T2D} == {(64, "fwd"), (128, "fwd"), (64, "dgrad"), (128, "dgrad")}
    # width limits, forward orientation: (W, variant) on both sides
    fw = {(r.shape[2], r.shape[3], r.shape[4], r.variant) for r in ROWS if r.op == "fwd" and r.halo == 1}
    fw |= {(c.shape[2], c.shape[3], c.shape[4], c.variant) for c in TILE_CASES if c.op == "fwd" and c.shape[5:] == (3, 1, 1)}
    for inside, outside in (((96, 64, 64, T2D), (112, 64, 64, G)), ((96, 64, 64, H128), (97, 64, 64, G)), ((96, 128, 64, H256), (97, 128, 64, G)),
                            ((64, 128, 128, H256), (65, 128, 128, G)), ((48, 64, 128, H128), (49, 64, 128, H256)),
                            ((64, 64, 128, T2D), (80, 64, 128, G))):
        assert inside in fw and outside in fw, (inside, outside)
    assert {r.halo for r in ROWS} == {1, 2, 3}
    assert len({r.name for r in ROWS}) == len(ROWS)
    # odd chunk counts of the double-buffered halo (32 channels a chunk) in both orientations, half-filled column tiles at both widths
    chunks = {((r.shape[3] if r.op == "fwd" else r.shape[4]) // 32, r.op) for r in ROWS if r.variant == H256}
    assert {(3, "fwd"), (5, "fwd"), (3, "dgrad"), (5, "dgrad")} <= chunks
    half = {(r.bn, r.op) for r in ROWS if r.variant == H256 and gemm_dims(r)[1] % r.bn}
    assert half == {(64, "fwd"), (128, "fwd"), (64, "dgrad"), (128, "dgrad")}


def test_tile_order_covers_every_pixel_once():
    """the reordering of the rows into tile order: a permutation on every row; on the t2d rows tile t = (image, tile row, tile column)
    holds the pixels (8 ty .. 8 ty + 7) x (16 tx .. 16 tx + 15) of ONE image in (y, x) order, as koaf_gemm_kernel's M_PT branch maps them"""
    seen = 0
    for row in ROWS:
        order = tile_order(row)
        N, H, W = row.shape[:3]
        assert torch.equal(order.sort().values, torch.arange(N * H * W)), row.name
        if row.variant != T2D:
            assert torch.equal(order, torch.arange(N * H * W)), row.name
            continue
        seen += 1
        txn, tpi = W // 16, (H // 8) * (W // 16)
        for t in range(N * tpi):
            img, ty, tx = t // tpi, (t % tpi) // txn, t % txn
            px = order[128 * t:128 * t + 128]
            n, yy, xx = px // (H * W), (px // W) % H, px % W
            assert bool((n == img).all()) and bool((yy // 8 == ty).all()) and bool((xx // 16 == tx).all()), (row.name, t)
            assert torch.equal((yy % 8) * 16 + xx % 16, torch.arange(128)), (row.name, t)
    assert seen >= 9
