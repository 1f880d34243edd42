"""CPU guard of tests/test_tiles_gpu.py: every row of its shape table still gets the tile it claims.

koaf_gemm_pick_tile (host code; the library loads without a GPU) shrinks a 128 tile while the grid is under its fill rule.  A later
change to that rule -- or to the shapes -- fails here, on any machine, instead of silently turning the production-tile parity
cases back into 64 x 64 runs.  The rows of the 3x3 halo kernels, which set their tile themselves, are asked through
koaf_gemm_part_rows on the descriptor koaf_conv2d_fwd forms (placeholder addresses: the planning code reads no memory)."""
import ctypes
import subprocess
from pathlib import Path

import pytest

from test_tiles_gpu import E, G, H128, H256, PERSIST, S, TILE_CASES, conv_out, gemm_dims, n_tiles


def _gemm(M, N, K):
    from oaprogressionmmf_amd import _lib
    g = _lib.KoafGemm()
    g.M, g.N, g.K = M, N, K
    g.nb0 = g.nb1 = g.splitk = 1
    return g


def _conv3_fwd_gemm(case, M, Ng, K):
    """3x3 / stride 1 / pad 1 forward over activation plane images with weight plane images, as koaf_conv2d_fwd forms it"""
    N, H, W, Cin, Cout, k, s, p = case.shape
    g = _gemm(M, Ng, K)
    fake = 0x10000
    g.A.kind, g.A.gather, g.A.planes, g.A.zeros, g.A.plane_stride = 2, 1, fake, fake, N * H * W * Cin
    g.A.H, g.A.W, g.A.C, g.A.CS, g.A.PH, g.A.PW = H, W, Cin, Cin, conv_out(H, k, s, p), conv_out(W, k, s, p)
    g.A.KH, g.A.KW, g.A.stride, g.A.pad, g.A.pad_w = k, k, s, p, p
    g.A.fscale = 16.0
    g.B.kind, g.B.planes, g.B.amax, g.B.ld, g.B.plane_stride = 2, fake, fake, K, Cout * K
    g.fmt, g.C, g.ldc = 1, fake, Cout
    return g


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.name for c in TILE_CASES])
def test_shape_table_rows_get_the_tile_they_claim(case):
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    worked = 0
    for M, Ng, K in gemm_dims(case):
        if K == 0:
            continue
        worked += 1
        if case.op == "fwd" and case.shape[5:] == (3, 1, 1):
            # the halo kernels set their tile themselves (W = 65: past their limit, the picker's tile again)
            assert L.koaf_gemm_part_rows(ctypes.byref(_conv3_fwd_gemm(case, M, Ng, K))) == -(-M // case.bm), case.name
            if case.variant in (H128, H256):
                continue
        bm, bn = ctypes.c_int32(), ctypes.c_int32()
        assert L.koaf_gemm_pick_tile(ctypes.byref(_gemm(M, Ng, K)), ctypes.byref(bm), ctypes.byref(bn)) == 0
        assert (bm.value, bn.value) == (case.bm, case.bn), (case.name, M, Ng, K)
        if case.walks:
            assert n_tiles(M, Ng, case.bm, case.bn) > PERSIST, case.name
    assert worked


def test_table_reaches_every_variant_it_is_there_for():
    """the table itself: streamed at 128 x 128 and 128 x 64, a walking persistent launch, block-wide 128-row kernels in both storage
    modes, stride 2 at 128 rows, both sides of the W = 64 | 65 edge (each row's claim is asserted from the launch record on the GPU)"""
    have = {(c.variant, c.bm, c.bn, c.walks, c.store, c.shape[6]) for c in TILE_CASES}
    for want in ((S, 128, 128, False, "fp32", 1), (S, 128, 64, False, "fp32", 1), (S, 128, 128, True, "fp32", 1),
                 (G, 128, 128, False, "fp32", 1), (G, 128, 64, False, "fp32", 1), (G, 128, 128, True, "fp32", 1),
                 (G, 128, 128, False, "bf16", 1), (G, 128, 64, False, "bf16", 1), (G, 128, 128, True, "bf16", 1),
                 (E, 128, 128, True, "fp32", 1), (G, 128, 128, False, "fp32", 2), (G, 128, 128, True, "fp32", 2),
                 (G, 128, 128, False, "bf16", 2), (H128, 128, 64, False, "fp32", 1), (H256, 256, 128, False, "fp32", 1),
                 (G, 64, 64, False, "fp32", 1)):
        assert want in have, want
    assert len({c.name for c in TILE_CASES}) == len(TILE_CASES)


def test_launch_record_layout_and_switch(tmp_path):
    """KoafLaunchRec: the ctypes layout is the C layout; the record is off by default, empty when switched on without a launch, and
    switching returns the previous setting (no GPU needed: nothing is launched)"""
    from oaprogressionmmf_amd import _lib, ops
    src = tmp_path / "rec.c"
    src.write_text('#include "koaf.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(KoafLaunchRec),'
                   'offsetof(KoafLaunchRec,bm),offsetof(KoafLaunchRec,act16),offsetof(KoafLaunchRec,emit));return 0;}\n')
    exe = tmp_path / "rec"
    subprocess.run(["gcc", "-I", str(Path(__file__).resolve().parent.parent / "include"), str(src), "-o", str(exe)], check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = _lib.KoafLaunchRec
    assert c == [ctypes.sizeof(R), R.bm.offset, R.act16.offset, R.emit.offset]
    assert ops.launch_log(True) is False            # off by default
    try:
        assert ops.launch_log_read() == []
        assert ops.launch_log(True) is True
    finally:
        assert ops.launch_log(False) is True
    assert ops.launch_log(False) is False
