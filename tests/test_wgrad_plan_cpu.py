"""CPU guard of tests/test_wgrad_gpu.py: every row of its table still gets the split-K plan it claims.

wgrad_plan (koaf_conv.hip) and the ring kernel's k-range count (koaf_wgrad3.hip) are host code and the library loads without a
GPU: the split count of every row is recovered from the workspace functions -- koaf_conv2d_wgrad_ws = (splitk + 16) * Cout * k^2 *
Cin, koaf_gconv3x3_wgrad_ws = splitk * C * 576 -- and held against the row.  From splitk and the contracted pixels the k-range
geometry of koaf_gemm_kernel (kchunk = roundup32(ceil(K / splitk))) gives each row's empty and short trailing splits and whether
the XCD remap runs.  A later change to the plan -- or to the shapes -- fails here, on any machine, instead of silently turning the
split-K parity cases back into two- and three-split runs."""
import pytest

from test_tiles_gpu import n_tiles
from test_wgrad_gpu import G, RING, WGRAD_CASES, dims, ring_geometry, ring_takes, split_geometry, two_level_reduce


def plan_of(case):
    """(splitk, empty, rows of the last live split) as the library plans the row"""
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    M, Ng, P = dims(case)
    if case.kind == "grouped":
        N, H, W, C, s = case.shape
        ws = L.koaf_gconv3x3_wgrad_ws(N, H, W, C, s)
        assert ws % (C * 576) == 0, case.name
        splitk = ws // (C * 576)
    else:
        N, H, W, Cin, Cout, k, s, p = case.shape
        ws, n = L.koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, k, k, s, p), M * Ng
        assert ws > 0 and ws % n == 0, case.name
        if case.variant == RING:
            # the larger of the GEMM's and the ring's workspace; at these shapes the ring's (its k-ranges outnumber the GEMM's splits)
            D, nchunk, nk, ncomb, empty = ring_geometry(case)
            assert ring_takes(case), case.name
            assert ws >= (nk + 16) * n and ws == (nk + 16) * n, (case.name, ws, nk)
            per = -(-nchunk // nk)
            return nk, empty, nchunk - (nk - empty - 1) * per
        assert not ring_takes(case), case.name
        splitk = ws // n - 16
    return (splitk,) + split_geometry(P, splitk)[1:]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c.name for c in WGRAD_CASES])
def test_table_rows_get_the_split_plan_they_claim(case):
    splitk, empty, last = plan_of(case)
    assert splitk == case.splitk, (case.name, splitk)
    assert empty == case.empty, (case.name, empty)
    assert last >= 1, case.name
    if case.variant == RING:
        assert not case.remap, case.name                  # (the ring deals its k-ranges to the XCDs itself)
        return
    assert case.remap == (splitk > 1 and splitk % 8 == 0), (case.name, splitk)
    # the tile rule of wgrad_plan, restated: 128 rows from M = 128 on; 128 columns from N = 128 on (the launch record is the judge)
    M, Ng, P = dims(case)
    want = (64, 64) if case.kind == "grouped" else (128 if M >= 128 else 64, 128 if Ng >= 128 else 64)
    assert (case.bm, case.bn) == want, case.name
    assert P >= 512 * (splitk - 1), case.name               # at least 512 k-rows per split asked for


def test_table_reaches_every_plan_it_is_there_for():
    """the table itself (each row's claim is asserted from the launch record on the GPU)"""
    rows = []
    for c in WGRAD_CASES:
        M, Ng, P = dims(c)
        splitk, empty, last = plan_of(c)
        gemm = c.variant == G
        rows.append(dict(c=c, gemm=gemm, tiles=n_tiles(M, Ng, c.bm, c.bn), splitk=splitk, empty=empty, last=last,
                         batch=c.shape[3] // 64 if c.kind == "grouped" else 1, two=two_level_reduce(splitk, M * Ng) and c.kind != "grouped"))

    def have(what, pred):
        assert any(pred(r) for r in rows), what
    for bm, bn in ((128, 128), (128, 64), (64, 128)):
        have(f"a remapped plan with several tiles per split at {bm} x {bn}",
             lambda r: r["gemm"] and r["c"].remap and r["tiles"] > 1 and (r["c"].bm, r["c"].bn) == (bm, bn))
    have("a non-remapped plan with splitk > 1", lambda r: r["gemm"] and not r["c"].remap and r["splitk"] > 1)
    have("an empty split", lambda r: r["gemm"] and r["empty"] > 0)
    have("a last live split shorter than one k-tile", lambda r: r["gemm"] and r["last"] < 32)
    have("a two-level reduce", lambda r: r["gemm"] and r["two"])
    have("a batched remapped plan", lambda r: r["gemm"] and r["c"].remap and r["batch"] > 1)
    have("act16 3 on a dense split plan", lambda r: r["c"].kind == "dense" and r["c"].store == "bf16" and r["splitk"] > 3)
    have("act16 3 on a grouped split plan", lambda r: r["c"].kind == "grouped" and r["c"].store == "bf16" and r["splitk"] > 3)
    have("the production 1x1 combination past 3 splits",
         lambda r: r["c"].kind == "dense" and r["c"].call == "apply_prologue" and r["c"].shape[5] == 1 and r["splitk"] > 3)
    have("the plane-image GEMM at 128 x 128 where the ring refuses W < 16",
         lambda r: r["c"].kind == "planes" and r["c"].shape[2] < 16 and (r["c"].bm, r["c"].bn) == (128, 128))
    have("wgrad3x3_ring_kernel<8>", lambda r: r["c"].variant == RING and 2 * ring_geometry(r["c"])[0] + 3 <= 8)
    have("wgrad3x3_ring_kernel<16>", lambda r: r["c"].variant == RING and 8 < 2 * ring_geometry(r["c"])[0] + 3 <= 16)
    have("ring k-ranges of different lengths", lambda r: r["c"].variant == RING and r["empty"] > 0 and r["last"] == 1)
    have("the ring's refusal past W = 189", lambda r: r["c"].kind == "ring" and r["gemm"] and r["c"].shape[2] > 189)
    # both sides of each ring edge, one column apart
    widths = {r["c"].shape[2]: r["c"].variant for r in rows if r["c"].kind == "ring"}
    assert (widths[61], widths[62], widths[189], widths[190]) == (RING, RING, RING, G)
    assert len({c.name for c in WGRAD_CASES}) == len(WGRAD_CASES)


def test_slabs_keyword_is_optional():
    """ops.conv2d_wgrad / ops.gconv3x3_wgrad: `slabs=None` keeps the allocation inside the call"""
    import inspect
    from oaprogressionmmf_amd import ops
    for f in (ops.conv2d_wgrad, ops.gconv3x3_wgrad):
        assert inspect.signature(f).parameters["slabs"].default is None


@pytest.mark.parametrize("N,H,W", [(1, 9, 9), (1, 8, 70), (3, 33, 50), (2, 384, 384), (1280, 384, 384)])
def test_stem_slab_count_and_statistics_rows(N, H, W):
    """The stem's weight gradient sums min(1024, N * ceil(OH / 4) * ceil(OW / 16)) slabs and its forward writes N * ceil(OH / 4)
    statistics rows: both counts decide the order of fp32 sums, so they are part of what the library computes (koaf_stem.hip:
    SM_TH, SW_TILE_W).  Read back through koaf_stem_wgrad_ws = (slabs + 16) * 49 * 64 and koaf_stem_stats_rows."""
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    bands, tiles_w = -(-OH // 4), -(-OW // 16)
    assert L.koaf_stem_stats_rows(N, H) == N * bands
    assert L.koaf_stem_wgrad_ws(N, H, W) == (min(1024, N * bands * tiles_w) + 16) * 49 * 64
