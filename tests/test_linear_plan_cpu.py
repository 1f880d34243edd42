"""CPU guard of tests/test_dense_plans_gpu.py: every row of its Linear table still gets the plan it claims.

linear_tile / linear_splitk (koaf_linear.hip) are host code and the library loads without a GPU: the split count of a row is
recovered from the workspace function -- koaf_linear_ws(M, N, K) = splitk * M * N for the forward, koaf_linear_ws(M, K, N) =
splitk * M * K for the data gradient, 0 when the call is not split -- and held against the row.  From the split count and the
contracted length the k-range geometry of koaf_gemm_kernel (kchunk = roundup32(ceil(K / splitk))) gives each row's last-split
length and whether the XCD remap runs.  A later change to the plan -- or to the shapes -- fails here, on any machine, instead of
silently turning the split and scalar-kernel rows into something else."""
import pytest

from test_dense_plans_gpu import HEAD, LINEAR_ROWS, row_id, vector_path
from test_wgrad_gpu import split_geometry


def narrow_head(M, N, K):
    """koaf_linear.hip narrow_head, restated"""
    return N <= 8 and M * N <= 4096 and K >= 64


def splits_of(M, N, K):
    """split count of the Linear GEMM M x N over K as the library plans it"""
    from oaprogressionmmf_amd import _lib
    ws = _lib.lib().koaf_linear_ws(M, N, K)
    assert ws % (M * N) == 0, (M, N, K, ws)
    return ws // (M * N) if ws else 1


def linear_tile(M, N):
    """koaf_linear.hip linear_tile, restated (the launch record is the judge)"""
    if M >= 512 and N >= 512:
        return 128, 128
    return (64, 64) if N < 1024 else (64, 128)


@pytest.mark.parametrize("r", LINEAR_ROWS, ids=[row_id(r) for r in LINEAR_ROWS])
def test_table_rows_get_the_plan_they_claim(r):
    head = narrow_head(r.M, r.N, r.K)
    assert (r.fwd == HEAD) == head and (r.dgrad == HEAD) == head, row_id(r)
    if head:
        return
    for plan, (M, N, K) in ((r.fwd, (r.M, r.N, r.K)), (r.dgrad, (r.M, r.K, r.N))):
        bm, bn, sk = plan
        assert splits_of(M, N, K) == sk, (row_id(r), (M, N, K), splits_of(M, N, K))
        assert 1 <= sk <= 8
        if not vector_path(r):
            assert (bm, bn) == (64, 64), row_id(r)               # plan_tiles: the scalar kernels are 64 x 64
        elif sk > 1:
            assert (bm, bn) == linear_tile(M, N), row_id(r)
        if sk > 1:
            kchunk, empty, last = split_geometry(K, sk)
            assert empty == 0 and last >= 1 and K // sk >= 256, (row_id(r), kchunk, empty, last)


def test_table_reaches_every_plan_it_is_there_for():
    plans = {}
    for r in LINEAR_ROWS:
        if r.fwd != HEAD:
            plans[("fwd", r.M, r.N, r.K)] = (r.fwd, r.K, vector_path(r))
            plans[("dgrad", r.M, r.N, r.K)] = (r.dgrad, r.N, vector_path(r))

    def last(key):
        (bm, bn, sk), K, _ = plans[key]
        return split_geometry(K, sk)[0], split_geometry(K, sk)[2]
    # the geometry each row's comment states
    assert last(("fwd", 8, 2048, 600)) == (320, 280)
    assert last(("fwd", 200, 512, 1500)) == (320, 220)
    assert last(("dgrad", 3000, 2048, 512)) == (416, 384)
    assert last(("fwd", 8, 2048, 514)) == (288, 226) and last(("dgrad", 8, 514, 2048)) == (288, 226)

    def have(what, pred):
        assert any(pred(*v) for v in plans.values()), what
    for sk in (2, 4, 5, 8):
        have(f"{sk} splits", lambda p, K, vec, sk=sk: p[2] == sk)
    for tile in ((64, 64), (64, 128), (128, 128)):
        have(f"a split plan on the {tile} tile", lambda p, K, vec, tile=tile: vec and p[2] > 1 and p[:2] == tile)
    have("the XCD remap", lambda p, K, vec: p[2] > 1 and p[2] % 8 == 0)
    have("a split plan without the remap", lambda p, K, vec: p[2] > 1 and p[2] % 8 != 0)
    have("split-K on the scalar kernels", lambda p, K, vec: not vec and p[2] > 1)
    have("the scalar kernels unsplit", lambda p, K, vec: not vec and p[2] == 1)
    have("an unsplit 128 x 128 plan", lambda p, K, vec: vec and p == (128, 128, 1))
    # both sides of each term of the head boundary
    heads = {(r.M, r.N, r.K) for r in LINEAR_ROWS if r.fwd == HEAD}
    assert {(8, 2, 64), (8, 2, 65), (512, 8, 128)} <= heads and not {(8, 2, 63), (513, 8, 128), (8, 9, 128)} & heads
    assert len({row_id(r) for r in LINEAR_ROWS}) == len(LINEAR_ROWS)


def test_stem_wgrad_slabs_keyword_is_optional():
    """ops.stem_wgrad: `slabs=None` keeps the allocation inside the call"""
    import inspect
    from oaprogressionmmf_amd import ops
    assert inspect.signature(ops.stem_wgrad).parameters["slabs"].default is None
