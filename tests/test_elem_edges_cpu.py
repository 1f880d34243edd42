"""The references, generators and bounds of test_elem_edges_gpu.py (elem_refs.py), checked without a GPU: against torch's own
float64 ops where torch has the op, against the library's host-side geometry query, and against an fp32 emulation of the column
kernels' summation order -- which must stay inside the bound, and leave it when one row is dropped."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elem_refs as R
from elem_refs import U

WIDTHS = [4, 8, 128, 512, 1024, 2048, 3072]
GROWN = [(70001, 64, 1024), (1500, 2048, 256), (16500, 64, 256)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_col_geom_twin_matches_the_library():
    """koaf_colpart_rows / koaf_layernorm_bwd_ws / koaf_colsum_ws are host code: the Python twin of col_geom gives their answers"""
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    widths = WIDTHS + [16, 64, 256, 4096, 6, 12, 20, 1536, 2, 1028, 5120]
    rows = [1, 2, 15, 16, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000, 65536, 65537, 70001, 1 << 20, (1 << 20) + 1]
    for C in widths:
        for r in rows:
            g = R.col_geom(r, C, 1024)
            assert L.koaf_colpart_rows(r, C) == (g["nblk"] if g else -1), (r, C)
            g = R.col_geom(r, C, 256)
            assert L.koaf_layernorm_bwd_ws(r, C) == (g["nblk"] * 2 * C if g else -1), (r, C)
            assert L.koaf_colsum_ws(r, C) == (g["nblk"] * C if g else 0), (r, C)
    for C in (6, 12, 20, 1536):
        assert R.col_geom(8, C) is None
    for C in WIDTHS:
        g = R.col_geom(10, C)
        assert g["RP"] == R.col_rp(C) and g["rpb"] == 4 * g["RP"] and g["CV"] * g["RP"] == 256
    assert R.col_rp(4) == 256 and R.col_geom(1, 3072)["nchunk"] == 3
    assert [R.col_geom(r, C, mb)["rpb"] for r, C, mb in GROWN] == [80, 6, 80]
    assert R.EW_CAP == 1 << 21


def test_case_a_rows_reach_every_branch():
    for C in WIDTHS:
        RP = R.col_rp(C)
        rows = R.case_a_rows(C)
        assert 1 in rows and 4 * RP in rows and 4 * RP + 1 in rows and (RP == 1 or RP - 1 in rows)
        nblk = [R.col_geom(r, C)["nblk"] for r in rows]
        assert 1 in nblk and 2 in nblk and 4 in nblk
        assert R.col_geom(4 * RP, C)["nblk"] == 1 and R.col_geom(4 * RP + 1, C)["nblk"] == 2
        assert rows[-1] % (4 * RP) != 0 and rows[-1] % RP != 0 or RP == 1


@pytest.mark.parametrize("C", WIDTHS)
def test_summation_bound_holds_for_the_kernel_order_and_catches_a_dropped_row(C):
    for i, rows in enumerate(R.case_a_rows(C)):
        _emulation_case(rows, C, 1024, 10 + i)


@pytest.mark.parametrize("rows,C,max_blk", GROWN)
def test_summation_bound_where_the_blocks_grow(rows, C, max_blk):
    _emulation_case(rows, C, max_blk, 20)


def _emulation_case(rows, C, max_blk, seed):
    g = gen(seed)
    x = (torch.randn(rows, C, generator=g) * 2.0 + torch.randn(C, generator=g)[None, :]).numpy()
    x64 = x.astype(np.float64)
    sq32 = (x * x).astype(np.float32)                      # one rounding of the term
    for terms32, ref, absref, tr in ((x, x64.sum(0), np.abs(x64), 0), (sq32, (x64 * x64).sum(0), x64 * x64, 1)):
        bound = R.col_bound(rows, C, max_blk, tr, torch.from_numpy(absref)).numpy()
        err = np.abs(R.emulate_colsum(terms32, max_blk).astype(np.float64) - ref)
        assert (err <= bound).all(), (rows, C, tr, float((err / bound).max()))
        # the last row left out (`rend - 1`): off by that row's term, about sum|t| / rows -- beyond the bound wherever the term is
        # not itself below it, which is most channels at every shape
        err = np.abs(R.emulate_colsum(terms32, max_blk, drop_row=rows - 1).astype(np.float64) - ref)
        big = absref[rows - 1] > 2 * bound
        assert big.mean() >= 0.5, (rows, C, tr, float(big.mean()))
        assert (err[big] > bound[big]).all(), (rows, C, tr)


def test_mask_generator_leaves_no_borderline_element():
    g = gen(30)
    C = 64
    sc, sh = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3
    c = R.draw_preact(g, (70001, C), sc, sh)
    assert not R.borderline(c, sc, sh).any()
    # outside the margin the fp32 sign is the exact one, fused or not
    z64 = c.double() * sc.double() + sh.double()
    assert torch.equal((c * sc + sh) > 0, z64 > 0) and torch.equal(torch.addcmul(sh, c, sc) > 0, z64 > 0)
    # and the test sees a planted one: c = -sh / sc makes the pre-activation vanish to within its rounding
    c[5] = -sh / sc
    assert R.borderline(c, sc, sh)[5].any()
    # the exact grid: sc * c + sh carries no rounding at all
    sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    sh = torch.randint(-8, 9, (C,), generator=g).float() / 16
    c = R.draw_grid(g, (3, 9, 10, C))
    assert torch.equal((c * sc + sh).double(), c.double() * sc.double() + sh.double())
    assert int((c * sc + sh == 0).sum()) > 0


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 1, 7), (2, 7, 1), (1, 2, 2), (3, 5, 8), (2, 9, 6), (2, 12, 13)])
def test_maxpool_reference_is_torch_max_pool2d_first_maximum(N, H, W):
    g = gen(40 + H + W)
    C = 8
    for ties in (False, True):
        a = torch.relu(R.draw_grid(g, (N, H, W, C), step=0.5 if ties else 2.0 ** -4)).double()      # (coarse grid, half zeros: many ties)
        y, am = R.maxpool_ref(a)
        leaf = a.permute(0, 3, 1, 2).clone().requires_grad_(True)
        y_t, idx = F.max_pool2d(leaf, 3, 2, 1, return_indices=True)
        assert torch.equal(y, y_t.detach().permute(0, 2, 3, 1))
        # torch's flat index iy * W + ix of the maximum it took == the window position the reference recorded
        OH, OW = R.pool_out(H), R.pool_out(W)
        oy, ox = torch.arange(OH)[None, :, None, None], torch.arange(OW)[None, None, :, None]
        flat = (oy * 2 - 1 + am.long() // 3) * W + (ox * 2 - 1 + am.long() % 3)
        assert torch.equal(flat, idx.permute(0, 2, 3, 1)), "the reference's tie rule is not torch's (first maximum, row-major)"
        dy = torch.randn(N, OH, OW, C, generator=g)
        y_t.backward(dy.double().permute(0, 3, 1, 2))
        da, ab = R.maxpool_bwd_ref(dy, am, H, W)
        da2, ab2 = R.maxpool_bwd_gather_ref(dy, am, H, W)
        want = leaf.grad.permute(0, 2, 3, 1)
        assert (da - want).abs().max() <= 1e-15 and (da2 - want).abs().max() <= 1e-15
        assert (ab - ab2).abs().max() <= 1e-15 and (ab >= da.abs() - 1e-15).all()


def test_pointwise_and_layernorm_references_are_torch_float64():
    g = gen(50)
    x = (torch.randn(4001, generator=g) * 3).double().requires_grad_(True)
    y = F.gelu(x)
    assert (R.gelu_ref(x.detach()) - y.detach()).abs().max() < 1e-15
    y.backward(torch.ones_like(y))
    assert (R.gelu_grad_ref(x.detach()) - x.grad).abs().max() < 1e-15
    x = torch.randn(5, 256, generator=g) * 3 + 1
    gam, bet = torch.randn(256, generator=g), torch.randn(256, generator=g)
    yr, m, rs = R.layernorm_ref(x, gam, bet, 1e-5)
    assert (yr - F.layer_norm(x.double(), (256,), gam.double(), bet.double(), 1e-5)).abs().max() < 1e-13
    assert (m - x.double().mean(1)).abs().max() < 1e-15


def test_augment_reference_layout():
    g = gen(60)
    B, Rr, Cc, S = 3, 6, 6, 2
    raw = (torch.rand(B, Rr, Cc, S, generator=g) * 0.7 + 0.3) * 300
    unit = lambda b: (raw[b].double() - raw[b].double().min()) / (raw[b].double().max() - raw[b].double().min())     # noqa: E731
    prm = torch.tensor([[1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 2.0, 1.0], [math.cos(math.pi / 2), math.sin(math.pi / 2), 0.5, 1.0]])
    y = R.augment_ref(raw, prm, 0.4, 0.2)
    assert y.shape == raw.shape and y.dtype == torch.float64
    assert ((y[0] - (unit(0) - 0.4) / 0.2).abs().max()) < 1e-14                     # not rotated, no gamma
    assert ((y[1] - (unit(1) ** 2 - 0.4) / 0.2).abs().max()) < 1e-12                # rotated by 0 == not rotated
    # (cos, sin) = (0, 1) on a square image: out[r][c] = in[c][C - 1 - r], a quarter turn
    assert ((y[2] - (torch.rot90(unit(2), 1, (0, 1)) ** 0.5 - 0.4) / 0.2).abs().max()) < 1e-9
    # 45 degrees: the corners sample outside the image and read zeros
    prm = torch.tensor([[math.cos(math.pi / 4), math.sin(math.pi / 4), 0.0, 1.0]] * B)
    y = R.augment_ref(raw, prm, 0.4, 0.2)
    assert (y[:, 0, 0] - (0.0 - 0.4) / 0.2).abs().max() < 1e-12
    y32 = R.augment_ref(raw, prm, 0.4, 0.2, dtype=torch.float32)
    assert y32.dtype == torch.float32 and (y32.double() - y).abs().max() < 1e-4


@pytest.mark.parametrize("n", [100, 520])
def test_exact_attention_scores(n):
    h, d, scale = 4, 16, 0.5
    q, k, v = R.exact_attention_qk(gen(70 + n), n, h, d)
    assert set(q.abs().unique().tolist()) <= {0.0, 1.0, 2.0, 4.0}
    assert float(k.abs().max()) <= 8 and torch.equal(k * 2, (k * 2).round())
    # every operand is a bf16 value: the first of the three pieces holds it all
    assert torch.equal(q.bfloat16().float(), q) and torch.equal(k.bfloat16().float(), k)
    s64 = torch.einsum("ihd,jhd->hij", q.double(), k.double()) * scale
    assert torch.equal((torch.einsum("ihd,jhd->hij", q, k) * scale).double(), s64)
    assert float(s64.max()) >= 150 and float(s64.min()) <= -150
    # the model's own scale (h d)^-0.5 = 1 / 8 cannot bring these operands past expf's overflow
    assert 4 * 8 * d * (h * d) ** -0.5 < 88
    # what a softmax without the maximum does here
    assert not torch.isfinite(torch.exp(s64.float()) / torch.exp(s64.float()).sum(-1, keepdim=True)).all()
    assert torch.isfinite(s64.float().softmax(-1)).all()


def test_bound_helpers():
    assert R.gamma(1) == pytest.approx(U, rel=1e-6) and R.gamma(1000) > 1000 * U
    assert R.col_chain(1, 64, 1024, 0) == 4 + 15 + 0 + 1
    assert R.col_chain(70001, 64, 1024, 3) == 5 + 15 + 3 + 1
    assert R.col_chain(1500, 2048, 256, 0) == 6 + 0 + 0 + 1
    assert R.cdiv(7, 2) == 4 and R.pool_out(1) == 1 and R.pool_out(2) == 1 and R.pool_out(514) == 257
