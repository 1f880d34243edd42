"""The references, generators and bounds of test_elem_edges_gpu.py (elem_refs.py), checked without a GPU: against torch's own
float64 ops where torch has the op, against the library's host-side geometry query, and against an fp32 emulation of the column
kernels' summation order -- which must stay inside the bound, and leave it when one row is dropped.  Likewise what
test_elem_edges_bf16_gpu.py rests on: the bf16 generators, the bound of a stored output, the rounding table (round to nearest even
in integer arithmetic passes it; truncation, round-half-away and a read at fp32 stride do not), the plane images' reference."""
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


# =================================================================================================
# bf16 activation storage (test_elem_edges_bf16_gpu.py): generators, the stored-output bound, the rounding table
# =================================================================================================
def test_bf16_generators_draw_bf16_values():
    g = gen(80)
    C = 64
    # the exact grid: its values, and relu(sc * c + sh) with sc in {0.5, 1, 2} and sh a multiple of 1 / 16, are bf16 values -- the
    # exact pool cases compare a bf16 y bit for bit with the float64 reference
    c = R.draw_grid(g, (3, 9, 10, C))
    assert torch.equal(c.bfloat16().float(), c) and torch.equal(R.stored(c, torch.bfloat16), c)
    for s in (0.5, 1.0, 2.0):
        for h in range(-8, 9):
            a = torch.relu(c * s + h / 16)
            assert torch.equal(a.bfloat16().float(), a), (s, h)
    assert torch.equal(torch.relu(c * 0.5 + 0.25).bfloat16().float(), torch.relu(c * 0.5 + 0.25))      # (the ties case)
    # a bf16 draw: every value is a bf16 value, and none is borderline -- tested AFTER the rounding
    sc, sh = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3
    c = R.draw_preact(g, (70001, C), sc, sh, store=torch.bfloat16)
    assert c.dtype == torch.float32 and torch.equal(c.bfloat16().float(), c)
    assert not R.borderline(c, sc, sh).any()
    z64 = c.double() * sc.double() + sh.double()
    assert torch.equal((c * sc + sh) > 0, z64 > 0) and torch.equal(torch.addcmul(sh, c, sc) > 0, z64 > 0)
    # fp32 storage leaves the draw as it was: the fp32 cases see the values they always saw
    x = torch.randn(100, generator=gen(81))
    assert R.stored(x, torch.float32) is x or torch.equal(R.stored(x, torch.float32), x)
    assert torch.equal(R.draw_preact(gen(82), (50, C), sc, sh), R.draw_preact(gen(82), (50, C), sc, sh, store=torch.float32))


def test_stored16_bound():
    g = gen(83)
    # a value within B of the reference, rounded to bf16 by torch, is within the bound: normal values, subnormal ones, B = 0 and B > 0
    v = torch.cat([torch.randn(20000, generator=g) * 3, torch.randn(20000, generator=g) * 2.0 ** -128,
                   torch.randn(5000, generator=g) * 2.0 ** -126, torch.zeros(10)])
    assert int(((v != 0) & (v.abs() < 2.0 ** -126)).sum()) > 10000               # (the CPU keeps fp32 subnormals)
    for rel in (0.0, 3 * U):
        B = rel * v.double().abs()
        ref = v.double() + B * (torch.rand(v.shape, generator=g).double() * 2 - 1)
        B = (v.double() - ref).abs()                                            # (the distance as float64 formed it)
        err = (v.bfloat16().double() - ref).abs()
        assert (err <= R.stored16_bound(ref, B)).all()
        assert not (err <= B + 2.0 ** -9 * ref.abs()).all()                     # the typical error, 2^-9, is not a bound
    # it is the bound, not the typical error: a value just below a tie errs by almost u16 |ref|, twice test_bf16_gpu.py's 2^-9
    ref = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float64)
    err = (ref.float().bfloat16().double() - ref).abs()
    assert err > 0.99 * R.U16 * ref and err <= R.stored16_bound(ref, 0.0)
    assert float(R.stored16_bound(torch.zeros(1, dtype=torch.float64), 0.0)) == 2.0 ** -134
    assert R.U16 == 2.0 ** -8


def test_bf16_round_table_and_the_mistakes_it_catches():
    c, idt = R.bf16_round_cases()
    assert c.dtype == idt.dtype == torch.bfloat16 and c.numel() == idt.numel() and c.numel() % 4 == 0
    cb, c64, d64 = R.bf16_bits(c), c.double(), idt.double()
    # every non-negative pattern of c, subnormals and +Inf included
    assert set(range(0, 0x7F81)) <= set(cb.tolist())
    s64 = c64 + d64
    fin = torch.isfinite(s64)
    assert torch.equal((c.float() + idt.float()).double()[fin], s64[fin])            # the fp32 sum is exact
    exp = R.bf16_round_expect(c, idt)
    eb, e64 = R.bf16_bits(exp), exp.double()
    # torch's conversion is to nearest: no bf16 value is nearer to the exact sum than the one it chose ...
    r64 = s64.clamp_min(0)
    normal = fin & (r64 < 2.0 ** 127)
    up = (R._bf16_from_bits(eb[normal] + 1).double() - r64[normal]).abs()
    dn = (R._bf16_from_bits((eb[normal] - 1).clamp_min(0)).double() - r64[normal]).abs()
    here = (e64[normal] - r64[normal]).abs()
    assert (here <= up).all() and (here <= dn).all()
    # ... ties go to the even pattern ...
    tie = normal & (here_full(e64, r64) > 0) & (d64.abs() * 2 == ulp_of(cb)) & (cb >= 0x0180) & (cb < 0x7F7F)
    assert int(tie.sum()) > 60000 and bool(((eb[tie] & 1) == 0).all())
    # ... subnormal results are kept ...
    sub = fin & (r64 > 0) & (r64 < 2.0 ** -126)
    assert int(sub.sum()) >= 127 and bool((e64[sub] > 0).all()) and bool((e64[(cb >= 1) & (cb < 0x80) & (d64 == 0)] == c64[(cb >= 1) & (cb < 0x80) & (d64 == 0)]).all())
    # ... the largest finite bf16 + 1/2 ulp goes to Inf (as fp32 max does), + 1/4 ulp stays ...
    top = cb == 0x7F7F
    assert bool(torch.isinf(e64[top & (d64 == 2.0 ** 119)]).all()) and int((top & (d64 == 2.0 ** 119)).sum()) == 1
    assert bool((e64[top & (d64 == 2.0 ** 118)] == c64[top & (d64 == 2.0 ** 118)]).all()) and int((top & (d64 == 2.0 ** 118)).sum()) == 1
    assert torch.isinf(torch.tensor(torch.finfo(torch.float32).max).bfloat16().float())
    # ... negative sums are +0, a NaN on either side stays one
    neg = fin & (s64 < 0)
    assert int(neg.sum()) > 30000 and bool((eb[neg] == 0).all())
    assert int(torch.isnan(c.float()).sum()) == 1 and int(torch.isnan(idt.float()).sum()) == 1 and int((eb == 0x7FC0).sum()) == 2
    # the mutation checks: round to nearest even in integer arithmetic passes; truncation and round-half-away fail
    v = (c.float() + idt.float()).relu()
    assert torch.equal(R.bf16_bits(R.emulate_bf16_store(v, "rne")), eb)
    for how in ("trunc", "away"):
        assert int((R.bf16_bits(R.emulate_bf16_store(v, how)) != eb).sum()) > 30000, how


def ulp_of(bits):
    """spacing of bf16 at the non-negative pattern `bits` (float64)"""
    e = (bits >> 7).clamp(1, 254)
    return torch.ldexp(torch.ones(bits.shape, dtype=torch.float64), (e - 134).to(torch.int32))


def here_full(e64, r64):
    d = (e64 - r64).abs()
    return torch.where(torch.isfinite(d), d, torch.zeros_like(d))


def test_reading_a_bf16_tensor_at_fp32_stride_fails_the_colstats_bound():
    g = gen(84)
    rows, C = 240, 64
    x = R.stored(torch.randn(rows, C, generator=g) * 2.0 + torch.randn(C, generator=g)[None, :], torch.bfloat16)
    half = rows // 2
    ref64 = x[:half].double()
    bound = R.col_bound(half, C, 1024, 0, ref64.abs()).numpy()
    good = np.abs(R.emulate_colsum(x[:half].numpy()).astype(np.float64) - ref64.sum(0).numpy())
    assert (good <= bound).all()
    bad32 = R.misread_bf16_as_fp32(x.bfloat16())
    assert bad32.shape == (half, C) and torch.isfinite(bad32).all()
    # what it reads: the odd element of each pair in the upper half of the dword, the even one as noise below bf16's last bit
    assert torch.equal(bad32.reshape(-1).bfloat16().float().sub(x.reshape(-1)[1::2]).abs() <= R.U16 * x.reshape(-1)[1::2].abs() * 2,
                       torch.ones(half * C, dtype=torch.bool))
    bad = np.abs(R.emulate_colsum(bad32.numpy()).astype(np.float64) - ref64.sum(0).numpy())
    assert (bad > bound).all()


# =================================================================================================
# activation plane images: the reference, the bound and the bit comparison of hi on an fp32 emulation of the kernel
# =================================================================================================
def test_act_scale_is_frexp():
    assert R.act_scale(None, 0.0) == 1.0 and R.act_scale(None, 16.0) == 16.0 and R.act_scale(0.0) == 1.0
    assert R.act_scale(1.0) == 2.0 ** 14 and R.act_scale(0.75) == 2.0 ** 15 and R.act_scale(3e4) == 1.0 and R.act_scale(32768.0) == 0.5
    assert R.act_scale(1e-9) == 2.0 ** 44
    for a in (1e-9, 0.3, 1.0, 7.5, 3e4):          # amax * scale lies in [2^14, 2^15): inside the fp16 range with a binade to spare
        assert 2.0 ** 14 <= a * R.act_scale(a) < 2.0 ** 15


@pytest.mark.parametrize("store", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tf", [0, 1, 2])
def test_act_planes_bound_and_undecided_share_on_the_emulation(tf, store):
    """the seeds of the GPU cases: the float64 reference alone leaves at most 1e-3 of a case's elements undecided, and an fp32
    emulation of the kernel passes every assert the kernel is held to; a hi piece that was truncated instead of rounded does not"""
    for C, n8 in R.ACT_SHAPES:
        cs = R.act_case(C, n8, tf, store)
        fsc = R.act_scale(None if cs["amax"] is None else float(cs["amax"]), cs["fscale"])
        hi, lo = R.emulate_act_planes(tf, cs["x"], fsc, cs["sc"], cs["sh"], cs["x2"], cs["sc2"])
        share = R.act_planes_check(hi, lo, tf, cs, f"emulation tf {tf} C {C} n8 {n8}")
        assert share <= 1e-3, (tf, C, n8, share)
        assert tf != 0 or share == 0.0
    # mutations, on the last case: hi truncated toward zero (lo still the residual's fp16: hi + lo stays inside the bound, the bit
    # comparison sees it); lo dropped (the bound sees it)
    ref, e, raw, k = R.act_planes_ref(tf, cs["x"], fsc, cs["sc"], cs["sh"], cs["x2"], cs["sc2"])
    if tf == 0 and store == torch.bfloat16:
        # a bf16 value times a power of two has 8 significand bits: it IS an fp16 value, nothing is rounded and lo is zero
        assert torch.equal(hi.double(), ref) and not lo.any()
        return
    hb = hi.view(torch.int16)
    up = (hi.double().abs() > ref.abs()) & (hi != 0)
    assert int(up.sum()) > 100
    hi_t = torch.where(up, hb - 1, hb).view(torch.float16)
    lo_t = (ref - hi_t.double()).half()
    with pytest.raises(AssertionError, match="bit for bit"):
        R.act_planes_check(hi_t, lo_t, tf, cs, "truncated hi")
    with pytest.raises(AssertionError, match="beyond"):
        R.act_planes_check(hi, torch.zeros_like(lo), tf, cs, "no lo")
