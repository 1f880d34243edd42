"""GPU: the kernels of the input-gradient path through the C ABI (ops.*), against float64 torch on the CPU.
 * koaf_stem_dgrad: the stem's data gradient, at BWD = 4e-6 like every other gradient contraction (test_kernels_gpu.py); the
   BatchNorm-backward operand formed on load against the materialised one at 2e-6 (the stem weight gradient's bar), with the conv
   output stored as fp32 and as bf16; bit-equal on repeat (gather form, no atomics).  Shapes: one tile, odd sizes, an image
   smaller than a tile (8 x 8), widths of several tiles / of the forward kernels' column bands (401, 790);
 * koaf_bn_bwd_finalize_eval: dc = sc*dz, dgamma / dbeta the train-mode sums, both at 1e-6;
 * koaf_slice_unfold inverts koaf_slice_fold bit for bit; koaf_rowdot against float64 at 1e-6, bit-equal on repeat."""
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import BWD, nhwc, packw, rel_err, rnd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,H,W", [(3, 40, 40), (2, 35, 31), (1, 8, 8), (2, 30, 401), (1, 9, 790)])
def test_stem_dgrad(dev, N, H, W):
    from oaprogressionmmf_amd import ops
    w = rnd(64, 3, 7, 7, scale=147 ** -0.5)
    x3 = rnd(N, 1, H, W).double().repeat(1, 3, 1, 1).requires_grad_(True)
    y_ref = F.conv2d(x3, w.double(), stride=2, padding=3)
    dy = rnd(*y_ref.shape)
    y_ref.backward(dy.double())
    dx_ref = x3.grad.sum(1)                                   # the three repeated channels fold into one
    w1t = ops.stem_fold_w(packw(w).to(dev))
    dyd = nhwc(dy).to(dev)
    dx = ops.stem_dgrad(dyd, w1t, N, H, W)
    assert dx.shape == (N, H, W)
    err = rel_err(dx, dx_ref)
    print(f"\n[stem_dgrad {N}x{H}x{W}] rel err {err:.2e}")
    assert err < BWD
    assert torch.equal(ops.stem_dgrad(dyd, w1t, N, H, W), dx)


@pytest.mark.parametrize("N,H,W", [(3, 70, 58), (1, 9, 401)])
def test_stem_dgrad_forms_the_batchnorm_backward_on_load(dev, N, H, W):
    """dc0 = coef0*dz + coef3 - coef2*c0 formed in the kernel's loader (KoafBnApply, as koaf_stem_wgrad takes it) against the
    materialised dc0, with c0 stored as fp32 and as bf16"""
    from oaprogressionmmf_amd import ops
    C = 64
    x = rnd(N, H, W).to(dev)
    w1t = ops.stem_fold_w(rnd(64, 7, 7, 3, scale=0.1).to(dev))
    gam, bet = (rnd(C) * 0.2 + 1).to(dev), (rnd(C) * 0.1).to(dev)
    for dt in (torch.float32, torch.bfloat16):
        c0 = ops.stem_fwd(x, w1t, N, H, W, dtype=dt)
        H1, W1 = c0.shape[1], c0.shape[2]
        rows = N * H1 * W1
        saved = ops.bn_finalize(ops.colstats(c0, rows, C), C, rows, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev),
                                torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)
        y, am = ops.maxpool_fwd(c0, saved, N, H1, W1, C)
        dy = rnd(*y.shape).to(dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ap = ops.bn_bwd(None, c0, saved, rows, C, rows, dg, db, 2, fused=True, pool=(dy, am, N, H1, W1))
        assert isinstance(ap, ops.BnApply)
        dx_ref = ops.stem_dgrad(ap.materialize(), w1t, N, H, W)
        dx = ops.stem_dgrad(ap, w1t, N, H, W)
        err = rel_err(dx, dx_ref)
        print(f"\n[stem_dgrad apply {N}x{H}x{W} c0 {dt}] rel err vs materialised {err:.2e}")
        assert err < 2e-6
        assert torch.equal(ops.stem_dgrad(ap, w1t, N, H, W), dx)


@pytest.mark.parametrize("rows,C", [(5000, 64), (777, 256)])
def test_batchnorm_backward_eval_mode(dev, rows, C):
    """an eval-mode BatchNorm is y = sc*c + sh with constant coefficients: dc = sc*dz; dgamma / dbeta are the sums the train-mode
    call forms from the same record (here: the running statistics)"""
    from oaprogressionmmf_amd import ops
    c = (rnd(rows, C) * 2.0 + rnd(C)[None, :]).to(dev)
    gamma, beta = (rnd(C) * 0.5 + 1.0).to(dev), (rnd(C) * 0.2).to(dev)
    rm, rv = (rnd(C) * 0.1).to(dev), (torch.rand(C) + 0.5).to(dev)
    saved = ops.bn_finalize(None, C, 0, gamma, beta, rm, rv, None, 0.1, 1e-5, False)
    g = rnd(rows, C).to(dev)
    dz_ref = (g * ((c * saved[2] + saved[3]) > 0)).double()
    dg_t, db_t, dg_e, db_e = (torch.empty(C, device=dev) for _ in range(4))
    ops.bn_bwd(g.clone(), c, saved, rows, C, rows, dg_t, db_t, 2, fused=False)
    dc = ops.bn_bwd(g.clone(), c, saved, rows, C, rows, dg_e, db_e, 2, fused=False, train=False)
    assert rel_err(dc, saved[2].double() * dz_ref) < 1e-6
    assert rel_err(dg_e, dg_t.double()) < 1e-6 and rel_err(db_e, db_t.double()) < 1e-6
    # against the definition as well: dgamma = sum dz * xhat (running statistics), dbeta = sum dz
    xhat = (c.double() - saved[0].double()) * saved[1].double()
    assert rel_err(dg_e, (dz_ref * xhat).sum(0)) < 1e-5 and rel_err(db_e, dz_ref.sum(0)) < 1e-5
    # the recipe form (formed on load by the convolutions): same coefficients, its scale bound holds
    ap = ops.bn_bwd(g.clone(), c, saved, rows, C, rows, dg_e, db_e, 2, fused=True, train=False)
    assert isinstance(ap, ops.BnApply)
    assert torch.equal(ap.coef[0], saved[2]) and not ap.coef[1:].any()
    m = ap.materialize()
    assert rel_err(m, saved[2].double() * dz_ref) < 1e-6
    assert float(ap.amax) >= float(m.abs().max())
    # frozen parameters: the same dc, nothing reduced
    dc2 = ops.bn_bwd(g.clone(), c, saved, rows, C, rows, None, None, 2, fused=False, train=False)
    assert torch.equal(dc2, dc)


def test_slice_unfold_inverts_slice_fold(dev):
    from oaprogressionmmf_amd import ops
    B, R, Cc, S = 2, 12, 20, 5
    x = rnd(B, R, Cc, S).to(dev)
    f = ops.slice_fold(x, B, R, Cc, S)
    assert torch.equal(f, x.permute(0, 3, 1, 2).reshape(B * S, R, Cc))
    assert torch.equal(ops.slice_unfold(f, B, R, Cc, S), x)


def test_rowdot(dev):
    from oaprogressionmmf_amd import ops
    B, n = 3, 70001
    a, b = rnd(B, n).to(dev), rnd(B, n).to(dev)
    out = ops.rowdot(a, b)
    assert rel_err(out, (a.double() * b.double()).sum(1)) < 1e-6
    assert torch.equal(ops.rowdot(a, b), out)
    a4 = a[:, :70000].reshape(B, 1, 250, 280).contiguous()
    assert rel_err(ops.rowdot(a4, a4), (a4.double() ** 2).sum((1, 2, 3))) < 1e-6
