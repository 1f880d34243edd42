"""CPU: the float64 references and the bounds of loss_optim_refs.py.
 * the loss formulas against F.cross_entropy autograd in float64; the optimizer steps, four chained, against torch.optim on
   float64 parameters, for every option the GPU tests use
 * every bound from both sides with the fp32 numpy restatements of the kernels' arithmetic: the clean restatement (with and
   without fused multiply-adds) stays inside, a planted fault lands outside."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_optim_refs as R


def gen(seed):
    return torch.Generator().manual_seed(seed)


# =================================================================================================
# softmax losses
# =================================================================================================
def _autograd64(x, tg, cw, gamma_, focal, mean):
    xx = x.double().clone().requires_grad_(True)
    wd = None if cw is None else cw.double()
    if focal:
        logpt = -F.cross_entropy(xx, tg, weight=wd, reduction="none")
        l = -((1 - logpt.exp()) ** gamma_) * logpt
        loss = l.mean() if mean else l.sum()
    else:
        l = F.cross_entropy(xx, tg, weight=wd, reduction="none")
        loss = F.cross_entropy(xx, tg, weight=wd)
    loss.backward()
    return l.detach(), loss.detach(), xx.grad


@pytest.mark.parametrize("shape", [(7, 3, 1), (2, 5, 13), (3, 2, 4), (4, 1, 3)])
def test_loss_reference_against_autograd(shape):
    B, C, S = shape
    x, tg, _ = R.loss_inputs(B, C, S, 11, margins=(0, 1, 4, 8))
    x = x + torch.randn(B, C, S, generator=gen(1)) * 0.3        # (any fp32 input, not only the grid)
    tg = tg.clone()
    tg.view(-1)[1] = -100
    cws = [None] if C == 1 else [None, torch.tensor([0.5, 2.0, 0.0, 1.25, 0.75][:C])]
    for cw in cws:
        for focal, gamma_, mean in [(False, 0.0, True), (True, 0.0, True), (True, 1.0, False), (True, 2.0, True), (True, 3.5, False),
                                    (True, 0.5, True)]:
            if C == 1 and focal and gamma_ in (0.5,):
                continue                                         # (0^-0.5 * 0: NaN in torch too)
            if cw is not None and gamma_ == 0.5:
                continue                                         # (a zero class weight: the same 0^-0.5)
            l, loss, d = _autograd64(x, tg, cw, gamma_, focal, mean)
            ref = R.softmax_loss_ref(x, tg, cw, gamma_, focal, mean)
            what = f"{shape} cw {cw is not None} focal {focal} gamma {gamma_} mean {mean}"
            assert torch.allclose(ref["l"], l, rtol=1e-12, atol=1e-15), what
            assert torch.allclose(ref["d"], d, rtol=1e-11, atol=1e-16), what
            assert abs(float(ref["loss"]) - float(loss)) <= 1e-13 * max(1.0, abs(float(loss))), what
            assert float(ref["d"].movedim(1, -1).reshape(-1, C)[1].abs().max()) == 0.0 and ref["nbad"] == 0


def test_loss_reference_out_of_range_labels_and_all_ignored():
    x, tg, _ = R.loss_inputs(5, 3, 1, 12)
    bad = tg.clone()
    bad[2] = 7
    bad[4] = -100
    ref = R.softmax_loss_ref(x, bad, None, 2.0, True, True)
    ok = R.softmax_loss_ref(x[[0, 1, 3]], tg[[0, 1, 3]], None, 2.0, True, False)
    assert ref["nbad"] == 1 and float(ref["d"][[2, 4]].abs().max()) == 0.0
    assert abs(float(ref["loss"]) - float(ok["loss"]) / 5) < 1e-15          # the focal mean still divides by every element
    ce = R.softmax_loss_ref(x, bad, None, 0.0, False, True)
    assert abs(float(ce["loss"]) - float(F.cross_entropy(x[[0, 1, 3]].double(), tg[[0, 1, 3]]))) < 1e-14
    allign = R.softmax_loss_ref(x, torch.full_like(tg, -100), None, 0.0, False, True)
    assert np.isnan(float(allign["loss"])) and float(allign["d"].abs().max()) == 0.0
    assert np.isnan(float(F.cross_entropy(x.double(), torch.full((5, 1), -100))))


def test_loss_inputs_are_exact_under_the_offsets():
    x, tg, grp = R.loss_inputs(3, 5, 101, 13)
    assert float(x.abs().max()) < 16 and torch.equal(x * 1024, (x * 1024).round())
    for c in (64.0, 1024.0, -1024.0):
        assert torch.equal((x + c) - c, x)
    groups = R.loss_groups()
    assert len(groups) == 11 and int(grp.max()) == 10
    xs, t, g = x.movedim(1, -1).reshape(-1, 5).double(), tg.reshape(-1), grp.reshape(-1)
    oh = F.one_hot(t, 5).bool()
    margin = xs[oh] - xs.masked_fill(oh, -1e9).max(1).values
    want = torch.tensor([a * s for a, s in groups], dtype=torch.float64)[g]
    assert torch.equal(margin, want)


LOSS_CASES = [(37, 3, 1), (3, 2, 2731), (8193, 2, 1), (2, 5, 4097), (255, 1, 1)]


@pytest.mark.parametrize("shape", LOSS_CASES)
def test_loss_bounds_hold_the_clean_restatement(shape):
    """the fp32 restatement of the kernel's arithmetic and summation order meets every group's bar and the loss scalar's, at
    offsets 0, 64 and 1024, bit-equal across them"""
    B, C, S = shape
    n = B * S
    x, tg, grp = R.loss_inputs(B, C, S, 20)
    tg = tg.clone()
    tg.view(-1)[[0, n - 1]] = -100
    cw = None if C == 1 else torch.tensor([0.5, 2.0, 0.0, 1.25, 0.75][:C])
    ng = len(R.loss_groups())
    for w in (None, cw) if C > 1 else (None,):
        for focal, gamma_, mean in [(False, 0.0, True), (True, 2.0, True), (True, 3.5, False), (True, 0.0, True)]:
            ref = R.softmax_loss_ref(x, tg, w, gamma_, focal, mean)
            ly, dy = R.torch_loss_fp32(x, tg, w, gamma_, focal, mean)
            l0, d0 = R.loss_kernel_f32(x, tg, w, gamma_, focal, mean)
            wm = (not focal) and w is not None
            for r in R.loss_group_report(d0, ref, dy, grp, ng, n, C, gamma_, focal, wm):
                assert r["ok"], (shape, focal, gamma_, r)
            assert R.loss_scalar_report(l0, ref, ly, n, C, gamma_, focal, wm)["ok"]
            for c in (64.0, 1024.0, -1024.0):
                lc, dc = R.loss_kernel_f32(x + c, tg, w, gamma_, focal, mean)
                assert lc == l0 and torch.equal(dc, d0), (shape, focal, gamma_, c)


@pytest.mark.parametrize("focal", [True, False])
def test_loss_bounds_catch_lse_formed_on_the_maximum(focal):
    """lse = m + log s, then x - lse: at offset 64 every log-probability is rounded to ulp(64) / 2 -- outside the group bars,
    and not bit-equal to offset 0"""
    B, C, S = 4096, 3, 1
    x, tg, grp = R.loss_inputs(B, C, S, 21)
    ng = len(R.loss_groups())
    ref = R.softmax_loss_ref(x, tg, None, 2.0, focal, True)
    _, dy = R.torch_loss_fp32(x, tg, None, 2.0, focal, True)
    l0, d0 = R.loss_kernel_f32(x, tg, None, 2.0, focal, True, lse_form=True)
    l64, d64 = R.loss_kernel_f32(x + 64.0, tg, None, 2.0, focal, True, lse_form=True)
    assert not torch.equal(d64, d0)
    rep = R.loss_group_report(d64, ref, dy, grp, ng, B * S, C, 2.0, focal, False)
    bad = [r for r in rep if not r["ok"]]
    print(f"lse form at +64, focal {focal}: groups outside: {[(r['group'], round(r['err'] / r['bar'], 1)) for r in bad]}")
    assert bad
    l1k, d1k = R.loss_kernel_f32(x + 1024.0, tg, None, 2.0, focal, True, lse_form=True)
    assert not all(r["ok"] for r in R.loss_group_report(d1k, ref, dy, grp, ng, B * S, C, 2.0, focal, False))
    # (the loss scalar does not show it: the roundings of lse average out over the batch, which is why the groups are held)


def test_loss_bounds_catch_a_counted_ignored_element_and_a_dropped_chunk():
    B, C, S = 3, 3, 2731                # 8193 elements: the grid form, three chunks, the last of one element
    n = B * S
    x, tg, grp = R.loss_inputs(B, C, S, 22)
    tg = tg.clone()
    tg.view(-1)[[0, 4095, 4096, n - 1]] = -100
    cw = torch.tensor([0.5, 2.0, 1.25])
    ng = len(R.loss_groups())
    ref = R.softmax_loss_ref(x, tg, cw, 0.0, False, True)
    ly, dy = R.torch_loss_fp32(x, tg, cw, 0.0, False, True)
    l, d = R.loss_kernel_f32(x, tg, cw, 0.0, False, True, count_ignored=True)
    assert not R.loss_scalar_report(l, ref, ly, n, C, 0.0, False, True)["ok"]
    assert not all(r["ok"] for r in R.loss_group_report(d, ref, dy, grp, ng, n, C, 0.0, False, True))
    for focal in (True, False):
        ref = R.softmax_loss_ref(x, tg, cw, 2.0, focal, True)
        ly, _ = R.torch_loss_fp32(x, tg, cw, 2.0, focal, True)
        for k in (0, 2):                # (the last chunk holds ONE element, an ignored one: its partial is 0, dropping it shows nothing)
            l, _ = R.loss_kernel_f32(x, tg, cw, 2.0, focal, True, drop_chunk=k)
            ok = R.loss_scalar_report(l, ref, ly, n, C, 2.0, focal, not focal)["ok"]
            assert ok == (k == 2), (focal, k)
    # with a counted last element the one-element chunk shows too
    tg2 = tg.clone()
    tg2.view(-1)[n - 1] = 1
    x2 = x.clone()
    x2.view(B, C, S)[-1, :, -1] = torch.tensor([8.0, -8.0, 0.0])        # (a large loss: 16 among 8193 elements of about 3)
    ref = R.softmax_loss_ref(x2, tg2, None, 0.0, False, True)
    ly, _ = R.torch_loss_fp32(x2, tg2, None, 0.0, False, True)
    l, _ = R.loss_kernel_f32(x2, tg2, None, 0.0, False, True, drop_chunk=2)
    assert not R.loss_scalar_report(l, ref, ly, n, C, 0.0, False, False)["ok"]


def test_emulate_sum_chains():
    assert R.sum_chain(1) == 9 and R.sum_chain(8192) == 40 and R.sum_chain(8193) == 16 + 8 + 1 + 8
    assert R.sum_chain(256 * 4096 + 1) == 16 + 8 + 2 + 8
    v = np.ones(12289, dtype=np.float32)
    assert R.emulate_sum(v) == 12289 and R.emulate_sum(v, drop_chunk=3) == 12288 and R.emulate_sum(v[:255]) == 255


# =================================================================================================
# optimizer steps
# =================================================================================================
N = 37


def _chain(opt_cls, kw, step_fn):
    """four chained steps of torch.optim on float64 parameters against step_fn(state, g, s) -> state, fed exact double scalars"""
    ins = R.optim_inputs(N, 30)
    p = torch.nn.Parameter(ins["p"].double().clone())
    opt = opt_cls([p], **kw)
    state = {"p": ins["p"].double().clone()}
    for s in range(4):
        g = torch.randn(N, generator=gen(40 + s)).double()
        p.grad = g.clone()
        opt.step()
        state = step_fn(state, g, s)
        assert torch.allclose(state["p"], p.detach(), rtol=1e-13, atol=1e-15), (kw, s)
    return state, opt.state[p]


@pytest.mark.parametrize("kw", [dict(), dict(momentum=0.9), dict(momentum=0.9, dampening=0.1), dict(momentum=0.9, nesterov=True),
                                dict(weight_decay=0.01), dict(momentum=0.9, weight_decay=0.01, maximize=True),
                                dict(momentum=0.9, nesterov=True, weight_decay=0.01, maximize=True)])
def test_sgd_reference_against_torch(kw):
    mom = kw.get("momentum", 0.0)
    sc = dict(lr=0.05, mu=mom, omd=1.0 - kw.get("dampening", 0.0), wd=kw.get("weight_decay", 0.0), sign=-1.0 if kw.get("maximize") else 1.0)

    def step(st, g, s):
        out, _ = R.sgd_step64(st["p"], g, st.get("buf"), sc, mom=mom > 0, nest=kw.get("nesterov", False), first=(s == 0))
        return out
    st, ts = _chain(torch.optim.SGD, dict(lr=0.05, **kw), step)
    if mom:
        assert torch.allclose(st["buf"], ts["momentum_buffer"], rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("alpha", [0.99, 0.3])
@pytest.mark.parametrize("kw", [dict(), dict(centered=True), dict(momentum=0.9), dict(centered=True, momentum=0.9),
                                dict(centered=True, momentum=0.9, weight_decay=0.01, maximize=True)])
def test_rmsprop_reference_against_torch(kw, alpha):
    sc = dict(lr=1e-3, alpha=alpha, oma=1.0 - alpha, eps=1e-8, wd=kw.get("weight_decay", 0.0), mu=kw.get("momentum", 0.0),
              sign=-1.0 if kw.get("maximize") else 1.0)
    z = torch.zeros(N, dtype=torch.float64)

    def step(st, g, s):
        out, _ = R.rms_step64(st["p"], g, st.get("sq", z), st.get("gavg", z) if kw.get("centered") else None,
                              st.get("buf", z) if kw.get("momentum") else None, sc)
        return out
    st, ts = _chain(torch.optim.RMSprop, dict(lr=1e-3, alpha=alpha, **kw), step)
    for mine, theirs in (("sq", "square_avg"), ("gavg", "grad_avg"), ("buf", "momentum_buffer")):
        if mine in st:
            assert torch.allclose(st[mine], ts[theirs], rtol=1e-12, atol=1e-15), mine


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("cls", [torch.optim.Adam, torch.optim.AdamW])
def test_adam_reference_against_torch(cls, amsgrad):
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.01
    z = torch.zeros(N, dtype=torch.float64)

    def step(st, g, s):
        t = s + 1
        sc = dict(lr=lr, omb1=1.0 - b1, b2=b2, omb2=1.0 - b2, eps=eps, wd=wd, step_size=lr / (1 - b1 ** t), bc2_sqrt=np.sqrt(1 - b2 ** t))
        out, _ = R.adam_step64(st["p"], g, st.get("m", z), st.get("v", z), st.get("vmax", z) if amsgrad else None, sc,
                               adamw=cls is torch.optim.AdamW)
        return out
    st, ts = _chain(cls, dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=amsgrad), step)
    assert torch.allclose(st["m"], ts["exp_avg"], rtol=1e-13, atol=1e-16) and torch.allclose(st["v"], ts["exp_avg_sq"], rtol=1e-13, atol=1e-18)
    if amsgrad:
        assert torch.allclose(st["vmax"], ts["max_exp_avg_sq"], rtol=1e-13, atol=1e-18)


def test_kernel_scalars_are_the_floats_the_entry_points_form():
    sc = R.adam_scalars(1e-3, 0.9, 0.999, 1e-8, 0.01, 1000)
    assert sc["omb2"] == float(np.float32(1.0 - 0.999)) != float(np.float32(1.0) - np.float32(0.999))
    assert sc["step_size"] == float(np.float32(float(np.float32(1e-3)) / (1.0 - 0.9 ** 1000)))
    assert R.rms_scalars(1e-3, alpha=0.3)["oma"] == float(np.float32(0.7)) and R.sgd_scalars(0.1, dampening=0.1)["omd"] == float(np.float32(0.9))
    h = R.adam_hyper_ref(np.float32(1e-3), 0.9, 0.999, 1)
    assert abs(h[1] - 1e-2) < 1e-9 and abs(h[2] - np.sqrt(1e-3)) < 1e-9


def _fractions(out32, ref, bnd):
    return {k: R.worst_fraction(out32[k], ref[k].numpy(), bnd[k].numpy()) for k in ref}


SGD_VARIANTS = [dict(), dict(mom=True), dict(mom=True, damp=0.1), dict(mom=True, nest=True)]


@pytest.mark.parametrize("n", [3, 5, 1025])
def test_optimizer_bounds_from_both_sides(n):
    ins = R.optim_inputs(n, 50 + n)
    worst = 0.0
    # ---- SGD
    for v in SGD_VARIANTS:
        for maximize in (False, True):
            for first in (False, True):
                sc = R.sgd_scalars(0.05, 0.9 if v.get("mom") else 0.0, v.get("damp", 0.0), 0.01, maximize)
                kw = dict(mom=v.get("mom", False), nest=v.get("nest", False), first=first)
                buf = ins["buf"] if v.get("mom") else None
                ref, bnd = R.sgd_step64(ins["p"], ins["g"], buf, sc, **kw)
                for fused in (False, True):
                    fr = _fractions(R.sgd_kernel_f32(ins["p"], ins["g"], buf, sc, fused=fused, **kw), ref, bnd)
                    assert max(fr.values()) <= 1.0, ("sgd", v, fused, fr)
                    worst = max(worst, *fr.values())
                if n % 4:
                    assert max(_fractions(R.sgd_kernel_f32(ins["p"], ins["g"], buf, sc, skip_tail=True, **kw), ref, bnd).values()) > 1.0
                if v.get("mom") and first:
                    assert max(_fractions(R.sgd_kernel_f32(ins["p"], ins["g"], buf, sc, ignore_first=True, **kw), ref, bnd).values()) > 1.0
                if v.get("mom"):
                    assert _fractions(R.sgd_kernel_f32(ins["p"], ins["g"], buf, sc, wd_after_moment=True, **kw), ref, bnd)["buf"] > 1.0
    # ---- RMSprop
    for cen in (False, True):
        for mom in (False, True):
            for alpha in (0.99, 0.3):
                sc = R.rms_scalars(1e-3, alpha, 1e-8, 0.01, 0.9 if mom else 0.0)
                a = (ins["p"], ins["g"], ins["sq"], ins["gavg"] if cen else None, ins["buf"] if mom else None, sc)
                ref, bnd = R.rms_step64(*a)
                for fused in (False, True):
                    fr = _fractions(R.rms_kernel_f32(*a, fused=fused), ref, bnd)
                    assert max(fr.values()) <= 1.0, ("rmsprop", cen, mom, alpha, fused, fr)
                    worst = max(worst, *fr.values())
                if n % 4:
                    assert max(_fractions(R.rms_kernel_f32(*a, skip_tail=True), ref, bnd).values()) > 1.0
                assert _fractions(R.rms_kernel_f32(*a, wd_after_moment=True), ref, bnd)["sq"] > 1.0
    # ---- Adam / AdamW
    for adamw in (False, True):
        for ams in (False, True):
            for step in (1, 2, 1000):
                sc = R.adam_scalars(1e-3, 0.9, 0.999, 1e-8, 0.01, step)
                a = (ins["p"], ins["g"], ins["m"], ins["v"], ins["vmax"] if ams else None, sc)
                ref, bnd = R.adam_step64(*a, adamw=adamw)
                for fused in (False, True):
                    out = R.adam_kernel_f32(*a, adamw=adamw, fused=fused)
                    fr = _fractions({k: out[k] for k in ("p", "m", "v")}, {k: ref[k] for k in ("p", "m", "v")}, bnd)
                    assert max(fr.values()) <= 1.0, ("adam", adamw, ams, step, fused, fr)
                    worst = max(worst, *fr.values())
                    if ams:         # the written-back maximum: bit-equal to max(vmax, v') of the kernel's own v'
                        assert np.array_equal(out["vmax"], np.maximum(ins["vmax"].numpy(), out["v"]))
                if n % 4:
                    out = R.adam_kernel_f32(*a, adamw=adamw, skip_tail=True)
                    assert max(_fractions({k: out[k] for k in ("p", "m", "v")}, {k: ref[k] for k in ("p", "m", "v")}, bnd).values()) > 1.0
                if not adamw:
                    assert R.worst_fraction(R.adam_kernel_f32(*a, wd_after_moment=True)["m"], ref["m"].numpy(), bnd["m"].numpy()) > 1.0
                if ams:
                    out = R.adam_kernel_f32(*a, adamw=adamw, no_writeback=True)
                    assert not np.array_equal(out["vmax"], np.maximum(ins["vmax"].numpy(), out["v"]))
    print(f"n {n}: worst fraction of a bound the clean restatements use: {worst:.3f}")
    assert worst > 0.02          # (the bounds are not vacuous: clean fp32 arithmetic uses a visible share of them)


def test_optimizer_inputs_cover_both_sides_of_the_amsgrad_maximum():
    ins = R.optim_inputs(64, 60)
    sc = R.adam_scalars(1e-3, 0.9, 0.999, 1e-8, 0.0, 2)
    ref, _ = R.adam_step64(ins["p"], ins["g"], ins["m"], ins["v"], ins["vmax"], sc)
    below = ins["vmax"].double() < ref["v"]
    assert int(below.sum()) == 32 and bool(below[0::2].all()) and not bool(below[1::2].any())
    assert bool((ins["gavg"].abs() <= 0.5 * ins["sq"].sqrt()).all()) and float(ins["sq"].min()) > 0
