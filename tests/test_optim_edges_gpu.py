"""Per-element parity of the optimizer steps (koaf_optim.hip: SGD, RMSprop, Adam / AdamW) at their edges: lengths below one 16-byte
vector (the scalar tail alone), around a block, the second trip of the grid-stride loop; every template instantiation and run-time
flag; the device-`hyper` path; amsgrad's written-back maximum; special values; unaligned views.

test_optim_losses_gpu.py runs four steps against torch.optim in fp32 and compares whole tensors by a ratio of norms.  Here ONE step
starts from random, non-trivial operands and state (v, sq, vmax >= 0), and the parameter and every state buffer are compared per
element with the float64 step of loss_optim_refs.py on the same fp32 inputs, fed the scalars exactly as the kernel receives them.
Every bar is u * (the absolute error count of loss_optim_refs.{sgd,rms,adam}_step64, counted from the kernel source: one rounding
u, sqrtf and the division 2 u, a fused multiply-add counted as two roundings), bit equality (the hyper path, amsgrad's maximum,
the spare elements, the gradient), or a class (finite | inf | NaN) for the planted special values.  test_loss_optim_refs_cpu.py
shows that clean fp32 arithmetic, with and without fused multiply-adds, meets the bars and that planted faults do not.

Measured on an MI355X (they document; every bar is computed in the test): the worst fraction of a bound that is used, over all lengths
and variants -- SGD p 0.36, buf 0.62; RMSprop p 1.00 (0.998), sq 0.77, gavg 0.98, buf 0.48; Adam p 1.00 (0.999), m 0.90, v 0.59;
AdamW p 0.51, m 0.95, v 0.76.  The fractions near 1 are the last subtraction's rounding u |p'| beside an update far below p: the bound
has no slack there and needs none.  In SGD's terms (bound = gamma(k) * terms) that is a measured k of 2.9 of 8 for p (Nesterov), 2.5 of 4
for buf.  koaf_adam_hyper: 0 ulp from float32 of the float64 formulas at steps 1, 2, 1000 and 100000.  amsgrad's maximum: a NaN second
moment left a finite vmax (fmaxf drops a NaN) where torch.maximum keeps it -- the special-value case found it; the kernel now keeps it."""
import numpy as np
import pytest
import torch

import loss_optim_refs as R
from test_elem_edges_gpu import CAP, needs_default_cap

pytestmark = pytest.mark.gpu

PAD, SENT = 5, 12345.0          # spare elements after n, filled with a sentinel and checked untouched
LENGTHS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025]
BIG = 4 * (CAP + 1) + 3         # one vector beyond the capped grid's reach: the second trip of the grid-stride loop, and a 3-element tail
LR, WD = 0.05, 0.01


def _dev(ins, dev, *keys):
    return {k: ins[k].clone().to(dev) for k in keys}


def _biteq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))        # (NaN compares equal to itself here)


def _hold(d, ins, ref, bnd, n, what, skip=None):
    """p and every state buffer within its per-element bound (skip: planted special elements), the spare elements and g untouched"""
    keep = np.ones(n, dtype=bool)
    if skip is not None:
        keep[skip] = False
    for k in ref:
        got = d[k].cpu()
        assert torch.equal(got[n:], torch.full((PAD,), SENT)), f"{what}: {k} written beyond n"
        f = R.worst_fraction(got[:n].numpy()[keep], ref[k].numpy()[keep], bnd[k].numpy()[keep]) if k in bnd else None
        if f is not None:
            print(f"FRACTION {what} n {n} {k}: {f:.3f}")
            assert f <= 1.0, f"{what} n {n}: {k} uses {f:.2f} of its bound"
    for k in d:
        if k not in ref:
            assert _biteq(d[k].cpu(), ins[k]), f"{what}: {k} was written"


SGD_VARIANTS = [("plain", dict()), ("momentum", dict(momentum=0.9)), ("dampening", dict(momentum=0.9, dampening=0.1)),
                ("nesterov", dict(momentum=0.9, nesterov=True))]


def _sgd(ops, dev, n, seed, kw, maximize, first, nan_buf=False, hyper=None, host_lr=LR):
    ins = R.optim_inputs(n, seed, PAD, SENT)
    mom = kw.get("momentum", 0.0)
    if nan_buf:
        ins["buf"][:n] = float("nan")
    d = _dev(ins, dev, "p", "g", *(["buf"] if mom else []))
    ops.sgd_step(d["p"], d["g"], d.get("buf"), n, host_lr, momentum=mom, dampening=kw.get("dampening", 0.0), wd=WD,
                 nesterov=kw.get("nesterov", False), maximize=maximize, first=first, hyper=hyper)
    sc = R.sgd_scalars(LR, mom, kw.get("dampening", 0.0), WD, maximize)
    ref, bnd = R.sgd_step64(ins["p"][:n], ins["g"][:n], ins["buf"][:n] if mom else None, sc, mom=mom > 0, nest=kw.get("nesterov", False), first=first)
    return ins, d, ref, bnd


@pytest.mark.parametrize("n", LENGTHS)
def test_sgd_step_edges(dev, n):
    """K (loss_optim_refs.sgd_step64): g' 2, buf 4, Nesterov's step 6, p that + 2 -- over |p| + |lr| (the step's terms)"""
    from oaprogressionmmf_amd import ops
    for name, kw in SGD_VARIANTS:
        for maximize in (False, True):
            for first in ((False, True) if kw else (False,)):
                ins, d, ref, bnd = _sgd(ops, dev, n, 1000 + n, kw, maximize, first, nan_buf=first)
                if first:
                    assert torch.isfinite(d["buf"][:n]).all(), f"sgd {name}: a first step read its buffer"
                _hold(d, ins, ref, bnd, n, f"sgd {name} maximize {maximize} first {first}")


def _rms(ops, dev, n, seed, cen, mom, alpha, hyper=None, host_lr=1e-3, maximize=False):
    ins = R.optim_inputs(n, seed, PAD, SENT)
    d = _dev(ins, dev, "p", "g", "sq", *(["gavg"] if cen else []), *(["buf"] if mom else []))
    ops.rmsprop_step(d["p"], d["g"], d["sq"], n, host_lr, alpha=alpha, eps=1e-8, wd=WD, momentum=0.9 if mom else 0.0,
                     gavg=d.get("gavg"), buf=d.get("buf"), maximize=maximize, hyper=hyper)
    sc = R.rms_scalars(1e-3, alpha, 1e-8, WD, 0.9 if mom else 0.0, maximize)
    ref, bnd = R.rms_step64(ins["p"][:n], ins["g"][:n], ins["sq"][:n], ins["gavg"][:n] if cen else None, ins["buf"][:n] if mom else None, sc)
    return ins, d, ref, bnd


@pytest.mark.parametrize("n", LENGTHS)
def test_rmsprop_step_edges(dev, n):
    """all four of CEN x MOM with weight decay; alpha 0.99 and 0.3 run both branches of the lerp form.  The centered variance
    sq - ga^2 carries its cancellation per element (loss_optim_refs.rms_step64: E(var) / var); |gavg| <= 0.5 sqrt(sq) keeps it <= 5/3 + wd's share"""
    from oaprogressionmmf_amd import ops
    for cen in (False, True):
        for mom in (False, True):
            for alpha in (0.99, 0.3):
                ins, d, ref, bnd = _rms(ops, dev, n, 2000 + n, cen, mom, alpha, maximize=(alpha == 0.3))
                _hold(d, ins, ref, bnd, n, f"rmsprop cen{int(cen)}mom{int(mom)} alpha {alpha}")


B1, B2, EPS = 0.9, 0.999, 1e-8


def _adam(ops, dev, n, seed, adamw, ams, step, hyper=None, host_lr=1e-3, host_step=None):
    ins = R.optim_inputs(n, seed, PAD, SENT)
    d = _dev(ins, dev, "p", "g", "m", "v", *(["vmax"] if ams else []))
    ops.adam_step(d["p"], d["g"], d["m"], d["v"], n, host_lr, B1, B2, EPS, WD, step if host_step is None else host_step, adamw=adamw,
                  hyper=hyper, vmax=d.get("vmax"))
    sc = R.adam_scalars(1e-3, B1, B2, EPS, WD, step)
    ref, bnd = R.adam_step64(ins["p"][:n], ins["g"][:n], ins["m"][:n], ins["v"][:n], ins["vmax"][:n] if ams else None, sc, adamw=adamw)
    return ins, d, ref, bnd


def _hold_vmax(d, ins, n, what):
    """amsgrad: the written-back maximum is bit-equal to max(vmax, v') of the kernel's own v', and both sides of it occur"""
    v1, x0, x1 = d["v"][:n].cpu(), ins["vmax"][:n], d["vmax"][:n].cpu()
    assert torch.equal(x1, torch.maximum(x0, v1)), what + ": vmax is not max(vmax, v') bit for bit"
    if n >= 2:
        assert bool((x0 < v1)[0::2].all()) and bool((x0 > v1)[1::2].all()), what + ": the inputs do not reach both sides of the maximum"


@pytest.mark.parametrize("n", LENGTHS)
def test_adam_step_edges(dev, n):
    from oaprogressionmmf_amd import ops
    for adamw in (False, True):
        for ams in (False, True):
            for step in (1, 2, 1000):
                what = f"{'adamw' if adamw else 'adam'} amsgrad {ams} step {step}"
                ins, d, ref, bnd = _adam(ops, dev, n, 3000 + n, adamw, ams, step)
                _hold(d, ins, ref, bnd, n, what)
                if ams:
                    _hold_vmax(d, ins, n, what)


@needs_default_cap
@pytest.mark.parametrize("opt", ["sgd", "rmsprop", "adam"])
def test_second_trip_of_the_grid_stride_loop(dev, opt):
    """4 * (CAP + 1) + 3 elements: thread 0 of block 0 takes a second vector, the tail follows it; each optimizer's fullest variant"""
    from oaprogressionmmf_amd import ops
    n = BIG
    if opt == "sgd":
        ins, d, ref, bnd = _sgd(ops, dev, n, 4001, dict(momentum=0.9, nesterov=True), True, False)
    elif opt == "rmsprop":
        ins, d, ref, bnd = _rms(ops, dev, n, 4002, True, True, 0.99)
    else:
        ins, d, ref, bnd = _adam(ops, dev, n, 4003, False, True, 2)
        _hold_vmax(d, ins, n, "adam big")
    _hold(d, ins, ref, bnd, n, f"{opt} fullest")
    # (the second trip's vector and the tail are the last 7 elements: they moved)
    assert bool((d["p"][n - 7:n].cpu() != ins["p"][n - 7:n]).all())


@pytest.mark.parametrize("n", [3, 1025])
def test_hyper_path_is_bit_equal_to_the_host_scalars(dev, n):
    """lr / first (SGD, RMSprop) and lr, step_size, bc2_sqrt (Adam) read from the device: the same bits as the host-scalar path; the
    host values handed over beside `hyper` are wrong on purpose"""
    from oaprogressionmmf_amd import ops
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)       # noqa: E731
    for first in (True, False):
        step = torch.full((1,), 0 if first else 3, dtype=torch.int32, device=dev)
        lr = torch.full((1,), LR, device=dev)
        hyper = torch.zeros(2, device=dev)
        ops.optim_hyper(step, lr, hyper)
        assert hyper.cpu().tolist() == [float(np.float32(LR)), 1.0 if first else 0.0] and int(step) == (1 if first else 4)
        for name, kw in SGD_VARIANTS:
            _, a, _, _ = _sgd(ops, dev, n, 5000 + n, kw, False, first)
            _, b, _, _ = _sgd(ops, dev, n, 5000 + n, kw, False, not first, hyper=hyper, host_lr=123.0)
            assert same(a, b), f"sgd {name} first {first}"
    lr = torch.full((1,), 1e-3, device=dev)
    hyper = torch.zeros(2, device=dev)
    ops.optim_hyper(torch.zeros(1, dtype=torch.int32, device=dev), lr, hyper)
    for cen in (False, True):
        for mom in (False, True):
            _, a, _, _ = _rms(ops, dev, n, 5100 + n, cen, mom, 0.99)
            _, b, _, _ = _rms(ops, dev, n, 5100 + n, cen, mom, 0.99, hyper=hyper, host_lr=123.0)
            assert same(a, b), f"rmsprop cen {cen} mom {mom}"
    for t in (1, 2, 1000):
        step = torch.full((1,), t - 1, dtype=torch.int32, device=dev)
        hyper = torch.zeros(3, device=dev)
        ops.adam_hyper(step, lr, B1, B2, hyper)
        for adamw in (False, True):
            for ams in (False, True):
                _, a, _, _ = _adam(ops, dev, n, 5200 + n, adamw, ams, t)
                _, b, _, _ = _adam(ops, dev, n, 5200 + n, adamw, ams, t, hyper=hyper, host_lr=123.0, host_step=7)
                assert same(a, b), f"adam adamw {adamw} amsgrad {ams} step {t}"


@pytest.mark.parametrize("step0", [0, 1, 999, 99999])
def test_adam_hyper_values(dev, step0):
    """hyper = float32 of the float64 formulas {lr, lr / (1 - b1^t), sqrt(1 - b2^t)} at t = step0 + 1, within 1 ulp (the device's
    pow is not the host's); the step comes back incremented"""
    from oaprogressionmmf_amd import ops
    step = torch.full((1,), step0, dtype=torch.int32, device=dev)
    lr = torch.full((1,), 3e-4, device=dev)
    hyper = torch.zeros(3, device=dev)
    ops.adam_hyper(step, lr, B1, B2, hyper)
    assert int(step) == step0 + 1
    want = R.adam_hyper_ref(np.float32(3e-4), B1, B2, step0 + 1)
    got = hyper.cpu().numpy()
    assert got[0] == np.float32(3e-4)
    for i in (1, 2):
        w32 = np.float32(want[i])
        ulps = abs(float(got[i]) - float(w32)) / float(np.spacing(w32))
        print(f"HYPER step {step0 + 1} [{i}]: got {got[i]!r} want {w32!r} ({ulps:.1f} ulp)")
        assert ulps <= 1.0, (step0, i, got[i], w32)


def _cls(t):
    t = torch.as_tensor(t)
    return torch.where(torch.isnan(t), 2, torch.where(torch.isinf(t), 1, 0))


SPECIAL = {5: 0.0, 10: 1e20, 15: float("nan"), 1024: float("nan")}     # three vectors of the body, and the scalar tail


def _plant(ins, n, state_keys):
    for i, gv in SPECIAL.items():
        ins["g"][i] = gv
        if gv == 0.0:
            for k in state_keys:
                ins[k][i] = 0.0


def _neighbours(n):
    skip = sorted(SPECIAL)
    near = sorted({j for i in skip if i < 1024 for j in range(i // 4 * 4, i // 4 * 4 + 4)} - set(skip))
    return skip, near


def test_special_values_land_in_torchs_class(dev):
    """g = 0 on zero state, g = 1e20 (its square overflows), g = NaN: every output lands in the class (finite | inf | NaN) of one step
    of torch.optim in fp32 on the CPU; the other elements -- their neighbours in the same 16-byte vector among them -- stay
    within the bound"""
    from oaprogressionmmf_amd import ops
    n = 1025
    skip, near = _neighbours(n)

    def torch_step(cls, ins, state, **kw):
        p = torch.nn.Parameter(ins["p"][:n].clone())
        opt = cls([p], foreach=False, **kw)
        opt.state[p] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()}
        p.grad = ins["g"][:n].clone()
        opt.step()
        return p.detach(), opt.state[p]

    def hold(d, ins, ref, bnd, tp, ts, names, what):
        _hold(d, ins, ref, bnd, n, what, skip=skip)
        assert set(near) <= set(range(n)) - set(skip)
        for mine, theirs in names.items():
            want = tp if theirs is None else ts[theirs]
            assert torch.equal(_cls(d[mine][:n].cpu())[skip], _cls(want)[skip]), \
                f"{what}: {mine} at {skip}: {d[mine][:n].cpu()[skip].tolist()} vs torch {want[skip].tolist()}"

    # SGD, Nesterov momentum with weight decay
    ins = R.optim_inputs(n, 6001, PAD, SENT)
    _plant(ins, n, ["buf"])
    d = _dev(ins, dev, "p", "g", "buf")
    ops.sgd_step(d["p"], d["g"], d["buf"], n, LR, momentum=0.9, wd=WD, nesterov=True)
    ref, bnd = R.sgd_step64(ins["p"][:n], ins["g"][:n], ins["buf"][:n], R.sgd_scalars(LR, 0.9, 0.0, WD), mom=True, nest=True)
    tp, ts = torch_step(torch.optim.SGD, ins, dict(momentum_buffer=ins["buf"][:n]), lr=LR, momentum=0.9, weight_decay=WD, nesterov=True)
    hold(d, ins, ref, bnd, tp, ts, dict(p=None, buf="momentum_buffer"), "sgd special")
    # RMSprop, centered with momentum
    ins = R.optim_inputs(n, 6002, PAD, SENT)
    _plant(ins, n, ["sq", "gavg", "buf"])
    d = _dev(ins, dev, "p", "g", "sq", "gavg", "buf")
    ops.rmsprop_step(d["p"], d["g"], d["sq"], n, 1e-3, wd=WD, momentum=0.9, gavg=d["gavg"], buf=d["buf"])
    ref, bnd = R.rms_step64(ins["p"][:n], ins["g"][:n], ins["sq"][:n], ins["gavg"][:n], ins["buf"][:n], R.rms_scalars(1e-3, 0.99, 1e-8, WD, 0.9))
    tp, ts = torch_step(torch.optim.RMSprop, ins, dict(step=torch.tensor(3.0), square_avg=ins["sq"][:n], grad_avg=ins["gavg"][:n],
                                                       momentum_buffer=ins["buf"][:n]), lr=1e-3, weight_decay=WD, momentum=0.9, centered=True)
    hold(d, ins, ref, bnd, tp, ts, dict(p=None, sq="square_avg", gavg="grad_avg", buf="momentum_buffer"), "rmsprop special")
    # Adam and AdamW with amsgrad
    for cls, adamw in ((torch.optim.Adam, False), (torch.optim.AdamW, True)):
        ins = R.optim_inputs(n, 6003, PAD, SENT)
        _plant(ins, n, ["m", "v", "vmax"])
        d = _dev(ins, dev, "p", "g", "m", "v", "vmax")
        ops.adam_step(d["p"], d["g"], d["m"], d["v"], n, 1e-3, B1, B2, EPS, WD, 2, adamw=adamw, vmax=d["vmax"])
        ref, bnd = R.adam_step64(ins["p"][:n], ins["g"][:n], ins["m"][:n], ins["v"][:n], ins["vmax"][:n], R.adam_scalars(1e-3, B1, B2, EPS, WD, 2), adamw=adamw)
        tp, ts = torch_step(cls, ins, dict(step=torch.tensor(1.0), exp_avg=ins["m"][:n], exp_avg_sq=ins["v"][:n], max_exp_avg_sq=ins["vmax"][:n]),
                            lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD, amsgrad=True)
        hold(d, ins, ref, bnd, tp, ts, dict(p=None, m="exp_avg", v="exp_avg_sq", vmax="max_exp_avg_sq"), f"adam special adamw {adamw}")


def test_unaligned_views_are_refused(dev):
    """a view starting one element into a buffer: refused with the library's error before anything is launched, the buffers unchanged"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    n = 16
    ins = R.optim_inputs(n + 1, 7001)
    d = _dev(ins, dev, *ins)
    v = {k: t[1:] for k, t in d.items()}
    calls = [("sgd", lambda a: ops.sgd_step(a["p"], a["g"], a["buf"], n, LR, momentum=0.9)),
             ("rmsprop", lambda a: ops.rmsprop_step(a["p"], a["g"], a["sq"], n, 1e-3, momentum=0.9, gavg=a["gavg"], buf=a["buf"])),
             ("adam", lambda a: ops.adam_step(a["p"], a["g"], a["m"], a["v"], n, 1e-3, B1, B2, EPS, WD, 1, vmax=a["vmax"]))]
    for name, call in calls:
        with pytest.raises(KoafError, match="unaligned"):
            call(v)
        for one in ("p", "g"):          # one unaligned operand among aligned ones is enough
            mixed = {k: (v[k] if k == one else d[k][:n]) for k in d}
            with pytest.raises(KoafError, match="unaligned"):
                call(mixed)
    torch.cuda.synchronize()
    for k in d:
        assert torch.equal(d[k].cpu(), ins[k]), k

