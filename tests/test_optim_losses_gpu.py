"""GPU: the native SGD / RMSprop / BCE registry entries against the torch classes the reference registers
(koafusion/various/_optimizers.py:47-52, _losses.py:111-117), which run on the CPU here as the reference.
 * kernels: four steps of fixed gradients over an odd length (vector body + scalar tail), every option
 * optimizer classes on a registry model, all four keys (Adam / AdamW share the base class of the other two): only the update
   rule is compared (torch is fed the device run's gradients)
 * resume through save_train_state / load_train_state, into a fresh native instance and into torch.optim
 * captured steps (run.GraphedTrainStep) bit-identical to eager ones, with a scheduler step between replays
 * BCELoss / BCEWithLogitsLoss against torch in float64: loss, gradient, options, the grid form's determinism
Tolerances are the ones of the Adam and loss tests of test_kernels_gpu.py / test_run_gpu.py: the same kind of arithmetic against
the same kind of reference."""
import pytest
import torch
import torch.nn.functional as F

import procedural as P
from common import rel
from test_models_gpu import build, t

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- kernels ---------------------------------------------------------------------------------------------------------------
N_ODD = 10007          # odd: 2501 16-byte vectors + a 3-element tail, an unaligned end


@pytest.mark.parametrize("kw", [dict(), dict(momentum=0.9), dict(momentum=0.9, dampening=0.1), dict(momentum=0.9, nesterov=True),
                                dict(weight_decay=1e-4), dict(momentum=0.9, maximize=True)],
                         ids=["plain", "momentum", "dampening", "nesterov", "weight_decay", "maximize"])
def test_sgd_kernel_against_torch(dev, kw):
    from oaprogressionmmf_amd import ops
    p0, gs = _rnd(N_ODD, seed=1), [_rnd(N_ODD, seed=10 + s) for s in range(4)]
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([pr], lr=0.05, **kw)
    pd = p0.clone().to(dev)
    buf = torch.zeros(N_ODD, device=dev) if kw.get("momentum") else None
    for s in range(4):
        pr.grad = gs[s].clone()
        opt.step()
        ops.sgd_step(pd, gs[s].to(dev), buf, N_ODD, 0.05, momentum=kw.get("momentum", 0.0), dampening=kw.get("dampening", 0.0),
                     wd=kw.get("weight_decay", 0.0), nesterov=kw.get("nesterov", False), maximize=kw.get("maximize", False),
                     first=(s == 0))
        e = rel_err(pd, pr.detach())
        print(f"sgd {kw} step {s}: parameters {e:.3e}")
        assert e < 1e-6
    if buf is not None:
        e = rel_err(buf, opt.state[pr]["momentum_buffer"])
        print(f"sgd {kw}: momentum_buffer {e:.3e}")
        assert e < 1e-6
    assert rel_err(pd, p0) > 1e-3             # (it moved)


@pytest.mark.parametrize("kw", [dict(), dict(centered=True), dict(momentum=0.9),
                                dict(centered=True, momentum=0.9, weight_decay=1e-4)],
                         ids=["default", "centered", "momentum", "centered_momentum_wd"])
def test_rmsprop_kernel_against_torch(dev, kw):
    from oaprogressionmmf_amd import ops
    p0, gs = _rnd(N_ODD, seed=2), [_rnd(N_ODD, seed=20 + s) for s in range(4)]
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.RMSprop([pr], lr=1e-3, **kw)
    pd = p0.clone().to(dev)
    st = {"square_avg": torch.zeros(N_ODD, device=dev)}
    if kw.get("centered"):
        st["grad_avg"] = torch.zeros(N_ODD, device=dev)
    if kw.get("momentum"):
        st["momentum_buffer"] = torch.zeros(N_ODD, device=dev)
    for s in range(4):
        pr.grad = gs[s].clone()
        opt.step()
        ops.rmsprop_step(pd, gs[s].to(dev), st["square_avg"], N_ODD, 1e-3, alpha=0.99, eps=1e-8, wd=kw.get("weight_decay", 0.0),
                         momentum=kw.get("momentum", 0.0), gavg=st.get("grad_avg"), buf=st.get("momentum_buffer"))
        e = rel_err(pd, pr.detach())
        print(f"rmsprop {kw} step {s}: parameters {e:.3e}")
        assert e < 1e-6
    for k, v in st.items():
        e = rel_err(v, opt.state[pr][k])
        print(f"rmsprop {kw}: {k} {e:.3e}")
        assert e < 1e-6
    assert rel_err(pd, p0) > 1e-4


def test_device_step_state_drives_lr_and_first(dev):
    """koaf_optim_hyper: the step kernels take lr and `first` from the device (the host values are ignored)"""
    from oaprogressionmmf_amd import ops
    n = 1003
    p0, g = _rnd(n, seed=3), _rnd(n, seed=4)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    lr = torch.full((1,), 0.05, device=dev)
    hyper = torch.zeros(2, device=dev)
    pa, pb = p0.clone().to(dev), p0.clone().to(dev)
    ba, bb = torch.full((n,), 7.0, device=dev), torch.zeros(n, device=dev)      # (a first step must not read the buffer)
    for s in range(3):
        ops.optim_hyper(step, lr, hyper)
        ops.sgd_step(pa, g.to(dev), ba, n, 123.0, momentum=0.9, first=(s != 0), hyper=hyper)      # host lr / first: wrong on purpose
        ops.sgd_step(pb, g.to(dev), bb, n, 0.05, momentum=0.9, first=(s == 0))
        assert hyper.tolist() == [pytest.approx(0.05), 1.0 if s == 0 else 0.0]
    assert int(step) == 3
    assert torch.equal(pa, pb) and torch.equal(ba, bb)
    qa, qb = p0.clone().to(dev), p0.clone().to(dev)
    sa, sb = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr.fill_(2e-3)
    ops.optim_hyper(step, lr, hyper)
    ops.rmsprop_step(qa, g.to(dev), sa, n, 123.0, hyper=hyper)
    ops.rmsprop_step(qb, g.to(dev), sb, n, 2e-3)
    assert torch.equal(qa, qb) and torch.equal(sa, sb)


# ---- optimizer classes on a registry model ------------------------------------------------------------------------------------
OPTS = {"SGD": dict(lr=1e-3, momentum=0.9, weight_decay=1e-4),
        "RMSprop": dict(lr=1e-5, momentum=0.5, centered=True, weight_decay=1e-4),    # (small: RMSprop's first steps are ~10 lr per weight)
        "Adam": dict(lr=1e-4, weight_decay=1e-4),
        "AdamW": dict(lr=1e-4, weight_decay=1e-2),
        "Adam-amsgrad": dict(lr=1e-4, amsgrad=True)}                                 # (the class is the part before the dash)


def _small_case(dev, seed):
    cfg = P.cfg_xr1mr1(xr=(64, 64), mr=(64, 64, 3), depth=1)
    B = 2
    xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, seed)]
    y = t(P.make_target("target", B, seed)).to(dev)
    return cfg, xs, y


def _backward(m, opt, loss_fn, xs, y):
    opt.zero_grad()
    logits = m(*xs)["main"]
    loss_fn(logits.squeeze(1), y.long().squeeze(1)).backward()
    return logits.detach().clone()


def _hand_grads(cpu_params, m):
    for cp, p in zip(cpu_params, m.parameters()):
        cp.grad = None if p.grad is None else p.grad.detach().cpu().contiguous().clone()


@pytest.mark.parametrize("name", ["SGD", "RMSprop", "Adam", "AdamW", "Adam-amsgrad"])
def test_optimizer_class_on_a_registry_model(dev, name):
    """three steps: the update rule alone against torch.optim on CPU copies fed the device run's gradients"""
    cls = name.split("-")[0]
    from oaprogressionmmf_amd.arena import get_arena
    from oaprogressionmmf_amd.various import dict_losses, dict_optimizers
    # (the fusion model with two MRI branches: the `mlp_head0` tensors of its cls-less aggregators never receive a gradient)
    cfg = P.cfg_full(xr=(96, 96), mr1=(64, 64, 6), mr2=(64, 64, 5), depth=1)
    xs = [t(a).to(dev) for a in P.model_inputs(cfg, 2, 9)]
    y = t(P.make_target("target", 2, 9)).to(dev)
    loss_fn = dict_losses["FocalLoss"](reduction="mean", gamma=2.0, num_classes=2)
    m = build(cfg, dev).train()
    opt = dict_optimizers[cls](m.parameters(), **OPTS[name])
    assert type(opt).__module__.startswith("oaprogressionmmf_amd")
    cpu_params = [torch.nn.Parameter(p.detach().cpu().contiguous().clone()) for p in m.parameters()]
    start = [cp.detach().clone() for cp in cpu_params]
    ref = getattr(torch.optim, cls)(cpu_params, **OPTS[name])
    logits0 = _backward(m, opt, loss_fn, xs, y)
    arena = get_arena(m)
    epoch0 = arena.epoch
    for it in range(3):
        if it:
            _backward(m, opt, loss_fn, xs, y)
        _hand_grads(cpu_params, m)
        opt.step()
        ref.step()
    assert arena.epoch == epoch0 + 3
    worst, moved, idle = 0.0, 0, 0
    for (k, p), cp, p0 in zip(m.named_parameters(), cpu_params, start):
        if p.grad is None:
            idle += 1
            assert torch.equal(p.detach().cpu(), p0), f"{k}: no gradient, yet it changed"
            continue
        e = rel(p.detach().cpu().numpy(), cp.detach().numpy())
        worst = max(worst, e)
        assert e < 1e-6, f"{name}: {k} differs from torch.optim.{cls} by {e:.3e}"
        moved += int(not torch.equal(p.detach().cpu(), p0))
    print(f"{name}: worst parameter rel err {worst:.3e}; {moved} tensors moved, {idle} without gradient")
    assert moved > 0 and idle > 0
    logits3 = _backward(m, opt, loss_fn, xs, y)              # the next eager forward multiplies with the new weights
    assert not torch.equal(logits0, logits3)
    # the exported state is torch's: same entries as the reference optimizer's
    sd, sd_ref = opt.state_dict(), ref.state_dict()
    assert sorted(sd["state"]) == sorted(sd_ref["state"])
    for i, st in sd_ref["state"].items():
        assert set(sd["state"][i]) == set(st)
        for k2, v in st.items():
            assert rel(torch.as_tensor(sd["state"][i][k2]).numpy(), torch.as_tensor(v).numpy()) < 1e-6, (i, k2)


@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_resume_and_torch_interop(dev, tmp_path, name):
    """a run interrupted after two steps and resumed in a fresh model + optimizer continues bit-identically, and torch.optim's
    class, loaded with the exported state on CPU copies, makes the same third step"""
    from oaprogressionmmf_amd.run import train_step
    from oaprogressionmmf_amd.various import dict_losses, dict_optimizers, load_train_state, save_train_state
    cfg, xs, y = _small_case(dev, 9)
    loss_fn = dict_losses["FocalLoss"](reduction="mean", gamma=2.0, num_classes=2)

    def fresh():
        m = build(cfg, dev).train()
        return m, dict_optimizers[name](m.parameters(), **OPTS[name])
    m1, o1 = fresh()
    for _ in range(2):
        train_step(m1, loss_fn, o1, xs, y)
    path = save_train_state(tmp_path / "state.pth", m1, o1, epoch=7)
    train_step(m1, loss_fn, o1, xs, y)                                   # uninterrupted third step
    m2, o2 = fresh()
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)                                                   # must be overwritten by the load
    assert load_train_state(path, m2, o2) == {"epoch": 7}
    sd = o2.state_dict()                                                  # (parked: the fresh model has adopted no arena yet)
    assert len(sd["state"]) > 0
    if name == "RMSprop":
        assert all(float(v["step"]) == 2.0 for v in sd["state"].values())
    cpu_params = [torch.nn.Parameter(p.detach().cpu().contiguous().clone()) for p in m2.parameters()]
    ref = getattr(torch.optim, name)(cpu_params, **OPTS[name])
    ref.load_state_dict(sd)
    _backward(m2, o2, loss_fn, xs, y)
    _hand_grads(cpu_params, m2)
    o2.step()
    ref.step()
    for (k, a), b, cp in zip(m1.named_parameters(), m2.parameters(), cpu_params):
        assert torch.equal(a, b), f"resumed run diverged at {k}"
        assert rel(b.detach().cpu().numpy(), cp.detach().numpy()) < 1e-6, f"torch.optim.{name} continues differently at {k}"


@pytest.mark.parametrize("name,kw,calls", [("SGD", dict(lr=1e-3, momentum=0.9, weight_decay=1e-4), 5),
                                           ("RMSprop", dict(lr=1e-7, weight_decay=1e-4), 4)])   # (RMSprop's first steps move EVERY weight by ~10 lr: at 1e-5 the loss is at zero after one)
def test_graphed_train_step_replay_is_bit_identical_to_eager(dev, name, kw, calls):
    """run.GraphedTrainStep with the native optimizers (capturable=True): two warm-up calls, then the captured step replayed,
    == the same steps run eagerly, bit for bit; the learning rate changes between two replays (a scheduler step), and SGD's
    `first` flag comes from the device step count.  Same model, sizes and stream handling as the graphed-Adam test."""
    from oaprogressionmmf_amd.run import GraphedTrainStep
    from oaprogressionmmf_amd.various import dict_losses, dict_optimizers
    cfg = P.cfg_full(xr=(96, 96), mr1=(64, 64, 6), mr2=(64, 64, 5), depth=1, dropout=0.1)
    B = 2
    xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, 11)]
    ys = t(P.make_target("target", B, 11)).to(dev)
    loss_fn = dict_losses["FocalLoss"](reduction="mean", gamma=2.0, num_classes=2)
    runs = []
    for warmup in (100, 2):                              # never captures / captures at the third call
        m = build(cfg, dev).train()
        opt = dict_optimizers[name](m.parameters(), capturable=True, **kw)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: 0.5 ** e)
        step = GraphedTrainStep(m, loss_fn, opt, xs, ys, warmup=warmup, seed=4242)
        losses, logits = [], []
        for it in range(calls):
            if it == 3:
                sched.step()                             # a scheduler step between two replays
            lg, ls = step(xs, ys)
            losses.append(float(ls))
            logits.append(lg.clone())
        assert (step.graph is not None) == (warmup == 2)
        assert opt.param_groups[0]["lr"] == pytest.approx(kw["lr"] * 0.5)
        sd = opt.state_dict()
        assert len(sd["state"]) > 0
        if name == "RMSprop":
            assert {float(v["step"]) for v in sd["state"].values()} == {float(calls)}
        else:
            assert all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
        runs.append((losses, logits, {k: p.detach().clone() for k, p in m.named_parameters()}))
    (l0, g0, p0), (l1, g1, p1) = runs
    assert l0 == l1, (l0, l1)
    assert len(set(l0)) == calls                         # the steps differ (training moves, fresh dropout masks)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


@pytest.mark.parametrize("name", ["SGD", "Adam", "AdamW", "RMSprop"])
def test_capturable_refuses_a_loose_parameter(dev, name):
    from oaprogressionmmf_amd.various import dict_optimizers
    p = torch.nn.Parameter(torch.zeros(8, device=dev))
    p.grad = torch.ones(8, device=dev)
    with pytest.raises(RuntimeError, match="arena parameters only"):
        dict_optimizers[name]([p], lr=0.1, capturable=True).step()
    dict_optimizers[name]([p], lr=0.1).step()             # without it a loose device parameter is updated on its own
    assert float(p.detach().abs().min()) > 0


# ---- BCE ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(64,), (37, 5), (2, 3, 70, 71)]                # the last one is beyond one block's reach: the grid form


def _bce_inputs(shape, logits, seed):
    g = torch.Generator().manual_seed(seed)
    n = 1
    for d in shape:
        n *= d
    x = torch.randn(n, generator=g) * 3.0
    tg = torch.rand(n, generator=g)                       # soft targets ...
    tg[::5] = tg[::5].round()                             # ... and hard ones
    if logits:
        x[:10] = torch.tensor([30.0, -30.0, 50.0, -50.0, 0.0, 30.0, -30.0, 50.0, -50.0, 0.0])
        tg[:10] = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.5, 0.0, 1.0, 0.0, 1.0, 1.0])
    else:
        x = torch.sigmoid(x)
        x[:6] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
        tg[:6] = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.3, 0.7])
    return x.reshape(shape), tg.reshape(shape)


def _bce_check(dev, key, x, tg, reduction, weight=None, pos_weight=None, seed=0):
    from oaprogressionmmf_amd.various import dict_losses
    kw = dict(weight=weight, reduction=reduction)
    if pos_weight is not None:
        kw["pos_weight"] = pos_weight
    loss_fn = dict_losses[key](**kw).to(dev)
    xd = x.clone().to(dev).requires_grad_(True)
    out = loss_fn(xd, tg.to(dev))
    x64 = x.double().requires_grad_(True)
    w64 = None if weight is None else weight.double()
    if key == "bce_loss":
        ref = F.binary_cross_entropy(x64, tg.double(), weight=w64, reduction=reduction)
    else:
        ref = F.binary_cross_entropy_with_logits(x64, tg.double(), weight=w64, reduction=reduction,
                                                 pos_weight=None if pos_weight is None else pos_weight.double())
    assert out.shape == ref.shape
    up = (torch.rand(x.shape, generator=torch.Generator().manual_seed(seed + 77)) + 0.5) if reduction == "none" else torch.tensor(1.0)
    out.backward(up.to(dev))
    ref.backward(up.double())
    d = (out.detach().cpu().double() - ref.detach()).abs()
    bound = 2e-6 * ref.detach().abs().clamp(min=1.0)
    # The gradient, three ways.  The planted probabilities 0 / 1 against the opposite target have gradients of +-1e12 (torch's
    # 1e-12 clamp of the denominator), which alone make up the norm of the whole tensor: the norm-relative error is therefore
    # also taken over the elements away from the clamp, and every element is checked on its own -- |d - ref| <= 1e-5 *
    # max(|ref|, unit), unit = |upstream| * weight * (1 / n for the mean) * max(1, pos_weight): the size of the terms the
    # gradient is a difference of (lw * sigmoid(x) - pw * t; (x - t) over a denominator <= 1/4), each of them rounded at 6e-8.
    got, want = xd.grad.detach().cpu().double(), x64.grad
    ge = rel_err(got, want)
    plain = want.abs() < 1e6
    ge_plain = rel_err(got[plain], want[plain])
    unit = up.double().abs().expand(x.shape) * (1.0 if weight is None else weight.double().expand(x.shape))
    unit = unit * (1.0 / x.numel() if reduction == "mean" else 1.0) * (1.0 if pos_weight is None else max(1.0, float(pos_weight.max())))
    ratio = (got - want).abs() / (1e-5 * torch.maximum(want.abs(), unit))
    print(f"{key} {tuple(x.shape)} {reduction} w={weight is not None} pw={pos_weight is not None}: "
          f"loss err / bound {float((d / bound).max()):.3f}, gradient rel err {ge:.3e} (away from the clamp: {ge_plain:.3e}, "
          f"{int(plain.sum())} of {plain.numel()} elements), worst element err / bound {float(ratio.max()):.3f}")
    assert bool((d <= bound).all()), float((d / bound).max())
    assert ge < 1e-5 and ge_plain < 1e-5
    assert int(plain.sum()) >= plain.numel() - 8 and float(want[plain].abs().max()) > 0
    assert bool((ratio <= 1.0).all()), (float(ratio.max()), int(ratio.argmax()))
    return out.detach(), xd.grad.detach()


@pytest.mark.parametrize("shape", SHAPES, ids=["64", "37x5", "2x3x70x71"])
@pytest.mark.parametrize("key", ["bce_loss", "bce_wlogits_loss"])
def test_bce_against_torch_float64(dev, key, shape):
    logits = key == "bce_wlogits_loss"
    x, tg = _bce_inputs(shape, logits, seed=len(shape))
    g = torch.Generator().manual_seed(5)
    w_full = torch.rand(shape, generator=g) + 0.5
    w_last = torch.rand(shape[-1], generator=g) + 0.5     # broadcast against the input, as torch does
    pw = (torch.rand(shape[-1], generator=g) * 3.0 + 0.25) if logits else None
    for reduction in ("mean", "sum", "none"):
        _bce_check(dev, key, x, tg, reduction)
        _bce_check(dev, key, x, tg, reduction, weight=w_full)
        if logits:
            _bce_check(dev, key, x, tg, reduction, pos_weight=pw)
            _bce_check(dev, key, x, tg, reduction, weight=w_last, pos_weight=pw)
        else:
            _bce_check(dev, key, x, tg, reduction, weight=w_last)


@pytest.mark.parametrize("key", ["bce_loss", "bce_wlogits_loss"])
def test_bce_grid_form_is_deterministic(dev, key):
    x, tg = _bce_inputs(SHAPES[-1], key == "bce_wlogits_loss", seed=8)
    for reduction in ("mean", "sum"):
        a = _bce_check(dev, key, x, tg, reduction)
        b = _bce_check(dev, key, x, tg, reduction)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_bce_probability_out_of_range_is_counted_not_propagated(dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.various import dict_losses
    x, tg = _bce_inputs((37, 5), False, seed=6)
    ok = torch.ones_like(x, dtype=torch.bool)
    x[3, 1], x[20, 4], x[30, 0] = 1.5, -0.25, float("nan")
    ok[3, 1] = ok[20, 4] = ok[30, 0] = False
    ops.numerics_status(reset=True)
    xd = x.clone().to(dev).requires_grad_(True)
    out = dict_losses["bce_loss"](reduction="sum")(xd, tg.to(dev))
    out.backward()
    st = ops.numerics_status(reset=True)
    assert st["nonfinite"] == 3, st
    assert bool((xd.grad.cpu()[~ok] == 0).all()) and bool(torch.isfinite(xd.grad).all())
    ref = F.binary_cross_entropy(x[ok].double(), tg[ok].double(), reduction="sum")
    assert abs(float(out.detach()) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
    gref = (x.double() - tg.double()) / ((1 - x.double()) * x.double()).clamp(min=1e-12)     # torch's backward, in-range elements
    got = xd.grad.cpu().double()
    assert bool(((got - gref)[ok].abs() <= 1e-5 * gref[ok].abs().clamp(min=1.0)).all())      # (they keep their gradient)
