"""GPU: gradient accumulation over micro-batches (run.train_step_accum / run.GradientFold) and global-norm clipping
(various.clip_grad_norm_, train_step(max_grad_norm=...), GraphedTrainStep(max_grad_norm=...)) on registry models: the two
smallest shapes that cover both trunk kinds (resnet18 basic blocks, resnet50 bottlenecks) and the slice-fusion transformer.
Dropout is 0 everywhere; the backward kernels are deterministic, so most statements here are bit for bit."""
import hashlib
import inspect
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import procedural as P
from common import check_grads_branchy, rel
from test_models_gpu import build, t

pytestmark = pytest.mark.gpu

F32 = np.float32
SMOOTH_TOL = inspect.signature(check_grads_branchy).parameters["smooth_tol"].default      # the project's bar: 1e-4
CFGS = {"xr1cnn-resnet18": lambda: P.cfg_xr1cnn(arch="resnet18", size=160),
        "mr1-resnet50": lambda: P.cfg_mr1(arch="resnet50", shape=(160, 160, 6), depth=1)}


def _loss_fn():
    from oaprogressionmmf_amd.various import dict_losses
    return dict_losses["FocalLoss"](reduction="mean", gamma=2.0, num_classes=2)


def _batch(cfg, B, seed, dev):
    return [t(a).to(dev) for a in P.model_inputs(cfg, B, seed)], t(P.make_target("target", B, seed)).to(dev)


def _cut(batch, lo, hi):
    xs, ys = batch
    return [x[lo:hi].contiguous() for x in xs], ys[lo:hi].contiguous()


def _bits(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=F32)).view(np.uint32)


def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _backward(m, loss_fn, opt, batch):
    opt.zero_grad()
    loss_fn(m(*batch[0])["main"].squeeze(1), batch[1].long().squeeze(1)).backward()


def _arena(m):
    from oaprogressionmmf_amd.arena import get_arena
    return get_arena(m)


def _sgd(m, lr, **kw):
    from oaprogressionmmf_amd.various import dict_optimizers
    return dict_optimizers["SGD"](m.parameters(), lr=lr, **kw)


def _grad_norm64(m):
    return float(np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in m.parameters() if p.grad is not None)))


def _coef_np(max_norm, norm):
    c = F32(max_norm) / (F32(norm) + F32(1e-6))
    return c if not (c > F32(1.0)) else F32(1.0)


@pytest.mark.parametrize("name", list(CFGS))
def test_fold_is_the_weighted_sum_of_its_micro_gradients(dev, name):
    """train mode, micro-batches of 2 and 1 samples (w = 2/3, 1/3): the gradient train_step_accum leaves in G is
    np.float32(w0) * g0 + np.float32(w1) * g1 of the micro-gradients taken one by one from the same state, bit for bit, and
    BatchNorm's running buffers are those of the one-by-one run (two updates per step)"""
    from oaprogressionmmf_amd.run import micro_batch_weights, train_step_accum
    cfg, loss_fn = CFGS[name](), _loss_fn()
    full = _batch(cfg, 3, 21, dev)
    mbs = [_cut(full, 0, 2), _cut(full, 2, 3)]
    m = build(cfg, dev).train()
    sd0 = _state(m)
    opt = _sgd(m, 0.0)
    parts = []
    for mb in mbs:
        _backward(m, loss_fn, opt, mb)
        parts.append(_arena(m).G.detach().cpu().numpy().copy())
    bufs = {k: b.detach().clone() for k, b in m.named_buffers()}
    m.load_state_dict(sd0)
    logits, loss, norm = train_step_accum(m, loss_fn, _sgd(m, 0.0), mbs)
    assert norm is None and len(logits) == 2 and logits[0].shape[0] == 2 and logits[1].shape[0] == 1
    w = micro_batch_weights([2, 1])
    want = F32(w[0]) * parts[0] + F32(w[1]) * parts[1]
    got = _arena(m).G.detach().cpu().numpy()
    assert np.abs(want).max() > 0.0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for k, b in m.named_buffers():
        assert torch.equal(b, bufs[k]), k
    for k, v in m.named_parameters():
        assert torch.equal(v, sd0[k]), k                       # lr = 0: the step itself moved nothing


@pytest.mark.parametrize("name", list(CFGS))
def test_accumulated_equals_the_large_batch_in_eval_mode(dev, name):
    """eval(): BatchNorm on its running statistics, samples independent -- batch 4 in one backward against 2 + 2 accumulated is
    the same mathematics in another summation order, with no ReLU branch events between the two.  Bar: the project's own for
    parameters not subject to branch events (common.check_grads_branchy's smooth_tol, 1e-4), per-parameter relative L2.
    The measured worst value is printed (pytest -s)."""
    from oaprogressionmmf_amd.run import train_step_accum
    cfg, loss_fn = CFGS[name](), _loss_fn()
    full = _batch(cfg, 4, 22, dev)
    m = build(cfg, dev).eval()
    opt = _sgd(m, 0.0)
    _backward(m, loss_fn, opt, full)
    big = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    train_step_accum(m, loss_fn, opt, [_cut(full, 0, 2), _cut(full, 2, 4)])
    acc = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(acc) == sorted(big) and len(big) > 10
    errs = {k: rel(acc[k].cpu().numpy(), big[k].cpu().numpy()) for k in big}
    worst = max(errs, key=errs.get)
    print(f"accumulated vs large batch [{name}]: worst relative L2 {errs[worst]:.3e} at {worst}")
    assert errs[worst] <= SMOOTH_TOL, (worst, errs[worst])


@pytest.mark.parametrize("name,optname", [("xr1cnn-resnet18", "SGD"), ("mr1-resnet50", "SGD"), ("xr1cnn-resnet18", "Adam")])
def test_clipping_inside_train_step(dev, name, optname):
    """max_grad_norm at half the measured norm: the gradient the optimizer reads is numpy's fp32 g * coef bit for bit (coef the
    fp32 expression of the returned norm), the returned norm is within one fp32 ulp of the float64 norm of the unclipped
    gradient, and the parameters are those of a step on that scaled gradient -- for SGD (lr 1, no momentum) exactly
    p - g * coef.  At twice the norm the parameters are those of a run without the argument."""
    from oaprogressionmmf_amd.run import train_step
    from oaprogressionmmf_amd.various import dict_optimizers
    cfg, loss_fn = CFGS[name](), _loss_fn()
    xs, ys = _batch(cfg, 2, 23, dev)
    m = build(cfg, dev).train()
    sd0 = _state(m)

    def make_opt():
        return _sgd(m, 1.0) if optname == "SGD" else dict_optimizers["Adam"](m.parameters(), lr=1e-3, weight_decay=1e-4)

    def params():
        return {k: p.detach().clone() for k, p in m.named_parameters()}
    # plain step: the unclipped gradient (left in G) and where it takes the parameters
    p0 = _arena(m).P.detach().cpu().numpy().copy()
    assert len(train_step(m, loss_fn, make_opt(), xs, ys)) == 2
    g = _arena(m).G.detach().cpu().numpy().copy()
    n64 = _grad_norm64(m)
    assert n64 > 0.0 and abs(n64 - float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))) <= 1e-9 * n64
    plain = params()
    # clipped at half the norm
    m.load_state_dict(sd0)
    mx = 0.5 * n64
    _, _, norm = train_step(m, loss_fn, make_opt(), xs, ys, max_grad_norm=mx)
    norm = norm.cpu().numpy()
    assert abs(float(norm) - n64) <= float(np.spacing(F32(n64))), (float(norm), n64)
    coef = _coef_np(mx, norm)
    assert 0.49 < float(coef) < 0.51
    scaled = g * coef
    assert np.array_equal(_bits(_arena(m).G), scaled.view(np.uint32))
    clipped = params()
    if optname == "SGD":
        assert np.array_equal(_bits(_arena(m).P), (p0 - scaled).view(np.uint32))
    # the same update from a gradient scaled by hand: the scale reached the fused optimizer launch's input
    m.load_state_dict(sd0)
    opt = make_opt()
    _backward(m, loss_fn, opt, (xs, ys))
    assert np.array_equal(_bits(_arena(m).G), g.view(np.uint32))
    _arena(m).G.copy_(torch.from_numpy(scaled))
    opt.step()
    for k, v in m.named_parameters():
        assert torch.equal(v, clipped[k]), k
    assert any(not torch.equal(plain[k], clipped[k]) for k in plain)
    # twice the norm: nothing is clipped
    m.load_state_dict(sd0)
    _, _, norm2 = train_step(m, loss_fn, make_opt(), xs, ys, max_grad_norm=2.0 * n64)
    assert _bits(norm2) == _bits(norm)
    for k, v in m.named_parameters():
        assert torch.equal(v, plain[k]), k


@pytest.mark.parametrize("name", list(CFGS))
def test_graphed_train_step_with_clipping_replays_bit_identical_to_eager(dev, name):
    """GraphedTrainStep(max_grad_norm=...): one eager step, then the captured step replayed three times == four eager steps:
    norm, coefficient and scale live on the device, so the clip is part of the graph.  The bound is below every step's norm:
    the clip is active in all of them."""
    from oaprogressionmmf_amd.run import GraphedTrainStep
    from oaprogressionmmf_amd.various import dict_optimizers
    cfg, loss_fn = CFGS[name](), _loss_fn()
    xs, ys = _batch(cfg, 2, 24, dev)
    mx = 1e-3
    runs = []
    for warmup in (100, 1):                                  # never captures / captures at the second call
        m = build(cfg, dev).train()
        opt = dict_optimizers["Adam"](m.parameters(), lr=2e-5, weight_decay=1e-4, capturable=True)
        step = GraphedTrainStep(m, loss_fn, opt, xs, ys, warmup=warmup, seed=4242, max_grad_norm=mx)
        out = []
        for it in range(4):
            lg, ls, nm = step(xs, ys)
            out.append((lg.clone(), ls.clone(), nm.clone()))
        assert (step.graph is not None) == (warmup == 1)
        runs.append((out, {k: p.detach().clone() for k, p in m.named_parameters()}))
    (o0, p0), (o1, p1) = runs
    for a, b in zip(o0, o1):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(float(nm) > mx for _, _, nm in o0) and len({float(nm) for _, _, nm in o0}) == 4
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


def test_a_changed_gradient_set_raises(dev):
    from oaprogressionmmf_amd.run import GradientFold
    cfg, loss_fn = CFGS["xr1cnn-resnet18"](), _loss_fn()
    full = _batch(cfg, 2, 25, dev)
    m = build(cfg, dev).train()
    opt = _sgd(m, 0.0)
    fold = GradientFold(m)
    assert fold.A is None                                    # allocated at the first fold only
    _backward(m, loss_fn, opt, _cut(full, 0, 1))
    fold.add(0.5)
    assert fold.A is not None and fold.A.shape == _arena(m).G.shape
    [p for p in m.parameters() if p.dim() == 4][-1].requires_grad_(False)
    _backward(m, loss_fn, opt, _cut(full, 1, 2))
    with pytest.raises(RuntimeError, match="changed between the micro-batches"):
        fold.add(0.5, last=True)


# ---- two ranks on one GPU (gloo moves the buckets), two micro-batches per rank, clipping ---------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    sys.path.insert(0, str(here))
    sys.path.insert(0, str(here.parent))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oaprogressionmmf_amd.parallel import DataParallelRCCL
        from oaprogressionmmf_amd.run import GradientFold, train_step_accum
        dev = torch.device("cuda", 0)
        loss_fn = _loss_fn()

        class Recording(GradientFold):
            def add(self, w, last=False, norm_type=None):
                self.seen.append(_arena(self.module).G.detach().cpu().numpy().copy())
                return super().add(w, last=last, norm_type=norm_type)

        res = {}
        for name in CFGS:
            cfg = CFGS[name]()
            full = _batch(cfg, 4, 26, dev)
            mbs = [_cut(full, i, i + 1) for i in range(4)]
            # single process, four micro-batches (w = 1/4 each), no clip: the fold and the micro-gradients it saw
            ref = build(cfg, dev).eval()
            rec = Recording(ref)
            rec.seen = []
            train_step_accum(ref, loss_fn, _sgd(ref, 0.0), mbs, fold=rec)
            a = _arena(ref)
            single = a.G.detach().cpu().numpy().copy()
            mag = sum(np.abs(F32(0.25) * g).astype(np.float64) for g in rec.seen)
            slots = {k: a.slot(p) for k, p in ref.named_parameters() if p.grad is not None}
            n64 = float(np.sqrt(np.sum(single.astype(np.float64) ** 2)))
            # two ranks, micro-batches (0, 1) on rank 0 and (2, 3) on rank 1
            mod = build(cfg, dev).eval()
            ddp = DataParallelRCCL(mod, bucket_elems=4 * 1024 * 1024)
            mine = mbs[2 * rank:2 * rank + 2]
            train_step_accum(ddp, loss_fn, _sgd(mod, 0.0), mine)
            got = _arena(mod).G.detach().cpu().numpy()
            bad = []
            for k, (o, n) in slots.items():
                d = float(np.linalg.norm(got[o:o + n].astype(np.float64) - single[o:o + n]))
                bound = 4.0 * 2.0 ** -24 * float(np.linalg.norm(mag[o:o + n]))
                if not d <= bound:
                    bad.append((k, d, bound))
            _, _, norm = train_step_accum(ddp, loss_fn, _sgd(mod, 1.0), mine, max_grad_norm=0.5 * n64)
            torch.cuda.synchronize()
            res[name] = dict(bad=bad, ntensors=len(slots), norm=int(_bits(norm)), n64=n64, normf=float(norm),
                             magn=float(np.linalg.norm(mag)),
                             params=hashlib.sha256(_arena(mod).P.detach().cpu().numpy().tobytes()).hexdigest(),
                             moved=not np.array_equal(_arena(mod).P.detach().cpu().numpy(), _arena(ref).P.detach().cpu().numpy()))
        q.put((rank, None, res))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_two_ranks_accumulate_and_clip_alike(dev):
    """world of 2 on one device, eval() so that each micro-gradient is the same bits wherever it is computed (no per-replica
    BatchNorm buffers): (i) the gradient folded from two exchanged micro-batches per rank is the single-process fold of the
    four within the reassociation bound of four fp32 addends in another order, per tensor
    ||a - b|| <= 4 * 2^-24 * || sum_i |w_i g_i| ||; (ii) after a clipped step (bound at half the norm) both ranks report the
    same norm bits and hold the same parameter bits."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
    for rank, err, _ in res:
        assert err is None, f"rank {rank}:\n{err}"
    by_rank = {rank: r for rank, _, r in res}
    for name in CFGS:
        r0, r1 = by_rank[0][name], by_rank[1][name]
        for r in (r0, r1):
            assert r["ntensors"] > 10 and r["bad"] == [], (name, r["bad"][:3])
            # | ||a|| - ||b|| | <= ||a - b||, plus the norm kernel's one rounding to fp32
            assert abs(r["normf"] - r["n64"]) <= 4.0 * 2.0 ** -24 * r["magn"] + 2.0 ** -23 * r["n64"], (name, r["normf"], r["n64"])
            assert r["moved"]
        assert r0["norm"] == r1["norm"], (name, r0["normf"], r1["normf"])
        assert r0["params"] == r1["params"], name
