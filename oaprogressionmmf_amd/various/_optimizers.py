"""Optimizer / scheduler registries (reference: koafusion/various/_optimizers.py:4-67).

The registry's four optimizers (`SGD`, `Adam`, `AdamW`, `RMSprop`) are fused: one HIP launch per contiguous run of the flat
parameter arena (for the reference models: one or two launches for all 389 M elements) instead of torch's per-tensor loops, on
koaf_sgd_step / koaf_adam_step / koaf_rmsprop_step, with torch's constructor signatures, update rules (Adam: coupled L2 weight
decay, bias-corrected) and state_dict layouts.  Parameters whose `.grad` is None are skipped exactly like torch does (SURVEY Q4:
12 tensors of the cls-less aggregators never train).  What the four share is `_ArenaOptimizer`.
"""
import torch
from torch import optim

from .. import ops


class _ArenaOptimizer(optim.Optimizer):
    """What the fused optimizers share: the parameters that hold a gradient grouped by arena (foreign gradient tensors brought
    into the arena's gradient view), state buffers the size of the arena, named with torch's state_dict keys, one launch per
    contiguous run of parameters with a gradient, loose parameters, the device-resident step count / learning rate of captured
    steps, per-parameter update counts, torch's checkpoint layout and zero_grad's arena bookkeeping.  A subclass names the
    buffers a group uses (`_state_names`) and launches its kernel (`_launch`); where its update depends on the parameter's
    update count it says on what part of it (`_run_key`).  No CPU fallback: a CPU parameter raises."""
    _NAME = "optimizer"
    _NHYPER = 2          # floats the step kernel reads from the device in a captured step (koaf_optim_hyper: {lr, first})
    _HAS_STEP = False    # torch's per-parameter state carries a `step` entry

    def _init_flat(self, capturable, differentiable=False):
        if differentiable:
            raise ValueError(f"koaf {self._NAME}: differentiable=True is not supported (the update runs in a HIP kernel outside autograd)")
        self.capturable = bool(capturable)
        self._dev = {}       # capturable: (id(arena), id(group)) -> device step count / lr / hyper (see _dev_state)
        self._flat = {}      # id(arena) -> {state name: flat buffer like arena.P}
        self._loose = {}     # id(param) -> {state name: flat buffer} for parameters outside any arena
        self._steps = {}     # id(param) -> number of updates it has received (torch keeps `step` per parameter)
        self._pending = {}   # id(param) -> {state name: tensor} loaded before the parameter moved into its arena

    def _state_names(self, group):
        raise NotImplementedError

    def _run_key(self, n):
        """what a launch depends on of its parameters' update count n: parameters with equal keys share launches"""
        return False

    def _hyper(self, group, d):
        """captured steps: advance the device step count, derive what the step kernel reads from it"""
        ops.optim_hyper(d["step"], d["lr"], d["hyper"])

    def _launch(self, group, p, g, st, n, key, hyper):
        raise NotImplementedError

    def _gather(self, group, loose):
        """-> {id(arena): (arena, [parameters of `group` with a gradient])}; parameters outside any arena go to loose(p)"""
        by_arena = {}
        for p in group["params"]:
            if p.grad is None:
                continue
            a = getattr(p, "_koaf_arena", None)
            if a is not None and a.valid():
                gv = p._koaf_grad
                if p.grad.data_ptr() != gv.data_ptr():
                    gv.copy_(p.grad)       # a foreign gradient tensor: bring it into the arena
                    p.grad = gv
                by_arena.setdefault(id(a), (a, []))[1].append(p)
            else:
                if self.capturable:
                    # (its step count would live on the host: a captured step would replay with a frozen count)
                    raise RuntimeError(f"koaf {self._NAME}(capturable=True) updates arena parameters only: this parameter lives "
                                       "outside the model's arena (run one forward of the model before the first step)")
                loose(p)
        return by_arena

    def _require_device(self, p):
        if not p.is_cuda:
            raise RuntimeError(f"koaf {self._NAME} updates HIP-resident parameters only (no CPU fallback)")

    def _dev_state(self, a, group):
        key = (id(a), id(group))
        d = self._dev.get(key)
        if d is None:
            d = dict(step=torch.full((1,), int(getattr(self, "_resume_step", 0)), dtype=torch.int32, device=a.device),
                     lr=torch.full((1,), float(group["lr"]), device=a.device), hyper=torch.zeros(self._NHYPER, device=a.device),
                     lr_host=float(group["lr"]), params=set())
            self._dev[key] = d
        return d

    def sync_hyper(self):
        """copy the (scheduler-driven) learning rates to their device scalars; call outside a graph capture / before a replay"""
        for group in self.param_groups:
            for (aid, gid), d in self._dev.items():
                if gid == id(group) and d["lr_host"] != float(group["lr"]):
                    d["lr"].fill_(float(group["lr"]))
                    d["lr_host"] = float(group["lr"])

    def _sync_steps(self):
        """capturable: the per-parameter update counts torch's state_dict layout wants, from the device counters"""
        for d in self._dev.values():
            n = int(d["step"].item())
            for pid in d["params"]:
                self._steps[pid] = n

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)
        for group in self.param_groups:
            for p in group["params"]:
                a = getattr(p, "_koaf_arena", None)
                if a is not None:
                    a.grad_dirty = False

    @staticmethod
    def _bufs(stt, names, like):
        """the flat state buffers `names` of one arena / loose parameter (created zeroed on first use), sized like `like`"""
        for k in names:
            if k not in stt:
                stt[k] = torch.zeros(like.numel(), device=like.device)
        return stt

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._pending:
            self._place_pending()            # (placement is final here: the forward that produced the gradients ran)
        for group in self.param_groups:
            names = self._state_names(group)
            by_arena = self._gather(group, lambda p: self._step_loose(p, group, names))
            for a, plist in by_arena.values():
                stt = self._bufs(self._flat.setdefault(id(a), {}), names, a.P)
                if self.capturable:
                    d = self._dev_state(a, group)
                    if not torch.cuda.is_current_stream_capturing():
                        self.sync_hyper()
                    d["params"].update(id(p) for p in plist)
                    self._hyper(group, d)
                    runs = {False: plist}    # (one shared count: what depends on it comes from the device)
                else:
                    # one fused launch per contiguous run of parameters whose update counts share a key (SGD: all at their
                    # first update, or all past it; Adam: one count).  For the reference models: every trained parameter
                    # receives a gradient from the first step on
                    d, runs = None, {}
                    for p in plist:
                        n = self._steps.get(id(p), 0) + 1
                        self._steps[id(p)] = n
                        runs.setdefault(self._run_key(n), []).append(p)
                for key, ps in runs.items():
                    for lo, hi in a.active_ranges(ps):
                        self._launch(group, a.P[lo:hi], a.G[lo:hi], {k: stt[k][lo:hi] for k in names}, hi - lo, key,
                                     d["hyper"] if d else None)
                a.epoch += 1             # the weights changed under the arena's plane images (arena.ensure_planes)
        return loss

    def _step_loose(self, p, group, names):
        self._require_device(p)
        stt = self._bufs(self._loose.setdefault(id(p), {}), names, p)
        n = self._steps.get(id(p), 0) + 1
        self._steps[id(p)] = n
        pc = p.data.contiguous().view(-1)
        g = p.grad.contiguous().view(-1)
        self._launch(group, pc, g, stt, pc.numel(), self._run_key(n), None)
        if pc.data_ptr() != p.data.data_ptr():
            p.data.copy_(pc.view_as(p.data))

    # ---- checkpointing: torch.optim's state_dict layout, so either side resumes the other's run ----------
    def _views(self, p, names, create=False):
        """{state name: tensor of p's logical shape} (views of the flat buffers), or None when p has no state yet"""
        a = getattr(p, "_koaf_arena", None)
        if a is not None and a.valid():
            if id(a) not in self._flat and not create:
                return None
            stt = self._bufs(self._flat.setdefault(id(a), {}), names, a.P)
            o, n = a.slot(p)
            return {k: a._view(stt[k], o, n, p) for k in names}
        if id(p) not in self._loose and not create:
            return None
        stt = self._bufs(self._loose.setdefault(id(p), {}), names, p)
        return {k: stt[k].view(p.shape) for k in names}

    def _place_pending(self):
        """state loaded by load_state_dict() goes to the flat buffers once the parameters' final placement is known
        (a model adopts its arena at its first forward, which may come after the optimizer state was loaded)"""
        for g in self.param_groups:
            names = self._state_names(g)
            for p in g["params"]:
                loaded = self._pending.pop(id(p), None)
                if loaded is None:
                    continue
                self._require_device(p)
                for k, dst in self._views(p, names, create=True).items():
                    if k in loaded:
                        dst.copy_(loaded[k].to(device=p.device, dtype=torch.float32))
        self._pending = {}

    def state_dict(self):
        if self.capturable:
            self._sync_steps()
        sd = super().state_dict()            # param_groups with index lists; `state` is kept outside self.state
        state, idx = {}, 0
        for g in self.param_groups:
            names = self._state_names(g)
            for p in g["params"]:
                n = self._steps.get(id(p), 0)
                st = self._pending.get(id(p)) or (self._views(p, names) if n else None)   # loaded but not yet placed / live
                if st is not None and (names or self._HAS_STEP):     # never updated, or nothing to keep: torch has no entry either
                    ent = dict(step=torch.tensor(float(n))) if self._HAS_STEP else {}
                    for k in names:
                        ent[k] = st[k].detach().to("cpu").contiguous().clone() if k in st else torch.zeros(p.shape)
                    state[idx] = ent
                idx += 1
        sd["state"] = state
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        super().load_state_dict(dict(state={}, param_groups=groups))
        params = [(p, self._state_names(g)) for g in self.param_groups for p in g["params"]]
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(params):
            raise ValueError("loaded state dict has a different number of parameters")
        self._steps, self._pending = {}, {}
        for stt in list(self._flat.values()) + list(self._loose.values()):
            for buf in stt.values():
                buf.zero_()
        counts = set()
        for key, st in state_dict["state"].items():
            if key not in ids:
                raise KeyError(f"optimizer state for unknown parameter index {key}")
            p, names = params[ids.index(key)]
            loaded = {k: st[k].detach().clone() for k in names if st.get(k) is not None}
            for k, v in loaded.items():
                if tuple(v.shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state shape {tuple(v.shape)} != parameter shape {tuple(p.shape)}")
            self._pending[id(p)] = loaded
            # (torch's SGD keeps no count: a parameter that has a momentum buffer is past its first update)
            self._steps[id(p)] = int(round(float(st["step"]))) if "step" in st else 1
            counts.add(self._steps[id(p)])
        if self.capturable and counts:
            if len(counts) != 1:
                raise ValueError(f"capturable {self._NAME} keeps one update count for all parameters; the loaded state has several")
            self._resume_step = counts.pop()         # (device counters created later start here)
            for d in self._dev.values():
                d["step"].fill_(self._resume_step)


class Adam(_ArenaOptimizer):
    _NAME = "Adam"
    _NHYPER = 3          # koaf_adam_hyper: {lr, lr / (1 - b1^step), sqrt(1 - b2^step)}
    _HAS_STEP = True
    _ADAMW = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, capturable=False):
        """capturable (as in torch.optim.Adam): learning rate and step count live in device memory (koaf_adam_hyper), so that
        step() can be captured into a HIP graph and still advance on every replay (run.GraphedTrainStep); arena parameters
        only, one shared update count (every trained parameter receives a gradient every step)."""
        if lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        self._init_flat(capturable)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad)))

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if group.get("amsgrad") else ())

    def _run_key(self, n):
        return n             # the bias correction depends on the parameter's own update count

    def _hyper(self, group, d):
        b1, b2 = group["betas"]
        ops.adam_hyper(d["step"], d["lr"], b1, b2, d["hyper"])

    def _launch(self, group, p, g, st, n, key, hyper):
        b1, b2 = group["betas"]
        ops.adam_step(p, g, st["exp_avg"], st["exp_avg_sq"], n, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                      1 if hyper is not None else key, self._ADAMW, hyper=hyper, vmax=st.get("max_exp_avg_sq"))


class AdamW(Adam):
    _ADAMW = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, capturable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         capturable=capturable)


class SGD(_ArenaOptimizer):
    """torch.optim.SGD (its constructor signature and defaults, its single-tensor update rule, its state_dict layout) on
    koaf_sgd_step.  foreach / fused are accepted and ignored: the update is always one fused pass per contiguous arena run.
    capturable (as on Adam): learning rate and step count live in device memory, for run.GraphedTrainStep; arena parameters
    only, one shared update count.  Consequence: the first-update flag is the shared count's, so a parameter that receives its
    first gradient AFTER the optimizer's first step is not seeded with it -- it reads its zero buffer, buf = (1 - dampening) * g',
    which is torch's result only for dampening == 0.  Every trained parameter of the registry models receives a gradient from
    the first step on; for anything else with a dampening, use capturable=False (per-parameter flags)."""
    _NAME = "SGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, capturable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._init_flat(capturable, differentiable)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=bool(nesterov), maximize=bool(maximize), foreach=foreach,
                                      differentiable=False, fused=fused))

    def _state_names(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _run_key(self, n):
        return n == 1        # the first update differs from the later ones: the momentum buffer starts as the gradient

    def _launch(self, group, p, g, st, n, first, hyper):
        ops.sgd_step(p, g, st.get("momentum_buffer"), n, group["lr"], momentum=group["momentum"], dampening=group["dampening"],
                     wd=group["weight_decay"], nesterov=group["nesterov"], maximize=group["maximize"], first=first, hyper=hyper)


class RMSprop(_ArenaOptimizer):
    """torch.optim.RMSprop (constructor signature and defaults, single-tensor update rule, state_dict layout) on
    koaf_rmsprop_step; foreach is accepted and ignored; capturable as on Adam / SGD."""
    _NAME = "RMSprop"
    _HAS_STEP = True

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if alpha < 0.0:
            raise ValueError(f"Invalid alpha value: {alpha}")
        self._init_flat(capturable, differentiable)
        # (`capturable` stays out of the groups: torch's RMSprop, handed this state on the CPU, must not take it for its own flag)
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=bool(centered),
                                      weight_decay=weight_decay, foreach=foreach, maximize=bool(maximize), differentiable=False))

    def _state_names(self, group):
        return ("square_avg",) + (("momentum_buffer",) if group["momentum"] > 0 else ()) + (("grad_avg",) if group["centered"] else ())

    def _launch(self, group, p, g, st, n, key, hyper):
        ops.rmsprop_step(p, g, st["square_avg"], n, group["lr"], alpha=group["alpha"], eps=group["eps"], wd=group["weight_decay"],
                         momentum=group["momentum"], gavg=st.get("grad_avg"), buf=st.get("momentum_buffer"),
                         maximize=group["maximize"], hyper=hyper)


def warmup_static_decay_factor(epoch, epochs_warmup, epochs_static, warmup_factor=0.1, decay_factor=0.9):
    """lambda(epoch) of CustomWarmupStaticDecayLR (_optimizers.py:6-27): linear warm-up from warmup_factor
    to 1 over epochs_warmup, flat for epochs_static, then decay_factor ** (epochs past the flat part)."""
    flat_end = epochs_warmup + epochs_static
    if epoch <= epochs_warmup:
        return warmup_factor + (1. - warmup_factor) * epoch / float(epochs_warmup)
    if epoch <= flat_end:
        return 1.
    return decay_factor ** (epoch - flat_end)


def warmup_multistep_factor(epoch, epochs_warmup, mstep_milestones, warmup_factor=0.1, mstep_factor=0.1):
    """lambda(epoch) of CustomWarmupMultiStepLR (_optimizers.py:32-44)."""
    if epoch <= epochs_warmup:
        return warmup_factor + (1. - warmup_factor) * epoch / float(epochs_warmup)
    passed = sum(epoch >= epochs_warmup + ms for ms in mstep_milestones)
    return mstep_factor ** passed


def CustomWarmupStaticDecayLR(optimizer, epochs_warmup, epochs_static, epochs_decay, warmup_factor=0.1,
                              decay_factor=0.9, **kwargs):
    return optim.lr_scheduler.LambdaLR(
        optimizer=optimizer,
        lr_lambda=lambda e: warmup_static_decay_factor(e, epochs_warmup, epochs_static, warmup_factor, decay_factor))


def CustomWarmupMultiStepLR(optimizer, epochs_warmup, mstep_milestones, warmup_factor=0.1, mstep_factor=0.1,
                            **kwargs):
    return optim.lr_scheduler.LambdaLR(
        optimizer=optimizer,
        lr_lambda=lambda e: warmup_multistep_factor(e, epochs_warmup, mstep_milestones, warmup_factor, mstep_factor))


# same keys as _optimizers.py:47-52 / :54-67
dict_optimizers = {
    "SGD": SGD,
    "Adam": Adam,
    "AdamW": AdamW,
    "RMSprop": RMSprop,
}

dict_schedulers = {
    "LambdaLR": optim.lr_scheduler.LambdaLR,
    "MultiplicativeLR": optim.lr_scheduler.MultiplicativeLR,
    "StepLR": optim.lr_scheduler.StepLR,
    "MultiStepLR": optim.lr_scheduler.MultiStepLR,
    "ExponentialLR": optim.lr_scheduler.ExponentialLR,
    "CosineAnnealingLR": optim.lr_scheduler.CosineAnnealingLR,
    "ReduceLROnPlateau": optim.lr_scheduler.ReduceLROnPlateau,
    "CyclicLR": optim.lr_scheduler.CyclicLR,
    "OneCycleLR": optim.lr_scheduler.OneCycleLR,
    "CosineAnnealingWarmRestarts": optim.lr_scheduler.CosineAnnealingWarmRestarts,
    "CustomWarmupStaticDecayLR": CustomWarmupStaticDecayLR,
    "CustomWarmupMultiStepLR": CustomWarmupMultiStepLR,
}
