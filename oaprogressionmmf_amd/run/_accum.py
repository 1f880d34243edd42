"""One optimizer step over several micro-batches: the way to an effective batch larger than what fits the device.

After each micro-batch's backward the gradient arena G is folded into an accumulator A of the same shape by koaf_grad_fold --
A = w_0 G, A += w_i G, and on the last micro-batch G = A + w_k G, so that the optimizer (and the clip before it) finds the
folded gradient where it always finds the gradient.  With w_i = b_i / sum(b_j) and a mean-reduced loss the result is the
gradient of the mean over ALL samples, ragged last micro-batch included.  Product and sum are rounded separately and no kernel
uses atomics: the folded gradient is the fp32 expression ((w_0 g_0 + w_1 g_1) + ...) + w_k g_k bit for bit.

BatchNorm sees micro-batches: batch statistics are per micro-batch and the running averages move k times per optimizer step,
exactly as k small steps would move them.  The reference driver has no key for any of this (one batch, one step)."""
import torch

from .. import ops
from .._lib import KoafError
from ..arena import get_arena
from ..various._clip import clip_runs
from ._steps import downscale_inputs


def micro_batch_weights(sizes):
    """[b_0, b_1, ...] samples per micro-batch -> [b_i / sum(b_j)]: the fold weights under a mean-reduced loss"""
    sizes = [int(b) for b in sizes]
    if not sizes or any(b <= 0 for b in sizes):
        raise ValueError(f"micro-batch sizes must be a non-empty list of positive counts, got {sizes}")
    total = sum(sizes)
    return [b / total for b in sizes]


class GradientFold(object):
    """fold = GradientFold(model);  per micro-batch, after backward (and the data-parallel exchange): fold.add(w_i, last=...)

    Owns the accumulator A (shaped like arena.G, allocated at the first fold: 1.56 GB on the headline model, nothing for users
    who never accumulate).  Only the runs of G that received gradients are touched.  The set of parameters with a gradient must
    not change between the micro-batches of one step (A would hold terms the last fold never reads): that raises."""

    def __init__(self, model):
        self.module = getattr(model, "module", model) if hasattr(model, "reduce_gradients") else model
        if any(not p.is_cuda for p in self.module.parameters()):
            raise KoafError("GradientFold accumulates HIP-resident gradients only (no CPU fallback exists)")
        self.A = None
        self._arena = None
        self._set = None        # ids of the parameters with a gradient at the first micro-batch of the running step
        self._runs = None

    def _begin(self):
        a = get_arena(self.module)
        if a is not self._arena:
            self._arena, self.A = a, None
        params = [p for p in a.params if p.grad is not None]
        for p in params:
            if p.grad.data_ptr() != p._koaf_grad.data_ptr():
                raise RuntimeError("GradientFold folds gradients written into the arena: call optimizer.zero_grad() (set_to_none) "
                                   "before every micro-batch's backward")
        return a, params

    @torch.no_grad()
    def add(self, w, last=False, norm_type=None):
        """fold the gradients of the micro-batch that just ran, weight w.  last: write the folded gradient back into G; with
        norm_type also take the norm partials of it in the same pass -> (runs of G, partials) for various.clip_runs"""
        a, params = self._begin()
        ids = [id(p) for p in params]
        first = self._set is None
        if first:
            self._set, self._runs = ids, a.active_ranges(params)
        elif ids != self._set:
            self._set = None
            raise RuntimeError("the set of parameters that received a gradient changed between the micro-batches of one step")
        runs = [a.G[lo:hi] for lo, hi in self._runs]
        partials = None
        if last:
            self._set = None
            if norm_type is not None:
                partials = ops.grad_norm_ws([g.numel() for g in runs], a.device)
        if first and last:                       # one micro-batch: G already is the gradient (w = 1)
            if partials is not None:
                for g, cut in zip(runs, partials[1]):
                    ops.grad_norm_part(g, cut, norm_type)
            return runs, partials
        if self.A is None:
            self.A = torch.empty_like(a.G)
        for i, ((lo, hi), g) in enumerate(zip(self._runs, runs)):
            ops.grad_fold(self.A[lo:hi], g, w, 2 if last else (0 if first else 1),
                          ws=partials[1][i] if partials is not None else None, norm_type=norm_type if partials is not None else 2.0)
        return runs, partials

    def reset(self):
        """forget a step that was abandoned between two micro-batches"""
        self._set = None


def train_step_accum(model, loss_fn, optimizer, micro_batches, downscale=None, max_grad_norm=None, fold=None):
    """zero_grad -> forward -> loss -> backward -> (all-reduce) -> fold for every (xs, ys) of `micro_batches`, then the clip
    (max_grad_norm, 2-norm) if asked, then ONE optimizer.step().  Under DataParallelRCCL every micro-batch is exchanged as a
    plain step's is (the fold is linear), and the norm is taken after the exchange: every rank clips by the same coefficient.
    fold: a GradientFold to reuse across steps (else it is kept on the model).
    Returns ([logits per micro-batch], loss averaged over all samples, gradient norm or None), all on the device; nothing
    here synchronises the host."""
    micro_batches = list(micro_batches)
    weights = micro_batch_weights([ys.shape[0] for _, ys in micro_batches])
    if fold is None:
        fold = model.__dict__.get("_koaf_grad_fold")
        if fold is None:
            fold = model.__dict__["_koaf_grad_fold"] = GradientFold(model)
    fold.reset()
    scale = getattr(model, "scale_loss", None)
    reduce = getattr(model, "reduce_gradients", None)
    logits_all, total, out = [], None, None
    for i, ((xs, ys), w) in enumerate(zip(micro_batches, weights)):
        xs = downscale_inputs(xs, downscale)
        optimizer.zero_grad()
        logits = model(*xs)["main"]
        loss = loss_fn(logits.squeeze(1), ys.long().squeeze(1))
        (scale(loss) if scale is not None else loss).backward()
        if reduce is not None:
            reduce()
        out = fold.add(w, last=i == len(micro_batches) - 1, norm_type=2.0 if max_grad_norm is not None else None)
        logits_all.append(logits.detach())
        total = loss.detach() * w if total is None else total + loss.detach() * w
    norm = clip_runs(out[0], max_grad_norm, 2.0, partials=out[1]) if max_grad_norm is not None else None
    optimizer.step()
    return logits_all, total, norm
