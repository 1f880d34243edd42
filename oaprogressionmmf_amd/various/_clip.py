"""Gradient-norm clipping over the flat gradient arena: torch.nn.utils.clip_grad_norm_'s signature and semantics on
koaf_grad_norm_part / koaf_grad_norm_final / koaf_grad_scale -- one partial-sum launch per contiguous run of arena.G that holds
gradients, one finalize over all partials, one scale per run -- instead of hundreds of per-tensor torch launches and a host
sync.  Norm and clip coefficient stay in device memory, so the whole sequence can sit inside a captured train step; an unclipped
step (coefficient exactly 1) costs the scale pass one scalar read per block and no traffic.  The reference has no key for it."""
import torch

from .. import ops
from .._lib import KoafError
from ..arena import grads_by_arena


def clip_runs(runs, max_norm, norm_type=2.0, partials=None, error_if_nonfinite=False):
    """runs: flat fp32 slices of gradient arenas.  partials: (ws, cuts) from ops.grad_norm_ws already filled by the pass that
    wrote the runs (the last fold of an accumulated step), else they are taken here.  -> the total norm, a device scalar"""
    ops.norm_kind(norm_type)
    if partials is None:
        partials = ops.grad_norm_ws([g.numel() for g in runs], runs[0].device)
        for g, cut in zip(runs, partials[1]):
            ops.grad_norm_part(g, cut, norm_type)
    norm, coef = ops.grad_norm_final(partials[0], float(max_norm), norm_type)
    if error_if_nonfinite and not bool(torch.isfinite(norm)):          # (the one place that reads the norm back)
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it "
                           "cannot be clipped. To disable this error and scale the gradients by the non-finite norm anyway, "
                           "set `error_if_nonfinite=False`")
    for g in runs:
        ops.grad_scale(g, coef)
    return norm


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for parameters that live in a model's arena (HIP device only, no CPU path); norm_type 2 or
    inf.  Returns the total norm as a device scalar tensor; nothing synchronises the host unless error_if_nonfinite.
    `foreach` is accepted and ignored: the passes always run over whole arena runs."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    ops.norm_kind(norm_type)
    for p in parameters:
        if not p.is_cuda:
            raise KoafError("clip_grad_norm_ clips HIP-resident gradients only (no CPU fallback exists)")
    by_arena = grads_by_arena(parameters)
    if not by_arena:
        return torch.zeros((), device=parameters[0].device) if parameters else torch.tensor(0.0)
    runs = [a.G[lo:hi] for a, ps in by_arena.values() for lo, hi in a.active_ranges(ps)]
    return clip_runs(runs, max_norm, norm_type, error_if_nonfinite=error_if_nonfinite)
