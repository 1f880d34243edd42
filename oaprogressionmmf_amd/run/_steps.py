"""One train iteration / one inference batch / one validation pass (reference: koafusion/run/train_prog_fus.py:100-236,
koafusion/run/eval_prog_fus.py:262-303)."""
import numpy as np
import torch

from .. import ops, preproc
from .._lib import KoafError
from ..various._clip import clip_grad_norm_


def downscale_inputs(xs, factors):
    """"Last-chance preprocessing" of both drivers (train_prog_fus.py:111-123, eval_prog_fus.py:245-276):
    factors is config.model.downscale -- falsy, or one scale tuple (or falsy) per modality."""
    if not factors:
        return tuple(xs)
    out = []
    for x, f in zip(xs, factors):
        if f:
            x = preproc.PTInterpolate(scale_factor=tuple(f))(x).contiguous()
        out.append(x)
    return tuple(out)


def train_step(model, loss_fn, optimizer, xs, ys, downscale=None, *, max_grad_norm=None):
    """zero_grad -> forward -> loss -> backward -> (all-reduce) -> Adam, the optimize branch of
    train_prog_fus.py:132-168.  `model` may be a registry model or a DataParallelRCCL wrapper.
    Returns (logits, loss), both on the device; nothing here synchronises the host.
    max_grad_norm (an extension, the reference has no key for it): clip the optimizer's gradients to this total 2-norm between
    the exchange and the update (various.clip_grad_norm_: every rank clips by the same coefficient); the norm, a device
    scalar, is then returned as a third value.  None: not one launch more than without the argument."""
    xs = downscale_inputs(xs, downscale)
    optimizer.zero_grad()
    logits = model(*xs)["main"]
    loss = loss_fn(logits.squeeze(1), ys.long().squeeze(1))
    scale = getattr(model, "scale_loss", None)
    (scale(loss) if scale is not None else loss).backward()
    reduce = getattr(model, "reduce_gradients", None)
    if reduce is not None:
        reduce()
    if max_grad_norm is not None:
        norm = clip_grad_norm_([p for group in optimizer.param_groups for p in group["params"]], max_grad_norm)
        optimizer.step()
        return logits.detach(), loss.detach(), norm
    optimizer.step()
    return logits.detach(), loss.detach()


def train_epoch(model, loss_fn, optimizer, batches, downscale=None):
    """the optimize branch of `ProgressionPrediction.train_epoch` (train_prog_fus.py:132-168) over an iterable of (xs, ys) device
    batches: one train_step each, the losses read back once at the end (no per-step host sync), and ONE look at the numerics
    status words per epoch (ops.check_numerics: clamped activations / non-finite operand scales raise a RuntimeWarning).
    Returns the list of per-step losses (python floats)."""
    losses = []
    for xs, ys in batches:
        losses.append(train_step(model, loss_fn, optimizer, xs, ys, downscale)[1])
    out = [float(v) for v in torch.stack(losses).cpu()] if losses else []
    if losses:
        ops.check_numerics()
    return out


def softmax_rows_(x):
    """in-place row softmax of a contiguous fp32 (rows, n) device tensor (koaf_softmax_rows)"""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.ndim == 2):
        raise KoafError("softmax_rows_: contiguous fp32 (rows, n) device tensor required")
    if x.shape[0]:
        ops.softmax_rows_(x)
    return x


def predict_batch(model, xs, downscale=None):
    """Inference on one batch (eval_prog_fus.py:262-303).  Returns (logits, proba) device tensors of shape
    (B, classes); the model must already be in eval() mode, autograd is off inside."""
    with torch.no_grad():
        xs = downscale_inputs(xs, downscale)
        logits = model(*xs)["main"]
        logits = logits.contiguous()      # (B, head*cls), "b head cls -> b (head cls)" in every model
        proba = softmax_rows_(logits.clone())
    return logits, proba


def val_epoch(model, loss_fn, batches, downscale=None, *, target, kws_metrics=None, calibration=None):
    """`ProgressionPrediction.val_epoch` (train_prog_fus.py:172-236) over an iterable of (xs, ys) device batches; the model must
    already be in eval() mode.  Per batch one forward (predict_batch) and the loss of its logits, all under no_grad; the
    probabilities and targets stay on the device and go to various.calc_metrics_v2 as device tensors, the losses are read back
    once at the end and the numerics status words are looked at once per pass: no per-batch host sync.
    target: config.data.target (calc_metrics_v2 refuses names it does not know); kws_metrics: further keyword arguments of
    calc_metrics_v2 (bootstrap, kws_ppv, kws_bs).  calibration: None, or a dict of keyword arguments of various.calc_calibration
    (n_bins, strategy, thresholds, bootstrap, kws_bs; {} for its defaults) -- epoch-w then gains a "calibration" entry, the
    calibration table of the same device tensors.
    Returns the reference's dict: {"batch-w": {"loss_prog": [np.round(loss, 3), ...]}, "epoch-w": calc_metrics_v2(...)} --
    fit() reads its checkpoint criterion from it (the mean of loss_prog, or epoch-w's b_accuracy / avg_precision)."""
    from ..various._metrics import calc_metrics_v2
    losses, probas, targets = [], [], []
    with torch.no_grad():
        for xs, ys in batches:
            logits, proba = predict_batch(model, xs, downscale)
            losses.append(loss_fn(logits.squeeze(1), ys.long().squeeze(1)))
            probas.append(proba)
            targets.append(ys.reshape(-1))
        if not losses:
            raise ValueError("val_epoch: no batches")
        loss_host = torch.stack(losses).cpu()
        prog_target, prog_pred_proba = torch.cat(targets), torch.cat(probas, dim=0)
        epoch_w = calc_metrics_v2(prog_target=prog_target, prog_pred_proba=prog_pred_proba, target=target, **(kws_metrics or {}))
        if calibration is not None:
            from ..various._calibration import calc_calibration
            epoch_w["calibration"] = calc_calibration(prog_target=prog_target, prog_pred_proba=prog_pred_proba, target=target,
                                                      **dict(calibration))
    ops.check_numerics()
    return {"batch-w": {"loss_prog": [np.round(float(v), 3) for v in loss_host]}, "epoch-w": epoch_w}
