"""The training step behind the backward pass: losses (koaf_loss.hip, koaf_bce.hip), optimizer steps and the gradient fold /
norm / scale helpers of accumulation and clipping (koaf_optim.hip)."""
import torch

from .._lib import KoafError, check, lib
from ._base import _empty, _ptr, _stream


def focal_loss(logits, target, gamma, mean=True, focal=True, class_weight=None):
    """logits (B, C[, d0, d1, ...]) contiguous, target (B[, d0, d1, ...]) int64, class_weight (C,) or None -> (loss, dlogits)"""
    B, C = logits.shape[0], logits.shape[1]
    S = 1
    for d in logits.shape[2:]:
        S *= int(d)
    if tuple(target.shape) != (B,) + tuple(logits.shape[2:]):
        raise KoafError(f"loss: target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
    loss = _empty((), logits)
    dl = torch.empty_like(logits)
    nws = lib().koaf_loss_ws(B, S)          # (segmentation-sized inputs: the grid form's partial sums)
    ws = _empty((nws,), logits) if nws > 0 else None
    if focal:
        check(lib().koaf_focal_loss(_ptr(logits), _ptr(target), _ptr(class_weight), _ptr(loss), _ptr(dl), B, C, S, gamma,
                                    1 if mean else 0, _ptr(ws), _stream()), "focal_loss")
    else:
        check(lib().koaf_ce_loss(_ptr(logits), _ptr(target), _ptr(class_weight), _ptr(loss), _ptr(dl), B, C, S, _ptr(ws), _stream()), "ce_loss")
    return loss, dl


_BCE_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def bce_loss(x, target, weight=None, pos_weight=None, from_logits=False, reduction="mean"):
    """x, target, weight (or None): contiguous fp32 tensors of one shape; pos_weight (C,) = x's last dimension, or None
    -> (loss, dx): loss a scalar (mean | sum) or of x's shape (none); dx = d loss / d x for an upstream gradient of 1"""
    if reduction not in _BCE_REDUCTIONS:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    for t in (x, target, weight, pos_weight):
        _ptr(t)                                  # (CPU tensors stop here)
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise KoafError("bce_loss: contiguous fp32 tensors only")
    n = x.numel()
    if n == 0:
        raise KoafError("bce_loss: empty input")
    C = int(x.shape[-1]) if x.dim() > 0 else 1
    for name, t in (("target", target), ("weight", weight)):
        if t is not None and tuple(t.shape) != tuple(x.shape):
            raise KoafError(f"bce_loss: {name} shape {tuple(t.shape)} does not match the input's {tuple(x.shape)}")
    if pos_weight is not None and (not from_logits or pos_weight.numel() != C):
        raise KoafError("bce_loss: pos_weight belongs to the logits form and has the input's last dimension")
    loss = torch.empty_like(x) if reduction == "none" else _empty((), x)
    dx = torch.empty_like(x)
    nws = lib().koaf_bce_ws(n) if reduction != "none" else 0
    ws = _empty((nws,), x) if nws > 0 else None
    check(lib().koaf_bce_loss(_ptr(x), _ptr(target), _ptr(weight), _ptr(pos_weight), _ptr(loss), _ptr(dx), n, C,
                              1 if from_logits else 0, _BCE_REDUCTIONS[reduction], _ptr(ws), _stream()), "bce_loss")
    return loss, dx


def adam_step(p, g, m, v, n, lr, b1, b2, eps, wd, step, adamw=False, hyper=None, vmax=None):
    """hyper: optional device float[3] from adam_hyper() -- lr and step then come from the device (captured steps);
    vmax: amsgrad's running maximum of the second moment (updated in place)"""
    check(lib().koaf_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, lr, b1, b2, eps, wd, step, 1 if adamw else 0,
                               _ptr(hyper), _ptr(vmax), _stream()), "adam_step")


def adam_hyper(step, lr, b1, b2, hyper):
    """++step (int32 device scalar); hyper[3] = {lr, lr / (1 - b1^step), sqrt(1 - b2^step)} from the device scalars"""
    if step.dtype != torch.int32 or not step.is_cuda:
        raise KoafError("adam_hyper: step is an int32 device scalar")
    check(lib().koaf_adam_hyper(step.data_ptr(), _ptr(lr), b1, b2, _ptr(hyper), _stream()), "adam_hyper")


def sgd_step(p, g, buf, n, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, maximize=False, first=False, hyper=None):
    """torch.optim.SGD's update over n elements in place; buf: the momentum buffer (None without a momentum), written but not
    read when `first`; hyper: optional device float[2] from optim_hyper() -- lr and first then come from the device"""
    check(lib().koaf_sgd_step(_ptr(p), _ptr(g), _ptr(buf), n, lr, momentum, dampening, wd, 1 if nesterov else 0,
                              1 if maximize else 0, 1 if first else 0, _ptr(hyper), _stream()), "sgd_step")


def rmsprop_step(p, g, sq, n, lr, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0, gavg=None, buf=None, maximize=False, hyper=None):
    """torch.optim.RMSprop's update over n elements in place; gavg: the gradient average of the centered form (None: plain),
    buf: the momentum buffer (None exactly when momentum == 0); hyper: optional device float[2] from optim_hyper()"""
    check(lib().koaf_rmsprop_step(_ptr(p), _ptr(g), _ptr(sq), _ptr(gavg), _ptr(buf), n, lr, alpha, eps, wd, momentum,
                                  1 if maximize else 0, _ptr(hyper), _stream()), "rmsprop_step")


def optim_hyper(step, lr, hyper):
    """++step (int32 device scalar); hyper[2] = {lr, step == 1} from the device scalars (captured SGD / RMSprop steps)"""
    if step.dtype != torch.int32 or not step.is_cuda:
        raise KoafError("optim_hyper: step is an int32 device scalar")
    check(lib().koaf_optim_hyper(step.data_ptr(), _ptr(lr), _ptr(hyper), _stream()), "optim_hyper")


def norm_kind(norm_type):
    """torch's norm_type -> the library's norm kind: 0 for the 2-norm, 1 for the inf-norm; anything else is a ValueError"""
    nt = float(norm_type)
    if nt == 2.0:
        return 0
    if nt == float("inf"):
        return 1
    raise ValueError(f"norm_type {norm_type!r}: the gradient norm kernels know 2 and inf")


def _flat32(name, *ts):
    for t in ts:
        _ptr(t)                                  # (CPU tensors stop here)
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous()):
            raise KoafError(f"{name}: flat contiguous fp32 tensors only")


def grad_norm_ws(sizes, device):
    """-> (ws, [one slice of it per range]): the float64 workspace of the norm partials of ranges of `sizes` elements, laid end
    to end for one grad_norm_final (one 8-byte slot per block: koaf_grad_norm_ws)"""
    L = lib()
    slots = [L.koaf_grad_norm_ws(int(n)) // 2 for n in sizes]
    ws = torch.empty(sum(slots), device=device, dtype=torch.float64)
    cuts, o = [], 0
    for s in slots:
        cuts.append(ws[o:o + s])
        o += s
    return ws, cuts


def grad_fold(acc, g, w, mode, ws=None, norm_type=2.0):
    """mode 0: acc = w * g;  1: acc += w * g;  2: g = acc + w * g, and with `ws` (its slice from grad_norm_ws) the norm partials of the new g.
    Flat fp32 device tensors of one length; product and sum are rounded separately."""
    _flat32("grad_fold", acc, g)
    if acc.numel() != g.numel():
        raise KoafError(f"grad_fold: {acc.numel()} and {g.numel()} elements")
    check(lib().koaf_grad_fold(_ptr(acc), _ptr(g), g.numel(), w, mode, norm_kind(norm_type) if ws is not None else 0, _ptr(ws),
                               _stream()), "grad_fold")


def grad_norm_part(g, ws, norm_type=2.0):
    """block partials of the norm of the flat fp32 device tensor g -> ws (its slice from grad_norm_ws)"""
    _flat32("grad_norm_part", g)
    check(lib().koaf_grad_norm_part(_ptr(g), g.numel(), norm_kind(norm_type), _ptr(ws), _stream()), "grad_norm_part")


def grad_norm_final(ws, max_norm, norm_type=2.0):
    """every partial of ws (one or several ranges, end to end) -> (norm, coef) device scalars, coef = min(1, max_norm / (norm + 1e-6))"""
    out = torch.empty(2, device=ws.device, dtype=torch.float32)
    check(lib().koaf_grad_norm_final(_ptr(ws), 2 * ws.numel(), norm_kind(norm_type), max_norm, _ptr(out[0:1]), _ptr(out[1:2]),
                                     _stream()), "grad_norm_final")
    return out[0], out[1]


def grad_scale(g, coef):
    """g *= coef (a device scalar) in place; no memory traffic when coef is exactly 1"""
    _flat32("grad_scale", g)
    check(lib().koaf_grad_scale(_ptr(g), g.numel(), _ptr(coef), _stream()), "grad_scale")
