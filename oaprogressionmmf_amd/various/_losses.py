"""Loss registry `dict_losses` (reference: koafusion/various/_losses.py:13-117).

FocalLoss / CrossEntropyLoss run forward+backward in one HIP kernel (koaf_focal_loss / koaf_ce_loss), BCELoss /
BCEWithLogitsLoss (the torch classes the reference registers, _losses.py:111-117) in koaf_bce_loss.
Kept quirk: FocalLoss ignores batch_avg/class_avg/num_classes and warns about redundant kwargs.
"""
import logging

import torch
from torch import nn

from .._lib import KoafError
from ..functional import BCEFn, LossFn

logging.basicConfig()
logger = logging.getLogger("losses")
logger.setLevel(logging.DEBUG)


def _weight_on(class_weight, like):
    """class_weight (None | tensor | sequence) as a contiguous fp32 tensor on the logits' device"""
    if class_weight is None:
        return None
    return torch.as_tensor(class_weight, dtype=torch.float32).to(like.device).contiguous()


class CrossEntropyLoss(nn.Module):
    def __init__(self, num_classes, batch_avg=True, batch_weight=None, class_avg=True, class_weight=None, **kwargs):
        super().__init__()
        self.num_classes = num_classes
        self.batch_avg = batch_avg
        self.class_avg = class_avg
        self.batch_weight = batch_weight
        self.class_weight = class_weight
        logger.warning(f"Redundant loss function arguments:\n{repr(kwargs)}")

    def forward(self, input, target, **kwargs):
        """nn.CrossEntropyLoss(weight=class_weight) on (b, ch[, d0, d1, ...]) logits (_losses.py:36,49)"""
        return LossFn.apply(input, target, 0.0, True, False, _weight_on(self.class_weight, input))


class FocalLoss(nn.Module):
    def __init__(self, num_classes=2, batch_avg=True, batch_weight=None, class_avg=True, class_weight=None, gamma=2,
                 reduction="mean", **kwargs):
        super().__init__()
        self.num_classes = num_classes
        self.batch_avg = batch_avg
        self.class_avg = class_avg
        self.batch_weight = batch_weight
        self.class_weight = class_weight
        if reduction not in ("mean", "sum"):
            raise ValueError("Unknown `reduction` value")
        self.reduction = reduction
        self.gamma = gamma
        logger.warning(f"Redundant loss function arguments:\n{repr(kwargs)}")

    def forward(self, input, target, **kwargs):
        """input (b, ch[, d0, d1, ...]) logits, target (b[, d0, d1, ...]) int64 -> scalar: mean|sum over all elements of
        -(1-pt)^gamma * logpt with logpt = -F.cross_entropy(input, target, weight=class_weight, reduction='none')"""
        if input.dim() < 2:
            raise ValueError("FocalLoss: logits need a class dimension (b, ch, ...)")
        return LossFn.apply(input, target, float(self.gamma), self.reduction == "mean", True, _weight_on(self.class_weight, input))


class _BCEBase(nn.Module):
    _LOGITS = False

    def __init__(self, weight=None, reduction="mean", pos_weight=None):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"{reduction} is not a valid value for reduction")
        self.reduction = reduction
        # buffers, as in torch: the reference driver moves the loss with .to(device)
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32))
        self.register_buffer("pos_weight", None if pos_weight is None else torch.as_tensor(pos_weight, dtype=torch.float32))

    def _mismatch(self, input, target):
        raise NotImplementedError

    def forward(self, input, target):
        """input and target of any equal shape -> scalar (mean | sum) or a tensor of that shape (none)"""
        if tuple(target.shape) != tuple(input.shape):
            raise ValueError(self._mismatch(input, target))
        if not input.is_cuda:
            raise KoafError(f"koaf {type(self).__name__} needs tensors on a HIP device (no CPU fallback exists)")
        like = input.detach()
        x = input if input.dtype == torch.float32 else input.float()
        t = target.detach().to(device=like.device, dtype=torch.float32)
        w = pw = None
        if self.weight is not None:            # torch broadcasts it against the input: the kernel reads it element by element
            w = self.weight.to(like.device).expand(like.shape).contiguous()
        if self.pos_weight is not None:        # one value per class, the last dimension
            C = int(like.shape[-1]) if like.dim() else 1
            pw = self.pos_weight.to(like.device).reshape(-1)
            if pw.numel() not in (1, C):
                raise ValueError(f"pos_weight of {pw.numel()} values does not match the input's last dimension {C}")
            pw = pw.expand(C).contiguous()
        return BCEFn.apply(x, t, w, pw, self._LOGITS, self.reduction)


class BCELoss(_BCEBase):
    """nn.BCELoss on probabilities (the log terms clamped at -100 like torch's).  A probability outside [0, 1] -- a device
    assert in torch -- gives zero loss and zero gradient and shows in ops.numerics_status()["nonfinite"]."""

    def __init__(self, weight=None, reduction="mean"):
        super().__init__(weight=weight, reduction=reduction)

    def _mismatch(self, input, target):
        return (f"Using a target size ({target.size()}) that is different to the input size ({input.size()}) is deprecated. "
                "Please ensure they have the same size.")


class BCEWithLogitsLoss(_BCEBase):
    """nn.BCEWithLogitsLoss (stable log-sum-exp form); pos_weight: one value per class of the last dimension"""
    _LOGITS = True

    def __init__(self, weight=None, reduction="mean", pos_weight=None):
        super().__init__(weight=weight, reduction=reduction, pos_weight=pos_weight)

    def _mismatch(self, input, target):
        return f"Target size ({target.size()}) must be the same as input size ({input.size()})"


dict_losses = {
    "bce_loss": BCELoss,
    "bce_wlogits_loss": BCEWithLogitsLoss,
    "CrossEntropyLoss": CrossEntropyLoss,
    "FocalLoss": FocalLoss,
}
