"""What every kernel family's wrappers share: pointers and the stream handed to libkoaf, the numerics status words of
koaf_core.hip, the live-profiler hooks, and the argument checks of the device-side evaluation families."""
import contextlib
import ctypes
import sys

import torch

from .._lib import KoafError, check, lib

_i32 = ctypes.c_int32
_pkg = sys.modules[__package__]     # the live profiler's list is installed as ops.PROFILE, on the package: read it there, per call


def _prof_begin():
    if _pkg.PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(e0, family, flops, tag="", elems=0, mpp=6):
    """elems: fp32 elements the call must move through HBM if every operand travels exactly once (its algorithmic bytes / 4);
    mpp: matrix instructions per fp32 product of the call's contraction scheme (6: bf16 x 3, 3: fp16 x 2; koaf.h KoafGemm.fmt)"""
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    _pkg.PROFILE.append((family, flops, e0, e1, tag, 4.0 * elems, mpp))


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise KoafError("koaf ops need tensors on a HIP device (no CPU fallback exists)")
    if t.dtype not in (torch.float32, torch.int64, torch.uint8, torch.float64, torch.bfloat16, torch.int32):   # float64: reduction workspaces, metric scores; bfloat16: activation storage mode; int32: metric ranks / indices
        raise KoafError(f"unexpected dtype {t.dtype}")
    return t.data_ptr()


_STATUS = None       # device int32[4]: the library's numerics status words (koaf.h koaf_set_status_buffer)
_STATUS_DEV = None   # the device they live on: the library holds ONE pointer, the one of the device this process computes on
_STATUS_BY_DEV = {}


def _a16(t):
    """the `act16` argument of the entry points (koaf.h): 1 when the call's activation tensor is stored as bf16"""
    return 1 if (t is not None and t.dtype == torch.bfloat16) else 0


def _act16(what, **acts):
    """the `act16` argument of a call whose activation tensors are `acts` (name=tensor or None): all of them fp32, or all of them
    bf16.  The entry points take every pointer as float* and read all of a call's activations at the one width act16 names, so a
    call that mixes the two storages would read (or write) a two-byte tensor four bytes per element, past its end: refused here,
    naming the call and the argument, before anything is launched"""
    first = dt = None
    for name, t in acts.items():
        if t is None:
            continue
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise KoafError(f"{what}: {name} is an fp32 or bf16 activation tensor, got {t.dtype}")
        if dt is None:
            first, dt = name, t.dtype
        elif t.dtype != dt:
            raise KoafError(f"{what}: {name} is {t.dtype} but {first} is {dt}: the activations of one call share one storage")
    return 1 if dt == torch.bfloat16 else 0


def _grads32(what, **grads):
    """gradients are never stored as bf16 (koaf.h): refuse a gradient argument (name=tensor or None) that is not fp32"""
    for name, t in grads.items():
        if t is not None and t.dtype != torch.float32:
            raise KoafError(f"{what}: {name} is an fp32 gradient tensor, got {t.dtype}")


def _stream():
    if _STATUS is None or _STATUS_DEV != torch.cuda.current_device():
        _status_buffer()
    return torch.cuda.current_stream().cuda_stream


def _status_buffer():
    """register the status words every kernel launch may bump: one buffer per device, the library pointing at the CURRENT
    device's (one process = one GPU is the product's layout; a process that moves to another device re-registers there instead
    of letting that device's kernels add into a peer's memory)"""
    global _STATUS, _STATUS_DEV
    d = torch.cuda.current_device()
    if _STATUS is None or _STATUS_DEV != d:
        if d not in _STATUS_BY_DEV:
            _STATUS_BY_DEV[d] = torch.zeros(4, dtype=torch.int32, device=torch.device("cuda", d))
        _STATUS, _STATUS_DEV = _STATUS_BY_DEV[d], d
        check(lib().koaf_set_status_buffer(_STATUS.data_ptr()), "set_status_buffer")
    return _STATUS


def numerics_status(reset=False):
    """{"saturated": ..., "nonfinite": ...} since the last reset (one small device-to-host copy: call it per epoch, not per step).
    saturated: activation elements (or GEMM tiles holding some) that left the fp16 range of the fixed activation scale
    (|x| > 4094) and were clamped, or were not finite; nonfinite: NaN / Inf that reached an operand's scale scalar (the GEMM
    then returned NaN everywhere) or a BatchNorm's coefficients."""
    st = _status_buffer()
    torch.cuda.synchronize(st.device)        # (encoder lanes / side streams add too: every stream of the device has landed)
    v = st.cpu().tolist()
    if reset:
        st.zero_()
    return {"saturated": int(v[0]) & 0xffffffff, "nonfinite": int(v[1]) & 0xffffffff}


def check_numerics(reset=True):
    """numerics_status() + a RuntimeWarning when anything was flagged; returns the status dict"""
    import warnings
    st = numerics_status(reset=reset)
    if st["saturated"]:
        warnings.warn(f"koaf: {st['saturated']} activation elements / tiles exceeded the fixed activation scale's range (|x| > 4094 behind "
                      f"a BatchNorm) and were clamped in the convolution operands: results are no longer at fp32 rounding level",
                      RuntimeWarning, stacklevel=2)
    if st["nonfinite"]:
        warnings.warn(f"koaf: non-finite values reached {st['nonfinite']} operand scales / BatchNorm coefficients (a diverged run)",
                      RuntimeWarning, stacklevel=2)
    return st


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


def conv_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------------------
# argument checks of the wrappers that take caller-made buffers (metrics, mriprep, clin)
# ------------------------------------------------------------------------------------------------
_DTYPE_NAME = {torch.int32: "int32", torch.int64: "int64", torch.float64: "fp64", torch.float32: "fp32"}


def check_tensor(what, name, t, dtype, shape=None, like=None, nonempty=False, where="the HIP device"):
    """refuse `t` unless it is a contiguous `dtype` tensor on like's device (no `like`: on a HIP device), of `shape` and non-empty
    where asked; `where` is how the refusal names that device"""
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous() or (nonempty and t.numel() == 0) \
            or (shape is not None and tuple(t.shape) != tuple(shape)) or (t.device != like.device if like is not None else not t.is_cuda):
        raise KoafError(f"{what}: {name} is a {'non-empty ' if nonempty else ''}contiguous {_DTYPE_NAME[dtype]} tensor"
                        f"{'' if shape is None else ' ' + str(list(shape))} on {where}, got "
                        f"{(tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t)}")


def out_buffer(what, out, shape, dtype, like, where, fresh=torch.empty):
    """`out` when it is the contiguous `dtype` tensor of `shape` on like's device (`where` in the refusal); None: a fresh one"""
    if out is None:
        return fresh(shape, dtype=dtype, device=like.device)
    if out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != tuple(shape) or out.device != like.device:
        raise KoafError(f"{what}: out is contiguous {_DTYPE_NAME[dtype]} {list(shape)} on {where}, got {tuple(out.shape)} {out.dtype}")
    return out


class FlagWord(object):
    """A family's device flag word, made from its text table {bit: text}: new(device) is a zeroed int32 [1] word its kernels raise
    bits of, raise_(word) the ValueError("; "-joined texts) of a word read back from the device; 0 passes.  `where` is how the
    family's refusals name the device its arguments share."""

    def __init__(self, text, where="the HIP device"):
        self.text, self.mask, self.where = text, sum(text), where

    def new(self, device):
        return torch.zeros(1, dtype=torch.int32, device=device)

    def raise_(self, word):
        word = int(word) & self.mask
        if word:
            raise ValueError("; ".join(text for bit, text in self.text.items() if word & bit))

    @contextlib.contextmanager
    def own(self, what, flag, like):
        """around a launch: the caller's word, checked -- or, for None, an own word that is read back when the block is done (the
        one host sync) and raised from"""
        mine = flag is None
        if mine:
            flag = self.new(like.device)
        check_tensor(what, "flag", flag, torch.int32, (1,), like, where=self.where)
        yield flag
        if mine:
            self.raise_(flag.item())
