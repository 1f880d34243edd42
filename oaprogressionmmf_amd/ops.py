"""Tensor-level wrappers over the libkoaf C ABI.

Every function takes/returns `torch.Tensor`s that live on a HIP device (torch is used for device
memory and streams only) and launches hand-written gfx950 kernels on torch's current stream.
Activations are NHWC fp32.  Nothing here falls back to torch math: a CPU tensor or a missing
library raises.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from ._lib import KoafBnApply, KoafBnb, KoafEmit, KoafGemm, KoafError, KoafLaunchRec, KoafTail, KoafWImg, KoafWPlane, check, defines, lib

_i32 = ctypes.c_int32

# Convolutions run on the fp16 contraction scheme (koaf.h: KoafGemm.fmt 1) whenever their operands' scales are known
# (weights: arena plane images; gradients: the amax the BatchNorm backward leaves behind).  KOAF_CONV_FMT=bf16 keeps them
# on the bf16 x 3 scheme for A/B runs.
import os
CONV_F16 = os.environ.get("KOAF_CONV_FMT", "f16") != "bf16"
# The gathered (3x3) convolution kernels read activation plane images (koaf_act_planes) wherever use_aplanes says they pay; the
# aplanes= arguments below override that per call (False: the fp32 loaders).  A convolution's forward images are kept for its
# weight gradient only where the caller asks (keep_planes=): keeping them everywhere fragments the caching allocator's pool.
ACT_SCALE = defines()["KOAF_ACT_SCALE"]      # the fixed activation scale of the fp16 scheme (koaf.h)

# Optional live profiler (bench.py): when a list is installed here every MFMA-GEMM based call is bracketed
# by two events recorded on the stream the kernel is launched on (torch's current stream) and logged as
# (family, algorithmic_flops, start_event, end_event).
PROFILE = None


def _prof_begin():
    if PROFILE is None:
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
    PROFILE.append((family, flops, e0, e1, tag, 4.0 * elems, mpp))


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


def _a16(t):
    """the `act16` argument of the entry points (koaf.h): 1 when the call's activation tensor is stored as bf16"""
    return 1 if (t is not None and t.dtype == torch.bfloat16) else 0


def _stream():
    if _STATUS is None or _STATUS_DEV != torch.cuda.current_device():
        _status_buffer()
    return torch.cuda.current_stream().cuda_stream


_STATUS_BY_DEV = {}


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


def _img(wimg):
    """ctypes view of a weight's plane images: wimg = (F, D, amax) device tensors (F / D may be None) or None"""
    if wimg is None:
        return None
    f, d, amax = wimg
    for t in (f, d):
        if t is not None and (not t.is_cuda or t.dtype != torch.int16):
            raise KoafError("weight plane images are int16 (fp16 bit patterns) tensors on the HIP device")
    return ctypes.byref(KoafWImg(f=f.data_ptr() if f is not None else None, d=d.data_ptr() if d is not None else None,
                                 amax=_ptr(amax)))


class BnApply(object):
    """A gradient w.r.t. a conv output that exists only as its BatchNorm-backward recipe: dc = coef0*dz + coef3 - coef2*c
    (coef [4][C] and the scale bound `amax` from koaf_bn_bwd_finalize).  conv2d_dgrad / conv2d_wgrad take it in place of the
    dy tensor and form dc in their loaders (koaf.h KoafOperand.tf 2), so dc never travels through HBM; materialize()
    writes it out for consumers that are not such GEMMs."""
    __slots__ = ("dz", "c", "coef", "amax", "mean", "rows", "C", "_koaf_planes")

    def __init__(self, dz, c, coef, amax, mean, rows, C):
        self.dz, self.c, self.coef, self.amax, self.mean, self.rows, self.C = dz, c, coef, amax, mean, rows, C
        self._koaf_planes = None        # activation plane images of dc, cut by the first convolution that wants them

    def struct(self):
        return ctypes.byref(KoafBnApply(dz=_ptr(self.dz), c=_ptr(self.c), coef=_ptr(self.coef), amax=_ptr(self.amax)))

    def tensors(self):
        """everything a kernel launched with this recipe reads (to be kept alive / recorded for a second stream)"""
        return (self.dz, self.c, self.coef, self.amax, self._koaf_planes, getattr(self.c, "_koaf_xplanes", None))

    def materialize(self, out=None, want_amax=False):
        dc = out if out is not None else torch.empty(self.c.shape, device=self.c.device, dtype=torch.float32)
        amax = torch.zeros(1, device=self.c.device, dtype=torch.float32) if want_amax else None
        check(lib().koaf_bn_bwd_apply(_ptr(self.dz), _ptr(self.c), _ptr(self.mean), _ptr(self.coef), _ptr(dc), self.rows, self.C,
                                      _ptr(amax), _a16(self.c), _stream()), "bn_bwd_apply")
        if want_amax:
            dc._koaf_amax = amax
        return dc


def _dy_args(dy, dy_amax):
    """(dy pointer, dy_amax pointer, KoafBnApply* or None, reference tensor) of a gradient given as a tensor or as a BnApply"""
    if isinstance(dy, BnApply):
        return None, None, dy.struct(), dy.dz
    return _ptr(dy), _ptr(dy_amax), None, dy


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


def conv_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------
def act_planes(x, npix, C, tf=0, sc=None, sh=None, x2=None, sc2=None, amax=None, fscale=0.0):
    """fp16 piece planes [2][npix][C] (+ the zero chunk) of x (tf 0), relu(sc*x+sh) (tf 1) or sc*x + sh - sc2*x2 (tf 2), times
    the operand scale (scale(*amax) or fscale): the A operand of the gathered convolution kernels (koaf.h koaf_act_planes)."""
    L = lib()
    out = torch.empty(L.koaf_act_planes_elems(npix, C), device=x.device, dtype=torch.int16)
    check(L.koaf_act_planes(_ptr(x), _ptr(x2), npix, C, tf, _ptr(sc), _ptr(sh), _ptr(sc2), _ptr(amax), float(fscale),
                            out.data_ptr(), _a16(x2 if tf == 2 else x), _stream()), "act_planes")
    return out


def set_conv3x3_halo(mode):
    """how 3x3 / stride-1 convolutions over plane images run: 0 / False per-tap gather kernel, 1 / True halo kernel with the
    shape picked per layer (default), 2 / 3 the 256- / 128-row halo shape; returns the previous mode (koaf.h
    koaf_set_conv3x3_halo)"""
    return lib().koaf_set_conv3x3_halo(int(mode))


def set_stream(on):
    """the streamed kernel for dense 1x1 / stride-1 convolutions and their data gradients (koaf.h koaf_set_stream): True (default) /
    False = the block-wide loader; returns the previous setting"""
    return bool(lib().koaf_set_stream(1 if on else 0))


def launch_log(on):
    """the host-side record of koaf_gemm launches (koaf.h koaf_launch_log; tests): clears it and switches it on / off; returns the
    previous setting"""
    return bool(lib().koaf_launch_log(1 if on else 0))


def launch_log_read():
    """the launches recorded since launch_log(True): one dict per koaf_gemm launch, in launch order -- variant ("koaf_gemm",
    "koaf_gemm/stream", "/emit", "/halo", "/halo128", "/t2d"; "koaf_wgrad3/ring": the 3x3 weight-gradient ring kernel, splitk = its
    k-ranges), bm, bn, tiles, grid_x (< tiles: persistent blocks walk), splitk, nbatch, fmt, a_tf, b_tf, act16, M, N, K, emit"""
    L = lib()
    n = min(L.koaf_launch_log_read(None, 0), 4096)        # (launches seen; the record keeps the first 4096)
    buf = (KoafLaunchRec * max(n, 1))()
    L.koaf_launch_log_read(buf, n)
    return [{f: (getattr(r, f).decode() if f == "variant" else getattr(r, f)) for f, _ in KoafLaunchRec._fields_} for r in buf[:n]]


def use_aplanes(wimg, KH, KW, C):
    """activation plane images pay where a kernel gathers (every element is otherwise converted KH*KW times)"""
    return wimg is not None and KH * KW > 1 and C % 32 == 0


def conv2d_fwd(x, w, N, H, W, Cin, Cout, KH, KW, stride, pad, in_sc=None, in_sh=None, stats=False, shift=None, wimg=None,
               aplanes=None, tail_idt=None, tail_out=None, tail_idsaved=None, keep_planes=False, emit=None):
    """x [N,H,W,Cin] (any view with that memory), w packed [Cout,KH,KW,Cin] -> y [N,OH,OW,Cout],
    (part, rows) per-tile column statistics if stats, summed about `shift` [Cout] (hand the same tensor to bn_finalize).
    wimg = (F, D, amax) plane images of w (arena.weight_planes) or None: with them the contraction runs on the fp16
    scheme (KoafGemm.fmt 1: half the matrix instructions, same accuracy), the weight tiles DMA'd from F.
    tail_idt (1x1 / stride 1 with wimg): x is the PREVIOUS block's raw last conv output c3, in_sc / in_sh its BatchNorm
    coefficients and tail_idt that block's identity: the input y = relu(in_sc*x + in_sh + tail_idt) (the bottleneck tail) is
    formed on load and written to tail_out (allocated here when None); returns (y, part, tail_out).  tail_idsaved: the block had a
    downsample branch -- tail_idt is that branch's raw conv output and tail_idsaved its BatchNorm record (mean, invstd, sc, sh).
    keep_planes: the activation plane images cut for this call stay attached to the output for its weight gradient.
    emit = (sc, sh): the coefficients of the BatchNorm BEHIND this convolution are already known (eval mode, a stage rebuilt in
    backward): the epilogue also cuts the plane images of relu(sc*y + sh) -- bit for bit what the following 3x3 convolution's
    act_planes pre-pass would cut after reading y back -- and leaves them on the output (y._koaf_eplanes), where that convolution
    finds them."""
    L = lib()
    OH, OW = conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad)
    if tail_idt is not None and tail_out is None:
        tail_out = torch.empty_like(x)     # (before the output, like the element-wise tail pass it replaces: same allocation order,
        #                                     same caching-allocator block reuse -- the other order cost 17 GB of reserved memory)
    y = _empty((N, OH, OW, Cout), x, dtype=x.dtype)            # (bf16 activation storage: the output follows the input)
    part, rows = None, _i32(0)
    if stats:
        nrows = L.koaf_conv2d_stats_rows(N * OH * OW, Cout)
        part = _empty((nrows, 2, Cout), x)
    e0 = _prof_begin()
    if aplanes is None:
        aplanes = use_aplanes(wimg, KH, KW, Cin) and wimg[0] is not None and stride == 1     # (stride 2: the pre-pass
        #                                           would cut four times the pixels the kernel reads)
    xpl = None
    tail = None
    if tail_idt is not None:
        tail = ctypes.byref(KoafTail(idt=_ptr(tail_idt), y_out=_ptr(tail_out),
                                     idt_sc=_ptr(tail_idsaved[2]) if tail_idsaved is not None else None,
                                     idt_sh=_ptr(tail_idsaved[3]) if tail_idsaved is not None else None))
        aplanes = False
    if torch.is_tensor(aplanes):
        xpl = aplanes                   # images cut by the caller (act_planes with this call's transform and ACT_SCALE)
    elif aplanes:
        ep = getattr(x, "_koaf_eplanes", None)
        if ep is not None:              # (consumed once: the images live on with the convolution that takes them)
            del x._koaf_eplanes
        if (ep is not None and in_sc is not None and ep[1].data_ptr() == in_sc.data_ptr() and ep[2].data_ptr() == in_sh.data_ptr()
                and ep[0].numel() == L.koaf_act_planes_elems(N * H * W, Cin)):      # (the same coefficient memory: rows of one BatchNorm record)
            xpl = ep[0]                 # cut by the producing convolution's epilogue (emit): no pre-pass over x
        else:
            xpl = act_planes(x, N * H * W, Cin, 1 if in_sc is not None else 0, in_sc, in_sh, fscale=ACT_SCALE)
    epl, em = None, None
    if emit is not None:
        epl = torch.empty(L.koaf_act_planes_elems(N * OH * OW, Cout), device=x.device, dtype=torch.int16)
        em = ctypes.byref(KoafEmit(planes=epl.data_ptr(), sc=_ptr(emit[0]), sh=_ptr(emit[1])))
    check(L.koaf_conv2d_fwd(_ptr(x), _ptr(w), _ptr(y), N, H, W, Cin, Cout, KH, KW, stride, pad, _ptr(in_sc),
                            _ptr(in_sh), _ptr(part), ctypes.addressof(rows), _ptr(shift) if stats else None,
                            _img(wimg), xpl.data_ptr() if xpl is not None else None, tail, em, _a16(x), _stream()), "conv2d_fwd")
    if epl is not None:
        y._koaf_eplanes = (epl, emit[0], emit[1])
    if xpl is not None and not torch.is_tensor(aplanes) and keep_planes:
        y._koaf_xplanes = xpl       # ride on the output: this conv's weight gradient reads them instead of cutting them again
    _prof_end(e0, "gemm", 2.0 * N * OH * OW * Cout * KH * KW * Cin,
              f"conv_fwd k{KH}s{stride} {Cin}->{Cout} px{N*OH*OW}" + (" +tail" if tail is not None else ""),
              N * H * W * Cin * (3 if tail is not None else 1) + Cout * KH * KW * Cin + N * OH * OW * Cout * (2 if epl is not None else 1),
              mpp=3 if wimg is not None else 6)
    if stats:
        part = part[:rows.value]
    if tail is not None:
        return y, part, tail_out
    return y, part


def conv2d_dgrad(dy, w, N, H, W, Cin, Cout, KH, KW, stride, pad, residual=None, bnb=None, wimg=None, dy_amax=None,
                 aplanes=None):
    """dx = conv_transpose(dy, w) (+residual).  bnb = dict(mode, c, saved[, y][, c2, saved2]): fuse the
    BatchNorm(+ReLU)-backward reduction of the layer that produced x into the epilogue; then returns
    (dz, part [rows][nsum][Cin]) instead of dx (+ the device scalar max |dz| as a third element when bnb has "dz_amax": True).
    wimg + dy_amax (device scalar max |dy|): fp16 scheme.  dy may be a BnApply (needs wimg with its D image).
    aplanes (None = where it pays: gathered kernels with a D image; stride 2 too -- dy is the SMALL tensor there and its four
    parity-class GEMMs gather from the same images): dy is cut ONCE into activation plane images (the BatchNorm-backward
    apply included) and the kernel's input tiles are DMA'd from them."""
    L = lib()
    dyp, amp, app, like = _dy_args(dy, dy_amax)
    a16 = _a16(dy.c) if isinstance(dy, BnApply) else (_a16(bnb["c"]) if bnb is not None else 0)
    dx = _empty((N, H, W, Cin), like)
    if aplanes is None:
        aplanes = (use_aplanes(wimg, KH, KW, Cout) and wimg[1] is not None and stride in (1, 2) and
                   (app is not None or dy_amax is not None))
    e0 = _prof_begin()
    dypl = None
    if aplanes:
        dypl = _dy_planes(dy, dy_amax, N * conv_out(H, KH, stride, pad) * conv_out(W, KW, stride, pad), Cout)
    dypp = dypl.data_ptr() if dypl is not None else None
    fl = 2.0 * N * conv_out(H, KH, stride, pad) * conv_out(W, KW, stride, pad) * Cout * KH * KW * Cin
    tag = f"conv_dgrad k{KH}s{stride} {Cin}->{Cout} px{N*H*W}"
    el = N * conv_out(H, KH, stride, pad) * conv_out(W, KW, stride, pad) * Cout + Cout * KH * KW * Cin + N * H * W * Cin
    el += N * H * W * Cin if residual is not None else 0
    mpp = 3 if (wimg is not None and (dy_amax is not None or app is not None)) else 6
    if app is not None:
        el += N * conv_out(H, KH, stride, pad) * conv_out(W, KW, stride, pad) * Cout      # (dz and c are both read)
        tag += " apply"
    if bnb is None:
        check(L.koaf_conv2d_dgrad(dyp, _ptr(w), _ptr(dx), N, H, W, Cin, Cout, KH, KW, stride, pad,
                                  _ptr(residual), _img(wimg), amp, app, dypp, a16, _stream()), "conv2d_dgrad")
        _prof_end(e0, "gemm", fl, tag, el, mpp=mpp)
        return dx
    sv, sv2 = bnb["saved"], bnb.get("saved2")
    dzmax = _empty((1,), like) if bnb.get("dz_amax") else None
    kb = KoafBnb(mode=bnb["mode"], dz_amax=_ptr(dzmax), c=_ptr(bnb["c"]), y=_ptr(bnb.get("y")), sc=_ptr(sv[2]), sh=_ptr(sv[3]),
                 mean=_ptr(sv[0]), invstd=_ptr(sv[1]), c2=_ptr(bnb.get("c2")),
                 mean2=_ptr(sv2[0]) if sv2 is not None else None, invstd2=_ptr(sv2[1]) if sv2 is not None else None)
    nsum = 3 if bnb.get("c2") is not None else 2
    part = _empty((L.koaf_conv2d_dgrad_bnb_rows(N, H, W, Cin, stride), nsum, Cin), like)
    rows = _i32(0)
    check(L.koaf_conv2d_dgrad_bnb(dyp, _ptr(w), _ptr(dx), N, H, W, Cin, Cout, KH, KW, stride, pad,
                                  _ptr(residual), ctypes.byref(kb), _ptr(part), ctypes.addressof(rows), _img(wimg),
                                  amp, app, dypp, a16, _stream()), "conv2d_dgrad_bnb")
    el += N * H * W * Cin * (1 + (bnb.get("y") is not None) + (bnb.get("c2") is not None))
    _prof_end(e0, "gemm", fl, tag + " +bnb", el, mpp=mpp)
    if dzmax is not None:
        return dx, part[:rows.value], dzmax
    return dx, part[:rows.value]


def _dy_planes(dy, dy_amax, npo, Cout):
    """activation plane images of a gradient: a tensor at scale(*dy_amax), or a BnApply with its apply folded in -- cached on
    the BnApply (an immutable recipe), so the data gradient and the weight gradient of one convolution cut them once"""
    if isinstance(dy, BnApply):
        if dy._koaf_planes is None:
            dy._koaf_planes = act_planes(dy.dz, npo, Cout, 2, dy.coef[0], dy.coef[3], x2=dy.c, sc2=dy.coef[2], amax=dy.amax)
        return dy._koaf_planes
    return act_planes(dy, npo, Cout, 0, amax=dy_amax)


def _slab_ws(slabs, ws, like, what):
    """the split-K slab workspace of `ws` floats: the caller's (fp32, on the device, at least that large) or a fresh one"""
    if slabs is None:
        return _empty((ws,), like) if ws > 0 else None
    if not slabs.is_cuda or slabs.dtype != torch.float32 or not slabs.is_contiguous() or slabs.numel() < ws:
        raise KoafError(f"{what}: the slab workspace is a contiguous fp32 device tensor of at least {ws} elements")
    return slabs


def conv2d_wgrad(dy, x, dw, N, H, W, Cin, Cout, KH, KW, stride, pad, in_sc=None, in_sh=None, dy_amax=None, aplanes=None,
                 slabs=None):
    """writes dw (packed [Cout,KH,KW,Cin] memory); dy_amax (device scalar max |dy|): fp16 scheme; dy may be a BnApply.
    aplanes (None = gathered stride-1 kernels on the fp16 scheme): both operands from activation plane images (dy's are
    shared with conv2d_dgrad), moved K-major by LDS-DMA.
    slabs (None = allocated here): the split-K workspace, at least koaf_conv2d_wgrad_ws floats."""
    L = lib()
    dyp, amp, app, like = _dy_args(dy, dy_amax)
    slabs = _slab_ws(slabs, L.koaf_conv2d_wgrad_ws(N, H, W, Cin, Cout, KH, KW, stride, pad), like, "conv2d_wgrad")
    if aplanes is None:
        aplanes = (KH * KW > 1 and stride == 1 and Cin % 8 == 0 and Cout % 8 == 0 and
                   (app is not None or dy_amax is not None))
    e0 = _prof_begin()
    dypl = xpl = None
    if aplanes:
        npo = N * conv_out(H, KH, stride, pad) * conv_out(W, KW, stride, pad)
        dypl = _dy_planes(dy, dy_amax, npo, Cout)
        # x's images: the ones the forward convolution cut (they ride on its output = the BatchNorm input dy.c), else cut here
        xpl = getattr(dy.c, "_koaf_xplanes", None) if app is not None else None
        if xpl is None or xpl.numel() != L.koaf_act_planes_elems(N * H * W, Cin):
            xpl = act_planes(x, N * H * W, Cin, 1 if in_sc is not None else 0, in_sc, in_sh, fscale=ACT_SCALE)
    check(L.koaf_conv2d_wgrad(dyp, _ptr(x), _ptr(dw), N, H, W, Cin, Cout, KH, KW, stride, pad, _ptr(in_sc),
                              _ptr(in_sh), _ptr(slabs), amp, app, dypl.data_ptr() if dypl is not None else None,
                              xpl.data_ptr() if xpl is not None else None, _a16(x), _stream()), "conv2d_wgrad")
    npx = N * conv_out(H, KH, stride, pad) * conv_out(W, KW, stride, pad)
    _prof_end(e0, "gemm", 2.0 * npx * Cout * KH * KW * Cin,
              f"conv_wgrad k{KH}s{stride} {Cin}->{Cout} px{N*H*W}" + (" apply" if app is not None else ""),
              npx * Cout * (2 if app is not None else 1) + N * H * W * Cin + Cout * KH * KW * Cin,
              mpp=3 if (dy_amax is not None or app is not None) else 6)
    return dw


def gconv_expand_w(w, C, groups):
    """block-diagonal 64-channel slabs of a grouped 3x3 weight; with the convolutions on the fp16 scheme max |w| rides on the result
    (wexp._koaf_amax: the grouped calls then run three MFMAs per product instead of six, koaf.h)"""
    wexp = _empty((C // 64, 64, 9, 64), w)
    amax = torch.zeros(1, device=w.device, dtype=torch.float32) if CONV_F16 else None
    check(lib().koaf_gconv_expand_w(_ptr(w), _ptr(wexp), C, groups, _ptr(amax), _stream()), "gconv_expand_w")
    if amax is not None:
        wexp._koaf_amax = amax
    return wexp


def gconv_compress_dw(dwexp, dw, C, groups):
    check(lib().koaf_gconv_compress_dw(_ptr(dwexp), _ptr(dw), C, groups, _stream()), "gconv_compress_dw")
    return dw


def gconv3x3_fwd(x, wexp, N, H, W, C, stride, in_sc=None, in_sh=None, stats=False, shift=None):
    L = lib()
    OH, OW = conv_out(H, 3, stride, 1), conv_out(W, 3, stride, 1)
    y = _empty((N, OH, OW, C), x, dtype=x.dtype)
    part, rows = None, _i32(0)
    if stats:
        part = _empty(((N * OH * OW + 127) // 128, 2, C), x)
    e0 = _prof_begin()
    wam = getattr(wexp, "_koaf_amax", None)
    check(L.koaf_gconv3x3_fwd(_ptr(x), _ptr(wexp), _ptr(y), N, H, W, C, stride, _ptr(in_sc), _ptr(in_sh), _ptr(part),
                              ctypes.addressof(rows), _ptr(shift) if stats else None, _ptr(wam), _a16(x), _stream()), "gconv3x3_fwd")
    _prof_end(e0, "gemm", 2.0 * N * OH * OW * C * 9 * (C // 32), f"gconv_fwd s{stride} C{C} px{N*OH*OW}",   # algorithmic (32 groups)
              N * H * W * C + N * OH * OW * C + 9 * C * (C // 32), mpp=3 if (wam is not None and not _a16(x)) else 6)
    return y, part


def gconv3x3_dgrad(dy, wexp, N, H, W, C, stride):
    """dy with dy._koaf_amax (max |dy|, left by BnApply.materialize(want_amax=True)) and wexp with its max |w|: fp16 scheme"""
    dx = _empty((N, H, W, C), dy)
    e0 = _prof_begin()
    wam, dam = getattr(wexp, "_koaf_amax", None), getattr(dy, "_koaf_amax", None)
    if wam is None or dam is None:
        wam = dam = None
    check(lib().koaf_gconv3x3_dgrad(_ptr(dy), _ptr(wexp), _ptr(dx), N, H, W, C, stride, _ptr(wam), _ptr(dam), _stream()), "gconv3x3_dgrad")
    _prof_end(e0, "gemm", 2.0 * N * conv_out(H, 3, stride, 1) * conv_out(W, 3, stride, 1) * C * 9 * (C // 32),
              f"gconv_dgrad s{stride} C{C} px{N*H*W}",
              N * H * W * C + N * conv_out(H, 3, stride, 1) * conv_out(W, 3, stride, 1) * C + 9 * C * (C // 32), mpp=3 if wam is not None else 6)
    return dx


def gconv3x3_wgrad(dy, x, N, H, W, C, stride, in_sc=None, in_sh=None, slabs=None):
    """slabs (None = allocated here): the split-K workspace, at least koaf_gconv3x3_wgrad_ws floats"""
    L = lib()
    slabs = _slab_ws(slabs, L.koaf_gconv3x3_wgrad_ws(N, H, W, C, stride), dy, "gconv3x3_wgrad")
    dwexp = _empty((C // 64, 64, 9, 64), dy)
    e0 = _prof_begin()
    dam = getattr(dy, "_koaf_amax", None) if CONV_F16 else None
    check(L.koaf_gconv3x3_wgrad(_ptr(dy), _ptr(x), _ptr(dwexp), N, H, W, C, stride, _ptr(in_sc), _ptr(in_sh),
                                _ptr(slabs), _ptr(dam), _a16(x), _stream()), "gconv3x3_wgrad")
    _prof_end(e0, "gemm", 2.0 * N * conv_out(H, 3, stride, 1) * conv_out(W, 3, stride, 1) * C * 9 * (C // 32),
              f"gconv_wgrad s{stride} C{C} px{N*H*W}",
              N * H * W * C + N * conv_out(H, 3, stride, 1) * conv_out(W, 3, stride, 1) * C + 9 * C * (C // 32),
              mpp=3 if (dam is not None and not _a16(x)) else 6)
    return dwexp


def stem_fold_w(w):
    w1t = _empty((49, 64), w)
    check(lib().koaf_stem_fold_w(_ptr(w), _ptr(w1t), _stream()), "stem_fold_w")
    return w1t


def stem_fwd(x, w1t, N, H, W, dtype=torch.float32, stats=False, shift=None):
    """dtype: storage type of the output activation (torch.float32, or torch.bfloat16: koaf.h "bf16 ACTIVATION STORAGE");
    stats: -> (y, part): the column statistics of y about `shift`, collected by the kernel (what colstats(y) would reduce)"""
    L = lib()
    y = _empty((N, conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3), 64), x, dtype=dtype)
    part = _empty((L.koaf_stem_stats_rows(N, H), 2, 64), x) if stats else None
    check(L.koaf_stem_fwd(_ptr(x), _ptr(w1t), _ptr(y), N, H, W, _ptr(part), _ptr(shift) if stats else None, _a16(y), _stream()), "stem_fwd")
    return (y, part) if stats else y


def stem_wgrad(dy, x, dw, N, H, W, slabs=None):
    """writes dw (packed [64,7,7,3] memory); dy may be a BnApply (the stem BatchNorm's backward, formed on load).
    slabs (None = allocated here): the per-block slab workspace, at least koaf_stem_wgrad_ws floats."""
    L = lib()
    dyp, _, app, like = _dy_args(dy, None)
    slabs = _slab_ws(slabs, L.koaf_stem_wgrad_ws(N, H, W), like, "stem_wgrad")
    dw1t = _empty((49, 64), like)
    check(L.koaf_stem_wgrad(dyp, _ptr(x), _ptr(dw1t), N, H, W, _ptr(slabs), app, _a16(dy.c) if app is not None else 0, _stream()),
          "stem_wgrad")
    check(L.koaf_stem_unfold_dw(_ptr(dw1t), _ptr(dw), _stream()), "stem_unfold_dw")
    return dw


def stem_dgrad(dy, w1t, N, H, W):
    """dx [N,H,W] = the stem's data gradient w.r.t. the single-channel image (koaf_stem_dgrad: gather form, no atomics); dy
    [N,OH,OW,64] or a BnApply (the stem BatchNorm's backward, formed on load); w1t the folded weight of stem_fold_w"""
    dyp, _, app, like = _dy_args(dy, None)
    dx = _empty((N, H, W), like)
    check(lib().koaf_stem_dgrad(dyp, _ptr(w1t), _ptr(dx), N, H, W, app, _a16(dy.c) if app is not None else 0, _stream()), "stem_dgrad")
    return dx


# ------------------------------------------------------------------------------------------------
# batch norm
# ------------------------------------------------------------------------------------------------
def _colpart_rows(rows, C, what):
    """partial rows of the column reductions (koaf_colpart_rows); a width their geometry does not cover (C % 4, C / 4 not a
    divisor of 256 up to 1024, beyond it not a multiple of 1024) is refused here, before any tensor is sized from it"""
    n = lib().koaf_colpart_rows(rows, C)
    if n < 0:
        raise KoafError(f"{what}: unsupported C={C}")
    return n


def colstats(x, rows, C, shift=None):
    L = lib()
    part = _empty((_colpart_rows(rows, C, "colstats"), 2, C), x)      # (fp32 whatever the storage type of x)
    r = _i32(0)
    check(L.koaf_colstats(_ptr(x), rows, C, _ptr(part), ctypes.addressof(r), _ptr(shift), _a16(x), _stream()), "colstats")
    return part


def _reduce_ws(rows, C, like):
    """fp64 workspace of the two-stage partial-row reduction (None when one stage does)"""
    n = lib().koaf_bn_reduce_ws(rows, C)
    return torch.empty(n // 8, dtype=torch.float64, device=like.device) if n else None


def bn_finalize(part, C, count, gamma, beta, running_mean, running_var, nbt, momentum, eps, train, shift=None):
    """-> saved [4][C] = mean, invstd, sc, sh.  shift = the tensor the statistics in `part` were summed about (it may be
    running_mean itself: the kernel reads it before updating)"""
    saved = _empty((4, C), gamma if gamma is not None else running_mean)
    rows = part.shape[0] if part is not None else 0
    ws = _reduce_ws(rows, C, saved) if train else None
    check(lib().koaf_bn_finalize(_ptr(part), rows, C, count, _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                 _ptr(running_var), _ptr(nbt), momentum, eps, 1 if train else 0, _ptr(saved[0]),
                                 _ptr(saved[1]), _ptr(saved[2]), _ptr(saved[3]), _ptr(shift) if train else None, _ptr(ws),
                                 _stream()), "bn_finalize")
    return saved


def bn_add_relu(c, saved, rows, C, idt=None, idsaved=None, out=None):
    y = out if out is not None else torch.empty_like(c)
    check(lib().koaf_bn_add_relu(_ptr(c), _ptr(saved[2]), _ptr(saved[3]), _ptr(idt),
                                 _ptr(idsaved[2]) if idsaved is not None else None,
                                 _ptr(idsaved[3]) if idsaved is not None else None, _ptr(y), rows, C, _a16(c), _stream()),
          "bn_add_relu")
    return y


def bn_bwd(g, c, saved, rows, C, count, dgamma, dbeta, mask_mode, ymask=None, dz_out=None, dc_out=None, fused=False, pool=None,
           train=True):
    """Full BatchNorm(+ReLU mask) backward: reduce -> finalize -> dc.  g is the upstream gradient; with a mask the masked
    gradient dz is written to dz_out (default: in place over g).  fused=False: dc is written out (koaf_bn_bwd_apply) and
    returned; fused=True: returns a BnApply -- the recipe of dc for the GEMM loaders -- and nothing is written.
    train=False: the BatchNorm ran on its running statistics (`saved` holds them), so dc = sc*dz (koaf_bn_bwd_finalize_eval);
    dgamma / dbeta may be None (frozen parameters): they are then not written."""
    L = lib()
    if pool is not None:
        # g is the gradient of the max-pool behind this BatchNorm(+ReLU): pool = (pool_g [N,OH,OW,C], argmax, N, H, W); the pool's
        # input gradient is gathered by the reduction itself (koaf_bn_bwd_reduce_pool) and only the masked dz is written
        pg, am, pN, pH, pW = pool
        assert g is None and mask_mode == 2 and rows == pN * pH * pW
        dz = dz_out if dz_out is not None else _empty((pN, pH, pW, C), pg)
        part = _empty((_colpart_rows(rows, C, "bn_bwd_reduce_pool"), 2, C), pg)
        r = _i32(0)
        dzmax = _empty((1,), pg) if fused else None
        check(L.koaf_bn_bwd_reduce_pool(_ptr(pg), _ptr(am), _ptr(c), _ptr(saved[2]), _ptr(saved[3]), _ptr(saved[0]), _ptr(saved[1]),
                                        _ptr(dz), _ptr(part), ctypes.addressof(r), pN, pH, pW, C, _ptr(dzmax), _a16(c), _stream()),
              "bn_bwd_reduce_pool")
        return _bn_bwd_tail(part[:r.value], 2, 1, dz, c, saved, rows, C, count, dgamma, dbeta, dc_out, fused, dzmax, train)
    if mask_mode != 0 and dz_out is None:
        dz_out = g  # mask in place
    part = _empty((_colpart_rows(rows, C, "bn_bwd_reduce"), 2, C), g)
    r = _i32(0)
    dzmax = _empty((1,), g) if fused else None
    check(L.koaf_bn_bwd_reduce(_ptr(g), _ptr(c), _ptr(ymask), _ptr(saved[2]), _ptr(saved[3]), _ptr(saved[0]),
                               _ptr(saved[1]), mask_mode, _ptr(dz_out), _ptr(part), ctypes.addressof(r), rows, C,
                               _ptr(dzmax), _a16(c), _stream()), "bn_bwd_reduce")
    dz = dz_out if dz_out is not None else g
    return _bn_bwd_tail(part[:r.value], 2, 1, dz, c, saved, rows, C, count, dgamma, dbeta, dc_out, fused, dzmax, train)


def _bn_bwd_tail(part, nsum, i1, dz, c, saved, rows, C, count, dgamma, dbeta, dc_out, fused, dzmax, train=True):
    L = lib()
    coef = _empty((4 if fused else 3, C), dz)
    amax = _empty((1,), dz) if fused else None
    if train:
        check(L.koaf_bn_bwd_finalize(_ptr(part), part.shape[0], C, count, _ptr(saved[2]), _ptr(saved[1]), _ptr(dgamma),
                                     _ptr(dbeta), _ptr(coef), nsum, i1, _ptr(_reduce_ws(part.shape[0], C, dz)),
                                     _ptr(saved[0]) if fused else None, _ptr(dzmax), _ptr(amax), _stream()), "bn_bwd_finalize")
    else:
        # eval mode: dc = sc*dz; the partial sums only feed dgamma / dbeta and are left alone when neither is wanted
        want = dgamma is not None or dbeta is not None
        check(L.koaf_bn_bwd_finalize_eval(_ptr(part) if want else None, part.shape[0] if want else 0, C, _ptr(saved[2]), _ptr(dgamma),
                                          _ptr(dbeta), _ptr(coef), 4 if fused else 3, nsum, i1,
                                          _ptr(_reduce_ws(part.shape[0], C, dz)) if want else None, _ptr(dzmax), _ptr(amax),
                                          _stream()), "bn_bwd_finalize_eval")
    if fused:
        return BnApply(dz, c, coef, amax, saved[0], rows, C)
    dc = dc_out if dc_out is not None else torch.empty(c.shape, device=c.device, dtype=torch.float32)
    check(L.koaf_bn_bwd_apply(_ptr(dz), _ptr(c), _ptr(saved[0]), _ptr(coef), _ptr(dc), rows, C, None, _a16(c), _stream()),
          "bn_bwd_apply")
    return dc


def bn_bwd_from_part(part, nsum, i1, dz, c, saved, rows, C, count, dgamma, dbeta, dc_out=None, fused=False, dzmax=None, train=True):
    """BatchNorm backward when the reduction already happened in a dgrad epilogue: finalize (+ apply unless fused; fused
    needs dzmax, the device scalar max |dz| that epilogue left); train=False: the eval-mode backward, see bn_bwd."""
    if fused and dzmax is None:
        raise KoafError("bn_bwd_from_part(fused=True) needs dzmax (conv2d_dgrad with bnb['dz_amax'])")
    return _bn_bwd_tail(part, nsum, i1, dz, c, saved, rows, C, count, dgamma, dbeta, dc_out, fused, dzmax, train)


def maxpool_fwd(c, saved, N, H, W, C):
    OH, OW = conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1)
    y = _empty((N, OH, OW, C), c, dtype=c.dtype)
    am = _empty((N, OH, OW, C), c, dtype=torch.uint8)
    check(lib().koaf_maxpool_fwd(_ptr(c), _ptr(saved[2]), _ptr(saved[3]), _ptr(y), _ptr(am), N, H, W, C, _a16(c), _stream()),
          "maxpool_fwd")
    return y, am


def maxpool_bwd(dy, am, N, H, W, C):
    da = _empty((N, H, W, C), dy)
    check(lib().koaf_maxpool_bwd(_ptr(dy), _ptr(am), _ptr(da), N, H, W, C, _stream()), "maxpool_bwd")
    return da


def gap_fwd(y, N, HW, C):
    out = _empty((N, C), y)
    check(lib().koaf_gap_fwd(_ptr(y), _ptr(out), N, HW, C, _a16(y), _stream()), "gap_fwd")
    return out


def gap_bwd(dout, N, HW, C):
    dy = _empty((N, HW, C), dout)
    check(lib().koaf_gap_bwd(_ptr(dout), _ptr(dy), N, HW, C, _stream()), "gap_bwd")
    return dy


# ------------------------------------------------------------------------------------------------
# class-activation maps
# ------------------------------------------------------------------------------------------------
def cam(A, w, N, HW, C, relu=True):
    """cam[n][p] = sum_c A[n][p][c] * w[n][c] (clamped at 0 with `relu`) of an NHWC feature map A (fp32 or bf16 storage) and fp32
    weights w [N, C] -> (cam [N, HW], img_sum [N] = sum_p cam, img_max [N] = max_p |cam|), all fp32 (koaf_cam: fixed order)"""
    if A.dtype not in (torch.float32, torch.bfloat16) or w.dtype != torch.float32:
        raise KoafError(f"cam: an fp32 / bf16 feature map and fp32 weights, got {A.dtype} and {w.dtype}")
    if not (A.is_contiguous() and w.is_contiguous()) or A.numel() != N * HW * C or w.numel() != N * C:
        raise KoafError(f"cam: contiguous A [{N}, {HW}, {C}] and w [{N}, {C}], got {tuple(A.shape)} and {tuple(w.shape)}")
    out = torch.empty((N, HW), device=A.device, dtype=torch.float32)
    stat = torch.empty((2, N), device=A.device, dtype=torch.float32)
    check(lib().koaf_cam(_ptr(A), _ptr(w), _ptr(out), _ptr(stat[0]), _ptr(stat[1]), N, HW, C, 1 if relu else 0, _a16(A), _stream()),
          "cam")
    return out, stat[0], stat[1]


CAM_NORMALIZE = {None: 0, "sample": 1, "image": 2}


def cam_upsample(cam, img_max, out, B, K, h, w, H, W, strides, normalize=None):
    """image b*K + k of cam [B*K, h, w] resized to H x W (bilinear, align_corners=False), divided by a maximum (normalize: None,
    "sample" = the largest img_max of the sample's K images, "image" = its own) and written to out[b*sb + k*sk + i*si + j*sj],
    strides = (sb, sk, si, sj) in elements (koaf_cam_upsample: one write pass).  Elements of `out` no (b, k, i, j) reaches stay."""
    if normalize not in CAM_NORMALIZE:
        raise ValueError(f"Unknown normalize: {normalize}")
    if cam.dtype != torch.float32 or out.dtype != torch.float32 or not (cam.is_contiguous() and out.is_contiguous()):
        raise KoafError("cam_upsample: contiguous fp32 tensors only")
    if cam.numel() != B * K * h * w or (img_max is not None and (img_max.numel() != B * K or not img_max.is_contiguous())):
        raise KoafError(f"cam_upsample: cam [{B * K}, {h}, {w}] and img_max [{B * K}], got {tuple(cam.shape)}")
    sb, sk, si, sj = (int(s) for s in strides)
    if min(sb, sk, si, sj) <= 0 or (B - 1) * sb + (K - 1) * sk + (H - 1) * si + (W - 1) * sj >= out.numel():
        raise KoafError(f"cam_upsample: strides {(sb, sk, si, sj)} leave the {out.numel()} elements of out")
    check(lib().koaf_cam_upsample(_ptr(cam), _ptr(img_max), _ptr(out), B, K, h, w, H, W, sb, sk, si, sj, CAM_NORMALIZE[normalize],
                                  _stream()), "cam_upsample")
    return out


# ------------------------------------------------------------------------------------------------
# path attributions (integrated gradients, SmoothGrad)
# ------------------------------------------------------------------------------------------------
ATTR_MAX_J = defines()["KOAF_ATTR_MAX_J"]


def _attr_rows(what, x, base):
    """(B, n) of a contiguous fp32 (B, ...) tensor x; base: None, a python number or a tensor like x -> (tensor | None, value)"""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or not x.is_contiguous() or x.dim() < 1 or x.numel() == 0:
        raise KoafError(f"{what}: a contiguous, non-empty fp32 tensor (B, ...), got "
                        f"{(tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x)}")
    if torch.is_tensor(base):
        if base.dtype != torch.float32 or not base.is_contiguous() or tuple(base.shape) != tuple(x.shape) or base.device != x.device:
            raise KoafError(f"{what}: a baseline tensor is contiguous fp32 of x's shape {tuple(x.shape)} on x's device, got "
                            f"{tuple(base.shape)} {base.dtype} on {base.device}")
        return int(x.shape[0]), x.numel() // int(x.shape[0]), base, 0.0
    return int(x.shape[0]), x.numel() // int(x.shape[0]), None, 0.0 if base is None else float(base)


def _attr_coefs(what, c, like):
    """the J alphas / weights: a device fp32 vector [J], 1 <= J <= KOAF_ATTR_MAX_J"""
    if not torch.is_tensor(c) or c.dtype != torch.float32 or c.dim() != 1 or not c.is_contiguous() or c.device != like.device:
        raise KoafError(f"{what}: the coefficients are a contiguous fp32 vector on the tensors' device")
    if not 1 <= c.numel() <= ATTR_MAX_J:
        raise KoafError(f"{what}: 1 <= J <= {ATTR_MAX_J}, got J = {c.numel()}")
    return int(c.numel())


def path_points(x, alpha, base=None, mm=None, noise_level=0.0, seed=0, draw0=0):
    """out[j] = base + alpha[j] * (x - base) + sigma_b * z(seed, draw0 + j, b, i) -> [J, *x.shape] (koaf_path_points: x and base
    read once for all J; no fused operation).  base: None (zeros), a python number, or a tensor like x.  alpha: device fp32 [J].
    mm: the [B, 2] of ops.minmax(x, B), sigma_b = noise_level * (max_b - min_b); mm None or noise_level 0 draws nothing."""
    B, n, bt, bv = _attr_rows("path_points", x, base)
    J = _attr_coefs("path_points", alpha, x)
    if mm is not None and (mm.dtype != torch.float32 or not mm.is_contiguous() or tuple(mm.shape) != (B, 2) or mm.device != x.device):
        raise KoafError(f"path_points: mm is the contiguous fp32 [{B}, 2] of ops.minmax, got {tuple(mm.shape)} {mm.dtype}")
    if not (0 <= int(draw0) and int(draw0) + J <= 2 ** 31):
        raise KoafError(f"path_points: draw indices lie in [0, 2^31), got draw0 = {draw0}")
    out = torch.empty((J,) + tuple(x.shape), device=x.device, dtype=torch.float32)
    check(lib().koaf_path_points(_ptr(x), _ptr(bt), bv, _ptr(alpha), _ptr(out), J, B, n, _ptr(mm), float(noise_level),
                                 int(seed) & (2 ** 64 - 1), int(draw0), _stream()), "path_points")
    return out


def attr_fold(acc, g, w, square=False, first=False, x=None, base=None):
    """acc (=|+=) sum_j w[j] * f(g[j]) in index order, f the identity or (square) the square; g [J, *acc.shape], w device fp32
    [J]; first: write instead of accumulate.  With x given (the last chunk of an integrated-gradients path) the stored value is
    additionally multiplied by (x - base), base as in path_points (koaf_attr_fold: one pass, no fused operation).  Returns acc."""
    B, n, bt, bv = _attr_rows("attr_fold", acc, base if x is not None else None)
    J = _attr_coefs("attr_fold", w, acc)
    if not torch.is_tensor(g) or g.dtype != torch.float32 or not g.is_contiguous() or tuple(g.shape) != (J,) + tuple(acc.shape) \
            or g.device != acc.device:
        raise KoafError(f"attr_fold: g is contiguous fp32 [{J}, *{tuple(acc.shape)}] on acc's device, got "
                        f"{(tuple(g.shape), g.dtype) if torch.is_tensor(g) else type(g)}")
    if x is not None and (x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != tuple(acc.shape) or x.device != acc.device):
        raise KoafError(f"attr_fold: x is contiguous fp32 of acc's shape {tuple(acc.shape)}, got {tuple(x.shape)} {x.dtype}")
    check(lib().koaf_attr_fold(_ptr(acc), _ptr(g), _ptr(w), _ptr(x), _ptr(bt), bv, J, B, n, 1 if square else 0, 1 if first else 0,
                               1 if x is not None else 0, _stream()), "attr_fold")
    return acc


# ------------------------------------------------------------------------------------------------
# validation / evaluation metrics (calc_metrics_v2, calc_bootstrap)
# ------------------------------------------------------------------------------------------------
METRICS_MAX_N = defines()["KOAF_METRICS_MAX_N"]
METRICS_FLAG_TEXT = {1: "Input contains NaN or infinity.", 2: "a label other than 0 / 1 (binary targets only)",
                     4: "an index of the resampling matrix lies outside [0, n)"}      # (or a rank of `packed` outside its bins)


def metrics_flag(device):
    """a zeroed flag word for the three metric kernels (koaf.h: bit 0 a non-finite score, 1 a non-binary label, 2 a wild index)"""
    return torch.zeros(1, dtype=torch.int32, device=device)


def metrics_raise(word):
    """the ValueError of a flag word read back from the device (sklearn raises one for non-finite scores); 0 passes"""
    word = int(word) & 7
    if word:
        raise ValueError("; ".join(text for bit, text in METRICS_FLAG_TEXT.items() if word & bit))


def _metric_scores(what, s):
    """(n, stride) of a 1-D fp32 / fp64 device vector with a positive stride: a column of an (n, classes) tensor is read in place"""
    if not torch.is_tensor(s) or s.dtype not in (torch.float32, torch.float64) or s.dim() != 1 or s.numel() == 0 or s.stride(0) < 1:
        raise KoafError(f"{what}: the scores are a non-empty 1-D fp32 / fp64 device vector with a positive stride, got "
                        f"{(tuple(s.shape), s.dtype, s.stride()) if torch.is_tensor(s) else type(s)}")
    return int(s.numel()), int(s.stride(0))


def _metric_i32(what, name, t, like, shape=None):
    if not torch.is_tensor(t) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != like.device \
            or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise KoafError(f"{what}: {name} is a contiguous int32 tensor{'' if shape is None else ' ' + str(list(shape))} on the scores' "
                        f"device, got {(tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t)}")


def score_ranks(scores, labels=None, pos_label=1, flag=None):
    """rank[i] = #{j : scores[j] > scores[i]} (int32; ties share a rank, the comparison is made in the scores' own dtype) of a
    1-D fp32 / fp64 device vector of any positive stride, n <= METRICS_MAX_N (koaf_score_ranks: all-pairs counting).  With labels
    (int32 [n], values 0 / 1) also packed[i] = rank[i] << 1 | (labels[i] == pos_label), what curve_metrics / point_metrics read:
    -> (rank, packed).  flag: a metrics_flag() word the kernel raises bits of; None: an own word is read back here (a host
    sync) and a non-finite score or a non-binary label raises ValueError."""
    n, stride = _metric_scores("score_ranks", scores)
    if labels is not None:
        _metric_i32("score_ranks", "labels", labels, scores, (n,))
    own = flag is None
    if own:
        flag = metrics_flag(scores.device)
    _metric_i32("score_ranks", "flag", flag, scores, (1,))
    rank = torch.empty(n, dtype=torch.int32, device=scores.device)
    packed = torch.empty(n, dtype=torch.int32, device=scores.device) if labels is not None else None
    check(lib().koaf_score_ranks(_ptr(scores), 1 if scores.dtype == torch.float64 else 0, stride, n, _ptr(labels), int(pos_label),
                                 _ptr(rank), _ptr(packed), _ptr(flag), _stream()), "score_ranks")
    if own:
        metrics_raise(flag.item())
    return rank if labels is None else (rank, packed)


def curve_metrics(packed, idx=None, with_identity=True, pi0=0.12, out=None, flag=None):
    """out [rows, 8] fp64, row r = (n_pos, n_neg, roc_auc, avg_precision, avg_precision calibrated to the prevalence pi0, 0, 0, 0)
    of one resample of the n samples behind packed (score_ranks): row 0 the sample itself when with_identity, then one row per
    row of idx (int32 [R, m] device indices into the sample, m <= METRICS_MAX_N; None: no resamples).  One block per row
    (koaf_curve_metrics: integer histograms, fixed-order fp64 sums -- identical bits from run to run).  A row without positives or
    without negatives holds its counts and NaN.  flag as in score_ranks (a wild index is skipped and raises)."""
    if not torch.is_tensor(packed) or not packed.is_cuda:
        raise KoafError("curve_metrics: packed is the device tensor score_ranks returns")
    _metric_i32("curve_metrics", "packed", packed, packed)
    n = int(packed.numel())
    R = m = 0
    if idx is not None:
        _metric_i32("curve_metrics", "idx", idx, packed)
        if idx.dim() != 2 or idx.numel() == 0:
            raise KoafError(f"curve_metrics: idx is a non-empty [R, m] matrix, got {tuple(idx.shape)}")
        R, m = int(idx.shape[0]), int(idx.shape[1])
    rows = R + (1 if with_identity else 0)
    if rows == 0:
        raise KoafError("curve_metrics: neither the identity row nor an index matrix")
    if out is None:
        out = torch.empty((rows, 8), dtype=torch.float64, device=packed.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (rows, 8) or out.device != packed.device:
        raise KoafError(f"curve_metrics: out is contiguous fp64 [{rows}, 8] on packed's device, got {tuple(out.shape)} {out.dtype}")
    own = flag is None
    if own:
        flag = metrics_flag(packed.device)
    _metric_i32("curve_metrics", "flag", flag, packed, (1,))
    check(lib().koaf_curve_metrics(_ptr(packed), n, _ptr(idx), R, m, 1 if with_identity else 0, float(pi0), _ptr(out), _ptr(flag),
                                   _stream()), "curve_metrics")
    if own:
        metrics_raise(flag.item())
    return out


def point_metrics(scores, packed, thr=0.5, out=None, flag=None):
    """out [9] fp64 of the sample itself: out[0] the Youden cutoff as the reference's sensitivity_specificity_cutoff picks it
    (first maximum over the points roc_curve(drop_intermediate=True) keeps; a score value, or +inf), out[1:5] = (tn, fp, fn, tp)
    of `scores > thr`, out[5:9] the same of `scores >= cutoff` (koaf_point_metrics, one block).  scores / packed as in score_ranks."""
    n, stride = _metric_scores("point_metrics", scores)
    _metric_i32("point_metrics", "packed", packed, scores, (n,))
    if out is None:
        out = torch.empty(9, dtype=torch.float64, device=scores.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (9,) or out.device != scores.device:
        raise KoafError(f"point_metrics: out is contiguous fp64 [9] on the scores' device, got {tuple(out.shape)} {out.dtype}")
    own = flag is None
    if own:
        flag = metrics_flag(scores.device)
    _metric_i32("point_metrics", "flag", flag, scores, (1,))
    check(lib().koaf_point_metrics(_ptr(scores), 1 if scores.dtype == torch.float64 else 0, stride, _ptr(packed), n, float(thr),
                                   _ptr(out), _ptr(flag), _stream()), "point_metrics")
    if own:
        metrics_raise(flag.item())
    return out


def curve_points_len(n):
    """the fp64 length of curve_points' buffer for n samples: 8 + 8 * (n + 1), known before anything is computed"""
    return int(lib().koaf_curve_points_len(int(n)))


def curve_points(scores, packed, pi0=0.12, pi_of_negatives=False, out=None, flag=None):
    """The ROC / PR curve points of the sample itself in one fp64 buffer [curve_points_len(n)] (koaf_curve_points, one block): a
    header (n_pos, n_neg, T thresholds, K kept ROC thresholds, last_ind, 0, 0, 0) and eight arrays of n + 1 slots -- thr, rec,
    prec, prec calibrated to the prevalence pi0, roc fpr, roc tpr, roc thr, scratch; see koaf.h and parse_curve_points.
    pi_of_negatives: the calibration takes the share of the NEGATIVES as the sample's prevalence (the reference's
    np.sum(y_true) / n when class 0 is the positive one).  scores / packed / flag as in score_ranks."""
    n, stride = _metric_scores("curve_points", scores)
    _metric_i32("curve_points", "packed", packed, scores, (n,))
    need = curve_points_len(n)
    if out is None:
        out = torch.empty(need, dtype=torch.float64, device=scores.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (need,) or out.device != scores.device:
        raise KoafError(f"curve_points: out is contiguous fp64 [{need}] on the scores' device, got {tuple(out.shape)} {out.dtype}")
    own = flag is None
    if own:
        flag = metrics_flag(scores.device)
    _metric_i32("curve_points", "flag", flag, scores, (1,))
    check(lib().koaf_curve_points(_ptr(scores), 1 if scores.dtype == torch.float64 else 0, stride, _ptr(packed), n, float(pi0),
                                  1 if pi_of_negatives else 0, _ptr(out), _ptr(flag), _stream()), "curve_points")
    if own:
        metrics_raise(flag.item())
    return out


def parse_curve_points(buf):
    """the views into a HOST copy (numpy fp64) of curve_points' buffer: dict of n_pos, n_neg, T, K, last_ind and the arrays
    thr [T]; rec / prec / prec_cal [T + 1] (slot 0 the closing (0, 1) point); fpr / tpr / roc_thr [K + 1] (slot 0 the leading
    (0, 0, inf) point).  Slicing only: nothing is computed here."""
    n = (buf.shape[0] - 8) // 8 - 1
    P, N, T, K, last = (int(v) for v in buf[:5])
    a = buf[8:].reshape(8, n + 1)
    return {"n_pos": P, "n_neg": N, "T": T, "K": K, "last_ind": last, "thr": a[0, :T], "rec": a[1, :T + 1], "prec": a[2, :T + 1],
            "prec_cal": a[3, :T + 1], "fpr": a[4, :K + 1], "tpr": a[5, :K + 1], "roc_thr": a[6, :K + 1]}


def range_metrics(packed, idx=None, with_identity=True, pi0=0.12, recall_range=(0.0, 1.0), out=None, flag=None):
    """out [rows, 8] fp64, row r = (n_pos, n_neg, average precision over the recall range, best calibrated F1, the recall at the
    low end, at the high end, 0, 0) of one resample; rows / idx / with_identity / flag as in curve_metrics (koaf_range_metrics:
    one block per row, fixed-order fp64 sums).  pi0 None: the F1 is not calibrated."""
    if not torch.is_tensor(packed) or not packed.is_cuda:
        raise KoafError("range_metrics: packed is the device tensor score_ranks returns")
    _metric_i32("range_metrics", "packed", packed, packed)
    n = int(packed.numel())
    R = m = 0
    if idx is not None:
        _metric_i32("range_metrics", "idx", idx, packed)
        if idx.dim() != 2 or idx.numel() == 0:
            raise KoafError(f"range_metrics: idx is a non-empty [R, m] matrix, got {tuple(idx.shape)}")
        R, m = int(idx.shape[0]), int(idx.shape[1])
    rows = R + (1 if with_identity else 0)
    if rows == 0:
        raise KoafError("range_metrics: neither the identity row nor an index matrix")
    if out is None:
        out = torch.empty((rows, 8), dtype=torch.float64, device=packed.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (rows, 8) or out.device != packed.device:
        raise KoafError(f"range_metrics: out is contiguous fp64 [{rows}, 8] on packed's device, got {tuple(out.shape)} {out.dtype}")
    own = flag is None
    if own:
        flag = metrics_flag(packed.device)
    _metric_i32("range_metrics", "flag", flag, packed, (1,))
    lo, hi = recall_range
    check(lib().koaf_range_metrics(_ptr(packed), n, _ptr(idx), R, m, 1 if with_identity else 0, 0.0 if pi0 is None else float(pi0),
                                   float(lo), float(hi), _ptr(out), _ptr(flag), _stream()), "range_metrics")
    if own:
        metrics_raise(flag.item())
    return out


def confusion(y_true, y_pred, K, out=None, flag=None):
    """counts [K, K] int64, counts[t, p] = #{i : y_true[i] == t and y_pred[i] == p} of two int32 device vectors of class indices,
    K <= 32 (koaf_confusion: integer atomics only).  out: a ZEROED int64 [K, K] to add into.  A label outside [0, K) is skipped and
    raises flag bit 1 (flag as in score_ranks)."""
    if not torch.is_tensor(y_true) or not y_true.is_cuda or y_true.dim() != 1 or y_true.numel() == 0:
        raise KoafError("confusion: y_true is a non-empty 1-D int32 device vector")
    _metric_i32("confusion", "y_true", y_true, y_true)
    _metric_i32("confusion", "y_pred", y_pred, y_true, tuple(y_true.shape))
    K = int(K)
    if out is None:
        out = torch.zeros((max(K, 0), max(K, 0)), dtype=torch.int64, device=y_true.device)
    elif out.dtype != torch.int64 or not out.is_contiguous() or tuple(out.shape) != (K, K) or out.device != y_true.device:
        raise KoafError(f"confusion: out is contiguous int64 [{K}, {K}] on the labels' device, got {tuple(out.shape)} {out.dtype}")
    own = flag is None
    if own:
        flag = metrics_flag(y_true.device)
    _metric_i32("confusion", "flag", flag, y_true, (1,))
    check(lib().koaf_confusion(_ptr(y_true), _ptr(y_pred), int(y_true.numel()), K, _ptr(out), _ptr(flag), _stream()), "confusion")
    if own:
        metrics_raise(flag.item())
    return out


def pair_ranks(scores_a, scores_b, labels=None, pos_label=1, flag=None):
    """score_ranks over the UNION of two score columns of the same n samples (koaf_pair_ranks): element j < n is scores_a[j],
    element n + j is scores_b[j]; rank[j] = #{k : union[k] > union[j]} (int32 [2n]), so equal scores of the two models share a
    rank.  Both columns are 1-D device vectors of one dtype (fp32 or fp64), each read through its own positive stride,
    n <= METRICS_MAX_N // 2.  With labels (int32 [n]) also packed[j] = rank[j] << 1 | (labels[j mod n] == pos_label), what
    perm_metrics reads: -> (rank, packed).  flag as in score_ranks."""
    n, stride_a = _metric_scores("pair_ranks", scores_a)
    nb, stride_b = _metric_scores("pair_ranks", scores_b)
    if nb != n or scores_b.dtype != scores_a.dtype or scores_b.device != scores_a.device:
        raise KoafError(f"pair_ranks: two columns of one length, dtype and device, got {n} {scores_a.dtype} {scores_a.device} and "
                        f"{nb} {scores_b.dtype} {scores_b.device}")
    if labels is not None:
        _metric_i32("pair_ranks", "labels", labels, scores_a, (n,))
    own = flag is None
    if own:
        flag = metrics_flag(scores_a.device)
    _metric_i32("pair_ranks", "flag", flag, scores_a, (1,))
    rank = torch.empty(2 * n, dtype=torch.int32, device=scores_a.device)
    packed = torch.empty(2 * n, dtype=torch.int32, device=scores_a.device) if labels is not None else None
    check(lib().koaf_pair_ranks(_ptr(scores_a), stride_a, _ptr(scores_b), stride_b, 1 if scores_a.dtype == torch.float64 else 0, n,
                                _ptr(labels), int(pos_label), _ptr(rank), _ptr(packed), _ptr(flag), _stream()), "pair_ranks")
    if own:
        metrics_raise(flag.item())
    return rank if labels is None else (rank, packed)


def perm_metrics(packed, masks=None, with_identity=True, out=None, flag=None):
    """out [rows, 8] fp64, row r = (n_pos, n_neg, U_ref, U_cmp, ap_ref, ap_cmp, 0, 0) of one paired permutation of the n samples
    behind packed (pair_ranks, int32 [2n]): row 0 the sample as it is when with_identity, then one row per row of masks (int32
    [R, ceil(n / 32)] device words holding the bits of a uint32 matrix: sample i changes sides when bit i & 31 of word i >> 5 is
    set; None: no permutations).  U is the Mann-Whitney sum 2 * n_pos * n_neg * roc_auc as an exact integer, ap the average
    precision (koaf_perm_metrics: two blocks per row, integer histograms over the 2n union bins, fixed-order fp64 sums --
    identical bits from run to run).  flag as in score_ranks."""
    if not torch.is_tensor(packed) or not packed.is_cuda:
        raise KoafError("perm_metrics: packed is the device tensor pair_ranks returns")
    _metric_i32("perm_metrics", "packed", packed, packed)
    if packed.dim() != 1 or packed.numel() == 0 or packed.numel() % 2:
        raise KoafError(f"perm_metrics: packed holds 2n words, got {tuple(packed.shape)}")
    n = int(packed.numel()) // 2
    R = 0
    if masks is not None:
        _metric_i32("perm_metrics", "masks", masks, packed)
        if masks.dim() != 2 or masks.numel() == 0 or int(masks.shape[1]) != (n + 31) // 32:
            raise KoafError(f"perm_metrics: masks is a non-empty [R, {(n + 31) // 32}] matrix, got {tuple(masks.shape)}")
        R = int(masks.shape[0])
    rows = R + (1 if with_identity else 0)
    if rows == 0:
        raise KoafError("perm_metrics: neither the identity row nor a mask matrix")
    if out is None:
        out = torch.empty((rows, 8), dtype=torch.float64, device=packed.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (rows, 8) or out.device != packed.device:
        raise KoafError(f"perm_metrics: out is contiguous fp64 [{rows}, 8] on packed's device, got {tuple(out.shape)} {out.dtype}")
    own = flag is None
    if own:
        flag = metrics_flag(packed.device)
    _metric_i32("perm_metrics", "flag", flag, packed, (1,))
    check(lib().koaf_perm_metrics(_ptr(packed), n, _ptr(masks), R, 1 if with_identity else 0, _ptr(out), _ptr(flag), _stream()),
          "perm_metrics")
    if own:
        metrics_raise(flag.item())
    return out


# ------------------------------------------------------------------------------------------------
# raw MRI series -> input volumes (koaf_mriprep.hip)
# ------------------------------------------------------------------------------------------------
_SERIES_DTYPE = {torch.uint16: 2, torch.int16: 3, torch.float32: 4, torch.float64: 5}      # koaf.h: koaf_widen's codes and on
SERIES_FLAG_TEXT = {1: "the series holds NaN or infinity", 2: "the series holds a value outside [0, 65535]"}


def series_flag(device):
    """a zeroed flag word for series_hist (koaf.h: bit 0 a non-finite voxel, bit 1 a voxel outside [0, 65535])"""
    return torch.zeros(1, dtype=torch.int32, device=device)


def series_raise(word):
    """the ValueError of a series_hist flag word read back from the device; 0 passes"""
    word = int(word) & 3
    if word:
        raise ValueError("; ".join(text for bit, text in SERIES_FLAG_TEXT.items() if word & bit))


def _series_volume(what, x, ndim=None):
    """dtype code of a non-empty contiguous uint16 / int16 / fp32 / fp64 device tensor (of `ndim` axes)"""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype not in _SERIES_DTYPE or x.dim() != (ndim or x.dim()) or x.numel() == 0 \
            or not x.is_contiguous():
        raise KoafError(f"{what}: a non-empty contiguous {'' if ndim is None else str(ndim) + '-D '}uint16 / int16 / float32 / float64 tensor on the HIP device, got "
                        f"{(tuple(x.shape), x.dtype, x.device, x.is_contiguous()) if torch.is_tensor(x) else type(x)}")
    return _SERIES_DTYPE[x.dtype]


def _series_shift(what, shift):
    if not 2 <= int(shift) <= 8:
        raise KoafError(f"{what}: shift 2..8, got {shift}")
    return int(shift)


def t2_fit(vol, tes, nan_to=0.0, val_low=0.0, val_high=0.1, decimals=-1, margin=0, layout=0, out=None):
    """The reference's fit_t2_map on the device (koaf_t2_fit): vol (S, R, C, E) in its stored dtype (uint16 / int16 / fp32 / fp64,
    echo fastest), tes (S, E) fp64 -> fp64 T2 map, one launch.  decimals >= 0 also applies np.round(., decimals), margin > 0
    drops that many voxels at both ends of R and C, layout 0 gives (S, R', C'), layout 1 (R', C', S).  2 <= E <= 16."""
    dt = _series_volume("t2_fit", vol, 4)
    S, R, C, E = (int(v) for v in vol.shape)
    if not torch.is_tensor(tes) or tes.dtype != torch.float64 or tuple(tes.shape) != (S, E) or tes.device != vol.device \
            or not tes.is_contiguous():
        raise KoafError(f"t2_fit: tes is a contiguous fp64 [{S}, {E}] tensor on vol's device, got "
                        f"{(tuple(tes.shape), tes.dtype, tes.device) if torch.is_tensor(tes) else type(tes)}")
    if not 2 <= E <= 16:
        raise KoafError(f"t2_fit: 2..16 echoes, got {E} (with one echo the reference's own answer is rounding noise)")
    margin, decimals = int(margin), int(decimals)
    if margin < 0 or 2 * margin >= R or 2 * margin >= C:
        raise KoafError(f"t2_fit: margin {margin} leaves nothing of {R} x {C}")
    if layout not in (0, 1):
        raise KoafError(f"t2_fit: layout 0 = (S, R, C), 1 = (R, C, S), got {layout}")
    if decimals > 22:
        raise KoafError(f"t2_fit: at most 22 decimals (10^d exact in fp64), got {decimals}")
    RO, CO = R - 2 * margin, C - 2 * margin
    shape = (S, RO, CO) if layout == 0 else (RO, CO, S)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=vol.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != shape or out.device != vol.device:
        raise KoafError(f"t2_fit: out is contiguous fp64 {list(shape)} on vol's device, got {tuple(out.shape)} {out.dtype}")
    check(lib().koaf_t2_fit(vol.data_ptr(), dt, _ptr(tes), S, R, C, E, float(nan_to), float(val_low), float(val_high), decimals,
                            margin, int(layout), _ptr(out), _stream()), "t2_fit")
    return out


def series_hist(x, shift=3, bins=None, flag=None):
    """int32 [65536 >> shift] counts of astype(uint16)(x) >> shift over a contiguous uint16 / int16 / fp32 / fp64 device tensor
    (koaf_series_hist; integer atomics: deterministic).  bins: a tensor to add into (None: fresh zeros).  flag: a series_flag()
    word the kernel raises bits of; None: an own word is read back here (a host sync) and a non-finite or out-of-range voxel of a
    floating-point series raises ValueError."""
    dt = _series_volume("series_hist", x)
    shift = _series_shift("series_hist", shift)
    if x.numel() >= 1 << 31:
        raise KoafError(f"series_hist: fewer than 2^31 voxels, got {x.numel()}")
    nb = 65536 >> shift
    if bins is None:
        bins = torch.zeros(nb, dtype=torch.int32, device=x.device)
    _metric_i32("series_hist", "bins", bins, x, (nb,))
    own = flag is None
    if own:
        flag = series_flag(x.device)
    _metric_i32("series_hist", "flag", flag, x, (1,))
    check(lib().koaf_series_hist(x.data_ptr(), dt, x.numel(), shift, _ptr(bins), _ptr(flag), _stream()), "series_hist")
    if own:
        series_raise(flag.item())
    return bins


def percentile_index(n, q):
    """(k, gamma) of np.percentile(a, q) (method "linear") over n values: the result is lerp(a_(k), a_(min(k + 1, n - 1)), gamma)"""
    import math
    v = (n - 1) * (float(q) / 100.0)
    k = math.floor(v)
    return int(k), v - k


def series_quantiles(bins, n, q=(0.0, 99.9), shift=3, out=None):
    """fp64 [len(q)] device tensor of np.percentile(x >> shift, q) from the histogram series_hist made of the n voxels of x
    (koaf_series_quantiles, one block; bit-equal to numpy, and nothing is read back)."""
    shift = _series_shift("series_quantiles", shift)
    if not torch.is_tensor(bins) or not bins.is_cuda:
        raise KoafError("series_quantiles: bins is the device tensor series_hist returns")
    _metric_i32("series_quantiles", "bins", bins, bins, (65536 >> shift,))
    n, q = int(n), [float(v) for v in q]
    if not 0 < n < 1 << 31 or not 1 <= len(q) <= 8 or not all(0.0 <= v <= 100.0 for v in q):
        raise KoafError(f"series_quantiles: 0 < n < 2^31 and 1..8 percentiles within [0, 100], got n = {n}, q = {q}")
    pairs = [percentile_index(n, v) for v in q]
    if out is None:
        out = torch.empty(len(q), dtype=torch.float64, device=bins.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (len(q),) or out.device != bins.device:
        raise KoafError(f"series_quantiles: out is contiguous fp64 [{len(q)}] on the bins' device, got {tuple(out.shape)} {out.dtype}")
    ks = (ctypes.c_int64 * len(q))(*[p[0] for p in pairs])
    gs = (ctypes.c_double * len(q))(*[p[1] for p in pairs])
    check(lib().koaf_series_quantiles(_ptr(bins), shift, n, ctypes.addressof(ks), ctypes.addressof(gs), len(q), _ptr(out), _stream()),
          "series_quantiles")
    return out


def series_pack(x, limits, shift=3, margin=16, out_dtype=torch.uint8):
    """(R - 2m, C - 2m, S) uint8 / uint16 tensor: x (R, C, S) shifted right, clipped in fp64 to the device pair `limits` (what
    series_quantiles returned), truncated toward zero and cropped by `margin` >= 1 on the first two axes (koaf_series_pack)."""
    dt = _series_volume("series_pack", x, 3)
    shift = _series_shift("series_pack", shift)
    R, C, S = (int(v) for v in x.shape)
    margin = int(margin)
    if margin < 1 or 2 * margin >= R or 2 * margin >= C:
        raise KoafError(f"series_pack: margin {margin} of {R} x {C}: at least 1 (numpy's [0:-0] is empty) and below half of both")
    if x.numel() >= 1 << 31:
        raise KoafError(f"series_pack: fewer than 2^31 voxels, got {x.numel()}")
    if out_dtype not in (torch.uint8, torch.uint16):
        raise KoafError(f"series_pack: uint8 or uint16 output, got {out_dtype}")
    if not torch.is_tensor(limits) or limits.dtype != torch.float64 or tuple(limits.shape) != (2,) or limits.device != x.device \
            or not limits.is_contiguous():
        raise KoafError("series_pack: limits is a contiguous fp64 [2] tensor on x's device")
    out = torch.empty((R - 2 * margin, C - 2 * margin, S), dtype=out_dtype, device=x.device)
    check(lib().koaf_series_pack(x.data_ptr(), dt, R, C, S, shift, margin, _ptr(limits), out.data_ptr(),
                                 1 if out_dtype == torch.uint16 else 0, _stream()), "series_pack")
    return out


# ------------------------------------------------------------------------------------------------
# the clinical logistic-regression baseline (koaf_clin.hip)
# ------------------------------------------------------------------------------------------------
LOGREG_MAX_P = defines()["KOAF_LOGREG_MAX_P"]
CLIN_FLAG_TEXT = {1: "Input contains NaN or infinity", 2: "Found unknown categories during transform",
                  4: "This solver needs samples of at least 2 classes in the data, but the data contains only one class",
                  8: "a label other than 0 / 1, a negative sample weight or a fitting-row index outside the table"}


def clin_flag(device):
    """a zeroed flag word for clin_design / logreg_fit (koaf.h: bit 0 non-finite, 1 unknown category, 2 one class, 3 bad label)"""
    return torch.zeros(1, dtype=torch.int32, device=device)


def clin_raise(word):
    """the ValueError of a clin flag word read back from the device (scikit-learn raises one in each of these cases); 0 passes"""
    word = int(word) & 15
    if word:
        raise ValueError("; ".join(text for bit, text in CLIN_FLAG_TEXT.items() if word & bit))


def _clin_f64(what, name, t, shape=None, like=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() == 0 \
            or (shape is not None and tuple(t.shape) != tuple(shape)) or (like is not None and t.device != like.device):
        raise KoafError(f"{what}: {name} is a non-empty contiguous fp64 tensor{'' if shape is None else ' ' + str(list(shape))} on the HIP "
                        f"device, got {(tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t)}")


def clin_design(raw, ncat, cats, fit_idx=None, stats=None, flag=None):
    """The design matrix of a clinical table (koaf_clin_design): raw fp64 [V, n] holds one column per variable, ncat[v] is 0 for a
    continuous variable (StandardScaler: (x - mean) / population std, std 0 -> 1) and the number of categories otherwise
    (OneHotEncoder: one 0 / 1 column per entry of the sorted list cats[v], in that order).  stats None: mean and std are computed
    over the rows fit_idx (int32 device indices; None: all rows) and returned; stats [V, 2]: they are read.  -> (X [n, D], stats).
    flag: a clin_flag() word; None: an own word is read back here (a host sync), and a NaN / Inf or an unknown category raises
    ValueError as scikit-learn does."""
    _clin_f64("clin_design", "raw", raw)
    if raw.dim() != 2:
        raise KoafError(f"clin_design: raw is [V, n], got {tuple(raw.shape)}")
    V, n = int(raw.shape[0]), int(raw.shape[1])
    ncat = [int(c) for c in ncat]
    lists = [np.asarray(cats[v], np.float64).reshape(-1) if ncat[v] else np.zeros(0) for v in range(min(V, len(ncat)))]
    D = sum(c if c else 1 for c in ncat)
    if len(ncat) != V or V > 32 or D + 1 > LOGREG_MAX_P or any(c < 0 for c in ncat) or any(len(l) != c for l, c in zip(lists, ncat)):
        raise KoafError(f"clin_design: {V} variables with category counts {ncat} (D = {D}): at most 32 variables, D + 1 <= {LOGREG_MAX_P}, "
                        f"and one list of categories per categorical variable")
    for l in lists:
        if l.size and (np.isnan(l).any() or (np.diff(l) <= 0).any()):
            raise KoafError("clin_design: a category list is strictly increasing (np.unique)")
    fit = stats is None
    if fit:
        stats = torch.empty((V, 2), dtype=torch.float64, device=raw.device)
        if fit_idx is not None:
            _metric_i32("clin_design", "fit_idx", fit_idx, raw)
            if fit_idx.dim() != 1 or fit_idx.numel() == 0:
                raise KoafError("clin_design: fit_idx is a non-empty 1-D index vector")
    else:
        _clin_f64("clin_design", "stats", stats, (V, 2), raw)
    own = flag is None
    if own:
        flag = clin_flag(raw.device)
    _metric_i32("clin_design", "flag", flag, raw, (1,))
    X = torch.empty((n, D), dtype=torch.float64, device=raw.device)
    nc = (ctypes.c_int32 * V)(*ncat)
    flat = np.concatenate(lists) if lists else np.zeros(0)
    cs = (ctypes.c_double * max(1, flat.size))(*flat.tolist())
    nfit = int(fit_idx.numel()) if (fit and fit_idx is not None) else n
    check(lib().koaf_clin_design(_ptr(raw), n, V, ctypes.addressof(nc), ctypes.addressof(cs), _ptr(fit_idx) if fit else None, nfit,
                                 1 if fit else 0, _ptr(stats), _ptr(X), _ptr(flag), _stream()), "clin_design")
    if own:
        clin_raise(flag.item())
    return X, stats


def logreg_fit(X, y, sw, C=1.0, max_iter=100, tol=1e-10, out=None, flag=None):
    """K L2-penalised logistic regressions over the same rows in one launch (koaf_logreg_fit, one block per problem): X fp64
    [n, D], y int32 [n] of 0 / 1, sw fp64 [K, n] one sample-weight row per problem, a weight of 0 taking the row out of it.
    Damped Newton in fp64 on (1/S) sum s_i [log(1 + e^r_i) - y_i r_i] + |w|^2 / (2 C S) until |grad|_inf <= tol.
    -> (W [K, D + 1] with the intercept last, report [K, 4] = (steps, final |grad|_inf, final objective, step halvings)).
    out: a contiguous fp64 [K, D + 1] tensor to write W into.  flag as in clin_design (a one-class problem raises)."""
    _clin_f64("logreg_fit", "X", X)
    if X.dim() != 2:
        raise KoafError(f"logreg_fit: X is [n, D], got {tuple(X.shape)}")
    n, D = int(X.shape[0]), int(X.shape[1])
    if D + 1 > LOGREG_MAX_P or n < 2:
        raise KoafError(f"logreg_fit: at least 2 rows and D + 1 <= {LOGREG_MAX_P} columns with the intercept, got n = {n}, D = {D}")
    _metric_i32("logreg_fit", "y", y, X, (n,))
    _clin_f64("logreg_fit", "sw", sw, None, X)
    if sw.dim() != 2 or int(sw.shape[1]) != n:
        raise KoafError(f"logreg_fit: sw is [K, {n}], got {tuple(sw.shape)}")
    K = int(sw.shape[0])
    if not (float(C) > 0.0 and math.isfinite(float(C))) or int(max_iter) < 0 or not float(tol) >= 0.0:
        raise KoafError(f"logreg_fit: C > 0, max_iter >= 0 and tol >= 0, got {C}, {max_iter}, {tol}")
    if out is None:
        out = torch.empty((K, D + 1), dtype=torch.float64, device=X.device)
    else:
        _clin_f64("logreg_fit", "out", out, (K, D + 1), X)
    report = torch.empty((K, 4), dtype=torch.float64, device=X.device)
    own = flag is None
    if own:
        flag = clin_flag(X.device)
    _metric_i32("logreg_fit", "flag", flag, X, (1,))
    check(lib().koaf_logreg_fit(_ptr(X), _ptr(y), _ptr(sw), n, D, K, float(C), int(max_iter), float(tol), _ptr(out), _ptr(report),
                                _ptr(flag), _stream()), "logreg_fit")
    if own:
        clin_raise(flag.item())
    return out, report


def logreg_predict(W, Xt, y=None, mask=None, ensemble=False):
    """The K models W [K, D + 1] on the rows Xt [m, D] (koaf_logreg_predict) -> dict of decision [K, m], proba [K, m, 2] =
    (1 - p, p); with y (int32 [m]) and mask (int32 [K, m]) also logloss [K], sklearn.metrics.log_loss of model k over the rows its
    mask selects; with ensemble also ens_proba [m, 2], the mean over the K models, and ens_pred [m] (int32), its argmax."""
    _clin_f64("logreg_predict", "W", W)
    _clin_f64("logreg_predict", "Xt", Xt, None, W)
    if W.dim() != 2 or Xt.dim() != 2 or int(W.shape[1]) != int(Xt.shape[1]) + 1 or int(W.shape[1]) > LOGREG_MAX_P:
        raise KoafError(f"logreg_predict: W [K, D + 1] and Xt [m, D] with D + 1 <= {LOGREG_MAX_P}, got {tuple(W.shape)} and {tuple(Xt.shape)}")
    K, m, D = int(W.shape[0]), int(Xt.shape[0]), int(Xt.shape[1])
    if (y is None) != (mask is None):
        raise KoafError("logreg_predict: the log-loss needs both y and mask")
    dev = W.device
    res = {"decision": torch.empty((K, m), dtype=torch.float64, device=dev), "proba": torch.empty((K, m, 2), dtype=torch.float64, device=dev)}
    if y is not None:
        _metric_i32("logreg_predict", "y", y, W, (m,))
        _metric_i32("logreg_predict", "mask", mask, W, (K, m))
        res["logloss"] = torch.empty(K, dtype=torch.float64, device=dev)
    if ensemble:
        res["ens_proba"] = torch.empty((m, 2), dtype=torch.float64, device=dev)
        res["ens_pred"] = torch.empty(m, dtype=torch.int32, device=dev)
    check(lib().koaf_logreg_predict(_ptr(W), _ptr(Xt), m, D, K, _ptr(y), _ptr(mask), 1 if ensemble else 0, _ptr(res["decision"]),
                                    _ptr(res["proba"]), _ptr(res.get("logloss")), _ptr(res.get("ens_proba")), _ptr(res.get("ens_pred")),
                                    _stream()), "logreg_predict")
    return res


# ------------------------------------------------------------------------------------------------
# input plumbing
# ------------------------------------------------------------------------------------------------
def slice_fold(x, B, R, Cc, S):
    out = _empty((B * S, R, Cc), x)
    check(lib().koaf_slice_fold(_ptr(x), _ptr(out), B, R, Cc, S, _stream()), "slice_fold")
    return out


def slice_unfold(g, B, R, Cc, S):
    """"(b s) r c -> b r c s": g [B*S,R,C] -> [B,R,C,S], the transpose of slice_fold (its backward)"""
    out = _empty((B, R, Cc, S), g)
    check(lib().koaf_slice_unfold(_ptr(g), _ptr(out), B, R, Cc, S, _stream()), "slice_unfold")
    return out


def rowdot(a, b):
    """per-sample sum(a * b) of two contiguous fp32 tensors of one shape (B, ...) -> [B] (koaf_rowdot: fixed-order, no atomics)"""
    if tuple(a.shape) != tuple(b.shape) or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise KoafError(f"rowdot: two fp32 tensors of one shape, got {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
    a, b = a.contiguous(), b.contiguous()
    B = int(a.shape[0])
    n = a.numel() // B
    out = _empty((B,), a)
    ws = torch.empty(B * lib().koaf_rowdot_ws(n) // 2, device=a.device, dtype=torch.float64)      # (the fp64 block sums)
    check(lib().koaf_rowdot(_ptr(a), _ptr(b), B, n, _ptr(out), _ptr(ws), _stream()), "rowdot")
    return out


def resize(x, out_size):
    """F.interpolate(x, size given as recompute_scale_factor computes it, linear | bilinear | trilinear, align_corners=False) of
    a contiguous fp32 (B, CH, d0[, d1[, d2]]) tensor -> (B, CH, *out_size)  (koaf_resize)"""
    nd = x.dim() - 2
    if nd < 1 or nd > 3 or len(out_size) != nd:
        raise KoafError(f"resize: (B, CH, 1..3 spatial dims) tensors, got {tuple(x.shape)} -> {tuple(out_size)}")
    out = _empty(tuple(x.shape[:2]) + tuple(int(v) for v in out_size), x)
    ins = (ctypes.c_int32 * nd)(*[int(v) for v in x.shape[2:]])
    outs = (ctypes.c_int32 * nd)(*[int(v) for v in out_size])
    check(lib().koaf_resize(_ptr(x), _ptr(out), int(x.shape[0]) * int(x.shape[1]), nd, ctypes.addressof(ins), ctypes.addressof(outs),
                            _stream()), "resize")
    return out


def downscale2(x, B, R, Cc, S, fs):
    out = _empty((B, R // 2, Cc // 2, S // fs), x)
    check(lib().koaf_downscale2(_ptr(x), _ptr(out), B, R, Cc, S, fs, _stream()), "downscale2")
    return out


# ------------------------------------------------------------------------------------------------
# transformer pieces
# ------------------------------------------------------------------------------------------------
_WIDEN = {torch.uint8: 1, torch.uint16: 2, torch.int16: 3}


def widen(x):
    """uint8 / uint16 / int16 device tensor -> fp32 (koaf_widen); fp32 passes through"""
    if x.dtype == torch.float32:
        return x
    if x.dtype not in _WIDEN or not x.is_cuda:
        raise KoafError(f"widen: uint8 / uint16 / int16 tensors on the HIP device, got {x.dtype} on {x.device}")
    x = x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    check(lib().koaf_widen(x.data_ptr(), _WIDEN[x.dtype], _ptr(y), x.numel(), _stream()), "widen")
    return y


def minmax(x, B):
    """per-sample (min, max) of a contiguous batch -> [B, 2]"""
    n = x.numel() // B
    mm = _empty((B, 2), x)
    ws = _empty((B * lib().koaf_minmax_ws(n),), x)
    check(lib().koaf_minmax(_ptr(x), B, n, _ptr(mm), _ptr(ws), _stream()), "minmax")
    return mm


def augment(x, mm, params, B, R, C, S, mean, std):
    y = torch.empty_like(x)
    check(lib().koaf_augment(_ptr(x), _ptr(y), _ptr(mm), _ptr(params), B, R, C, S, mean, std, _stream()), "augment")
    return y


_STORED = {torch.float32: 0, **_WIDEN}


def _upload_bytes(host, dev):
    """a small host uint8 array -> device tensor on torch's current stream, through pinned memory and without waiting: a pageable
    copy makes the host wait for everything the stream still holds, once per batch.  The pinned block comes from torch's caching
    host allocator, which does not hand it out again before the copy has run."""
    pin = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    pin.numpy()[:] = host
    return pin.to(dev, non_blocking=True)


class HostWindowTable(object):
    """The host form of the per-sample table of koaf.h (8 x int64 per sample) with, optionally, the (cos, sin, exponent, rotated)
    rows of ops.augment behind it in the same bytes: built and CHECKED once by `window_rows`, then `upload(volumes)` fills in the
    addresses of this batch's volumes and sends everything in one pinned copy.  A transform whose geometry does not change from
    batch to batch (validation: centre crop, nothing random) keeps one of these per (stored shapes, flip pattern)."""

    def __init__(self, rows, prm, shapes, dtype, dense_step, win):
        B = rows.shape[0]
        self.buf = np.empty(64 * B + (16 * B if prm is not None else 0), dtype=np.uint8)
        self.rows = self.buf[:64 * B].view(np.int64).reshape(B, 8)
        self.rows[:] = rows
        self.prm = None
        if prm is not None:
            self.prm = self.buf[64 * B:].view(np.float32).reshape(B, 4)
            self.prm[:] = prm
        self.B, self.shapes, self.dtype, self.win = B, shapes, dtype, win
        self.offsets = None if dense_step is None else np.arange(B, dtype=np.int64) * dense_step      # dense: bytes from sample 0

    def upload(self, volumes):
        """volumes: the tensor / list of tensors the table was built for, or others of the same shapes and dtype
        -> (table [B, 8] int64 on the device, dtype code, (R, C, S)[, params [B, 4] fp32 on the device])"""
        B = self.B
        if self.offsets is not None:
            v0 = volumes
            if tuple(volumes.shape) != self.shapes or not volumes.is_contiguous():
                raise KoafError(f"window_table: built for one contiguous tensor {self.shapes}, got {tuple(volumes.shape)}")
            self.rows[:, 0] = self.offsets
            self.rows[:, 0] += volumes.data_ptr()
        else:
            v0 = volumes[0]
            if len(volumes) != B:
                raise KoafError(f"window_table: built for {B} volumes, got {len(volumes)}")
            for b, v in enumerate(volumes):
                if tuple(v.shape) != self.shapes[b] or v.dtype != self.dtype or v.device != v0.device or not v.is_contiguous():
                    raise KoafError(f"window_table: volume {b} is not the contiguous {self.shapes[b]} {self.dtype} tensor the table was built for")
                self.rows[b, 0] = v.data_ptr()
        if v0.dtype != self.dtype or not v0.is_cuda:
            raise KoafError(f"window_table: {self.dtype} volumes on the HIP device, got {v0.dtype} on {v0.device}")
        both = _upload_bytes(self.buf, v0.device)
        table = both[:64 * B].view(torch.int64).view(B, 8)
        if self.prm is None:
            return table, _STORED[self.dtype], self.win
        return table, _STORED[self.dtype], self.win, both[64 * B:].view(torch.float32).view(B, 4)


def window_rows(volumes, origins, masks, window, params=None):
    """-> HostWindowTable for `volumes` (see window_table for the arguments): every window is checked against its volume HERE, on
    the host -- the kernels follow the addresses"""
    nd = len(window)
    dense = torch.is_tensor(volumes)
    B = int(volumes.shape[0]) if dense else len(volumes)
    if nd not in (2, 3) or B < 1 or len(origins) != B or len(masks) != B:
        raise KoafError(f"window_table: a (R, C[, S]) window and one origin and mask per volume, got {tuple(window)} for {B} volumes")
    win = tuple(int(v) for v in window) + (1,) * (3 - nd)
    dt = volumes.dtype if dense else volumes[0].dtype
    if dt not in _STORED:
        raise KoafError(f"window_table: fp32 / uint8 / uint16 / int16 volumes, got {dt}")
    rows = np.zeros((B, 8), dtype=np.int64)
    rows[:, 1:4] = 1
    if dense:
        if volumes.dim() < nd + 1 or volumes.numel() != B * math.prod(volumes.shape[-nd:]):
            raise KoafError(f"window_table: one contiguous (B, 1, ...) tensor of {nd} stored axes, got {tuple(volumes.shape)}")
        rows[:, 1:1 + nd] = tuple(volumes.shape[-nd:])
        shapes, step = tuple(volumes.shape), volumes.numel() // B * volumes.element_size()
    else:
        for b, v in enumerate(volumes):
            sp = v.shape[-nd:]
            if len(sp) != nd or v.numel() != math.prod(sp):
                raise KoafError(f"window_table: volumes of {nd} axes behind axes of size 1, got {tuple(v.shape)}")
            rows[b, 1:1 + nd] = sp
        shapes, step = [tuple(v.shape) for v in volumes], None
    rows[:, 4:4 + nd] = np.asarray(origins, dtype=np.int64).reshape(B, nd)
    rows[:, 7] = np.asarray(masks, dtype=np.int64)
    sp, org = rows[:, 1:4], rows[:, 4:7]
    last = org + (1 - 2 * ((rows[:, 7:8] >> np.arange(3)) & 1)) * (np.asarray(win, dtype=np.int64) - 1)
    ok = (org >= 0) & (org < sp) & (last >= 0) & (last < sp)
    if min(win) < 1 or not ok.all() or (rows[:, 7] >> nd).any() or (rows[:, 7] < 0).any():
        b = int(np.argmin(ok.all(1)))
        raise KoafError(f"window_table: window {win} from origin {org[b].tolist()} (backwards mask {int(rows[b, 7])}) leaves the stored "
                        f"volume {sp[b].tolist()} of sample {b}")
    if params is not None:
        params = np.asarray(params, dtype=np.float32)
        if params.shape != (B, 4):
            raise KoafError(f"window_table: params is one (cos, sin, exponent, rotated) row per volume, got {params.shape}")
    return HostWindowTable(rows, params, shapes, dt, step, win)


def window_table(volumes, origins, masks, window, params=None):
    """The per-sample device table koaf_window_minmax / koaf_input_pipeline read the stored volumes through (koaf.h): `volumes`
    is B contiguous device tensors of one dtype (fp32 / uint8 / uint16 / int16), each (R0, C0[, S0]) behind leading axes of
    size 1 -- or ONE contiguous tensor (B, 1, R0, C0[, S0]), whose samples are addressed in place; `origins` [B][nd] the stored
    index of window voxel 0 per axis, `masks` [B] the bit mask of the axes walked backwards (1 = R, 2 = C, 4 = S), `window` =
    (R, C[, S]).  Every window is checked against its volume on the host (window_rows) and the table goes up in one pinned copy.
    -> (table [B, 8] int64 on the device, dtype code, (R, C, S)); keep the volumes alive until the kernels that read them have
    run.  With `params` (B rows of (cos, sin, exponent, rotated), what ops.augment takes) those travel in the same copy and come
    back as a fourth element, [B, 4] fp32 on the device."""
    return window_rows(volumes, origins, masks, window, params).upload(volumes)


@functools.lru_cache(maxsize=None)
def _window_ws(n):
    return int(lib().koaf_window_minmax_ws(n))


def window_minmax(table, dtype, window):
    """per-sample (min, max) over the R x C x S window of the stored volumes, straight from the stored type -> [B, 2] fp32
    (koaf_window_minmax; `table, dtype, window` as window_table returns them)"""
    B, (R, C, S) = int(table.shape[0]), window
    nws = B * _window_ws(R * C * S)
    buf = torch.empty((nws + 2 * B,), device=table.device, dtype=torch.float32)          # the partials, then the result
    mm = buf[nws:].view(B, 2)
    check(lib().koaf_window_minmax(_ptr(table), dtype, B, R, C, S, _ptr(mm), _ptr(buf), _stream()), "window_minmax")
    return mm


def input_pipeline(table, dtype, window, mm, params, mean, std, pool=1, pool_s=1, layout="rcs"):
    """stored volumes -> mean over pool x pool x pool_s of ((gamma(rotate(unit(window)))) - mean) / std, fp32
    (koaf_input_pipeline): (B, R/pool, C/pool, S/pool_s) for layout "rcs", (B, S/pool_s, R/pool, C/pool) for "ncdhw".
    mm [B, 2] as window_minmax leaves it, params [B, 4] as ops.augment takes them."""
    if layout not in ("rcs", "ncdhw"):
        raise KoafError(f"input_pipeline: layout is 'rcs' or 'ncdhw', got {layout!r}")
    B, (R, C, S) = int(table.shape[0]), window
    if pool not in (1, 2) or pool_s not in (1, 2) or R % pool or C % pool or S % pool_s:
        raise KoafError(f"input_pipeline: pools of 1 or 2 that divide the window, got {pool}, {pool_s} for {window}")
    shape = (B, S // pool_s, R // pool, C // pool) if layout == "ncdhw" else (B, R // pool, C // pool, S // pool_s)
    y = torch.empty(shape, device=table.device, dtype=torch.float32)
    check(lib().koaf_input_pipeline(_ptr(table), dtype, _ptr(y), _ptr(mm), _ptr(params), B, R, C, S, pool, pool_s,
                                    1 if layout == "ncdhw" else 0, mean, std, _stream()), "input_pipeline")
    return y


def linear_fwd(x, w, b, M, N, K, residual=None):
    L = lib()
    y = _empty((M, N), x)
    n = L.koaf_linear_ws(M, N, K)
    ws = _empty((n,), x) if n > 0 else None
    e0 = _prof_begin()
    check(L.koaf_linear_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(residual), _ptr(y), _ptr(ws), M, N, K, _stream()),
          "linear_fwd")
    _prof_end(e0, "gemm", 2.0 * M * N * K, f"linear_fwd M{M} N{N} K{K}",
              M * K + N * K + M * N * (2 if residual is not None else 1))
    return y


def linear_dgrad(dy, w, M, N, K, residual=None):
    L = lib()
    dx = _empty((M, K), dy)
    n = L.koaf_linear_ws(M, K, N)
    ws = _empty((n,), dy) if n > 0 else None
    e0 = _prof_begin()
    check(L.koaf_linear_dgrad(_ptr(dy), _ptr(w), _ptr(residual), _ptr(dx), _ptr(ws), M, N, K, _stream()),
          "linear_dgrad")
    _prof_end(e0, "gemm", 2.0 * M * N * K, f"linear_dgrad M{M} N{N} K{K}",
              M * N + N * K + M * K * (2 if residual is not None else 1))
    return dx


def linear_wgrad(dy, x, dw, db, M, N, K):
    L = lib()
    ws = None
    if db is not None:
        n = L.koaf_colsum_ws(M, N)
        ws = _empty((n,), dy) if n > 0 else None
    e0 = _prof_begin()
    check(L.koaf_linear_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), M, N, K, _stream()), "linear_wgrad")
    _prof_end(e0, "gemm", 2.0 * M * N * K, f"linear_wgrad M{M} N{N} K{K}", M * N + M * K + N * K)


def layernorm_fwd(x, gamma, beta, rows, D, eps):
    y = torch.empty_like(x)
    mean = _empty((rows,), x)
    rstd = _empty((rows,), x)
    check(lib().koaf_layernorm_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), rows, D, eps,
                                   _stream()), "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, rows, D):
    L = lib()
    dx = torch.empty_like(x)
    n = L.koaf_layernorm_bwd_ws(rows, D)
    if n < 0:
        raise KoafError(f"layernorm_bwd: unsupported D={D}")
    part = _empty((n,), x)
    check(L.koaf_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dgamma),
                               _ptr(dbeta), _ptr(part), rows, D, _stream()), "layernorm_bwd")
    return dx


def attention_fwd(qkv, B, n, h, d, scale):
    attn = _empty((B, h, n, n), qkv)
    out = _empty((B, n, h * d), qkv)
    e0 = _prof_begin()
    check(lib().koaf_attention_fwd(_ptr(qkv), _ptr(attn), _ptr(out), B, n, h, d, scale, _stream()), "attention_fwd")
    _prof_end(e0, "gemm", 4.0 * B * h * n * n * d, f"attn_fwd B{B} n{n}", B * n * h * d * 4 + B * h * n * n)
    return out, attn


def attention_bwd(dout, qkv, attn, B, n, h, d, scale):
    dqkv = torch.empty_like(qkv)
    ws = torch.empty_like(attn)
    e0 = _prof_begin()
    check(lib().koaf_attention_bwd(_ptr(dout), _ptr(qkv), _ptr(attn), _ptr(dqkv), _ptr(ws), B, n, h, d, scale,
                                   _stream()), "attention_bwd")
    _prof_end(e0, "gemm", 8.0 * B * h * n * n * d, f"attn_bwd B{B} n{n}", B * n * h * d * 7 + B * h * n * n)
    return dqkv


def gelu_fwd(x):
    y = torch.empty_like(x)
    check(lib().koaf_gelu_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), "gelu_fwd")
    return y


def gelu_bwd(dy, x):
    dx = torch.empty_like(x)
    check(lib().koaf_gelu_bwd(_ptr(dy), _ptr(x), _ptr(dx), x.numel(), _stream()), "gelu_bwd")
    return dx


def relu_fwd(x):
    y = torch.empty_like(x)
    check(lib().koaf_relu_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), "relu_fwd")
    return y


def relu_bwd(dy, y):
    dx = torch.empty_like(y)
    check(lib().koaf_relu_bwd(_ptr(dy), _ptr(y), _ptr(dx), y.numel(), _stream()), "relu_bwd")
    return dx


def dropout(x, p, seed, epoch=None):
    """epoch: optional int64 device scalar folded into the seed (functional.DeviceStepState)"""
    y = torch.empty_like(x)
    check(lib().koaf_dropout(_ptr(x), _ptr(y), x.numel(), p, seed, _ptr(epoch), _stream()), "dropout")
    return y


def dropout2d(x, N, HW, C, p, seed, epoch=None):
    y = torch.empty_like(x)
    check(lib().koaf_dropout2d(_ptr(x), _ptr(y), N, HW, C, p, seed, _ptr(epoch), _stream()), "dropout2d")
    return y


def counter_add(counter, delta=1):
    """counter (int64 device scalar) += delta, on the stream (a graph node when the step is captured)"""
    check(lib().koaf_counter_add(_ptr(counter), delta, _stream()), "counter_add")


def add(a, b):
    out = torch.empty_like(a)
    check(lib().koaf_add(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()), "add")
    return out


def colsum(x, out, rows, C, what="colsum"):
    """out [C] = column sums of x [rows][C] (bias-like gradients)"""
    L = lib()
    n = L.koaf_colsum_ws(rows, C)
    ws = _empty((n,), x) if n > 0 else None
    check(L.koaf_colsum(_ptr(x), _ptr(out), rows, C, _ptr(ws), _stream()), what)


def softmax_rows_(x):
    """in-place row softmax of a contiguous fp32 (rows, n) device tensor"""
    check(lib().koaf_softmax_rows(_ptr(x), x.shape[0], x.shape[1], _stream()), "softmax_rows")
    return x


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


def _rup(v, a):
    return (v + a - 1) // a * a


def wplane_entry(R, taps, C, src_off=0, f_off=0, tile0=0):
    """-> (KoafWPlane, nf, nd, ntiles): the table entry of one weight [R][taps][C] (koaf.h koaf_wplanes_build) whose F image
    (nf 16-bit elements) starts at f_off and whose D image (nd elements) follows at the next multiple of 64, and the tiles
    it adds to the table's running count"""
    Kp, Rp = _rup(taps * C, 32), _rup(R, 32)
    nf, nd = 2 * R * Kp, 2 * C * taps * Rp
    ent = KoafWPlane(src_off=src_off, f_off=f_off, d_off=f_off + _rup(nf, 64), tile0=tile0, R=R, taps=taps, C=C, Kp=Kp, Rp=Rp)
    return ent, nf, nd, (Rp // 32) * taps * (_rup(C, 32) // 32)


def wplanes_build(base, planes, amax, table, n, ntiles):
    """cut the plane images of the `n` weights that `table` (device bytes of KoafWPlane entries) describes: floats from `base`,
    images into `planes` (int16), max |w| per weight into `amax`"""
    if not planes.is_cuda or planes.dtype != torch.int16:
        raise KoafError("weight plane images are int16 (fp16 bit patterns) tensors on the HIP device")
    check(lib().koaf_wplanes_build(_ptr(base), planes.data_ptr(), _ptr(amax), ctypes.cast(_ptr(table), ctypes.POINTER(KoafWPlane)),
                                   n, ntiles, _stream()), "wplanes_build")


def build_weight_planes(w, R, taps, C):
    """(F, D, amax) fp16 plane images (int16 tensors) + device scalar max |w| of ONE weight w [R][taps][C] (packed conv
    weight): what arena.ParamArena keeps for every convolution weight of a model, for callers without an arena (tests,
    micro-benchmarks)."""
    ent, nf, nd, ntiles = wplane_entry(R, taps, C)
    planes = torch.zeros(ent.d_off + nd, device=w.device, dtype=torch.int16)
    amax = torch.zeros(1, device=w.device, dtype=torch.float32)
    tab = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).to(w.device)
    wplanes_build(w, planes, amax, tab, 1, ntiles)
    return planes[:nf], planes[ent.d_off:ent.d_off + nd], amax


def gemm(desc: KoafGemm):
    check(lib().koaf_gemm(ctypes.byref(desc), _stream()), "gemm")
