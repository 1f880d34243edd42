"""Convolutions: dense (koaf_conv.hip over the koaf_gemm*.hip kernels, koaf_wgrad1.hip, koaf_wgrad3.hip), grouped 3x3, the stem
(koaf_stem.hip), the activation / weight plane images they read (koaf_planes.hip) and the raw GEMM descriptor call."""
import ctypes
import os

import torch

from .._lib import KoafBnb, KoafEmit, KoafError, KoafGemm, KoafLaunchRec, KoafTail, KoafWImg, KoafWPlane, check, defines, lib
from ._base import _a16, _act16, _empty, _grads32, _i32, _prof_begin, _prof_end, _ptr, _stream, conv_out
from .bn import BnApply, _dy_args

# Convolutions run on the fp16 contraction scheme (koaf.h: KoafGemm.fmt 1) whenever their operands' scales are known
# (weights: arena plane images; gradients: the amax the BatchNorm backward leaves behind).  KOAF_CONV_FMT=bf16 keeps them
# on the bf16 x 3 scheme for A/B runs.
CONV_F16 = os.environ.get("KOAF_CONV_FMT", "f16") != "bf16"
# The gathered (3x3) convolution kernels read activation plane images (koaf_act_planes) wherever use_aplanes says they pay; the
# aplanes= arguments below override that per call (False: the fp32 loaders).  A convolution's forward images are kept for its
# weight gradient only where the caller asks (keep_planes=): keeping them everywhere fragments the caching allocator's pool.
ACT_SCALE = defines()["KOAF_ACT_SCALE"]      # the fixed activation scale of the fp16 scheme (koaf.h)


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


def act_planes(x, npix, C, tf=0, sc=None, sh=None, x2=None, sc2=None, amax=None, fscale=0.0):
    """fp16 piece planes [2][npix][C] (+ the zero chunk) of x (tf 0), relu(sc*x+sh) (tf 1) or sc*x + sh - sc2*x2 (tf 2), times
    the operand scale (scale(*amax) or fscale): the A operand of the gathered convolution kernels (koaf.h koaf_act_planes)."""
    L = lib()
    if tf == 2:         # x is the gradient dz (fp32), x2 the conv output c in either storage
        _grads32("act_planes", x=x)
        act16 = _act16("act_planes", x2=x2)
    else:               # x is the activation, in either storage; there is no second source
        if x2 is not None:
            raise KoafError(f"act_planes: x2 belongs to tf 2, got it with tf {tf}")
        act16 = _act16("act_planes", x=x)
    out = torch.empty(L.koaf_act_planes_elems(npix, C), device=x.device, dtype=torch.int16)
    check(L.koaf_act_planes(_ptr(x), _ptr(x2), npix, C, tf, _ptr(sc), _ptr(sh), _ptr(sc2), _ptr(amax), float(fscale),
                            out.data_ptr(), act16, _stream()), "act_planes")
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
    "koaf_gemm/stream", "/emit", "/halo", "/halo128", "/t2d"; "koaf_fwd1": the 256-row kernel of the dense 1x1 forward convolutions,
    grid_x = min(tiles, 256) where its blocks walk; "koaf_wgrad3/ring": the 3x3 weight-gradient ring kernel, splitk = its
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
# weight plane images, the raw GEMM
# ------------------------------------------------------------------------------------------------
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
