"""BatchNorm, its backward recipe BnApply, the column statistics, max-pool and global average pool (koaf_bn.hip)."""
import ctypes

import torch

from .._lib import KoafBnApply, KoafError, check, lib
from ._base import _act16, _empty, _grads32, _i32, _ptr, _stream, conv_out


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
        act16 = _act16("bn_bwd_apply", c=self.c)
        _grads32("bn_bwd_apply", dz=self.dz, out=out)
        dc = out if out is not None else torch.empty(self.c.shape, device=self.c.device, dtype=torch.float32)
        amax = torch.zeros(1, device=self.c.device, dtype=torch.float32) if want_amax else None
        check(lib().koaf_bn_bwd_apply(_ptr(self.dz), _ptr(self.c), _ptr(self.mean), _ptr(self.coef), _ptr(dc), self.rows, self.C,
                                      _ptr(amax), act16, _stream()), "bn_bwd_apply")
        if want_amax:
            dc._koaf_amax = amax
        return dc


def _dy_args(dy, dy_amax):
    """(dy pointer, dy_amax pointer, KoafBnApply* or None, reference tensor) of a gradient given as a tensor or as a BnApply"""
    if isinstance(dy, BnApply):
        return None, None, dy.struct(), dy.dz
    return _ptr(dy), _ptr(dy_amax), None, dy


def _colpart_rows(rows, C, what):
    """partial rows of the column reductions (koaf_colpart_rows); a width their geometry does not cover (C % 4, C / 4 not a
    divisor of 256 up to 1024, beyond it not a multiple of 1024) is refused here, before any tensor is sized from it"""
    n = lib().koaf_colpart_rows(rows, C)
    if n < 0:
        raise KoafError(f"{what}: unsupported C={C}")
    return n


def colstats(x, rows, C, shift=None):
    L = lib()
    act16 = _act16("colstats", x=x)
    part = _empty((_colpart_rows(rows, C, "colstats"), 2, C), x)      # (fp32 whatever the storage type of x)
    r = _i32(0)
    check(L.koaf_colstats(_ptr(x), rows, C, _ptr(part), ctypes.addressof(r), _ptr(shift), act16, _stream()), "colstats")
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
    act16 = _act16("bn_add_relu", c=c, idt=idt, out=out)
    y = out if out is not None else torch.empty_like(c)
    check(lib().koaf_bn_add_relu(_ptr(c), _ptr(saved[2]), _ptr(saved[3]), _ptr(idt),
                                 _ptr(idsaved[2]) if idsaved is not None else None,
                                 _ptr(idsaved[3]) if idsaved is not None else None, _ptr(y), rows, C, act16, _stream()),
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
    act16 = _act16("bn_bwd", c=c, ymask=ymask)
    _grads32("bn_bwd", g=g, dz_out=dz_out, dc_out=dc_out, **({} if pool is None else {"pool[0]": pool[0]}))
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
                                        _ptr(dz), _ptr(part), ctypes.addressof(r), pN, pH, pW, C, _ptr(dzmax), act16, _stream()),
              "bn_bwd_reduce_pool")
        return _bn_bwd_tail(part[:r.value], 2, 1, dz, c, saved, rows, C, count, dgamma, dbeta, dc_out, fused, dzmax, train)
    if mask_mode != 0 and dz_out is None:
        dz_out = g  # mask in place
    part = _empty((_colpart_rows(rows, C, "bn_bwd_reduce"), 2, C), g)
    r = _i32(0)
    dzmax = _empty((1,), g) if fused else None
    check(L.koaf_bn_bwd_reduce(_ptr(g), _ptr(c), _ptr(ymask), _ptr(saved[2]), _ptr(saved[3]), _ptr(saved[0]),
                               _ptr(saved[1]), mask_mode, _ptr(dz_out), _ptr(part), ctypes.addressof(r), rows, C,
                               _ptr(dzmax), act16, _stream()), "bn_bwd_reduce")
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
    check(L.koaf_bn_bwd_apply(_ptr(dz), _ptr(c), _ptr(saved[0]), _ptr(coef), _ptr(dc), rows, C, None, _act16("bn_bwd_apply", c=c), _stream()),
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
    act16 = _act16("maxpool_fwd", c=c)
    y = _empty((N, OH, OW, C), c, dtype=c.dtype)
    am = _empty((N, OH, OW, C), c, dtype=torch.uint8)
    check(lib().koaf_maxpool_fwd(_ptr(c), _ptr(saved[2]), _ptr(saved[3]), _ptr(y), _ptr(am), N, H, W, C, act16, _stream()),
          "maxpool_fwd")
    return y, am


def maxpool_bwd(dy, am, N, H, W, C):
    da = _empty((N, H, W, C), dy)
    check(lib().koaf_maxpool_bwd(_ptr(dy), _ptr(am), _ptr(da), N, H, W, C, _stream()), "maxpool_bwd")
    return da


def gap_fwd(y, N, HW, C):
    act16 = _act16("gap_fwd", y=y)
    out = _empty((N, C), y)
    check(lib().koaf_gap_fwd(_ptr(y), _ptr(out), N, HW, C, act16, _stream()), "gap_fwd")
    return out


def gap_bwd(dout, N, HW, C):
    dy = _empty((N, HW, C), dout)
    check(lib().koaf_gap_bwd(_ptr(dout), _ptr(dy), N, HW, C, _stream()), "gap_bwd")
    return dy
