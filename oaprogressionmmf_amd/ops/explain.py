"""Explanations: class-activation maps (koaf_cam.hip), the path attributions -- integrated gradients, SmoothGrad
(koaf_attr.hip) --, the occlusion maps (koaf_occl.hip), the modality coalitions and their Shapley values (koaf_coal.hip) and the
attention relevance of the fusion transformers (koaf_attnrel.hip)."""
import ctypes

import torch

from .._lib import KoafError, check, defines, lib
from ._base import _a16, _ptr, _stream, check_tensor, out_buffer


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
# occlusion sensitivity maps (koaf_occl.hip)
# ------------------------------------------------------------------------------------------------
def _occl_box(what, shape, window, strides):
    """the three host arrays of four the entry points take, from the extents behind the batch dimension (padded in front with
    ones)"""
    dims = tuple(int(d) for d in shape)
    window, strides = tuple(int(w) for w in window), tuple(int(s) for s in strides)
    if not 1 <= len(dims) <= 4 or len(window) != len(dims) or len(strides) != len(dims):
        raise KoafError(f"{what}: one to four extents behind the batch dimension, a window and strides of that rank, got {dims}, "
                        f"{window}, {strides}")
    if not all(1 <= s <= w <= d for d, w, s in zip(dims, window, strides)):
        raise KoafError(f"{what}: 1 <= strides <= window <= extents, got {strides}, {window}, {dims}")
    pad = (1,) * (4 - len(dims))
    return tuple((ctypes.c_int32 * 4)(*(pad + v)) for v in (dims, window, strides))


def occl_points(x, window, strides, k0, J, base=None):
    """out[j] = x with window k0 + j set to the baseline -> [J, *x.shape] (koaf_occl_points: x and base read once for all J).
    window / strides: one entry per dimension of x behind the batch; base as in path_points."""
    B, n, bt, bv = _attr_rows("occl_points", x, base)
    dims, win, st = _occl_box("occl_points", x.shape[1:], window, strides)
    out = torch.empty((int(J),) + tuple(x.shape), device=x.device, dtype=torch.float32)
    check(lib().koaf_occl_points(_ptr(x), _ptr(bt), bv, _ptr(out), int(J), B, dims, win, st, int(k0), _stream()), "occl_points")
    return out


def occl_slices(x, rows, window, strides, K_img, H, W, img_strides, base=None):
    """[nrows, 1, H, W]: image n of x with window k set to the baseline for every (k, n) of the device int32 table rows [nrows, 2],
    n = b * K_img + kk; img_strides = (sb, sk, si, sj) as run.cam_strides gives them (koaf_occl_slices: what the slice fold of
    the occluded input would hand the trunk, gathered straight from x)."""
    B, n, bt, bv = _attr_rows("occl_slices", x, base)
    dims, win, st = _occl_box("occl_slices", x.shape[1:], window, strides)
    check_tensor("occl_slices", "rows", rows, torch.int32, like=x, nonempty=True, where="x's device")
    if rows.dim() != 2 or rows.shape[1] != 2:
        raise KoafError(f"occl_slices: rows is [nrows, 2], got {tuple(rows.shape)}")
    sb, sk, si, sj = (int(s) for s in img_strides)
    out = torch.empty((int(rows.shape[0]), 1, int(H), int(W)), device=x.device, dtype=torch.float32)
    check(lib().koaf_occl_slices(_ptr(x), _ptr(bt), bv, _ptr(out), _ptr(rows), int(rows.shape[0]), B, dims, win, st, int(K_img), int(H),
                                 int(W), sb, sk, si, sj, _stream()), "occl_slices")
    return out


def occl_rows(cache, fresh, src):
    """out [J, N, ...]: out[j][n] = fresh[src[j][n]] where src[j][n] >= 0, else cache[n] (koaf_occl_rows: a byte copy of whole
    rows).  cache [N, ...] and fresh [F, ...] are contiguous, of one dtype and one row shape; fresh may be None (F = 0);
    src: device int32 [J, N]."""
    if not torch.is_tensor(cache) or not cache.is_contiguous() or cache.dim() < 1 or cache.numel() == 0:
        raise KoafError("occl_rows: cache is a contiguous, non-empty tensor [N, ...]")
    N = int(cache.shape[0])
    row_bytes = cache.numel() // N * cache.element_size()
    F = 0
    if fresh is not None:
        if not fresh.is_contiguous() or fresh.dtype != cache.dtype or fresh.device != cache.device or tuple(fresh.shape[1:]) != tuple(cache.shape[1:]):
            raise KoafError(f"occl_rows: fresh is contiguous [F, *{tuple(cache.shape[1:])}] {cache.dtype} on cache's device, got "
                            f"{tuple(fresh.shape)} {fresh.dtype}")
        F = int(fresh.shape[0])
    check_tensor("occl_rows", "src", src, torch.int32, like=cache, nonempty=True, where="cache's device")
    if src.dim() != 2 or src.shape[1] != N:
        raise KoafError(f"occl_rows: src is [J, {N}], got {tuple(src.shape)}")
    if row_bytes % 4:
        raise KoafError(f"occl_rows: rows of {row_bytes} bytes are no multiple of 4")
    J = int(src.shape[0])
    out = torch.empty((J,) + tuple(cache.shape), device=cache.device, dtype=cache.dtype)
    check(lib().koaf_occl_rows(_ptr(cache), _ptr(fresh) if F else None, _ptr(src), _ptr(out), J, N, F, row_bytes, _stream()), "occl_rows")
    return out


def occl_fold(delta, shape, window, strides):
    """the occlusion map [B, *shape] of the score differences delta [K, B]: per element the mean of delta[k] over the windows that
    cover it, summed in ascending k (koaf_occl_fold).  shape / window / strides: the extents behind the batch dimension."""
    check_tensor("occl_fold", "delta", delta, torch.float32, nonempty=True)
    if delta.dim() != 2:
        raise KoafError(f"occl_fold: delta is [K, B], got {tuple(delta.shape)}")
    dims, win, st = _occl_box("occl_fold", shape, window, strides)
    K, B = (int(s) for s in delta.shape)
    out = torch.empty((B,) + tuple(int(d) for d in shape), device=delta.device, dtype=torch.float32)
    check(lib().koaf_occl_fold(_ptr(delta), _ptr(out), K, B, dims, win, st, _stream()), "occl_fold")
    return out


# ------------------------------------------------------------------------------------------------
# modality coalitions and their Shapley values (koaf_coal.hip)
# ------------------------------------------------------------------------------------------------
COAL_MAX_M = defines()["KOAF_COAL_MAX_M"]


def _host_ints(what, name, seq):
    """a host table (a sequence, a numpy array or a CPU tensor of integers) as a list of python ints"""
    try:
        vals = seq.tolist() if hasattr(seq, "tolist") else list(seq)
        if any(isinstance(v, bool) or int(v) != v for v in vals):
            raise TypeError
        return [int(v) for v in vals]
    except (TypeError, ValueError, RuntimeError):
        raise KoafError(f"{what}: {name} is a host sequence of integers, got {type(seq).__name__}") from None


def coal_tokens(tx, t0, seg_off, masks, out=None):
    """out [J, B, L, D]: out[j, b, l] = tx[b, l] where bit seg(l) of masks[j] is set, else t0[b % B0, l] (koaf_coal_tokens: the
    final FeaT's input tokens of J coalitions; tx and t0 read once for all of them, no value changed).  tx [B, L, D], t0 [B0, L, D]
    with B0 in (1, B): fp32 on one device.  seg_off: host integers [M + 1], 0 = seg_off[0] < ... < seg_off[M] = L -- token l is
    input i's where seg_off[i] <= l < seg_off[i + 1]; masks: host integers [J], one bit per input, none at or above M <= COAL_MAX_M."""
    check_tensor("coal_tokens", "tx", tx, torch.float32, nonempty=True)
    if tx.dim() != 3:
        raise KoafError(f"coal_tokens: tx is [B, L, D], got {tuple(tx.shape)}")
    B, L, D = (int(s) for s in tx.shape)
    check_tensor("coal_tokens", "t0", t0, torch.float32, like=tx, nonempty=True, where="tx's device")
    if t0.dim() != 3 or tuple(t0.shape[1:]) != (L, D) or int(t0.shape[0]) not in (1, B):
        raise KoafError(f"coal_tokens: t0 is [1 | {B}, {L}, {D}], got {tuple(t0.shape)}")
    seg, msk = _host_ints("coal_tokens", "seg_off", seg_off), _host_ints("coal_tokens", "masks", masks)
    M, J = len(seg) - 1, len(msk)
    if not 1 <= M <= COAL_MAX_M or J < 1:
        raise KoafError(f"coal_tokens: seg_off holds M + 1 offsets, 1 <= M <= {COAL_MAX_M}, and masks at least one coalition, got "
                        f"{len(seg)} offsets and {J} masks")
    if seg[0] != 0 or seg[M] != L or any(a >= b for a, b in zip(seg, seg[1:])):
        raise KoafError(f"coal_tokens: seg_off ascends strictly from 0 to L = {L}, got {seg}")
    if any(not 0 <= m < (1 << M) for m in msk):
        raise KoafError(f"coal_tokens: a mask has one bit per input, none at or above M = {M}, got {msk}")
    out = out_buffer("coal_tokens", out, (J, B, L, D), torch.float32, tx, "tx's device")
    check(lib().koaf_coal_tokens(_ptr(tx), _ptr(t0), (ctypes.c_int32 * (M + 1))(*seg), (ctypes.c_uint32 * J)(*msk), _ptr(out), J, B,
                                 int(t0.shape[0]), L, D, M, _stream()), "coal_tokens")
    return out


def shapley_weights(M):
    """(w_phi [M], w_int [M - 1]) as python floats: w_phi[t] = t! (M - t - 1)! / M!, w_int[t] = t! (M - t - 2)! / (M - 1)!, each one
    correctly rounded quotient of two integers"""
    from math import factorial as f
    M = int(M)
    return [f(t) * f(M - t - 1) / f(M) for t in range(M)], [f(t) * f(M - t - 2) / f(M - 1) for t in range(M - 1)]


def shapley_fold(v, M):
    """(phi [B, M], inter [B, M, M], loo [B, M], solo [B, M]), fp64 device tensors, of the coalition values v [2^M, B] (fp32; row s
    = the coalition whose bit i says player i is present): the Shapley values, the Shapley interaction index (zero diagonal),
    v(N) - v(N - i) and v({i}) - v({}) (koaf_shapley_fold: fp64, subsets in ascending mask order)."""
    M = int(M)
    if not 1 <= M <= COAL_MAX_M:
        raise KoafError(f"shapley_fold: 1 <= M <= {COAL_MAX_M}, got M = {M}")
    check_tensor("shapley_fold", "v", v, torch.float32, nonempty=True)
    if v.dim() != 2 or v.shape[0] != 1 << M:
        raise KoafError(f"shapley_fold: v is [2^M = {1 << M}, B], got {tuple(v.shape)}")
    S, B = (int(s) for s in v.shape)
    wp, wi = shapley_weights(M)
    phi, loo, solo = (torch.empty((B, M), device=v.device, dtype=torch.float64) for _ in range(3))
    inter = torch.empty((B, M, M), device=v.device, dtype=torch.float64)
    check(lib().koaf_shapley_fold(_ptr(v), (ctypes.c_double * M)(*wp), (ctypes.c_double * (M - 1))(*wi) if M > 1 else None, _ptr(phi),
                                  _ptr(inter), _ptr(loo), _ptr(solo), S, B, M, _stream()), "shapley_fold")
    return phi, inter, loo, solo


# ------------------------------------------------------------------------------------------------
# attention relevance of the FeaT fusion (koaf_attnrel.hip)
# ------------------------------------------------------------------------------------------------
ATTN_MODES = ("mean", "max", "min", "grad")


def attn_layer(attn, mode, dout=None, qkv=None, out=None):
    """the per-layer matrix abar [B, n, n] of an attention tensor attn [B, h, n, n] (koaf_attn_layer).  mode "mean" | "max" | "min":
    attention rollout -- the heads fused, the identity added, rows divided by their sum.  mode "grad": mean_h relu(dP * attn) with
    dP = dout_i . V_j, from dout [B, n, h*d] (the gradient with respect to the attention core's output) and the fused projection
    qkv [B, n, 3*h*d]; dP is never stored."""
    if mode not in ATTN_MODES:
        raise ValueError(f"Unknown attention mode: {mode}")
    check_tensor("attn_layer", "attn", attn, torch.float32, nonempty=True)
    if attn.dim() != 4 or attn.shape[2] != attn.shape[3]:
        raise KoafError(f"attn_layer: attn is [B, h, n, n], got {tuple(attn.shape)}")
    B, h, n, _ = (int(s) for s in attn.shape)
    d = 1
    if mode == "grad":
        if dout is None or qkv is None:
            raise KoafError("attn_layer: mode grad needs dout [B, n, h*d] and qkv [B, n, 3*h*d]")
        check_tensor("attn_layer", "dout", dout, torch.float32, like=attn, nonempty=True, where="attn's device")
        if dout.dim() != 3 or tuple(dout.shape[:2]) != (B, n) or dout.shape[2] % h:
            raise KoafError(f"attn_layer: dout is [{B}, {n}, {h} * d], got {tuple(dout.shape)}")
        d = int(dout.shape[2]) // h
        check_tensor("attn_layer", "qkv", qkv, torch.float32, (B, n, 3 * h * d), attn, where="attn's device")
    elif dout is not None or qkv is not None:
        raise KoafError(f"attn_layer: mode {mode} takes no dout / qkv")
    out = out_buffer("attn_layer", out, (B, n, n), torch.float32, attn, "attn's device")
    check(lib().koaf_attn_layer(_ptr(attn), _ptr(dout), _ptr(qkv), _ptr(out), B, n, h, d, ATTN_MODES.index(mode), _stream()),
          "attn_layer")
    return out


def attn_apply(abar, r_in=None, add_identity=False, out=None):
    """r_out [B, q, n] = r_in [B, q, n] . abar [B, n, n] (+ r_in with add_identity): relevance rows carried through one layer from
    the left (koaf_attn_apply).  r_in None: the identity, q = n.  `out` may alias neither input."""
    check_tensor("attn_apply", "abar", abar, torch.float32, nonempty=True)
    if abar.dim() != 3 or abar.shape[1] != abar.shape[2]:
        raise KoafError(f"attn_apply: abar is [B, n, n], got {tuple(abar.shape)}")
    B, n, _ = (int(s) for s in abar.shape)
    q = n
    if r_in is not None:
        check_tensor("attn_apply", "r_in", r_in, torch.float32, like=abar, nonempty=True, where="abar's device")
        if r_in.dim() != 3 or r_in.shape[0] != B or r_in.shape[2] != n:
            raise KoafError(f"attn_apply: r_in is [{B}, q, {n}], got {tuple(r_in.shape)}")
        q = int(r_in.shape[1])
    out = out_buffer("attn_apply", out, (B, q, n), torch.float32, abar, "abar's device")
    for name, t in (("abar", abar), ("r_in", r_in)):
        if t is not None and out.numel() and t.numel() and out.data_ptr() < t.data_ptr() + 4 * t.numel() \
                and t.data_ptr() < out.data_ptr() + 4 * out.numel():
            raise KoafError(f"attn_apply: out aliases {name}")
    check(lib().koaf_attn_apply(_ptr(r_in), _ptr(abar), _ptr(out), B, q, n, 1 if add_identity else 0, _stream()), "attn_apply")
    return out


def attn_segsum(r, off, K, t, out=None):
    """out [B, K]: out[b, k] = sum of r[b, off + k*t : off + (k+1)*t] for a relevance row r [B, n] -- per-slice totals (t tokens a
    slice) or, with K = 1, a modality's total (koaf_attn_segsum: index order, one rounding)."""
    check_tensor("attn_segsum", "r", r, torch.float32, nonempty=True)
    if r.dim() != 2:
        raise KoafError(f"attn_segsum: r is [B, n], got {tuple(r.shape)}")
    B, n = (int(s) for s in r.shape)
    off, K, t = int(off), int(K), int(t)
    if off < 0 or K < 1 or t < 1 or off + K * t > n:
        raise KoafError(f"attn_segsum: the segment [{off}, {off} + {K} * {t}) leaves the row of n = {n}")
    out = out_buffer("attn_segsum", out, (B, K), torch.float32, r, "r's device")
    check(lib().koaf_attn_segsum(_ptr(r), _ptr(out), B, n, off, K, t, _stream()), "attn_segsum")
    return out
