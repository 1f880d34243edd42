"""The transformer's pieces and the element-wise layers: Linear (koaf_linear.hip), attention (koaf_attention.hip), LayerNorm /
GELU / ReLU / dropout / add / row softmax (koaf_rows.hip) and the column sums of bias gradients (koaf_bn.hip)."""
import torch

from .._lib import KoafError, check, lib
from ._base import _empty, _prof_begin, _prof_end, _ptr, _stream


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
