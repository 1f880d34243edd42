"""numpy float64 restatement of the attention-relevance rules (run/_attnrel.py, koaf_attnrel.hip), of the two-level hierarchy
they are carried through, and of the error bars the GPU tests hold the kernels to.

Rules.  Rollout (Abnar & Zuidema 2020): per layer F = fuse_h(A), A^ = (F + I) with rows divided by their sum; the transformer's
relevance is A^_L ... A^_1.  Gradient-weighted (Chefer et al. 2021, self-attention rule): Abar = mean_h relu(dA * A),
dA[b,h,i,j] = sum_k dout[b,i,h d + k] V[b,j,h,k], R = (I + Abar_L) ... (I + Abar_1).  Both are carried as rows from the left.

Bars, all in units of EPS = 2^-23 (one fp32 rounding is at most 2^-24 relative; EPS leaves a factor 2):
  rollout layer   every term is non-negative: |err| <= (h + 3) EPS value
  gradient layer  (d + h + 4) EPS mean_h(A * sum_k |dout_ik| |V_jk|): any summation order of the d products, the product with A, the
                  1-Lipschitz relu, the h additions and the division
  apply           a row of n non-negative terms: (n + 2) EPS value per layer
  segsum          t EPS value
and `carry` composes them through a chain to first order: with r^ = r + dr, M^ = M + dM (|dr| <= br, |dM| <= bM),
  |fl(r^ M^) - r M| <= br M + (r + br) bM + (n + 2) EPS (r + br)(M + bM)."""
import numpy as np

EPS = 2.0 ** -23
FUSE = {"mean": lambda a: a.mean(axis=1), "max": lambda a: a.max(axis=1), "min": lambda a: a.min(axis=1)}


def rollout_layer(attn, fuse="mean"):
    """attn [B,h,n,n] -> A^ [B,n,n]"""
    a = np.asarray(attn, dtype=np.float64)
    f = FUSE[fuse](a) + np.eye(a.shape[-1])
    return f / f.sum(axis=-1, keepdims=True)


def rollout_layer_bar(attn, fuse="mean"):
    h = np.asarray(attn).shape[1]
    return (h + 3) * EPS * rollout_layer(attn, fuse)


def _dv(dout, qkv, h):
    do = np.asarray(dout, dtype=np.float64)
    B, n, hd = do.shape
    d = hd // h
    v = np.asarray(qkv, dtype=np.float64)[..., 2 * hd:].reshape(B, n, h, d)          # '(qkv h d)': the third part is V
    return do.reshape(B, n, h, d), v, d


def grad_layer(attn, dout, qkv):
    """attn [B,h,n,n], dout [B,n,h*d], qkv [B,n,3*h*d] -> Abar [B,n,n]"""
    a = np.asarray(attn, dtype=np.float64)
    do, v, _ = _dv(dout, qkv, a.shape[1])
    dA = do.transpose(0, 2, 1, 3) @ v.transpose(0, 2, 3, 1)                              # [B,h,n,n]: sum_k dout[b,i,h,k] V[b,j,h,k]
    return np.maximum(dA * a, 0.0).mean(axis=1)


def grad_layer_bar(attn, dout, qkv):
    a = np.asarray(attn, dtype=np.float64)
    h = a.shape[1]
    do, v, d = _dv(dout, qkv, h)
    mag = np.abs(do).transpose(0, 2, 1, 3) @ np.abs(v).transpose(0, 2, 3, 1)
    return (d + h + 4) * EPS * (np.abs(a) * mag).mean(axis=1)


def chain(mats, add_identity=False):
    """[M_1 .. M_L] -> M'_L ... M'_1, M' = M (+ I)"""
    n = mats[0].shape[-1]
    R = np.broadcast_to(np.eye(n), mats[0].shape).copy()
    for M in mats:
        Mp = M + np.eye(n) if add_identity else M
        R = Mp @ R
    return R


def carry(r, br, mats, bars, add_identity=False):
    """rows r [B,q,n] (bar br) through the layers from the left, last layer first: r <- r M_l (+ r); -> (r, bar)"""
    for M, bM in zip(reversed(mats), reversed(bars)):
        n = M.shape[-1]
        out = r @ M
        bout = br @ M + (r + br) @ bM + (n + 2) * EPS * ((r + br) @ (M + bM))
        if add_identity:
            out, bout = out + r, bout + br + EPS * (out + r)
        r, br = out, bout
    return r, br


def segsum(r, br, off, K, t):
    """r [B,n] -> ([B,K], bar)"""
    B = r.shape[0]
    s = r[:, off:off + K * t].reshape(B, K, t).sum(axis=2)
    bs = br[:, off:off + K * t].reshape(B, K, t).sum(axis=2)
    return s, bs + t * EPS * (s + bs)


def relevance(final_mats, final_bars, ncls, segments, agg_mats, agg_bars, n_inputs, add_identity=False):
    """The hierarchy.  final_mats: the final FeaT's layer matrices [M_1 .. M_L] ([B,n,n], CLS first); segments: [(input, offset
    behind the CLS tokens, length, tokens per slice, aggregator key or None)]; agg_mats / agg_bars: {key: [M_1 .. M_L]}.
    -> {"tokens": [...], "slices": [...], "totals" [B, n_inputs], "cls_self" [B], and each with "_bar"}"""
    B, n, _ = final_mats[0].shape
    e = np.zeros((B, 1, n))
    e[:, 0, 0] = 1.0
    r, br = carry(e, np.zeros_like(e), final_mats, final_bars, add_identity)
    out = {"tokens": [None] * n_inputs, "slices": [None] * n_inputs, "tokens_bar": [None] * n_inputs, "slices_bar": [None] * n_inputs,
           "final": r[:, 0], "final_bar": br[:, 0]}
    tot, btot = np.zeros((B, n_inputs)), np.zeros((B, n_inputs))
    for i, off, length, per, key in segments:
        t, bt = r[:, :, ncls + off:ncls + off + length], br[:, :, ncls + off:ncls + off + length]
        if key is not None:
            t, bt = carry(t, bt, agg_mats[key], agg_bars[key], add_identity)
        t, bt = t[:, 0], bt[:, 0]
        out["tokens"][i], out["tokens_bar"][i] = t, bt
        out["slices"][i], out["slices_bar"][i] = segsum(t, bt, 0, t.shape[1] // per, per)
        s, bs = segsum(t, bt, 0, 1, t.shape[1])
        tot[:, i], btot[:, i] = s[:, 0], bs[:, 0]
    c, bc = segsum(r[:, 0], br[:, 0], 0, 1, ncls)
    out.update(totals=tot, totals_bar=btot, cls_self=c[:, 0], cls_self_bar=bc[:, 0])
    return out
