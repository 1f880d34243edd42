"""GPU: the three attention-relevance kernels (koaf_attnrel.hip) on their own against the float64 twin (attn_twin.py), under the
bars the twin states: every case runs twice and the two results are the same bits.

koaf_attn_layer, rollout modes: |err| <= (h + 3) 2^-23 value (all terms non-negative), row sums within (n + 3) 2^-23 of 1; the
inputs are softmax rows with a one-hot row per head (at another column per head: min-fusion gives an all-zero fused row from two
heads on) and a row with exact zeros.  Gradient rule: (d + h + 4) 2^-23 mean_h(A * sum_k |dout_ik| |V_jk|) computed by the twin
from the inputs, which is asserted to be below 1e-3 of max Abar, so it cannot hide a wrong kernel; dout and qkv are normal with a
few entries scaled by 1e3 (cancellation), and one dout row per sample aligned in sign with its V row (a positive product whatever
the draw, n = 1 included).  koaf_attn_apply: chains of 4, L (n + 2) 2^-23 value.  koaf_attn_segsum: t 2^-23 value."""
import numpy as np
import pytest
import torch

import attn_twin as T

pytestmark = pytest.mark.gpu

BS, HS, NS, DS = (1, 3), (1, 3, 8), (1, 5, 33, 65, 130), (1, 4, 20, 64)
SHAPES = [(B, h, n) for B in BS for h in HS for n in NS]
MODES = ("mean", "max", "min")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def softmax_rows(rng, B, h, n):
    """fp32 softmax rows of random scores; row 0 of head k is one-hot at column k % n, row 1 holds exact zeros (n >= 3)"""
    s = (3.0 * rng.standard_normal((B, h, n, n))).astype(np.float32)
    a = np.exp(s - s.max(axis=-1, keepdims=True))
    a = (a / a.sum(axis=-1, keepdims=True)).astype(np.float32)
    if n >= 2:
        a[:, :, 0, :] = 0.0
        for k in range(h):
            a[:, k, 0, k % n] = 1.0
    if n >= 3:
        a[:, :, 1, ::2] = 0.0
        a[:, :, 1, :] = (a[:, :, 1, :] / a[:, :, 1, :].sum(axis=-1, keepdims=True)).astype(np.float32)
    return a


def twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a, b), "two runs, the same bits"
    return a.cpu().numpy().astype(np.float64)


def check_rollout(dev, B, h, n, seed):
    from oaprogressionmmf_amd import ops
    a = softmax_rows(np.random.default_rng(seed), B, h, n)
    ad = _dev(a, dev)
    for mode in MODES:
        got = twice(lambda: ops.attn_layer(ad, mode))
        want = T.rollout_layer(a, mode)
        assert got.shape == (B, n, n)
        over = np.abs(got - want) - (h + 3) * T.EPS * want
        assert over.max() <= 0.0, (mode, B, h, n, float(np.abs(got - want).max()))
        assert np.abs(got.sum(axis=-1) - 1.0).max() <= (n + 3) * T.EPS
        if n >= 2:
            if mode == "min" and h >= 2:
                assert np.array_equal(got[:, 0], np.broadcast_to(np.eye(n)[0], (B, n))), "an all-zero fused row leaves the identity's"
        if n >= 3:
            z = want[:, 1] == 0.0
            assert z[:, 2::2].all() and (got[:, 1][z] == 0.0).all(), "exact zeros stay exact"


@pytest.mark.parametrize("B,h,n", SHAPES)
def test_attn_layer_rollout(dev, B, h, n):
    check_rollout(dev, B, h, n, 1000 * B + 10 * h + n)


def test_attn_layer_rollout_production_shape(dev):
    check_rollout(dev, 1, 8, 483, 7)


def grad_inputs(rng, B, h, n, d):
    a = softmax_rows(rng, B, h, n)
    do = rng.standard_normal((B, n, h * d)).astype(np.float32)
    qkv = rng.standard_normal((B, n, 3 * h * d)).astype(np.float32)
    for t in (do, qkv):
        flat = t.reshape(-1)
        flat[rng.choice(flat.size, size=max(1, flat.size // 97), replace=False)] *= 1e3
    # token 0's dout row takes the signs of its own V row: dP[b, :, 0, 0] = sum_k |dout| |V| > 0 for every head
    v0 = qkv[:, 0, 2 * h * d:]
    do[:, 0, :] = np.abs(do[:, 0, :]) * np.where(v0 < 0, -1.0, 1.0).astype(np.float32)
    return a, do, qkv


def check_grad(dev, B, h, n, d, seed):
    from oaprogressionmmf_amd import ops
    a, do, qkv = grad_inputs(np.random.default_rng(seed), B, h, n, d)
    ad, dd, qd = _dev(a, dev), _dev(do, dev), _dev(qkv, dev)
    got = twice(lambda: ops.attn_layer(ad, "grad", dout=dd, qkv=qd))
    want, bar = T.grad_layer(a, do, qkv), T.grad_layer_bar(a, do, qkv)
    assert got.shape == (B, n, n) and (got >= 0.0).all()
    assert want.max() > 0.0 and bar.max() < 1e-3 * want.max(), ("the bar is far below the values", B, h, n, d, bar.max(), want.max())
    err = np.abs(got - want)
    print(f"\n[grad {B} {h} {n} {d}] max err {err.max():.2e} max bar {bar.max():.2e} max Abar {want.max():.2e} "
          f"worst err / bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
    assert (err <= bar).all(), (B, h, n, d, float((err - bar).max()))


@pytest.mark.parametrize("B,h,n", SHAPES)
def test_attn_layer_gradient_rule(dev, B, h, n):
    for d in DS:
        check_grad(dev, B, h, n, d, 1000 * B + 100 * h + 10 * n + d)


def test_attn_layer_gradient_rule_production_shape(dev):
    check_grad(dev, 1, 8, 483, 256, 11)


def stochastic(rng, B, n, L):
    m = rng.random((L, B, n, n)).astype(np.float32) ** 4
    m[:, :, :, 0] += np.float32(1e-3)
    return [(x / x.sum(axis=-1, keepdims=True)).astype(np.float32) for x in m]


@pytest.mark.parametrize("add", (False, True), ids=("plain", "plus_identity"))
@pytest.mark.parametrize("B,n", [(1, 1), (3, 5), (2, 33), (1, 65), (3, 130), (1, 483)])
def test_attn_apply_chains(dev, B, n, add):
    """L = 4 matrices from the left, last first: the whole matrix (r_in NULL, q = n), the CLS row (q = 1), and five rows (a q that
    is no multiple of the kernel's row tile)"""
    from oaprogressionmmf_amd import ops
    L = 4
    mats = stochastic(np.random.default_rng(100 * B + n), B, n, L)
    md = [_dev(m, dev) for m in mats]
    want = T.chain([m.astype(np.float64) for m in mats], add_identity=add)

    def whole():
        r = ops.attn_apply(md[-1], None, add_identity=add)
        for m in reversed(md[:-1]):
            r = ops.attn_apply(m, r_in=r, add_identity=add)
        return r
    first = ops.attn_apply(md[-1], None, add_identity=add).cpu().numpy()
    assert np.array_equal(first, mats[-1] + np.eye(n, dtype=np.float32) if add else mats[-1]), "the identity from the left is exact"
    got = twice(whole)
    assert got.shape == (B, n, n)
    assert (np.abs(got - want) <= L * (n + 2) * T.EPS * want).all(), float((np.abs(got - want) / want).max())
    for q in sorted({1, min(5, n)}):
        e = np.zeros((B, q, n), dtype=np.float32)
        rows = [(3 * u) % n for u in range(q)]
        for u, i in enumerate(rows):
            e[:, u, i] = 1.0

        def some():
            r = _dev(e, dev)
            for m in reversed(md):
                r = ops.attn_apply(m, r_in=r, add_identity=add)
            return r
        gq = twice(some)
        assert gq.shape == (B, q, n)
        assert (np.abs(gq - want[:, rows]) <= L * (n + 2) * T.EPS * want[:, rows]).all(), (q, float(np.abs(gq - want[:, rows]).max()))


def test_attn_apply_refuses_aliasing(dev):
    from oaprogressionmmf_amd import _lib, ops
    from oaprogressionmmf_amd._lib import KoafError
    from oaprogressionmmf_amd.ops import _stream
    m = _dev(stochastic(np.random.default_rng(1), 2, 8, 1)[0], dev)
    r = torch.zeros(2, 8, 8, device=dev)
    keep = m.clone()
    for kw in (dict(r_in=r, out=r), dict(r_in=r, out=m), dict(r_in=None, out=m)):
        with pytest.raises(KoafError, match="aliases"):
            ops.attn_apply(m, **kw)
    L, EINVAL = _lib.lib(), _lib.defines()["KOAF_EINVAL"]
    assert L.koaf_attn_apply(r.data_ptr(), m.data_ptr(), r.data_ptr() + 4 * 8, 2, 8, 8, 0, _stream()) == EINVAL      # a partial overlap
    assert b"aliases" in L.koaf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(m, keep) and float(r.abs().sum()) == 0.0, "a refused call launches nothing"
    out = torch.empty(2, 8, 8, device=dev)
    assert ops.attn_apply(m, r_in=m.clone(), out=out) is out


@pytest.mark.parametrize("t", (1, 25))
@pytest.mark.parametrize("K", (1, 7, 160))
def test_attn_segsum(dev, K, t):
    from oaprogressionmmf_amd import _lib, ops
    from oaprogressionmmf_amd._lib import KoafError
    from oaprogressionmmf_amd.ops import _stream
    B, off = 3, 1 + (K + t) % 5
    n = off + K * t + 2
    r = (np.random.default_rng(K * 31 + t).random((B, n)).astype(np.float32)) ** 3
    rd = _dev(r, dev)
    got = twice(lambda: ops.attn_segsum(rd, off, K, t))
    want, _ = T.segsum(r.astype(np.float64), np.zeros((B, n)), off, K, t)
    assert got.shape == (B, K) and (np.abs(got - want) <= t * T.EPS * want).all()
    whole = twice(lambda: ops.attn_segsum(rd, 0, 1, n))
    assert (np.abs(whole[:, 0] - r.astype(np.float64).sum(axis=1)) <= n * T.EPS * whole[:, 0]).all()
    with pytest.raises(KoafError, match="leaves the row"):
        ops.attn_segsum(rd, off + 3, K, t)
    out = torch.full((B, K), -1.0, device=dev)
    L = _lib.lib()
    assert L.koaf_attn_segsum(rd.data_ptr(), out.data_ptr(), B, n, off + 3, K, t, _stream()) == _lib.defines()["KOAF_EINVAL"]
    assert b"leaves the row" in L.koaf_last_error()
    torch.cuda.synchronize()
    assert float((out + 1.0).abs().sum()) == 0.0, "a refused call launches nothing"
