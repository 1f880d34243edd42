"""Path attributions over the model's inputs (not in the reference): integrated gradients and SmoothGrad.

Both are weighted averages of run.input_gradients over modified copies of the inputs:

    IG_m = (x_m - b_m) * sum_k w_k * dF/dx_m (b + a_k (x - b))        (a_k, w_k): a quadrature rule on [0, 1]
    SG_m = 1/n * sum_d f(dF/dx_m (x + sigma * eps_d))                 f: identity | square;  sigma: a fraction of the range

The modified copies come from koaf_path_points (x and the baseline read once for a chunk of points, Gaussian noise drawn on the
device by a counter-based generator), the model sees `chunk` points folded into its batch dimension per pass, and
koaf_attr_fold adds the gradients that come back into the map in index order.  Nothing here reads a value back to the host."""
import numpy as np
import torch

from .. import ops
from ._explain import _forward_main, _targets, input_gradients

QUADRATURES = ("gausslegendre", "riemann_trapezoid", "riemann_left", "riemann_right", "riemann_middle")
SMOOTHGRAD_KINDS = ("smoothgrad", "smoothgrad_sq")


def quadrature(method="gausslegendre", n_steps=32):
    """-> (alphas, weights), float64 arrays of n_steps nodes in [0, 1] and weights that sum to 1 (captum's rules and names).
    gausslegendre: numpy's leggauss mapped from [-1, 1] (exact up to degree 2 n - 1);  riemann_left / _right / _middle: n equal
    cells, the node at the cell's left end / right end / centre;  riemann_trapezoid: n equally spaced nodes from 0 to 1, the end
    nodes with half weight (one node: the midpoint, the only one-node rule that integrates a linear function exactly)."""
    n = int(n_steps)
    if n < 1:
        raise ValueError(f"n_steps >= 1, got {n_steps}")
    if method == "gausslegendre":
        x, w = np.polynomial.legendre.leggauss(n)
        return 0.5 * (x + 1.0), 0.5 * w
    if method == "riemann_trapezoid":
        if n == 1:
            return np.array([0.5]), np.array([1.0])
        w = np.full(n, 1.0 / (n - 1))
        w[0] = w[-1] = 0.5 / (n - 1)
        return np.linspace(0.0, 1.0, n), w
    k = np.arange(n, dtype=np.float64)
    if method == "riemann_left":
        return k / n, np.full(n, 1.0 / n)
    if method == "riemann_right":
        return (k + 1.0) / n, np.full(n, 1.0 / n)
    if method == "riemann_middle":
        return (k + 0.5) / n, np.full(n, 1.0 / n)
    raise ValueError(f"Unknown quadrature method: {method}")


def resolve_baselines(xs, baselines):
    """-> per input None (zeros), a python float (a constant) or an fp32 tensor shaped like the input.
    `baselines`: None, one number for every input, or a sequence with one of the three forms per input."""
    if baselines is None or isinstance(baselines, (int, float)):
        baselines = (baselines,) * len(xs)
    if torch.is_tensor(baselines) or len(baselines) != len(xs):
        raise ValueError(f"baselines: None, a number, or one entry per input ({len(xs)}), each None, a number or a tensor")
    out = []
    for m, (x, b) in enumerate(zip(xs, baselines)):
        if b is None or isinstance(b, (int, float)):
            out.append(None if b is None else float(b))
        elif torch.is_tensor(b):
            if tuple(b.shape) != tuple(x.shape):
                raise ValueError(f"baselines[{m}]: a tensor baseline is shaped like its input {tuple(x.shape)}, got {tuple(b.shape)}")
            out.append(b.detach().to(device=x.device, dtype=torch.float32).contiguous())
        else:
            raise ValueError(f"baselines[{m}]: None, a number or a tensor, got {type(b).__name__}")
    return tuple(out)


def input_seed(seed, m):
    """the generator seed of input m: inputs of one shape must not share their noise"""
    return (int(seed) + m * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)


def _check_chunk(model, chunk, n):
    chunk = int(chunk)
    if not 1 <= chunk <= ops.ATTR_MAX_J:
        raise ValueError(f"1 <= chunk <= {ops.ATTR_MAX_J}, got {chunk}")
    if chunk > 1 and model.training:
        raise ValueError("chunk > 1 folds several path points into the batch dimension, which is exact only where samples do not "
                         "interact: put the model in eval() mode, or use chunk=1")
    return min(chunk, n)


def _inputs(xs):
    return tuple(x.detach().float().contiguous() for x in xs)


def _averaged(model, xs, target, coefs, weights, chunk, points, fold):
    """the loop both methods share: per chunk of J <= chunk coefficients, points(m, x, coefs[k0:k0+J], k0) -> [J, B, ...] per
    input, one input_gradients call at batch J * B, and fold(m, acc, g [J, B, ...], weights[k0:k0+J], first, last) per input"""
    n, B = coefs.numel(), xs[0].shape[0]
    tgt = _targets(target, xs)
    accs = tuple(torch.empty_like(x) for x in xs)
    for k0 in range(0, n, chunk):
        J = min(chunk, n - k0)
        pts = tuple(points(m, x, coefs[k0:k0 + J], k0).reshape((J * B,) + tuple(x.shape[1:])) for m, x in enumerate(xs))
        grads = input_gradients(model, pts, tgt.repeat(J, 1))
        del pts
        for m, (acc, g) in enumerate(zip(accs, grads)):
            fold(m, acc, g.contiguous().reshape((J,) + tuple(acc.shape)), weights[k0:k0 + J], k0 == 0, k0 + J == n)
    return accs


def integrated_gradients(model, xs, target, baselines=None, n_steps=32, method="gausslegendre", chunk=1, return_delta=False):
    """tuple shaped like `xs` of the integrated-gradients maps of logit[b, target_b] along the straight path from the baseline
    to the input, n_steps nodes of `method` (quadrature).  baselines: resolve_baselines.  chunk: path points per model pass, folded
    into the batch dimension (one input_gradients call at batch chunk * B; exact in eval() mode, refused in training mode).
    Parameters are left alone, as input_gradients leaves them.  return_delta: also the (B,) device tensor
    sum_m total[b, m] - (F(x)[b, t] - F(baseline)[b, t]) -- the quadrature's residual against completeness -- from one extra
    no-grad forward of inputs and baselines at batch 2 B (eval() mode for a meaningful figure)."""
    alphas, weights = quadrature(method, n_steps)
    chunk = _check_chunk(model, chunk, len(alphas))
    xs = _inputs(xs)
    bases = resolve_baselines(xs, baselines)
    dev = xs[0].device
    a32 = torch.as_tensor(alphas, dtype=torch.float32).to(dev)
    w32 = torch.as_tensor(weights, dtype=torch.float32).to(dev)

    def points(m, x, a, k0):
        return ops.path_points(x, a, base=bases[m])

    def fold(m, acc, g, w, first, last):
        ops.attr_fold(acc, g, w, first=first, x=xs[m] if last else None, base=bases[m])
    maps = _averaged(model, xs, target, a32, w32, chunk, points, fold)
    if not return_delta:
        return maps
    tgt = _targets(target, xs)
    ends = tuple(torch.cat([x, torch.zeros_like(x) if b is None else b if torch.is_tensor(b) else torch.full_like(x, b)])
                 for x, b in zip(xs, bases))
    with torch.no_grad():
        F = _forward_main(model, ends).float()
    B = xs[0].shape[0]
    gap = F[:B].gather(1, tgt) - F[B:].gather(1, tgt)
    return maps, attribution_totals(maps).sum(dim=1) - gap.reshape(-1)


def smoothgrad(model, xs, target, n_samples=16, noise_level=0.15, seed=0, kind="smoothgrad", chunk=1):
    """tuple shaped like `xs` of the mean ("smoothgrad") or mean squared ("smoothgrad_sq") gradient of logit[b, target_b] over
    n_samples Gaussian perturbations of the inputs, sigma = noise_level * (max - min) per sample and input (ops.minmax).
    Draw d of input m is z(input_seed(seed, m), d, b, i) for d in [0, n_samples) however the draws are chunked: the noise does
    not depend on `chunk` (path points per model pass, as in integrated_gradients).  noise_level 0 draws nothing."""
    if kind not in SMOOTHGRAD_KINDS:
        raise ValueError(f"Unknown smoothgrad kind: {kind}")
    n = int(n_samples)
    if n < 1:
        raise ValueError(f"n_samples >= 1, got {n_samples}")
    if not float(noise_level) >= 0.0:
        raise ValueError(f"noise_level >= 0, got {noise_level}")
    chunk = _check_chunk(model, chunk, n)
    xs = _inputs(xs)
    dev = xs[0].device
    ones = torch.ones(n, dtype=torch.float32, device=dev)
    w32 = torch.full((n,), 1.0 / n, dtype=torch.float32, device=dev)
    mms = tuple(ops.minmax(x, x.shape[0]) for x in xs) if float(noise_level) != 0.0 else (None,) * len(xs)

    def points(m, x, a, k0):
        return ops.path_points(x, a, mm=mms[m], noise_level=float(noise_level), seed=input_seed(seed, m), draw0=k0)

    def fold(m, acc, g, w, first, last):
        ops.attr_fold(acc, g, w, square=kind == "smoothgrad_sq", first=first)
    return _averaged(model, xs, target, ones, w32, chunk, points, fold)


def attribution_totals(maps):
    """(B, M) fp32 device tensor of the per-sample sums of the maps (koaf_rowdot against ones: fixed summation order) -- the
    counterpart of input_x_grad_totals for maps that already carry their input factor"""
    return torch.stack([ops.rowdot(mp.detach().float().contiguous(), torch.ones_like(mp, dtype=torch.float32)) for mp in maps], dim=1)
