"""GPU: koaf_path_points / koaf_attr_fold against numpy restatements of the arithmetic koaf.h pins.  Without noise both kernels
are bit-equal to numpy's fp32 (every difference, product and sum rounded on its own, in the stated order).  The generator is
checked three ways: determinism (the same bits whatever J, the split of the draws over calls, or the call), its values against
a float64 restatement of the header's recipe, and its statistics.
Shapes (B, n): one element; the clinical vector (rows of 9, no row 16-byte aligned); rows one short of the vector width; three
whole 4 x 256 lane sweeps plus a 3-element tail; one element beyond 2^20 (256 blocks and a one-element block; an odd n, so the
generator's last pair is cut) -- and two with n % 4 == 0, which are the ones that take the 16-byte path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (3, 9), (2, 1023), (2, 4 * 256 * 3 + 3), (1, 2 ** 20 + 1), (3, 12), (2, 4096 + 8)]
JS = (1, 5)
U64 = np.uint64
PAD = 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _rng(B, n, J, salt=0):
    return np.random.default_rng(1009 * salt + 31 * B + 7 * J + n)


def _values(r, shape):
    return (r.standard_normal(shape) * 10.0 ** r.uniform(-3, 3, shape)).astype(F32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the restatements ---------------------------------------------------------------------------
def path_np(x, alpha, base):
    """fp32, in the header's order: the difference, the product, the sum"""
    b = np.zeros_like(x) if base is None else base if isinstance(base, np.ndarray) else np.full_like(x, F32(base))
    d = x - b
    return np.stack([b + F32(a) * d for a in alpha])


def fold_np(acc, g, w, square, first, x=None, base=None):
    s = np.zeros_like(acc) if first else acc.copy()
    for j in range(g.shape[0]):
        s = s + F32(w[j]) * (g[j] * g[j] if square else g[j])
    if x is not None:
        b = np.zeros_like(x) if base is None else base if isinstance(base, np.ndarray) else np.full_like(x, F32(base))
        s = s * (x - b)
    return s


def mix64(z):
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def normals64(seed, draw, b, n):
    """float64 restatement of koaf.h's recipe: z(seed, draw, b, i) for i in [0, n)"""
    key = mix64(np.array([seed], dtype=U64) ^ mix64(np.array([(draw << 32) | b], dtype=U64)))
    h = mix64(key ^ mix64(np.arange((n + 1) // 2, dtype=U64)))
    u1 = ((h >> U64(40)).astype(np.float64) + 1.0) / 2.0 ** 24
    u2 = ((h >> U64(16)) & U64(0xFFFFFF)).astype(np.float64) / 2.0 ** 24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=1).reshape(-1)[:n]


def unit_noise(dev, B, n, J, seed, draw0=0):
    """z itself: x = base = 0 and sigma = 1 * (1 - 0), so out = (0 + alpha * 0) + 1 * z = z exactly"""
    from oaprogressionmmf_amd import ops
    mm = torch.tensor([[0.0, 1.0]] * B, device=dev)
    return ops.path_points(torch.zeros(B, n, device=dev), torch.ones(J, device=dev), mm=mm, noise_level=1.0, seed=seed, draw0=draw0)


# ---- path points, no noise ------------------------------------------------------------------------
@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("B,n", SHAPES)
def test_path_points_are_the_numpy_fp32_expression(dev, B, n, J):
    from oaprogressionmmf_amd import ops
    r = _rng(B, n, J)
    x, base = _values(r, (B, n)), _values(r, (B, n))
    alpha = r.uniform(0, 1, J).astype(F32)
    alpha[0] = 1.0
    if J > 1:
        alpha[-1] = 0.0
    xd, ad = _dev(x, dev), _dev(alpha, dev)
    for b_np, b_arg in ((base, _dev(base, dev)), (-0.75, -0.75), (None, None), (None, 0.0)):
        got = ops.path_points(xd, ad, base=b_arg)
        assert tuple(got.shape) == (J, B, n)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(path_np(x, alpha, b_np))), (type(b_arg).__name__,)
    # a noise level without mm, and mm with a zero level: nothing is drawn
    mm = ops.minmax(xd, B)
    want = _bits(path_np(x, alpha, None))
    assert np.array_equal(_bits(ops.path_points(xd, ad, mm=mm, noise_level=0.0, seed=3).cpu().numpy()), want)
    assert np.array_equal(_bits(ops.path_points(xd, ad, mm=None, noise_level=0.5, seed=3).cpu().numpy()), want)


# ---- the fold -----------------------------------------------------------------------------------
@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("B,n", SHAPES)
def test_fold_is_numpy_fp32_summed_in_index_order(dev, B, n, J):
    from oaprogressionmmf_amd import ops
    r = _rng(B, n, J, 1)
    g, acc0, x, base = _values(r, (J, B, n)), _values(r, (B, n)), _values(r, (B, n)), _values(r, (B, n))
    w = r.uniform(-1, 1, J).astype(F32)
    gd, wd, xd, bd = _dev(g, dev), _dev(w, dev), _dev(x, dev), _dev(base, dev)
    for square in (False, True):
        for first in (True, False):
            for fin_np, fin_arg in ((None, None), (("x", None), (xd, None)), (("x", 0.5), (xd, 0.5)), (("x", base), (xd, bd))):
                acc = _dev(acc0, dev)
                kw = {} if fin_arg is None else dict(x=fin_arg[0], base=fin_arg[1])
                out = ops.attr_fold(acc, gd, wd, square=square, first=first, **kw)
                assert out is acc
                with np.errstate(over="ignore", invalid="ignore"):
                    want = fold_np(acc0, g, w, square, first, *(() if fin_np is None else (x, fin_np[1])))
                assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want)), (square, first, fin_np is not None)
    assert np.array_equal(_bits(gd.cpu().numpy()), _bits(g)), "g is only read"


@pytest.mark.parametrize("B,n", SHAPES)
def test_fold_chunks_give_the_running_sum(dev, B, n):
    """J = 2 (first) and then J = 3 (accumulating, finishing): the five terms added in index order onto +0"""
    from oaprogressionmmf_amd import ops
    r = _rng(B, n, 5, 2)
    g, x = _values(r, (5, B, n)), _values(r, (B, n))
    w = r.uniform(0, 0.5, 5).astype(F32)
    gd, wd, xd = _dev(g, dev), _dev(w, dev), _dev(x, dev)
    acc = torch.full((B, n), float("nan"), device=dev)             # (`first` must overwrite)
    ops.attr_fold(acc, gd[:2], wd[:2], first=True)
    mid = fold_np(np.zeros((B, n), F32), g[:2], w[:2], False, True)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(mid))
    ops.attr_fold(acc, gd[2:], wd[2:], x=xd, base=-1.0)
    s = np.zeros((B, n), F32)
    for j in range(5):
        s = s + w[j] * g[j]
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(s * (x - F32(-1.0))))
    whole = torch.empty_like(acc)
    ops.attr_fold(whole, gd, wd, first=True, x=xd, base=-1.0)
    assert torch.equal(whole, acc)


def test_kernels_stay_inside_their_tensors(dev):
    """the entry points on ranges cut out of NaN-filled buffers (rows that start 4, not 16, bytes aligned): the sentinels on
    both sides survive"""
    from oaprogressionmmf_amd import _lib
    from oaprogressionmmf_amd.ops import _stream
    L = _lib.lib()
    for (B, n), J, off in (((3, 9), 5, 1), ((2, 1023), 5, 64), ((2, 4104), 5, 64), ((2, 4104), 1, 3)):
        r = _rng(B, n, J, 3)
        x, g = _values(r, (B, n)), _values(r, (J, B, n))
        alpha = r.uniform(0, 1, J).astype(F32)
        ad, xd, gd = _dev(alpha, dev), _dev(x, dev), _dev(g, dev)
        buf = torch.full((off + J * B * n + PAD,), float("nan"), device=dev)
        rc = L.koaf_path_points(xd.data_ptr(), None, 0.25, ad.data_ptr(), buf.data_ptr() + 4 * off, J, B, n, None, 0.0, 0, 0, _stream())
        assert rc == 0
        host = buf.cpu().numpy()
        assert np.isnan(host[:off]).all() and np.isnan(host[off + J * B * n:]).all()
        assert np.array_equal(_bits(host[off:off + J * B * n].reshape(J, B, n)), _bits(path_np(x, alpha, 0.25)))
        buf = torch.full((off + B * n + PAD,), float("nan"), device=dev)
        rc = L.koaf_attr_fold(buf.data_ptr() + 4 * off, gd.data_ptr(), ad.data_ptr(), xd.data_ptr(), None, 0.25, J, B, n, 0, 1, 1, _stream())
        assert rc == 0
        host = buf.cpu().numpy()
        assert np.isnan(host[:off]).all() and np.isnan(host[off + B * n:]).all()
        assert np.array_equal(_bits(host[off:off + B * n].reshape(B, n)), _bits(fold_np(x, g, alpha, False, True, x, 0.25)))


# ---- the generator --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", SHAPES)
def test_noise_is_a_function_of_seed_draw_sample_and_element(dev, B, n):
    from oaprogressionmmf_amd import ops
    r = _rng(B, n, 5, 4)
    x = _values(r, (B, n))
    xd = _dev(x, dev)
    mm = ops.minmax(xd, B)
    alpha = torch.ones(5, device=dev)
    kw = dict(mm=mm, noise_level=0.15, seed=1234567891011)
    a = ops.path_points(xd, alpha, **kw)
    assert torch.equal(a, ops.path_points(xd, alpha, **kw)), "the same arguments, the same bits"
    for j in range(5):
        one = ops.path_points(xd, alpha[:1], draw0=j, **kw)
        assert torch.equal(one[0], a[j]), f"draw {j} on its own"
    split = torch.cat([ops.path_points(xd, alpha[:2], draw0=0, **kw), ops.path_points(xd, alpha[:3], draw0=2, **kw)])
    assert torch.equal(split, a)
    z0, z1 = unit_noise(dev, B, n, 5, 1234567891011), unit_noise(dev, B, n, 5, 1234567891012)
    assert ((z1 - z0).abs() > 1e-6).float().mean().item() > 0.9, "another seed, other values"
    # sample b of a batch draws what it draws alone at index b ... which only a (seed, draw, b, i) generator can promise for
    # b = 0: row 0 of the batch against the batch cut to its first row
    alone = ops.path_points(xd[:1].contiguous(), alpha, mm=mm[:1].contiguous(), noise_level=0.15, seed=1234567891011)
    assert torch.equal(alone[:, 0], a[:, 0])
    # and the sum is the fp32 expression (path point + sigma * z), z taken from a unit-sigma call
    z = z0.cpu().numpy()
    mmh = mm.cpu().numpy()
    sigma = (F32(0.15) * (mmh[:, 1] - mmh[:, 0])).reshape(1, B, 1)
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(path_np(x, np.ones(5, F32), None) + sigma * z))


@pytest.mark.parametrize("B,n", SHAPES)
def test_noise_values_against_the_float64_recipe(dev, B, n):
    """absolute error <= 1e-5 in units of sigma: |z| <= sqrt(2 ln 2^24) = 5.77, where 16 fp32 ulps are 7.6e-6"""
    seed, draw0, J = 0xC0FFEE123456789, 3, 5
    z = unit_noise(dev, B, n, J, seed, draw0).cpu().numpy().astype(np.float64)
    worst = 0.0
    for j in range(J):
        for b in range(B):
            worst = max(worst, np.abs(z[j, b] - normals64(seed, draw0 + j, b, n)).max())
    print(f"\n[noise values ({B}, {n})] max |z - z64| = {worst:.2e}")
    assert worst <= 1e-5


def test_noise_statistics(dev):
    """2^22 values (2 draws x 2 samples x 2^20 elements); every bar is five standard errors"""
    z = unit_noise(dev, 2, 2 ** 20, 2, seed=20260318).cpu().numpy().astype(np.float64)
    assert np.isfinite(z).all()
    flat = z.reshape(-1)
    mean, var = flat.mean(), flat.var()

    def corr(a, b):
        return float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1])
    rows = z.reshape(4, -1)
    figs = dict(adjacent=corr(rows[:, :-1], rows[:, 1:]), partners=corr(rows[:, 0::2], rows[:, 1::2]),
                samples=corr(z[0, 0], z[0, 1]), draws=corr(z[0, 0], z[1, 0]))
    print(f"\n[noise statistics] mean {mean:.2e} variance - 1 {var - 1.0:.2e} max |z| {np.abs(flat).max():.3f} correlations {figs}")
    assert abs(mean) < 2.5e-3
    assert abs(var - 1.0) < 3.5e-3
    assert all(abs(c) < 5e-3 for c in figs.values()), figs
    assert np.abs(flat).max() <= 5.78


# ---- refusals ---------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(dev):
    from oaprogressionmmf_amd import _lib, ops
    from oaprogressionmmf_amd.ops import _stream
    L, EINVAL = _lib.lib(), _lib.defines()["KOAF_EINVAL"]
    B, n, J = 2, 12, 2
    x = torch.ones(B, n, device=dev)
    g = torch.ones(J, B, n, device=dev)
    c = torch.ones(J, device=dev)
    out = torch.full((J, B, n), 7.0, device=dev)
    acc = torch.full((B, n), 7.0, device=dev)
    X, G, C, O, A = (t.data_ptr() for t in (x, g, c, out, acc))
    for (j, b, m, xp, cp, op) in ((0, B, n, X, C, O), (65, B, n, X, C, O), (J, 0, n, X, C, O), (J, B, 0, X, C, O),
                                  (J, B, n, None, C, O), (J, B, n, X, None, O), (J, B, n, X, C, None)):
        assert L.koaf_path_points(xp, None, 0.0, cp, op, j, b, m, None, 0.0, 0, 0, _stream()) == EINVAL
        assert b"koaf_path_points" in L.koaf_last_error()
    for (j, b, m, ap, gp, wp, xp, fin) in ((0, B, n, A, G, C, X, 1), (65, B, n, A, G, C, X, 1), (J, 0, n, A, G, C, X, 1),
                                           (J, B, 0, A, G, C, X, 1), (J, B, n, None, G, C, X, 1), (J, B, n, A, None, C, X, 1),
                                           (J, B, n, A, G, None, X, 1), (J, B, n, A, G, C, None, 1)):
        assert L.koaf_attr_fold(ap, gp, wp, xp, None, 0.0, j, b, m, 0, 1, fin, _stream()) == EINVAL
        assert b"koaf_attr_fold" in L.koaf_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (acc == 7.0).all(), "a refused call launches nothing"
    assert L.koaf_attr_fold(A, G, C, None, None, 0.0, J, B, n, 0, 1, 0, _stream()) == 0      # (x is not needed without finish)
    assert (acc == 2.0).all()
    # the wrappers: dtype, contiguity, shape, device
    KoafError = _lib.KoafError
    for bad in (lambda: ops.path_points(x.double(), c), lambda: ops.path_points(x.t(), c), lambda: ops.path_points(x, c.cpu()),
                lambda: ops.path_points(x, torch.ones(65, device=dev)), lambda: ops.path_points(x, c, base=torch.zeros(B, n + 1, device=dev)),
                lambda: ops.path_points(x, c, mm=torch.zeros(B, 3, device=dev), noise_level=0.1),
                lambda: ops.path_points(x, c, draw0=-1), lambda: ops.path_points(x.cpu(), c.cpu()),
                lambda: ops.attr_fold(acc, g[:1], c), lambda: ops.attr_fold(acc, g.double(), c),
                lambda: ops.attr_fold(acc, g, c, x=x[:1]), lambda: ops.attr_fold(acc.t(), g, c)):
        with pytest.raises(KoafError):
            bad()
