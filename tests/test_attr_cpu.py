"""CPU: the host side of the path attributions (run.integrated_gradients / run.smoothgrad / explain_epoch's two keys).  The two
entry points are declared in koaf.h with the documented prototypes and built into the library at the unchanged ABI version; the
quadrature rules against numpy and against the integrals they must get exactly; argument handling that needs no device; and the
whole Python route -- chunking through the batch dimension, the fold order, the delta, the explain_epoch plumbing -- on a stub
model with the two ops replaced by torch restatements of their header definitions."""
import ctypes

import numpy as np
import pytest
import torch

N_STEPS = (1, 2, 5, 32)
METHODS = ("gausslegendre", "riemann_trapezoid", "riemann_left", "riemann_right", "riemann_middle")


def test_attr_entry_points_are_declared_and_built():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    P, I, L, F, U = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    # koaf_path_points(x, base, base_value, alpha, out, J, B, n, mm, noise_level, seed, draw0, stream)
    assert protos["koaf_path_points"] == (ctypes.c_int, [P, P, F, P, P, I, I, L, P, F, U, L, P])
    # koaf_attr_fold(acc, g, w, x, base, base_value, J, B, n, square, first, finish, stream)
    assert protos["koaf_attr_fold"] == (ctypes.c_int, [P, P, P, P, P, F, I, I, L, I, I, I, P])
    assert _lib.defines()["KOAF_VERSION"] == 200
    assert _lib.defines()["KOAF_ATTR_MAX_J"] == 64
    handle = _lib.lib()                            # (binds every declared symbol: a library without the two fails here)
    assert handle.koaf_path_points.argtypes == protos["koaf_path_points"][1]
    assert handle.koaf_attr_fold.argtypes == protos["koaf_attr_fold"][1]
    mk = (_lib.LIB_PATH.parent / "Makefile").read_text()
    rest = [ln for ln in mk.splitlines() if ln.startswith("REST_SRCS")]
    assert len(rest) == 1 and "koaf_attr.hip" in rest[0].split()


def test_attr_kernels_refuse_bad_arguments_without_a_device():
    """the argument checks run ahead of any launch: J, B, n below 1, J above the bound, a missing pointer"""
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                       # (never dereferenced: every call below is refused first)
    for J, B, n in ((0, 1, 1), (65, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.koaf_path_points(p, None, 0.0, p, p, J, B, n, None, 0.0, 0, 0, None) == _lib.defines()["KOAF_EINVAL"]
        assert b"koaf_path_points" in L.koaf_last_error()
        assert L.koaf_attr_fold(p, p, p, None, None, 0.0, J, B, n, 0, 1, 0, None) == _lib.defines()["KOAF_EINVAL"]
        assert b"koaf_attr_fold" in L.koaf_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        x, alpha, out = args
        assert L.koaf_path_points(x, None, 0.0, alpha, out, 1, 1, 1, None, 0.0, 0, 0, None) != 0
        assert L.koaf_attr_fold(args[0], args[1], args[2], None, None, 0.0, 1, 1, 1, 0, 1, 0, None) != 0
    assert L.koaf_attr_fold(p, p, p, None, None, 0.0, 1, 1, 1, 0, 1, 1, None) != 0          # finish without x
    assert b"finish needs x" in L.koaf_last_error()
    assert L.koaf_path_points(p, None, 0.0, p, p, 1, 1, 1, None, 0.0, 0, -1, None) != 0     # a negative draw index


@pytest.mark.parametrize("n", N_STEPS)
def test_quadrature_rules(n):
    from oaprogressionmmf_amd.run import quadrature
    a, w = quadrature("gausslegendre", n)
    x, wx = np.polynomial.legendre.leggauss(n)
    assert a.dtype == np.float64 and w.dtype == np.float64
    assert np.abs(a - 0.5 * (x + 1.0)).max() <= 1e-14 and np.abs(w - 0.5 * wx).max() <= 1e-14
    deg = 2 * n - 1
    assert abs(np.sum(w * a ** deg) - 1.0 / (deg + 1)) <= 1e-14                           # t^(2n-1) on [0, 1]: exact
    a, w = quadrature("riemann_trapezoid", n)
    assert abs(np.sum(w * (3.0 * a - 1.25)) - (1.5 - 1.25)) <= 1e-14                       # a linear function: exact
    for method in METHODS:
        a, w = quadrature(method, n)
        assert a.shape == w.shape == (n,) and a.dtype == np.float64 and w.dtype == np.float64
        assert abs(w.sum() - 1.0) <= 1e-14 and (w > 0).all() and (a >= 0).all() and (a <= 1).all()
        assert (np.diff(a) > 0).all()
    assert quadrature("gausslegendre", n)[0].tolist() == quadrature(n_steps=n)[0].tolist()  # the default, as in captum


def test_quadrature_known_answers_and_unknown_names():
    from oaprogressionmmf_amd.run import quadrature
    a, w = quadrature("riemann_right", 1)
    assert a.tolist() == [1.0] and w.tolist() == [1.0]
    assert quadrature("riemann_left", 2)[0].tolist() == [0.0, 0.5]
    assert quadrature("riemann_middle", 2)[0].tolist() == [0.25, 0.75]
    a, w = quadrature("riemann_trapezoid", 3)
    assert a.tolist() == [0.0, 0.5, 1.0] and w.tolist() == [0.25, 0.5, 0.25]
    for name in ("gauss_legendre", "simpson", "", None):
        with pytest.raises(ValueError, match="Unknown quadrature method"):
            quadrature(name, 4)
    with pytest.raises(ValueError):
        quadrature("gausslegendre", 0)


def test_baseline_forms():
    from oaprogressionmmf_amd.run._attr import input_seed, resolve_baselines
    xs = (torch.ones(2, 1, 4, 4), torch.ones(2, 9))
    assert resolve_baselines(xs, None) == (None, None)
    assert resolve_baselines(xs, -1.5) == (-1.5, -1.5)
    t = torch.full((2, 9), 2.0, dtype=torch.float64)
    got = resolve_baselines(xs, [0, t])
    assert got[0] == 0.0 and isinstance(got[0], float) and got[1].dtype == torch.float32 and torch.equal(got[1], t.float())
    assert resolve_baselines(xs, (None, 3))[1] == 3.0
    for bad in ([None], (None, None, None), torch.zeros(2, 9), (None, torch.zeros(2, 8)), (None, "zeros")):
        with pytest.raises(ValueError, match="baselines"):
            resolve_baselines(xs, bad)
    assert input_seed(5, 0) == 5 and input_seed(5, 1) != input_seed(5, 2) and 0 <= input_seed(2 ** 64 - 1, 3) < 2 ** 64


def _stub():
    """a smooth two-input stub with the product models' calling convention: (B, 2) logits"""
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 16).reshape(1, 1, 4, 4))
            self.c = torch.nn.Parameter(torch.linspace(0.5, -0.25, 9).reshape(1, 9))
            self.calls = []

        def forward(self, img, clin):
            self.calls.append(int(img.shape[0]))
            u = (img * self.a).flatten(1).sum(1) + (clin * self.c).sum(1)
            v = (img.flatten(1) ** 2).sum(1) * 0.1 - clin.sum(1)
            return torch.stack([torch.tanh(u) + 0.05 * u * u, v], dim=1)
    return Stub().eval()


def _path_points_t(x, alpha, base=None, mm=None, noise_level=0.0, seed=0, draw0=0):
    assert mm is None or noise_level == 0.0, "the restatement draws no noise"
    b = torch.zeros_like(x) if base is None else base if torch.is_tensor(base) else torch.full_like(x, base)
    return torch.stack([b + a * (x - b) for a in alpha])


def _attr_fold_t(acc, g, w, square=False, first=False, x=None, base=None):
    s = torch.zeros_like(acc) if first else acc.clone()
    for j in range(g.shape[0]):
        s = s + w[j] * (g[j] * g[j] if square else g[j])
    if x is not None:
        b = torch.zeros_like(x) if base is None else base if torch.is_tensor(base) else torch.full_like(x, base)
        s = s * (x - b)
    acc.copy_(s)
    return acc


@pytest.fixture
def torch_ops(monkeypatch):
    from oaprogressionmmf_amd import ops
    monkeypatch.setattr(ops, "path_points", _path_points_t)
    monkeypatch.setattr(ops, "attr_fold", _attr_fold_t)
    monkeypatch.setattr(ops, "rowdot", lambda a, b: (a * b).flatten(1).sum(1))
    return ops


def _inputs(B=3):
    g = torch.Generator().manual_seed(11)
    return (torch.randn(B, 1, 4, 4, generator=g), torch.randn(B, 9, generator=g)), torch.tensor([[1], [0], [0]][:B])


def test_training_mode_refuses_chunked_points_and_bad_sizes():
    from oaprogressionmmf_amd.run import integrated_gradients, smoothgrad
    m, (xs, y) = _stub(), _inputs()
    m.train()
    with pytest.raises(ValueError, match="eval\\(\\) mode"):
        integrated_gradients(m, xs, y, n_steps=4, chunk=2)
    with pytest.raises(ValueError, match="eval\\(\\) mode"):
        smoothgrad(m, xs, y, n_samples=4, chunk=2)
    m.eval()
    for bad in (0, 65):
        with pytest.raises(ValueError, match="chunk"):
            integrated_gradients(m, xs, y, chunk=bad)
    with pytest.raises(ValueError, match="Unknown quadrature method"):
        integrated_gradients(m, xs, y, method="simpson")
    with pytest.raises(ValueError, match="Unknown smoothgrad kind"):
        smoothgrad(m, xs, y, kind="vargrad")
    with pytest.raises(ValueError):
        smoothgrad(m, xs, y, n_samples=0)
    with pytest.raises(ValueError):
        smoothgrad(m, xs, y, noise_level=-0.1)
    assert m.calls == [], "every refusal comes ahead of the first model pass"


def test_integrated_gradients_route_on_a_stub(torch_ops):
    """completeness on a smooth stub (32 Gauss-Legendre nodes integrate it to fp32 rounding), the chunking (passes of chunk * B
    samples, the same maps), the three baseline forms, the delta's bookkeeping, and the bridge to gradient x input"""
    from oaprogressionmmf_amd.run import attribution_totals, input_gradients, integrated_gradients
    m, (xs, y) = _stub(), _inputs()
    bases = (-0.5, torch.full((3, 9), 0.25))
    maps, delta = integrated_gradients(m, xs, y, baselines=bases, n_steps=32, chunk=5, return_delta=True)
    assert m.calls == [15] * 6 + [6] + [6], "32 points in chunks of 5 at B = 3, then the two end points in one forward"
    assert all(mp.shape == x.shape for mp, x in zip(maps, xs)) and delta.shape == (3,)
    with torch.no_grad():
        Fx = m(*xs).gather(1, y)[:, 0]
        Fb = m(torch.full_like(xs[0], -0.5), bases[1]).gather(1, y)[:, 0]
    tot = attribution_totals(maps)
    assert tot.shape == (3, 2)
    assert (tot.sum(1) - (Fx - Fb)).abs().max() < 1e-5 * max(1.0, float(Fx.abs().max()))
    assert torch.allclose(delta, tot.sum(1) - (Fx - Fb), atol=1e-5)
    one = integrated_gradients(m, xs, y, baselines=bases, n_steps=32, chunk=1)
    for a, b in zip(maps, one):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    zero = integrated_gradients(m, xs, y, n_steps=4)
    same = integrated_gradients(m, xs, y, baselines=(0.0, torch.zeros(3, 9)), n_steps=4)
    for a, b in zip(zero, same):
        assert torch.equal(a, b)
    bridge = integrated_gradients(m, xs, y, n_steps=1, method="riemann_right")
    for a, x, g in zip(bridge, xs, input_gradients(m, xs, y)):
        assert torch.equal(a, x * g)
    assert all(p.requires_grad and p.grad is None for p in m.parameters())


def test_smoothgrad_route_on_a_stub(torch_ops):
    from oaprogressionmmf_amd.run import input_gradients, smoothgrad
    m, (xs, y) = _stub(), _inputs()
    grads = input_gradients(m, xs, y)
    for a, g in zip(smoothgrad(m, xs, y, n_samples=1, noise_level=0.0), grads):
        assert torch.equal(a, g)
    m.calls.clear()
    sq = smoothgrad(m, xs, y, n_samples=4, noise_level=0.0, kind="smoothgrad_sq", chunk=3)
    assert m.calls == [9, 3]
    for a, g in zip(sq, grads):
        assert torch.allclose(a, g * g, rtol=1e-6, atol=1e-9)


def test_explain_epoch_plumbing_on_a_stub(torch_ops):
    from oaprogressionmmf_amd.run import ensemble_explain_foldw, explain_epoch, integrated_gradients
    m, (xs, y) = _stub(), _inputs()
    modals = ("xr_pa", "clin")
    loader = [{"image__xr_pa": xs[0][lo:hi], "image__clin": xs[1][lo:hi], "target": y[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in ((0, 2), (2, 3))]
    seen = []

    def sink(ids, mods, maps):
        assert list(mods) == list(modals)
        seen.append((list(ids), maps))
    kw = dict(n_steps=5, method="riemann_middle", chunk=2, baselines=(0.5, None))
    acc = explain_epoch(m, loader, modals, device="cpu", explain_fn="integrated_gradients", sink=sink, explain_kwargs=kw)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "ig_attrs", "ig_percent", "ig_delta"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    assert m.calls == [4, 4, 2, 4, 2, 2, 1, 2], "5 points in chunks of 2 per batch (B = 2, then 1), plus the end points"
    want = integrated_gradients(m, xs, y, **kw)
    for i in range(2):
        assert torch.allclose(torch.cat([maps[i] for _, maps in seen]), want[i], rtol=1e-5, atol=1e-6)
    attrs = np.asarray(acc["ig_attrs"])
    assert attrs.shape == (3, 2) and len(acc["ig_delta"]) == 3 and all(isinstance(d, float) for d in acc["ig_delta"])
    np.testing.assert_allclose(attrs, np.stack([w.flatten(1).sum(1).numpy() for w in want], axis=1), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(np.asarray(acc["ig_percent"]).sum(1), 100.0, atol=2e-3)
    assert not any(torch.is_tensor(v) for vals in acc.values() for v in vals), "the returned lists hold no maps"
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="ig")
    np.testing.assert_allclose(np.asarray(ens["ig_percent"]) * 100.0, acc["ig_percent"], atol=2e-3)
    seen.clear()
    acc = explain_epoch(m, loader, modals, device="cpu", explain_fn="smoothgrad", sink=sink,
                        explain_kwargs=dict(n_samples=2, noise_level=0.0, kind="smoothgrad_sq"))
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "sg_attrs", "sg_percent"]
    full = [torch.cat([maps[i] for _, maps in seen]) for i in range(2)]
    np.testing.assert_allclose(np.asarray(acc["sg_attrs"]), np.stack([(x * mp).flatten(1).sum(1).numpy() for x, mp in zip(xs, full)], 1),
                               rtol=1e-5, atol=1e-7)
    assert (full[0] >= 0).all(), "explain_kwargs reached the function: the squared variant"
    # the keys that take no keywords refuse them; unknown keys keep raising
    with pytest.raises(ValueError, match="takes no explain_kwargs"):
        explain_epoch(m, loader, modals, device="cpu", explain_kwargs=dict(n_steps=3))
    with pytest.raises(ValueError, match="Unknown explain_fn: grad_cam"):
        explain_epoch(None, [], modals, explain_fn="grad_cam", explain_kwargs=None)
    for key in ("integrated_gradients", "smoothgrad"):
        assert explain_epoch(None, [], modals, explain_fn=key) == {}


def test_fold_ensemble_merges_the_ig_family():
    from oaprogressionmmf_amd.run import ensemble_explain_foldw
    raw = {0: dict(exam_knee_id=["a", "b"], target=[[1], [0]], modal_names=[["x", "c"]] * 2,
                   ig_attrs=[[0.3, -0.1], [0.0, 0.2]], ig_percent=[[75.0, 25.0], [0.0, 100.0]], ig_delta=[0.01, -0.02]),
           2: dict(exam_knee_id=["b", "a"], target=[[0], [1]], modal_names=[["x", "c"]] * 2,
                   ig_attrs=[[0.1, 0.1], [-0.2, 0.2]], ig_percent=[[50.0, 50.0], [50.0, 50.0]], ig_delta=[0.0, 0.03])}
    ens = ensemble_explain_foldw(raw, prefix="ig")
    assert ens["exam_knee_id"] == ["a", "b"] and ens["target"] == [[1], [0]]
    assert ens["ig_attrs__0"] == [[0.3, -0.1], [0.0, 0.2]] and ens["ig_attrs__2"] == [[-0.2, 0.2], [0.1, 0.1]]
    np.testing.assert_allclose(ens["ig_percent"], [[0.625, 0.375], [0.25, 0.75]], rtol=1e-15)
    sg = {k: {kk.replace("ig_", "sg_"): v for kk, v in d.items() if kk != "ig_delta"} for k, d in raw.items()}
    assert ensemble_explain_foldw(sg, prefix="sg")["sg_percent"] == ens["ig_percent"]
