"""GPU: run.integrated_gradients / run.smoothgrad / explain_epoch's two keys on the product model, on the configuration and
inputs of test_input_gradients_without_gap (XR 96 x 96, MRI 64 x 64 x 3 and 64 x 64 x 2, depth 1, B = 2), with_gap false and at
its default.  The float64 oracle receives the very path points / noisy copies the device produced (ops.path_points), so what
is compared is the averaged gradient of the same points; the bar is the project's gradient bar (common.check_grads_vs_truth)
with e32 = the oracle's own float32 distance from its float64 run for the same averaged quantity, the clinical input at 1e-4."""
import numpy as np
import pytest
import torch

import procedural as P
from common import check_grads_vs_truth, rel, top_relu_elems
from test_models_gpu import build, t
from test_run_gpu import MODALS

pytestmark = pytest.mark.gpu

B, SEED = 2, 31
BASES = (-0.5, -0.5, -0.5, None)           # a constant for the images, zeros for the clinical vector
_S = {}


def case(dev, with_gap=False):
    if with_gap not in _S:
        cfg = P.cfg_full(xr=(96, 96), mr1=(64, 64, 3), mr2=(64, 64, 2), depth=1)
        cfg["output_type"] = "main"
        cfg["fe"]["xr"]["with_gap"] = cfg["fe"]["mr"]["with_gap"] = with_gap
        xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, SEED)]
        y = t(P.make_target("target", B, SEED)).long().to(dev)
        _S[with_gap] = (cfg, build(cfg, dev).eval(), xs, y)
    return _S[with_gap]


def oracle_mean_gradients(cfg, pts, y, weights):
    """{dtype: [sum_j w_j dF/dx_m at point j]} of the eval-mode oracle in float64 and float32; pts: per input the [J, B, ...]
    fp32 points (cpu), evaluated as one batch of J * B samples"""
    from oracle import koafusion_cpu as O
    J = pts[0].shape[0]
    w = np.asarray(weights, dtype=np.float64)
    out = {}
    for dt in (torch.float64, torch.float32):
        om = O.OracleModel(cfg, fill=P.fill_value, dtype=dt)
        leaves = [p.reshape((J * B,) + tuple(p.shape[2:])).to(dt).requires_grad_(True) for p in pts]
        om(*leaves, train=False).reshape(J * B, -1).gather(1, y.cpu().repeat(J, 1)).sum().backward()
        out[dt] = [np.tensordot(w, x.grad.numpy().astype(np.float64).reshape((J,) + tuple(p.shape[1:])), axes=1)
                   for x, p in zip(leaves, pts)]
    return out


def held_to_the_gradient_bar(mine, ref, cfg, what):
    truth = {i: ref[torch.float64][i] for i in range(3)}
    e32 = {i: rel(ref[torch.float32][i], ref[torch.float64][i]) for i in range(3)}
    got = {i: mine[i].cpu().numpy() for i in range(3)}
    assert all(np.isfinite(g).all() for g in got.values())
    med, worst = check_grads_vs_truth(got, truth, e32, what, n_top=top_relu_elems(cfg, B))
    clin = rel(mine[3].cpu().numpy(), ref[torch.float64][3])
    print(f"\n[{what}] image inputs err/(e32+1e-4): median {med:.2f} worst {worst:.2f}; errors "
          f"{[f'{rel(got[i], truth[i]):.2e}' for i in range(3)]} (oracle e32 {[f'{e32[i]:.2e}' for i in range(3)]}); clinical {clin:.2e}")
    assert clin < 1e-4, f"{what}: clinical input off by {clin:.2e}"


def untouched(m):
    return all(p.requires_grad and p.grad is None for p in m.parameters())


@pytest.mark.parametrize("with_gap", [False, True])
def test_integrated_gradients_vs_oracle(dev, with_gap):
    """three Gauss-Legendre nodes: the averaged gradient (the fold without its last factor) and the finished map against the
    same quadrature over the oracle's float64 input gradients at the same points"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.run import input_gradients, integrated_gradients, quadrature
    cfg, m, xs, y = case(dev, with_gap)
    for p in m.parameters():
        p.grad = None
    alphas, weights = quadrature("gausslegendre", 3)
    a32, w32 = torch.tensor(alphas, dtype=torch.float32, device=dev), torch.tensor(weights, dtype=torch.float32, device=dev)
    pts = [ops.path_points(x, a32, base=b) for x, b in zip(xs, BASES)]
    ref = oracle_mean_gradients(cfg, [p.cpu() for p in pts], y, w32.cpu().numpy())
    grads = input_gradients(m, [p.reshape((3 * B,) + tuple(p.shape[2:])) for p in pts], y.repeat(3, 1))
    mean = [ops.attr_fold(torch.empty_like(x), g.contiguous().reshape((3,) + tuple(x.shape)), w32, first=True) for x, g in zip(xs, grads)]
    held_to_the_gradient_bar(mean, ref, cfg, f"IG averaged gradient, with_gap {with_gap}")
    maps = integrated_gradients(m, xs, y, baselines=BASES, n_steps=3, method="gausslegendre")
    assert all(mp.shape == x.shape and mp.dtype == torch.float32 for mp, x in zip(maps, xs))
    diff = [x.double().cpu().numpy() - (0.0 if b is None else b) for x, b in zip(xs, BASES)]
    ref_map = {dt: [d * g for d, g in zip(diff, ref[dt])] for dt in ref}
    held_to_the_gradient_bar(maps, ref_map, cfg, f"IG map, with_gap {with_gap}")
    assert untouched(m) and not any(x.requires_grad for x in xs)


def test_bridges_to_the_existing_maps(dev):
    """one right-Riemann node from the zero baseline is gradient x input, one noiseless sample is the gradient: the same
    kernels on the same operands, then w = 1 and the same fp32 product -- equal, not close"""
    from oaprogressionmmf_amd.run import input_gradients, integrated_gradients, saliency_maps, smoothgrad
    cfg, m, xs, y = case(dev)
    for a, b in zip(integrated_gradients(m, xs, y, n_steps=1, method="riemann_right", baselines=None),
                    saliency_maps(m, xs, y, kind="input_x_grad")):
        assert torch.equal(a, b)
    for a, b in zip(smoothgrad(m, xs, y, n_samples=1, noise_level=0), input_gradients(m, xs, y)):
        assert torch.equal(a, b)
    assert untouched(m)
    m.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            integrated_gradients(m, xs, y, n_steps=4, chunk=2)
        with pytest.raises(ValueError, match="eval"):
            smoothgrad(m, xs, y, n_samples=4, chunk=2)
    finally:
        m.eval()


def test_chunk_invariance(dev):
    """chunk = 1 against chunk = 3: the same kernels on another tiling of the batch dimension (1e-4, the figure
    test_explain_epoch_input_x_grad uses for that), for the path and for noisy copies; the noise itself is the same bits"""
    from oaprogressionmmf_amd.run import integrated_gradients, smoothgrad
    cfg, m, xs, y = case(dev)
    one = integrated_gradients(m, xs, y, baselines=BASES, n_steps=3, chunk=1)
    three = integrated_gradients(m, xs, y, baselines=BASES, n_steps=3, chunk=3)
    d = [rel(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(three, one)]
    print(f"\n[chunk invariance] IG {[f'{v:.2e}' for v in d]}")
    assert max(d) < 1e-4
    one = smoothgrad(m, xs, y, n_samples=3, noise_level=0.1, seed=5, chunk=1)
    three = smoothgrad(m, xs, y, n_samples=3, noise_level=0.1, seed=5, chunk=3)
    d = [rel(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(three, one)]
    print(f"[chunk invariance] SmoothGrad {[f'{v:.2e}' for v in d]}")
    assert max(d) < 1e-4
    assert untouched(m)


@pytest.mark.parametrize("kind", ["smoothgrad", "smoothgrad_sq"])
def test_smoothgrad_vs_oracle(dev, kind):
    """two draws at noise level 0.1: the noisy copies come from ops.path_points with smoothgrad's own seeds, go to the float64
    oracle as they are, and its mean (squared) gradient is the truth"""
    from oracle import koafusion_cpu as O
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.run import smoothgrad
    from oaprogressionmmf_amd.run._attr import input_seed
    cfg, m, xs, y = case(dev)
    n, level, seed = 2, 0.1, 77
    ones = torch.ones(n, device=dev)
    pts = [ops.path_points(x, ones, mm=ops.minmax(x, B), noise_level=level, seed=input_seed(seed, i)).cpu() for i, x in enumerate(xs)]
    assert all(rel(p[0].numpy(), p[1].numpy()) > 1e-2 for p in pts), "the draws differ"
    if "sg_ref" not in _S:
        ref = {}
        for dt in (torch.float64, torch.float32):
            om = O.OracleModel(cfg, fill=P.fill_value, dtype=dt)
            leaves = [p.reshape((n * B,) + tuple(p.shape[2:])).to(dt).requires_grad_(True) for p in pts]
            om(*leaves, train=False).reshape(n * B, -1).gather(1, y.cpu().repeat(n, 1)).sum().backward()
            ref[dt] = [x.grad.numpy().astype(np.float64).reshape((n,) + tuple(p.shape[1:])) for x, p in zip(leaves, pts)]
        _S["sg_ref"] = ref
    f = (lambda g: g * g) if kind == "smoothgrad_sq" else (lambda g: g)
    ref = {dt: [f(g).mean(axis=0) for g in gs] for dt, gs in _S["sg_ref"].items()}
    maps = smoothgrad(m, xs, y, n_samples=n, noise_level=level, seed=seed, kind=kind, chunk=2)
    held_to_the_gradient_bar(maps, ref, cfg, kind)
    assert untouched(m)


def test_delta_is_the_completeness_residual(dev):
    from oaprogressionmmf_amd.run import attribution_totals, integrated_gradients
    from oaprogressionmmf_amd.run._explain import _forward_main
    cfg, m, xs, y = case(dev)
    maps, delta = integrated_gradients(m, xs, y, baselines=BASES, n_steps=3, chunk=3, return_delta=True)
    assert delta.shape == (B,) and delta.dtype == torch.float32 and delta.is_cuda
    totals = attribution_totals(maps)
    assert totals.shape == (B, 4)
    for i, mp in enumerate(maps):
        want = mp.double().reshape(B, -1).sum(1)
        assert (totals[:, i].double() - want).abs().max() <= 1e-5 * max(1.0, float(want.abs().max()))
    with torch.no_grad():
        Fx = _forward_main(m, xs).gather(1, y)[:, 0]
        Fb = _forward_main(m, [torch.zeros_like(x) if b is None else torch.full_like(x, b) for x, b in zip(xs, BASES)]).gather(1, y)[:, 0]
    want = totals.sum(1) - (Fx - Fb)
    scale = max(1.0, float(Fx.abs().max()), float(Fb.abs().max()))
    print(f"\n[delta] {delta.tolist()} (recomputed {want.tolist()}; F(x) {Fx.tolist()} F(b) {Fb.tolist()})")
    assert (delta - want).abs().max().item() <= 1e-5 * scale
    assert untouched(m)


def test_explain_epoch_new_keys_and_old_outputs(dev):
    """the two new keys on F15's model and a 2 + 1 loader: key lists, every sample reaches the sink once, no maps in the lists,
    percentages sum to 100, explain_kwargs reach the function; the three existing keys give what they gave (modal ablation
    against fixture F13 under test_run_gpu.py's bars)"""
    from common import load
    from test_input_grads_models_gpu import case as f15_case
    from oaprogressionmmf_amd.run import (attribution_totals, ensemble_explain_foldw, explain_epoch, gradcam, input_gradients,
                                          integrated_gradients, smoothgrad)
    from oaprogressionmmf_amd.run._explain import input_x_grad_totals
    g, cfg, B3, m, xs, y = f15_case(dev)
    m.eval()
    for p in m.parameters():
        p.grad = None
    xc, yc = [x.cpu() for x in xs], y.cpu()
    cuts = ((0, 2), (2, 3))
    loader = [{**{f"image__{mm}": x[lo:hi] for mm, x in zip(MODALS, xc)}, "target": yc[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in cuts]
    seen = []

    def sink(ids, modals, maps):
        assert list(modals) == list(MODALS) and len(maps) == len(MODALS)
        seen.append((list(ids), maps))
    head = ["exam_knee_id", "target", "modal_names"]
    # integrated gradients
    kw = dict(n_steps=2, method="riemann_middle", chunk=2, baselines=(-0.5, -0.5, -0.5, None))
    acc = explain_epoch(m, loader, MODALS, explain_fn="integrated_gradients", sink=sink, explain_kwargs=kw)
    assert list(acc.keys()) == head + ["ig_attrs", "ig_percent", "ig_delta"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and acc["modal_names"] == [list(MODALS)] * 3
    assert [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    assert not any(torch.is_tensor(v) or isinstance(v, np.ndarray) for vals in acc.values() for v in vals), "no maps in the lists"
    for (lo, hi), (_, maps) in zip(cuts, seen):
        want, delta = integrated_gradients(m, [x[lo:hi] for x in xs], y[lo:hi], return_delta=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(maps, want)), "explain_kwargs reached the function"
        np.testing.assert_array_equal(np.asarray(acc["ig_attrs"][lo:hi], dtype=np.float32), attribution_totals(want).cpu().numpy())
        np.testing.assert_array_equal(np.asarray(acc["ig_delta"][lo:hi], dtype=np.float32), delta.cpu().numpy())
    assert np.asarray(acc["ig_attrs"]).shape == (3, 4)
    np.testing.assert_allclose(np.asarray(acc["ig_percent"]).sum(1), 100.0, atol=2e-3)
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="ig")
    np.testing.assert_allclose(np.asarray(ens["ig_percent"]) * 100.0, acc["ig_percent"], atol=2e-3)
    # SmoothGrad
    seen.clear()
    kw = dict(n_samples=2, noise_level=0.05, seed=9, chunk=2)
    acc = explain_epoch(m, loader, MODALS, explain_fn="smoothgrad", sink=sink, explain_kwargs=kw)
    assert list(acc.keys()) == head + ["sg_attrs", "sg_percent"]
    assert [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    assert not any(torch.is_tensor(v) or isinstance(v, np.ndarray) for vals in acc.values() for v in vals)
    for (lo, hi), (_, maps) in zip(cuts, seen):
        cut = [x[lo:hi] for x in xs]
        want = smoothgrad(m, cut, y[lo:hi], **kw)
        assert all(torch.equal(a, b) for a, b in zip(maps, want)), "explain_kwargs reached the function"
        np.testing.assert_array_equal(np.asarray(acc["sg_attrs"][lo:hi], dtype=np.float32), input_x_grad_totals(cut, want).cpu().numpy())
    np.testing.assert_allclose(np.asarray(acc["sg_percent"]).sum(1), 100.0, atol=2e-3)
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="sg")
    np.testing.assert_allclose(np.asarray(ens["sg_percent"]) * 100.0, acc["sg_percent"], atol=2e-3)
    assert all(p.requires_grad and p.grad is None for p in m.parameters())
    # the existing keys: unchanged
    f13 = load("f13_modal_abl.npz")
    acc = explain_epoch(m, loader, MODALS)
    assert list(acc.keys()) == head + ["modal_abl_attrs", "modal_abl_percent"]
    scale = max(1.0, np.abs(f13["logits"]).max())
    assert np.abs(np.asarray(acc["modal_abl_attrs"]) - f13["attrs"]).max() < 1e-3 * scale * 0.05
    assert np.abs(np.asarray(acc["modal_abl_percent"]) - f13["percent"]).max() < 0.05
    acc = explain_epoch(m, loader, MODALS, explain_fn="input_x_grad")
    assert list(acc.keys()) == head + ["ixg_attrs", "ixg_percent"]
    for lo, hi in cuts:
        cut = [x[lo:hi] for x in xs]
        np.testing.assert_array_equal(np.asarray(acc["ixg_attrs"][lo:hi], dtype=np.float32),
                                      input_x_grad_totals(cut, input_gradients(m, cut, y[lo:hi])).cpu().numpy())
    acc = explain_epoch(m, loader, MODALS, explain_fn="gradcam")
    assert list(acc.keys()) == head + ["gradcam_slice_scores"]
    cams = gradcam(m, [x[0:2] for x in xs], y[0:2].squeeze())
    for i, c in enumerate(cams):
        if c is None:
            assert acc["gradcam_slice_scores"][0][i] == []
        else:
            np.testing.assert_allclose(acc["gradcam_slice_scores"][0][i], c.slice_scores[0].cpu().numpy(), rtol=1e-5, atol=1e-7)
    with pytest.raises(ValueError, match="Unknown explain_fn: grad_cam"):
        explain_epoch(m, loader, MODALS, explain_fn="grad_cam")
    with pytest.raises(ValueError, match="takes no explain_kwargs"):
        explain_epoch(m, loader, MODALS, explain_fn="gradcam", explain_kwargs=dict(relu=False))
