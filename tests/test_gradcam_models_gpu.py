"""GPU: run.gradcam on the product models.

F16 (tests/golden/make_golden_gradcam.py): the imported reference's float64 signed low-resolution Grad-CAM maps of its three
trunks, with the reference's own float32 distance from them (`e32`), under the project's gradient bar (common.check_grads_vs_truth:
err / (e32 + 1e-4) <= 2 in the median, no tensor beyond 10 x; no ReLU-branch unit: Grad-CAM runs no backward through a trunk
ReLU, so the maps are continuous in the forward's rounding).  Plus what needs no reference:
the pooled identity sum_p cam[n, p] = sum_c g[n, c] pooled[n, c], the with_gap false path against float64 autograd, the volume
layouts, bf16 activation storage, what the call leaves behind, and explain_epoch(explain_fn="gradcam")."""
import copy
import json

import numpy as np
import pytest
import torch

import procedural as P
from common import check_grads_vs_truth, load, rel
from test_models_gpu import build, t
from test_run_gpu import MODALS

pytestmark = pytest.mark.gpu

_S = {}


def case(dev):
    """F16's model (= F13 / F15's), inputs and the seed's targets (F13's), built once for the module; F16's own targets are mixed
    classes set in its generator and are read from the fixture where the maps are compared"""
    if "case" not in _S:
        g = load("f16_gradcam.npz")
        cfg, B, seed = json.loads(str(g["cfg_json"])), int(g["B"]), int(g["seed"])
        xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, seed)]
        y = t(P.make_target("target", B, seed)).to(dev)
        _S["case"] = (g, cfg, B, build(cfg, dev).eval(), xs, y)
    return _S["case"]


def leaf_and_gradient(m, xs, y):
    """the test's own cut at the trunk outputs: {trunk: (its output as a leaf, d sum_b logit[b, y_b] / d leaf)}"""
    from oaprogressionmmf_amd.models import KoafTrunk
    leaves = {}

    def hook(mod, args, out):
        leaves[mod] = out.detach().requires_grad_(True)
        return leaves[mod]
    hs = [tr.register_forward_hook(hook) for tr in m.modules() if isinstance(tr, KoafTrunk)]
    try:
        out = m(*xs)
        out = out["main"] if isinstance(out, dict) else out
        sel = out.reshape(out.shape[0], -1).gather(1, y.long().reshape(-1, 1)).sum()
        trs = list(leaves)
        gs = torch.autograd.grad(sel, [leaves[tr] for tr in trs])
    finally:
        for h in hs:
            h.remove()
    return {tr: (leaves[tr].detach(), g.detach()) for tr, g in zip(trs, gs)}


def test_gradcam_vs_reference_fixture(dev):
    from oaprogressionmmf_amd.run import gradcam
    g, cfg, B, m, xs, _ = case(dev)
    y = t(g["target"]).to(dev)
    assert tuple(y.shape) == (B, 1) and len(np.unique(g["target"])) > 1, "F16 gathers a different class per sample"
    assert (g["pos_max"] > 0).all(), "F16 records a positive maximum for every (input, sample)"
    res = gradcam(m, xs, y, relu=False, normalize=None, upsample=False)
    assert len(res) == 4 and res[3] is None, "the clinical vector has no trunk"
    mine, truth = {}, {}
    for i in range(3):
        K = 1 if xs[i].dim() == 4 else int(xs[i].shape[-1])
        want = g[f"cam64:{i}"]
        assert tuple(res[i].map.shape) == (B, K) + want.shape[1:] and res[i].map.dtype == torch.float32
        assert tuple(res[i].slice_scores.shape) == (B, K) and res[i].slice_scores.dtype == torch.float32
        mine[i], truth[i] = res[i].map.reshape(want.shape).cpu().numpy(), want
    e32 = {i: float(g["e32"][i]) for i in range(3)}
    med, worst = check_grads_vs_truth(mine, truth, e32, "Grad-CAM maps vs F16")
    print(f"\n[F16] err/(e32+1e-4): median {med:.2f} worst {worst:.2f}; errors {[f'{rel(mine[i], truth[i]):.2e}' for i in range(3)]} "
          f"(e32 {[f'{e32[i]:.2e}' for i in range(3)]})")
    # the ReLU'd, normalised, resized maps of the same call: every (input, sample) has a peak.  The resize factor is 32, so the
    # output pixel nearest to the low-resolution maximum weighs it with 63/64 per axis (the other taps are >= 0): >= 0.969
    full = gradcam(m, xs, y)
    for i in range(3):
        assert full[i].map.shape == xs[i].shape
        top = full[i].map.reshape(B, -1).max(dim=1).values
        assert float(full[i].map.min()) >= 0.0 and float(top.max()) <= 1.0 and float(top.min()) > 0.96


@pytest.mark.parametrize("which", ["xr1cnn-resnet18", "mr1-cs", "mr1-rs"])
def test_gradcam_pooled_identity(dev, which):
    """behind the GAP: sum_p cam_signed[n, p] = sum_c g[n, c] * pooled[n, c] (ops.rowdot), within 1e-5 of sum |g * pooled|"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.run import gradcam
    if which == "xr1cnn-resnet18":
        cfg, B = P.cfg_xr1cnn(arch="resnet18", size=160), 3
    else:
        cfg, B = P.cfg_mr1(shape=(64, 96, 32), dims_view=which[-2:], depth=1), 2
    cfg["output_type"] = "main"
    xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, 5)]
    y = t(P.make_target("target", B, 5)).to(dev)
    m = build(cfg, dev).eval()
    (pooled, grad), = leaf_and_gradient(m, xs, y).values()
    N, C = pooled.shape[:2]
    assert pooled.shape[2:] == (1, 1)
    res, = gradcam(m, xs, y, relu=False, normalize=None, upsample=False)
    assert res.map.shape[0] * res.map.shape[1] == N
    want = ops.rowdot(grad.reshape(N, C).contiguous(), pooled.reshape(N, C).contiguous()).double()
    scale = ops.rowdot(grad.reshape(N, C).abs().contiguous(), pooled.reshape(N, C).abs().contiguous()).double()
    for got in (res.map.double().sum(dim=(2, 3)).reshape(N), res.slice_scores.double().reshape(N)):
        ratio = ((got - want).abs() / scale).max()
        print(f"\n[{which}] |sum_p cam - g . pooled| / sum |g * pooled|: {float(ratio):.2e}")
        assert float(ratio) <= 1e-5
    up, = gradcam(m, xs, y)
    assert up.map.shape == xs[0].shape and float(up.map.min()) >= 0.0 and float(up.map.max()) <= 1.0


REGISTRY = {
    "XR1Cnn-resnet34": lambda: P.cfg_xr1cnn(arch="resnet34", size=160),
    "XR1C1Cnn": lambda: P.cfg_xr1c1(arch="resnet18", size=160),
    "MR2CnnTrf": lambda: P.cfg_mr2(shape0=(160, 160, 4), shape1=(160, 160, 3)),
    "XR1MR1CnnTrf": lambda: P.cfg_xr1mr1(xr=(96, 96), mr=(64, 64, 3), depth=1),
    "MR1C1CnnTrf": lambda: P.cfg_mr1c1(mr=(96, 96, 6), depth=1),
}


@pytest.mark.parametrize("which", list(REGISTRY))
def test_gradcam_other_registry_models(dev, which):
    """the single-trunk, flat-fusion and extension classes the other tests do not build: one result per input, None where the
    input has no trunk, maps shaped like the inputs in [0, 1], and the pooled identity per trunk on the signed maps"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.run import _gradcam, gradcam
    cfg, B = REGISTRY[which](), 2
    cfg["output_type"] = "main"
    xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, 13)]
    y = t(P.make_target("target", B, 13)).to(dev)
    m = build(cfg, dev).eval()
    trunks = _gradcam._trunks(m)
    cut = leaf_and_gradient(m, xs, y)
    res, signed = gradcam(m, xs, y), gradcam(m, xs, y, relu=False, normalize=None, upsample=False)
    assert len(res) == len(xs) and [r is None for r in res] == [i not in trunks for i in range(len(xs))]
    for i, tr in trunks.items():
        assert res[i].map.shape == xs[i].shape and torch.isfinite(res[i].map).all()
        assert float(res[i].map.min()) >= 0.0 and float(res[i].map.max()) <= 1.0
        pooled, grad = cut[tr]
        N, C = pooled.shape[:2]
        want = ops.rowdot(grad.reshape(N, C).contiguous(), pooled.reshape(N, C).contiguous()).double()
        scale = ops.rowdot(grad.reshape(N, C).abs().contiguous(), pooled.reshape(N, C).abs().contiguous()).double()
        assert float(((signed[i].slice_scores.double().reshape(N) - want).abs() / scale).max()) <= 1e-5, (which, i)


def test_gradcam_without_gap(dev, monkeypatch):
    """with_gap false (F5's no-GAP configuration): the leaf is the feature map itself and the weights are the spatial mean of its
    gradient.  Truth: float64 autograd through the oracle, sum_c mean_yx(dA)_c * A_c on the maps its trunk returns.  The bar is
    the e32 one; e32 = the float32-vs-float64 distance of a CPU restatement of koaf_cam's formula on the model's own feature
    map and gradient."""
    from oracle import koafusion_cpu as O
    from oaprogressionmmf_amd.run import gradcam
    cfg, B = P.cfg_mr1(shape=(64, 96, 32), with_gap=False, depth=1), 1
    cfg["output_type"] = "main"
    xs = [t(a) for a in P.model_inputs(cfg, B, 11)]
    y = t(P.make_target("target", B, 11)).long()
    kept, trunk = [], O.trunk

    def keeping(*a, **k):
        out = trunk(*a, **k)
        out.retain_grad()
        kept.append(out)
        return out
    monkeypatch.setattr(O, "trunk", keeping)
    om = O.OracleModel(cfg, fill=P.fill_value, dtype=torch.float64)
    om(*xs, train=False).reshape(B, -1).gather(1, y).sum().backward()
    monkeypatch.setattr(O, "trunk", trunk)
    A64, = kept
    truth = (A64.detach() * A64.grad.mean(dim=(2, 3), keepdim=True)).sum(dim=1).numpy()
    m = build(cfg, dev).eval()
    xd, yd = [x.to(dev) for x in xs], y.to(dev)
    (A, gA), = leaf_and_gradient(m, xd, yd).values()
    assert A.shape == A64.shape and A.shape[2:] == (2, 3)
    A, gA = A.cpu(), gA.cpu()
    r32 = (A * gA.mean(dim=(2, 3), keepdim=True)).sum(dim=1)
    r64 = (A.double() * gA.double().mean(dim=(2, 3), keepdim=True)).sum(dim=1)
    e32 = rel(r32.numpy(), r64.numpy())
    res, = gradcam(m, xd, yd, relu=False, normalize=None, upsample=False)
    assert tuple(res.map.shape) == (B, 32, 2, 3)
    mine = res.map.reshape(truth.shape).cpu().numpy()
    med, worst = check_grads_vs_truth({0: mine}, {0: truth}, {0: e32}, "Grad-CAM, with_gap false")
    print(f"\n[with_gap false] error {rel(mine, truth):.2e} (restatement e32 {e32:.2e}): ratio {med:.2f}; vs the restatement "
          f"{rel(mine, r64.numpy()):.2e}")
    assert rel(mine, r64.numpy()) < 1e-5, "the kernels on the model's own map and gradient"


def test_gradcam_volume_layouts(dev):
    """the (B,1,R,C,S) volumes and the slice-major (B,1,S,R,C) ones (`volume_layout: ncdhw`) holding the same data: the same maps
    under the permutation, in [0, 1]; slice_scores = the per-slice sums of the un-normalised ReLU'd low-resolution map"""
    from oaprogressionmmf_amd.run import gradcam
    cfg = P.cfg_full(xr=(96, 96), mr1=(64, 64, 6), mr2=(64, 64, 5), depth=1)
    cfg["output_type"] = "main"
    cfg2 = copy.deepcopy(cfg)
    cfg2["fe"]["mr"]["volume_layout"] = "ncdhw"
    B = 2
    xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, 7)]
    xs2 = [xs[0], xs[1].permute(0, 1, 4, 2, 3).contiguous(), xs[2].permute(0, 1, 4, 2, 3).contiguous(), xs[3]]
    y = t(P.make_target("target", B, 7)).to(dev)
    m = build(cfg, dev).eval()
    a = gradcam(m, xs, y, upsample=True, normalize="sample")
    low = gradcam(m, xs, y, relu=True, normalize=None, upsample=False)
    b = gradcam(build(cfg2, dev).eval(), xs2, y, upsample=True, normalize="sample")
    assert a[3] is None and b[3] is None
    for i in range(3):
        assert a[i].map.shape == xs[i].shape and b[i].map.shape == xs2[i].shape
        same = b[i].map if i == 0 else b[i].map.permute(0, 1, 3, 4, 2)
        assert float((a[i].map - same).abs().max()) <= 1e-6, i              # (maps of magnitude <= 1; two instantiations of one blend)
        assert torch.equal(a[i].slice_scores, b[i].slice_scores)
        for r in (a[i], b[i]):
            assert float(r.map.min()) >= 0.0 and float(r.map.max()) <= 1.0
        want = low[i].map.double().sum(dim=(2, 3))
        assert float(low[i].map.min()) >= 0.0 and torch.equal(low[i].slice_scores, a[i].slice_scores)
        assert float((a[i].slice_scores.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # per-image normalisation: every slice with a non-zero map has its own peak ((63/64)^2 of 1.0 at the resize factor 32)
    img = gradcam(m, xs, y, normalize="image")
    tops = img[1].map.permute(0, 4, 1, 2, 3).reshape(B * 6, -1).max(dim=1).values
    has = low[1].map.reshape(B * 6, -1).max(dim=1).values > 0
    assert float(tops[has].min()) > 0.96 and float(tops.max()) <= 1.0 and float(tops[~has].abs().sum()) == 0.0


def test_gradcam_bf16_activation_storage(dev):
    """bf16 storage of the trunks' activations: the feature map arrives as bf16 and is widened in the kernel; the result is finite
    fp32 and within the distance test_bf16_gpu.py allows the mode's eval logits (3e-2)"""
    from oaprogressionmmf_amd.config import ConfigDict
    from oaprogressionmmf_amd.models import KoafTrunk, dict_models
    from oaprogressionmmf_amd.run import gradcam
    g, cfg, B, m32, xs, y = case(dev)
    base = gradcam(m32, xs, y, relu=False, normalize=None, upsample=False)
    m16 = dict_models[cfg["name"]](config=ConfigDict(dict(cfg, activation_storage="bf16")), path_weights=None)
    P.fill_state_dict(m16.state_dict())
    m16 = m16.to(dev).eval()
    assert all(tr.act_dtype == torch.bfloat16 for tr in m16.modules() if isinstance(tr, KoafTrunk))
    got = gradcam(m16, xs, y, relu=False, normalize=None, upsample=False)
    for i in range(3):
        err = rel(got[i].map.cpu().numpy(), base[i].map.cpu().numpy())
        print(f"\n[bf16 storage] input {i}: signed low-resolution map off the fp32 mode's by {err:.2e}")
        assert got[i].map.dtype == torch.float32 and torch.isfinite(got[i].map).all() and torch.isfinite(got[i].slice_scores).all()
        assert err < 3e-2
    up = gradcam(m16, xs, y)
    assert all(u.map.dtype == torch.float32 and torch.isfinite(u.map).all() and u.map.shape == x.shape for u, x in zip(up[:3], xs))


def _hygiene(m, frozen):
    from oaprogressionmmf_amd.models import KoafTrunk
    for tr in m.modules():
        if isinstance(tr, KoafTrunk):
            assert len(tr._forward_hooks) == 0 and tr.keep_features is False and tr.features is None
            assert "features" not in tr.__dict__ and "keep_features" not in tr.__dict__
    for p in m.parameters():
        assert p.grad is None and p.requires_grad == (p is not frozen)


def test_gradcam_leaves_the_model_as_it_found_it(dev, monkeypatch):
    from oaprogressionmmf_amd.run import _gradcam, gradcam
    g, cfg, B, m, xs, y = case(dev)
    for p in m.parameters():
        p.grad = None
    frozen = next(m.parameters())
    frozen.requires_grad_(False)
    try:
        a = gradcam(m, xs, y)
        _hygiene(m, frozen)
        b = gradcam(m, xs, y)
        for ra, rb in zip(a[:3], b[:3]):
            assert torch.equal(ra.map, rb.map) and torch.equal(ra.slice_scores, rb.slice_scores), "two calls, the same bits"
        assert not any(x.requires_grad for x in xs)
        forward = _gradcam._forward_main

        def failing(model, inputs):
            forward(model, inputs)                 # (the trunks ran: hooks fired, feature maps are stashed)
            raise RuntimeError("boom")
        monkeypatch.setattr(_gradcam, "_forward_main", failing)
        with pytest.raises(RuntimeError, match="boom"):
            gradcam(m, xs, y)
        _hygiene(m, frozen)
    finally:
        frozen.requires_grad_(True)


def test_explain_epoch_gradcam(dev):
    """explain_epoch(explain_fn="gradcam"): keys, order, the per-sample per-modality slice-score lists ([] for the clinical
    vector), the sink contract (every sample once, maps shaped like the inputs, None for the clinical vector, nothing of them
    in the lists); the modal-ablation output on the same loader is what it was (fixture F13, test_run_gpu.py's bars)"""
    from oaprogressionmmf_amd.run import explain_epoch, gradcam
    g, cfg, B, m, xs, y = case(dev)
    xc, yc = [x.cpu() for x in xs], y.cpu()
    loader = [{**{f"image__{mm}": x[lo:hi] for mm, x in zip(MODALS, xc)}, "target": yc[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in ((0, 2), (2, 3))]
    seen = []

    def sink(ids, modals, maps):
        assert list(modals) == list(MODALS) and len(maps) == len(MODALS) and maps[3] is None
        seen.append((list(ids), [mp.cpu() for mp in maps[:3]]))
    acc = explain_epoch(m, loader, MODALS, explain_fn="gradcam", sink=sink)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "gradcam_slice_scores"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and acc["modal_names"] == [list(MODALS)] * 3
    assert acc["target"] == yc.numpy().tolist()
    assert [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    whole = gradcam(m, xs, y)
    for b in range(3):
        row = acc["gradcam_slice_scores"][b]
        assert [len(r) for r in row] == [1, 6, 5, 0] and all(isinstance(v, float) for r in row for v in r)
        for i in range(3):
            want = whole[i].slice_scores[b].cpu().numpy()
            assert np.abs(np.asarray(row[i]) - want).max() <= 1e-4 * np.abs(whole[i].slice_scores.cpu().numpy()).max()
    for i in range(3):                      # (batches of 2 + 1 against one batch of 3: other tilings of the batch dimension)
        full = torch.cat([maps[i] for _, maps in seen])
        assert full.shape == xs[i].shape and float((full - whole[i].map.cpu()).abs().max()) <= 1e-3
    assert explain_epoch(m, loader, MODALS, explain_fn="gradcam").keys() == acc.keys()        # (no sink: the maps are dropped)
    # modal ablation: unchanged
    f13 = load("f13_modal_abl.npz")
    acc = explain_epoch(m, loader, MODALS)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "modal_abl_attrs", "modal_abl_percent"]
    scale = max(1.0, np.abs(f13["logits"]).max())
    assert np.abs(np.asarray(acc["modal_abl_attrs"]) - f13["attrs"]).max() < 1e-3 * scale * 0.05
    assert np.abs(np.asarray(acc["modal_abl_percent"]) - f13["percent"]).max() < 0.05
