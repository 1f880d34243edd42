"""GPU: input gradients of the product models (run.input_gradients / saliency_maps / explain_epoch "input_x_grad") against
fixture F15 -- the imported reference's float64 gradients of sum_b logit[b, y_b] with respect to its four inputs, with the
reference's own float32-vs-float64 distance per input (`e32`) -- under the project's gradient bar (common.check_grads_vs_truth:
err / (e32 + 1e-4) <= 2 in the median, no tensor beyond 10 x, never below the ReLU-branch unit).  The clinical vector has no
encoder ReLU below it and is held to 1e-4.  Eval-mode PARAMETER gradients (the BatchNorm backward on running statistics) are
checked against the oracle's float64 eval-mode gradients under the same bar with F15's parameter table."""
import numpy as np
import pytest
import torch

import procedural as P
from common import check_grads_vs_truth, rel, top_relu_elems
from input_grads_fixture import load_f15
from test_models_gpu import build, t
from test_run_gpu import MODALS

pytestmark = pytest.mark.gpu

_S = {}


def case(dev):
    """F15's model, inputs and targets (built once for the module)"""
    if "case" not in _S:
        import json
        g = load_f15()
        cfg, B, seed = json.loads(str(g["cfg_json"])), int(g["B"]), int(g["seed"])
        xs = [t(a).to(dev) for a in P.model_inputs(cfg, B, seed)]
        y = t(P.make_target("target", B, seed)).to(dev)
        assert np.array_equal(y.cpu().numpy(), g["target"])
        _S["case"] = (g, cfg, B, build(cfg, dev), xs, y)
    return _S["case"]


def check_inputs(grads, g, mode, cfg, B, what):
    """the three image inputs under the e32 bar, the clinical vector at 1e-4"""
    assert all(torch.isfinite(x).all() for x in grads)
    mine = {i: grads[i].cpu().numpy() for i in range(3)}
    truth = {i: g[f"g64:{mode}:{i}"] for i in range(3)}
    e32 = {i: float(g[f"e32:{mode}"][i]) for i in range(3)}
    for i in range(4):
        assert tuple(grads[i].shape) == tuple(g[f"g64:{mode}:{i}"].shape)
    med, worst = check_grads_vs_truth(mine, truth, e32, what, n_top=top_relu_elems(cfg, B))
    clin = rel(grads[3].cpu().numpy(), g[f"g64:{mode}:3"])
    print(f"\n[{what}] image inputs err/(e32+1e-4): median {med:.2f} worst {worst:.2f}; errors "
          f"{[f'{rel(mine[i], truth[i]):.2e}' for i in range(3)]} (e32 {[f'{e32[i]:.2e}' for i in range(3)]}); clinical {clin:.2e}")
    assert clin < 1e-4, f"{what}: clinical input gradient off by {clin:.2e}"


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_input_gradients_vs_reference(dev, mode):
    from oaprogressionmmf_amd.run import input_gradients
    g, cfg, B, m, xs, y = case(dev)
    if mode == "train":
        m = build(cfg, dev)              # (a train-mode forward moves the running statistics: not on the shared model)
    m.train(mode == "train")
    for p in m.parameters():
        p.grad = None
    grads = input_gradients(m, xs, y)
    check_inputs(grads, g, mode, cfg, B, f"input gradients, {mode} mode")
    assert all(p.grad is None and p.requires_grad for p in m.parameters()), "input_gradients leaves the parameters alone"
    assert not any(x.requires_grad for x in xs)


def test_eval_mode_backward_parameters_and_frozen_model(dev):
    """eval mode, parameters left trainable: the BatchNorm backward on running statistics (dc = sc*dz) gives the parameter
    gradients of the float64 eval-mode oracle; freezing the parameters changes no bit of the input gradients and leaves
    p.grad alone"""
    from oracle import koafusion_cpu as O
    from oaprogressionmmf_amd.run import input_gradients
    g, cfg, B, m, xs, y = case(dev)
    m.eval()
    for p in m.parameters():
        p.grad = None
    leaves = [x.detach().requires_grad_(True) for x in xs]
    m(*leaves).reshape(B, -1).gather(1, y.long()).sum().backward()
    check_inputs([x.grad for x in leaves], g, "eval", cfg, B, "input gradients, eval mode, trainable parameters")
    mine = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    om = O.OracleModel(cfg, fill=P.fill_value, dtype=torch.float64)
    lg = om(*[x.cpu() for x in xs], train=False)
    assert rel(lg.detach().numpy(), g["eval:logits64"]) < 1e-9, "oracle fp64 vs reference fp64"
    lg.reshape(B, -1).gather(1, y.cpu().long()).sum().backward()
    truth = {k: p.grad.numpy() for k, p in om.named_parameters() if p.grad is not None}
    assert sorted(mine) == sorted(truth), "parameters with a gradient"
    e32 = dict(zip([str(k) for k in g["eval:e32_keys"]], np.asarray(g["eval:e32_vals"], dtype=np.float64)))
    med, worst = check_grads_vs_truth(mine, truth, e32, "eval-mode parameter gradients", n_top=top_relu_elems(cfg, B))
    print(f"\n[eval-mode parameter gradients] err/(e32+1e-4): median {med:.2f} worst {worst:.2f}")
    for p in m.parameters():
        p.grad = None
        p.requires_grad_(False)
    try:
        frozen = [x.detach().requires_grad_(True) for x in xs]
        m(*frozen).reshape(B, -1).gather(1, y.long()).sum().backward()
        assert all(p.grad is None for p in m.parameters())
    finally:
        for p in m.parameters():
            p.requires_grad_(True)
    for a, b in zip(frozen, leaves):
        assert torch.equal(a.grad, b.grad)
    for a, b in zip(input_gradients(m, xs, y), leaves):
        assert torch.equal(a, b.grad)


def test_input_gradients_recompute_policies_and_single_stream(dev, monkeypatch):
    """activation recompute (per stage, per block, the early stages only) and the trunks run one after the other on the caller's
    stream instead of on encoder lanes: the same kernels on the same operands as the stored-activation lane run -- fp32 rounding
    at most (1e-6)"""
    from oaprogressionmmf_amd.models import KoafTrunk, _common
    from oaprogressionmmf_amd.run import input_gradients
    g, cfg, B, m, xs, y = case(dev)
    m.eval()
    base = input_gradients(m, xs, y)
    trunks = [tr for tr in m.modules() if isinstance(tr, KoafTrunk)]
    try:
        for policy in (True, "block", (0, 1)):
            for tr in trunks:
                tr.recompute = policy
            for a, b in zip(input_gradients(m, xs, y), base):
                assert rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-6, policy
    finally:
        for tr in trunks:
            tr.recompute = False
    monkeypatch.setattr(_common, "USE_LANES", False)
    for a, b in zip(input_gradients(m, xs, y), base):
        assert rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-6


def test_input_gradients_without_gap(dev):
    """with_gap false (spatial trunk outputs, no pooling in front of the tokens): against the float64 oracle, the bar's e32 being
    the oracle's own float32 distance from it on this graph"""
    from oracle import koafusion_cpu as O
    from oaprogressionmmf_amd.run import input_gradients
    cfg = P.cfg_full(xr=(96, 96), mr1=(64, 64, 3), mr2=(64, 64, 2), depth=1)
    cfg["output_type"] = "main"
    cfg["fe"]["xr"]["with_gap"] = cfg["fe"]["mr"]["with_gap"] = False
    B, seed = 2, 31
    xs = [t(a) for a in P.model_inputs(cfg, B, seed)]
    y = t(P.make_target("target", B, seed)).long()
    ref = {}
    for dt in (torch.float64, torch.float32):
        om = O.OracleModel(cfg, fill=P.fill_value, dtype=dt)
        leaves = [x.to(dt).requires_grad_(True) for x in xs]
        om(*leaves, train=False).reshape(B, -1).gather(1, y).sum().backward()
        ref[dt] = [x.grad.numpy() for x in leaves]
    m = build(cfg, dev).eval()
    grads = input_gradients(m, [x.to(dev) for x in xs], y.to(dev))
    mine = {i: grads[i].cpu().numpy() for i in range(3)}
    truth = {i: ref[torch.float64][i] for i in range(3)}
    e32 = {i: rel(ref[torch.float32][i], ref[torch.float64][i]) for i in range(3)}
    med, worst = check_grads_vs_truth(mine, truth, e32, "input gradients, with_gap false", n_top=top_relu_elems(cfg, B))
    clin = rel(grads[3].cpu().numpy(), ref[torch.float64][3])
    print(f"\n[with_gap false] image inputs err/(e32+1e-4): median {med:.2f} worst {worst:.2f} (oracle e32 {e32}); clinical {clin:.2e}")
    assert clin < 1e-4


def test_input_gradients_bf16_activation_storage(dev):
    """bf16 storage of the trunks' forward activations (a throughput mode with a measured error, test_bf16_gpu.py): the input
    gradients exist, are finite fp32 and stay near the fp32 mode's.  The bar is stated against the fp32 mode's own sensitivity:
    `sens` = how far ITS input gradient moves when ONE bf16 rounding (2^-9 relative) enters, at the image.  The storage mode puts
    the same rounding at K places of a trunk -- every conv output and every block output it stores, plus the pooled stem -- which
    are independent and each have no more depth below them than the image has, so their effects add in quadrature to at most
    sqrt(K) * sens.  (A first version of this test held the mode to 2 * sens, the factor test_bf16_gpu.py uses where both
    figures are saturated; that ignores the K sites.  Measured at that time: 0.23 on the radiograph trunk against sens 0.099.)
    The clinical vector's gradient passes through the fusion transformer only, whose trunk-feature inputs carry the mode's
    eval-mode error (3e-2 on logits in test_bf16_gpu.py): 3e-2."""
    from oaprogressionmmf_amd.config import ConfigDict
    from oaprogressionmmf_amd.models import KoafTrunk, dict_models
    from oaprogressionmmf_amd.run import input_gradients
    g, cfg, B, m32, xs, y = case(dev)
    m32.eval()
    base = input_gradients(m32, xs, y)
    pert = input_gradients(m32, [x.bfloat16().float() if x.dim() >= 4 else x for x in xs], y)
    m16 = dict_models[cfg["name"]](config=ConfigDict(dict(cfg, activation_storage="bf16")), path_weights=None)
    P.fill_state_dict(m16.state_dict())
    m16 = m16.to(dev).eval()
    assert all(tr.act_dtype == torch.bfloat16 for tr in m16.modules() if isinstance(tr, KoafTrunk))
    g16 = input_gradients(m16, xs, y)
    for i, trunk in enumerate((m16._fe0, m16._fe1, m16._fe2)):
        lay = trunk._koaf_layout()
        K = sum(isinstance(mod, torch.nn.Conv2d) for mod in trunk.modules()) + len(lay["blocks"]) + 1
        err, sens = rel(g16[i].cpu().numpy(), base[i].cpu().numpy()), rel(pert[i].cpu().numpy(), base[i].cpu().numpy())
        print(f"\n[bf16 storage] input {i}: error {err:.2e} (sensitivity to one input rounding {sens:.2e}, {K} rounding sites)")
        assert torch.isfinite(g16[i]).all() and g16[i].dtype == torch.float32
        assert err < K ** 0.5 * sens
    assert rel(g16[3].cpu().numpy(), base[3].cpu().numpy()) < 3e-2


def test_explain_epoch_input_x_grad(dev):
    """explain_epoch(explain_fn="input_x_grad"): the (B, M) totals are sum(x * grad) of the maps the sink received (float64 sum,
    1e-5), the sink sees every sample once and the lists hold no maps; saliency_maps agrees with input_gradients; the
    modal-ablation output is what it was (fixture F13, test_run_gpu.py's bars)"""
    from common import load
    from oaprogressionmmf_amd.run import ensemble_explain_foldw, explain_epoch, input_gradients, saliency_maps
    g, cfg, B, m, xs, y = case(dev)
    m.eval()
    xc, yc = [x.cpu() for x in xs], y.cpu()
    loader = [{**{f"image__{mm}": x[lo:hi] for mm, x in zip(MODALS, xc)}, "target": yc[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in ((0, 2), (2, 3))]
    seen = []

    def sink(ids, modals, maps):
        assert list(modals) == list(MODALS) and len(maps) == len(MODALS)
        seen.append((list(ids), [mp.double().cpu() for mp in maps]))
    acc = explain_epoch(m, loader, MODALS, explain_fn="input_x_grad", sink=sink)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "ixg_attrs", "ixg_percent"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and acc["modal_names"] == [list(MODALS)] * 3
    assert [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    want = np.concatenate([np.stack([mp.reshape(mp.shape[0], -1).sum(1).numpy() for mp in maps], axis=1) for _, maps in seen])
    attrs = np.asarray(acc["ixg_attrs"])
    assert attrs.shape == (3, 4) and all(tuple(mp.shape[1:]) == tuple(x.shape[1:]) for mp, x in zip(seen[0][1], xs))
    assert np.abs(attrs - want).max() <= 1e-5 * np.abs(want).max(), (attrs, want)
    np.testing.assert_allclose(np.asarray(acc["ixg_percent"]).sum(1), 100.0, atol=2e-3)
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="ixg")
    np.testing.assert_allclose(np.asarray(ens["ixg_percent"]) * 100.0, acc["ixg_percent"], atol=2e-3)
    # the maps: gradient x input of input_gradients, sample by sample (batches of 2 + 1 against one batch of 3: same kernels,
    # other tilings of the batch dimension -- fp32 rounding)
    grads = input_gradients(m, xs, y)
    full = [torch.cat([maps[i] for _, maps in seen]) for i in range(4)]
    for x, gr, mp in zip(xs, grads, full):
        assert rel(mp.numpy(), (x.double() * gr.double()).cpu().numpy()) < 1e-4
    for a, b in zip(saliency_maps(m, xs, y, kind="grad"), grads):
        assert torch.equal(a, b)
    for a, x, gr in zip(saliency_maps(m, xs, y, kind="input_x_grad"), xs, grads):
        assert torch.equal(a, x * gr)
    with pytest.raises(ValueError):
        saliency_maps(m, xs, y, kind="grad_cam")
    with pytest.raises(ValueError):
        explain_epoch(m, loader, MODALS, explain_fn="grad_cam")
    # modal ablation: unchanged
    f13 = load("f13_modal_abl.npz")
    acc = explain_epoch(m, loader, MODALS)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "modal_abl_attrs", "modal_abl_percent"]
    scale = max(1.0, np.abs(f13["logits"]).max())
    assert np.abs(np.asarray(acc["modal_abl_attrs"]) - f13["attrs"]).max() < 1e-3 * scale * 0.05
    assert np.abs(np.asarray(acc["modal_abl_percent"]) - f13["percent"]).max() < 0.05
