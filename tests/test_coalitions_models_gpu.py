"""GPU: run.modal_coalitions / run.modal_shapley / explain_epoch's "modal_shapley" key on the product model, on the configuration
and inputs of test_attr_models_gpu.case (XR 96 x 96, MRI 64 x 64 x 3 and 64 x 64 x 2, clinical, depth 1, B = 2) with the baselines
(-0.5, -0.5, -0.5, None): 16 coalitions.  The float64 oracle evaluates the 16 dense copies; the sparse pass -- two encoder passes
and fourteen passes of the final FeaT over spliced tokens -- is held to it, to the dense pass, to modal_ablation and to the count
of images the trunks may receive."""
import numpy as np
import pytest
import torch

import coal_twin as T
import procedural as P
from test_attr_models_gpu import B, BASES, case, untouched
from test_run_gpu import MODALS

pytestmark = pytest.mark.gpu

M, S = 4, 16
LOGIT_BAR = 1e-3          # the project's logit bar, relative to the reference's largest logit (README)
CHUNK_BAR = 1e-4          # the project's figure for another tiling of the batch dimension (test_occlusion_models_gpu.CHUNK_BAR)
_S = {}


def dense_copies(xs_np):
    """per input the [S * B, ...] batch of the 16 coalitions' copies, coalition-major"""
    out = []
    for m, x in enumerate(xs_np):
        b = np.zeros_like(x) if BASES[m] is None else np.full_like(x, BASES[m])
        out.append(np.concatenate([x if s >> m & 1 else b for s in range(S)]))
    return out


def oracle_values(cfg, xs, y):
    """(v_64 [S, B], max |F_64| over every logit of the pass): the eval-mode float64 oracle over the 16 x B dense copies as one batch"""
    if "oracle" not in _S:
        from oracle import koafusion_cpu as O
        batch = dense_copies([x.cpu().numpy() for x in xs])
        om = O.OracleModel(cfg, fill=P.fill_value, dtype=torch.float64)
        with torch.no_grad():
            F = om(*[torch.from_numpy(b).to(torch.float64) for b in batch], train=False).reshape(S * B, -1).double()
        v = F.gather(1, y.cpu().reshape(-1, 1).repeat(S, 1)).reshape(S, B).numpy()
        _S["oracle"] = (v, float(F.abs().max()))
    return _S["oracle"]


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def test_values_vs_oracle(dev):
    """First, on the oracle alone (a dead result could not hide under the bars), with bar = 1e-3 * max|F_64|: at least 6 of the 8
    |phi_64| exceed 20 bar and the largest 100 bar; max |phi_64 - loo_64| exceeds 10 bar; the largest |I_ij| exceeds 20 bar.
    Then sparse and dense at chunk 4: |v - v_64| <= bar; phi, loo, solo within 2 bar; interactions within 4 bar.
    Measured on an MI355X: oracle |phi_64| / bar 3.8 ... 237.5, 7 of 8 above 20; max |phi - loo| 17.9 bar; max |I_ij|
    34.2 bar; worst |v - v_64| 6.5e-7 = 1.1e-6 of max|F_64| = 0.5912 sparse, 8.3e-7 dense; phi 2.1e-7 / 4.4e-7, loo 5.4e-7 / 1.0e-6,
    solo 5.9e-7 / 5.4e-7, interaction 4.8e-7 / 4.2e-7."""
    from oaprogressionmmf_amd.run import ModalShapley, modal_shapley
    cfg, m, xs, y = case(dev, False)
    v64, fmax = oracle_values(cfg, xs, y)
    bar = LOGIT_BAR * fmax
    p64, i64, l64, s64 = T.shapley(v64)
    big = np.abs(p64) / bar
    print(f"\n[coalitions oracle] max|F_64| {fmax:.4f}, bar {bar:.3e}; |phi_64| / bar {np.sort(big.reshape(-1)).round(1).tolist()}; "
          f"max|phi - loo| {np.abs(p64 - l64).max() / bar:.1f} bar; max|I_ij| {np.abs(i64).max() / bar:.1f} bar")
    assert big.size == 8 and (big > 20).sum() >= 6 and big.max() > 100
    assert np.abs(p64 - l64).max() > 10 * bar
    assert np.abs(i64).max() > 20 * bar
    for sparse in (True, False):
        ms = modal_shapley(m, xs, y, baselines=BASES, chunk=4, sparse=sparse)
        assert isinstance(ms, ModalShapley) and ms.values.shape == (S, B) and ms.values.dtype == torch.float32 and ms.values.is_cuda
        assert ms.phi.shape == ms.loo.shape == ms.solo.shape == (B, M) and ms.interaction.shape == (B, M, M)
        assert all(t.dtype == torch.float64 and t.is_cuda for t in (ms.phi, ms.interaction, ms.loo, ms.solo))
        assert torch.equal(ms.v_full, ms.values[-1]) and torch.equal(ms.v_empty, ms.values[0])
        ev = np.abs(_np(ms.values) - v64).max()
        ep, el, es = (np.abs(_np(a) - b).max() for a, b in ((ms.phi, p64), (ms.loo, l64), (ms.solo, s64)))
        ei = np.abs(_np(ms.interaction) - i64).max()
        print(f"[coalitions vs oracle, sparse {sparse}] worst |v - v_64| {ev:.2e} = {ev / fmax:.2e} of max|F_64| (bar 1e-3); phi {ep:.2e}, "
              f"loo {el:.2e}, solo {es:.2e} (bar {2 * bar:.2e}); interaction {ei:.2e} (bar {4 * bar:.2e})")
        assert ev <= bar
        assert max(ep, el, es) <= 2 * bar
        assert ei <= 4 * bar
    assert untouched(m) and not any(x.requires_grad for x in xs)


@pytest.mark.parametrize("with_gap", [False, True])
def test_sparse_vs_dense(dev, with_gap):
    """the spliced-token pass against the plain one, chunk 1, 3 and 16: 1e-4 of the largest logit, the project's figure for another
    tiling of the batch dimension.  Not zero: the operand scales are per tensor and the batch differs."""
    from oaprogressionmmf_amd.run import modal_coalitions
    from oaprogressionmmf_amd.run._explain import _forward_main
    cfg, m, xs, y = case(dev, with_gap)
    with torch.no_grad():
        fmax = float(_forward_main(m, xs).abs().max())
    dense, masks = modal_coalitions(m, xs, y, baselines=BASES, chunk=1, sparse=False)
    assert masks == list(range(S))
    for chunk in (1, 3, 16):
        sparse, smasks = modal_coalitions(m, xs, y, baselines=BASES, chunk=chunk, sparse=True)
        assert smasks == masks
        err = float((sparse - dense).abs().max())
        print(f"\n[coalitions sparse vs dense, with_gap {with_gap}, chunk {chunk}] worst |v_s - v_d| {err:.2e} = {err / fmax:.2e} of max|F| "
              f"{fmax:.4f} (bar 1e-4)")
        assert err <= CHUNK_BAR * fmax
    assert untouched(m)


def test_bridge_to_modal_ablation(dev):
    """zero baselines, sparse=False, chunk=1: the leave-one-out differences are modal_ablation's -- the same forwards and the same
    subtraction: equal, not close; the sparse pass within twice the chunk bar (a difference holds two logits)"""
    from oaprogressionmmf_amd.run import modal_ablation, modal_shapley
    from oaprogressionmmf_amd.run._explain import _forward_main
    cfg, m, xs, y = case(dev, False)
    abl = modal_ablation(m, xs, y)
    with torch.no_grad():
        fmax = float(_forward_main(m, xs).abs().max())
    ms = modal_shapley(m, xs, y, baselines=None, chunk=1, sparse=False)
    assert torch.equal(ms.loo.float(), abl)
    sp = modal_shapley(m, xs, y, baselines=None, chunk=8, sparse=True)
    err = float((sp.loo.float() - abl).abs().max())
    print(f"\n[coalitions bridge] sparse loo - modal_ablation {err:.2e} = {err / fmax:.2e} of max|F| (bar 2e-4)")
    assert err <= 2 * CHUNK_BAR * fmax
    assert untouched(m)


def test_only_two_encoder_passes(dev):
    """the image rows every trunk is given over one sparse call: the intact inputs (B samples' images) and the baselines (one
    sample's: no baseline is a tensor) -- and nothing during the coalition chunks.  A tensor baseline makes the second pass B."""
    from oaprogressionmmf_amd.run import modal_coalitions
    cfg, m, xs, y = case(dev, False)
    seen = {}

    def counter(name):
        def hook(mod, args, out):
            seen.setdefault(name, []).append(int(args[0].shape[0]))
        return hook
    names = ("_fe0", "_fe1", "_fe2")
    handles = [getattr(m, n).register_forward_hook(counter(n)) for n in names]
    try:
        for chunk in (1, 5):
            seen.clear()
            modal_coalitions(m, xs, y, baselines=BASES, chunk=chunk, sparse=True)
            assert seen == {"_fe0": [B, 1], "_fe1": [3 * B, 3], "_fe2": [2 * B, 2]}, (chunk, seen)
        seen.clear()
        tb = (BASES[0], torch.full_like(xs[1], -0.5), BASES[2], BASES[3])
        vt, _ = modal_coalitions(m, xs, y, baselines=tb, chunk=5, sparse=True)
        assert seen == {"_fe0": [B, B], "_fe1": [3 * B, 3 * B], "_fe2": [2 * B, 2 * B]}, seen
        seen.clear()
        vd, _ = modal_coalitions(m, xs, y, baselines=BASES, chunk=1, sparse=False)
        assert seen == {"_fe0": [B] * S, "_fe1": [3 * B] * S, "_fe2": [2 * B] * S}, seen
    finally:
        for h in handles:
            h.remove()
    with torch.no_grad():
        fmax = float(vd.abs().max())
    assert float((vt - vd).abs().max()) <= CHUNK_BAR * fmax, "a tensor baseline of the same values gives the same coalitions"
    assert len(m._agg_final._forward_pre_hooks) == 0, "the hook on the final FeaT is gone"


def test_players(dev):
    """imaging against clinical: 4 coalitions, phi sums to v_full - v_empty, and the values are rows 0, 7, 8, 15 of the 16-coalition
    call -- equal for the dense pass at chunk 1 (the same forwards), within the sparse bar otherwise"""
    from oaprogressionmmf_amd.run import modal_coalitions, modal_shapley
    cfg, m, xs, y = case(dev, False)
    players = [[0, 1, 2], [3]]
    rows = [0, 7, 8, 15]
    full_d, _ = modal_coalitions(m, xs, y, baselines=BASES, chunk=1, sparse=False)
    grp_d, masks = modal_coalitions(m, xs, y, baselines=BASES, players=players, chunk=1, sparse=False)
    assert masks == rows and grp_d.shape == (4, B)
    assert torch.equal(grp_d, full_d[rows])
    fmax = float(full_d.abs().max())
    ms = modal_shapley(m, xs, y, baselines=BASES, players=players, chunk=8, sparse=True)
    assert ms.phi.shape == (B, 2) and ms.interaction.shape == (B, 2, 2) and ms.values.shape == (4, B)
    assert float((ms.values - full_d[rows]).abs().max()) <= CHUNK_BAR * fmax
    gap = ms.v_full.double() - ms.v_empty.double()
    eff = float((ms.phi.sum(1) - gap).abs().max())
    bound = 2 * (2 + 4) * 2.0 ** -53 * 2 * float(ms.values.abs().max())        # P times the phi bar of the kernel test at P = 2
    print(f"\n[coalitions players] efficiency residual {eff:.2e} (bound {bound:.2e})")
    assert eff <= bound
    # two players: phi_i = (solo_i + loo_i) / 2 and I_01 = loo_0 - solo_0
    assert torch.allclose(ms.phi, 0.5 * (ms.solo + ms.loo), rtol=0, atol=bound)
    assert torch.allclose(ms.interaction[:, 0, 1], ms.loo[:, 0] - ms.solo[:, 0], rtol=0, atol=2 * bound)


def test_explain_epoch_modal_shapley(dev):
    """the new key on F15's model and a 2 + 1 loader: key order, every sample reaches the sink once and in order as a ModalShapley
    tuple, explain_kwargs reach the function, percentages sum to 100, the efficiency residual within its bound, the fold ensemble
    reproduces the percentages, parameters untouched"""
    from test_input_grads_models_gpu import case as f15_case
    from oaprogressionmmf_amd.run import ModalShapley, ensemble_explain_foldw, explain_epoch, modal_shapley
    g, cfg, B3, m, xs, y = f15_case(dev)
    m.eval()
    for p in m.parameters():
        p.grad = None
    xc, yc = [x.cpu() for x in xs], y.cpu()
    cuts = ((0, 2), (2, 3))
    loader = [{**{f"image__{mm}": x[lo:hi] for mm, x in zip(MODALS, xc)}, "target": yc[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in cuts]
    seen = []

    def sink(ids, modals, ms):
        assert list(modals) == list(MODALS) and isinstance(ms, ModalShapley)
        seen.append((list(ids), ms))
    kw = dict(baselines=(-0.5, -0.5, -0.5, None), chunk=5, sparse=True)
    acc = explain_epoch(m, loader, MODALS, explain_fn="modal_shapley", sink=sink, explain_kwargs=kw)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "shap_attrs", "shap_percent", "shap_interactions", "shap_loo",
                                "shap_solo", "shap_delta"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and acc["modal_names"] == [list(MODALS)] * 3
    assert [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    assert not any(torch.is_tensor(v) or isinstance(v, np.ndarray) for vals in acc.values() for v in vals), "no tensors in the lists"
    for (lo, hi), (_, ms) in zip(cuts, seen):
        want = modal_shapley(m, [x[lo:hi] for x in xs], y[lo:hi], **kw)
        assert all(torch.equal(a, b) for a, b in zip(ms, want)), "explain_kwargs reached the function"
        np.testing.assert_array_equal(np.asarray(acc["shap_attrs"][lo:hi], dtype=np.float32), want.phi.float().cpu().numpy())
        np.testing.assert_array_equal(np.asarray(acc["shap_interactions"][lo:hi]), want.interaction.cpu().numpy())
        np.testing.assert_array_equal(np.asarray(acc["shap_loo"][lo:hi]), want.loo.cpu().numpy())
        np.testing.assert_array_equal(np.asarray(acc["shap_solo"][lo:hi]), want.solo.cpu().numpy())
    attrs = np.asarray(acc["shap_attrs"])
    assert attrs.shape == (3, 4) and np.abs(attrs).min() > 0 and np.asarray(acc["shap_interactions"]).shape == (3, 4, 4)
    np.testing.assert_allclose(np.asarray(acc["shap_percent"]).sum(1), 100.0, atol=2e-3)
    vmax = max(float(ms.values.abs().max()) for _, ms in seen)
    bound = 4 * (2 ** 3 + 4) * 2.0 ** -53 * 2 * vmax                            # M times the phi bar of the kernel test at M = 4
    assert len(acc["shap_delta"]) == 3 and np.abs(np.asarray(acc["shap_delta"])).max() <= bound
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="shap")
    np.testing.assert_allclose(np.asarray(ens["shap_percent"]) * 100.0, acc["shap_percent"], atol=2e-3)
    grp = explain_epoch(m, loader, MODALS, explain_fn="modal_shapley", explain_kwargs=dict(kw, players=[[0, 1, 2], [3]]))
    assert np.asarray(grp["shap_attrs"]).shape == (3, 2)
    assert untouched(m)
