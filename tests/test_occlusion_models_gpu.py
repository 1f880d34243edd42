"""GPU: run.occlusion / explain_epoch's "occlusion" key on the product model, on the configuration and inputs of
test_attr_models_gpu.case (XR 96 x 96, MRI 64 x 64 x 3 and 64 x 64 x 2, depth 1, B = 2): 4 + 8 + 4 + 3 = 19 windows.  The float64
oracle evaluates the dense occluded copies occl_twin.py builds; the sparse pass is held to it, to the dense pass, to the closed
form of the slice images it may encode, and to modal_ablation where one window is the whole input."""
import numpy as np
import pytest
import torch

import occl_twin as T
import procedural as P
from test_attr_models_gpu import B, case, untouched
from test_run_gpu import MODALS

pytestmark = pytest.mark.gpu

WINS = [(1, 48, 48), (1, 32, 32, 2), (1, 64, 32, 1), (1, 4)]
STRS = [(1, 48, 48), (1, 32, 32, 1), (1, 64, 32, 1), (1, 3)]
BASES = (-0.5, -0.5, -0.5, 0)
KS = (4, 8, 4, 3)
LOGIT_BAR = 1e-3          # the project's logit bar, relative to the reference's largest logit (README); a delta holds two logits
CHUNK_BAR = 1e-4          # test_chunk_invariance's figure for another tiling of the batch dimension; a delta holds two logits
_S = {}


def oracle_deltas(cfg, xs, y):
    """{dtype: ([delta_m (K_m, B)], max |F|)} of the eval-mode oracle in float64 and float32: the intact inputs and the twin's 19
    dense occluded copies per sample as one batch of (1 + 19) * B samples"""
    if "oracle" in _S:
        return _S["oracle"]
    from oracle import koafusion_cpu as O
    xn = [x.cpu().numpy() for x in xs]
    batch = [[x] for x in xn]
    for m, x in enumerate(xn):
        pts = T.points(x, T.masks(x.shape, WINS[m], STRS[m]), np.float32(BASES[m]))
        assert len(pts) == KS[m]
        for k in range(len(pts)):
            for i in range(len(xn)):
                batch[i].append(pts[k] if i == m else xn[i])
    n = 1 + sum(KS)
    yy = y.cpu().reshape(-1, 1).repeat(n, 1)
    out = {}
    for dt in (torch.float64, torch.float32):
        om = O.OracleModel(cfg, fill=P.fill_value, dtype=dt)
        with torch.no_grad():
            F = om(*[torch.from_numpy(np.concatenate(b)).to(dt) for b in batch], train=False).reshape(n * B, -1).double()
        sel = F.gather(1, yy).reshape(n, B)
        deltas, at = [], 1
        for K in KS:
            deltas.append((sel[0:1] - sel[at:at + K]).numpy())
            at += K
        out[dt] = (deltas, float(F.abs().max()))
    _S["oracle"] = out
    return out


def test_deltas_vs_oracle(dev):
    """|delta_device - delta_64| <= 2e-3 * max |F_64| (max over every logit of the oracle's pass), sparse and dense; first, on the
    oracle alone, the deltas are far above that bar -- a dead map could not hide under it.
    Measured on an MI355X: worst |delta - delta_64| 6.9e-7 = 1.2e-6 of max|F_64| = 0.5723, sparse and dense alike; the
    oracle's own fp32 is 7.7e-7 from its fp64; 53 % of the oracle's deltas lie above 10 x the bar, the largest at 36 x."""
    from oaprogressionmmf_amd.run import occlusion
    cfg, m, xs, y = case(dev, False)
    assert [tuple(x.shape[1:]) for x in xs] == [(1, 96, 96), (1, 64, 64, 3), (1, 64, 64, 2), (1, 9)]
    ref = oracle_deltas(cfg, xs, y)
    d64, fmax = ref[torch.float64]
    bar = 2 * LOGIT_BAR * fmax
    flat = np.abs(np.concatenate([d.reshape(-1) for d in d64]))
    e32 = max(np.abs(a - b).max() for a, b in zip(ref[torch.float32][0], d64))
    print(f"\n[occlusion oracle] max|F_64| {fmax:.4f}, bar {bar:.3e}; {flat.size} deltas: {100 * (flat > 10 * bar).mean():.0f} % above "
          f"10 x bar, largest {flat.max() / bar:.1f} x bar; oracle fp32 - fp64: {e32:.2e} ({e32 / fmax:.1e} of max|F|)")
    assert flat.size == 38 and (flat > 10 * bar).mean() >= 0.40 and flat.max() > 30 * bar
    for sparse in (True, False):
        maps, deltas = occlusion(m, xs, y, WINS, STRS, BASES, chunk=4, sparse=sparse, return_deltas=True)
        assert all(d.shape == (K, B) and d.dtype == torch.float32 and d.is_cuda for d, K in zip(deltas, KS))
        assert all(mp.shape == x.shape and mp.dtype == torch.float32 for mp, x in zip(maps, xs))
        err = [float(np.abs(d.cpu().numpy().astype(np.float64) - r).max()) for d, r in zip(deltas, d64)]
        print(f"[occlusion vs oracle, sparse {sparse}] worst |delta - delta_64| per input {[f'{e:.2e}' for e in err]} = "
              f"{max(err) / fmax:.2e} of max|F_64| (bar 2e-3)")
        assert max(err) <= bar
    assert untouched(m) and not any(x.requires_grad for x in xs)


def test_map_is_the_fold_of_the_deltas(dev):
    from oaprogressionmmf_amd.run import occlusion
    cfg, m, xs, y = case(dev, False)
    maps, deltas = occlusion(m, xs, y, WINS, STRS, BASES, chunk=3, return_deltas=True)
    for mp, d, x, w, s in zip(maps, deltas, xs, WINS, STRS):
        want = T.fold_map(d.cpu().numpy(), T.masks(tuple(x.shape), w, s))
        assert torch.equal(mp.cpu(), torch.from_numpy(want))
    part, pd = occlusion(m, xs, y, [None, WINS[1], None, None], [None, STRS[1], None, None], BASES, chunk=3, return_deltas=True)
    assert [p is None for p in part] == [True, False, True, True] and [p is None for p in pd] == [True, False, True, True]
    assert torch.equal(part[1], maps[1]), "an input's map does not depend on which other inputs are occluded"


@pytest.mark.parametrize("with_gap", [False, True])
def test_sparse_vs_dense(dev, with_gap):
    """the cached-feature pass against the plain one, chunk 1 and 3: 2e-4 of the largest logit -- twice the project's figure for
    another tiling of the batch dimension, once per logit.  Not zero: the operand scales are per tensor and the batch differs."""
    from oaprogressionmmf_amd.run import occlusion
    from oaprogressionmmf_amd.run._explain import _forward_main
    cfg, m, xs, y = case(dev, with_gap)
    with torch.no_grad():
        fmax = float(_forward_main(m, xs).abs().max())
    dense = occlusion(m, xs, y, WINS, STRS, BASES, chunk=1, sparse=False, return_deltas=True)[1]
    for chunk in (1, 3):
        sparse = occlusion(m, xs, y, WINS, STRS, BASES, chunk=chunk, sparse=True, return_deltas=True)[1]
        err = [float((a - b).abs().max()) for a, b in zip(sparse, dense)]
        print(f"\n[sparse vs dense, with_gap {with_gap}, chunk {chunk}] worst |delta_s - delta_d| per input {[f'{e:.2e}' for e in err]} = "
              f"{max(err) / fmax:.2e} of max|F| {fmax:.4f} (bar 2e-4)")
        assert max(err) <= 2 * CHUNK_BAR * fmax
    assert untouched(m)


def test_only_the_touched_slices_are_encoded(dev):
    """the image rows every trunk is given over one call: the intact forward, then for the windows of its own input the touched
    slice images alone -- and nothing for the windows of any other input"""
    from oaprogressionmmf_amd.run import occlusion, touched_images
    cfg, m, xs, y = case(dev, False)
    seen = {}

    def counter(name):
        def hook(mod, args, out):
            seen[name] = seen.get(name, 0) + int(args[0].shape[0])
        return hook
    handles = [getattr(m, n).register_forward_hook(counter(n)) for n in ("_fe0", "_fe1", "_fe2")]
    try:
        for chunk in (1, 3):
            seen.clear()
            occlusion(m, xs, y, WINS, STRS, BASES, chunk=chunk, sparse=True)
            t1 = sum(len(touched_images("rc", xs[1].shape, WINS[1], STRS[1], k)) for k in range(KS[1]))
            t2 = sum(len(touched_images("rc", xs[2].shape, WINS[2], STRS[2], k)) for k in range(KS[2]))
            assert (t1, t2) == (8 * 2, 4 * 1)
            assert seen == {"_fe0": B + 4 * B, "_fe1": 3 * B + t1 * B, "_fe2": 2 * B + t2 * B}, (chunk, seen)
        seen.clear()
        occlusion(m, xs, y, WINS, STRS, BASES, chunk=1, sparse=False)
        assert seen == {"_fe0": (1 + 19) * B, "_fe1": (1 + 19) * 3 * B, "_fe2": (1 + 19) * 2 * B}, seen
    finally:
        for h in handles:
            h.remove()
    assert not any("forward" in getattr(m, n).__dict__ for n in ("_fe0", "_fe1", "_fe2")), "the trunks are left as they were"


def test_bridge_to_modal_ablation(dev):
    """one window that is the whole input, baseline 0, is the modality ablation: the same forward on the same operands with
    sparse=False and chunk=1 -- equal, not close; the sparse pass within its bar against the dense one"""
    from oaprogressionmmf_amd.run import modal_ablation, occlusion
    from oaprogressionmmf_amd.run._explain import _forward_main
    cfg, m, xs, y = case(dev, False)
    abl = modal_ablation(m, xs, y)
    with torch.no_grad():
        fmax = float(_forward_main(m, xs).abs().max())
    for i, x in enumerate(xs):
        wins = [tuple(x.shape[1:]) if j == i else None for j in range(len(xs))]
        maps, deltas = occlusion(m, xs, y, wins, baselines=0, chunk=1, sparse=False, return_deltas=True)
        assert deltas[i].shape == (1, B) and torch.equal(deltas[i][0], abl[:, i]), i
        assert torch.equal(maps[i], deltas[i][0].reshape((B,) + (1,) * (x.dim() - 1)).expand_as(x)), "one window: its delta everywhere"
        sp = occlusion(m, xs, y, wins, baselines=0, chunk=1, sparse=True, return_deltas=True)[1]
        err = float((sp[i][0] - abl[:, i]).abs().max())
        print(f"\n[bridge, input {i}] sparse - modal_ablation {err:.2e} = {err / fmax:.2e} of max|F|")
        assert err <= 2 * CHUNK_BAR * fmax
    assert untouched(m)


def test_explain_epoch_occlusion(dev):
    """the new key on F15's model and a 2 + 1 loader: key order, every sample reaches the sink once and in order, the maps are
    run.occlusion's, a skipped input counts 0, percentages sum to 100, parameters untouched"""
    from test_input_grads_models_gpu import case as f15_case
    from oaprogressionmmf_amd.run import attribution_totals, ensemble_explain_foldw, explain_epoch, occlusion
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
    (_, H, W), (_, R1, C1, S1), (_, R2, C2, S2) = (tuple(x.shape[1:]) for x in xs[:3])
    wins = [(1, H // 2, W // 2), (1, R1, C1 // 2, (S1 + 1) // 2), (1, R2, C2, (S2 + 1) // 2), None]     # 4 + 4 + 2 windows
    kw = dict(sliding_window_shapes=wins, baselines=(-0.5, -0.5, -0.5, None), chunk=2)
    acc = explain_epoch(m, loader, MODALS, explain_fn="occlusion", sink=sink, explain_kwargs=kw)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "occl_attrs", "occl_percent"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and acc["modal_names"] == [list(MODALS)] * 3
    assert [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    assert not any(torch.is_tensor(v) or isinstance(v, np.ndarray) for vals in acc.values() for v in vals), "no maps in the lists"
    for (lo, hi), (_, maps) in zip(cuts, seen):
        want = occlusion(m, [x[lo:hi] for x in xs], y[lo:hi], **kw)
        assert maps[3] is None and want[3] is None
        assert all(torch.equal(a, b) for a, b in zip(maps[:3], want[:3])), "explain_kwargs reached the function"
        np.testing.assert_array_equal(np.asarray(acc["occl_attrs"][lo:hi], dtype=np.float32)[:, :3], attribution_totals(want[:3]).cpu().numpy())
    attrs = np.asarray(acc["occl_attrs"])
    assert attrs.shape == (3, 4) and (attrs[:, 3] == 0).all() and np.abs(attrs[:, :3]).min() > 0
    np.testing.assert_allclose(np.asarray(acc["occl_percent"]).sum(1), 100.0, atol=2e-3)
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="occl")
    np.testing.assert_allclose(np.asarray(ens["occl_percent"]) * 100.0, acc["occl_percent"], atol=2e-3)
    assert untouched(m)
