"""GPU: various.calc_metrics_v2 / calc_bootstrap end to end against fixture F18 (the reference's outputs), and run.val_epoch.
 * calc_metrics_v2 with device tensors and with numpy inputs, plain and bootstrap: the rounded outputs equal the reference's
   exactly (the generator keeps every unrounded value 1e-8 clear of a rounding tie), the unrounded ones are within 1e-10 (the
   kernels' bound, tests/test_metrics_kernels_gpu.py), with the reference's keys, key order and value types;
 * calc_bootstrap by metric name, including case g's skipped resamples (stratified=False);
 * val_epoch over three batches of the run tests' model: epoch-w is calc_metrics_v2 of the concatenated predict_batch
   probabilities, loss_prog the rounded per-batch losses (FocalLoss and CrossEntropyLoss, under no_grad), parameters and
   BatchNorm buffers unchanged, no gradient allocated."""
from pathlib import Path

import numpy as np
import pytest
import torch

import procedural as P
from test_models_gpu import build, t

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "f18_metrics.npz"
CASES = ("a", "b", "c", "d", "f", "g")
HEAD = ("sample_size", "num_pos", "num_neg")
KEYS_PLAIN = ("prevalence", "roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv", "cutoff", "youdens_index", "b_accuracy")
KEYS_BS = KEYS_PLAIN[:5]
TOL = 1e-10


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def case(F, c):
    R, seed, strat, pi0 = (int(v) for v in F[f"{c}:par"])
    return F[f"{c}:target"], F[f"{c}:proba"], {"n_bootstrap": R, "seed": seed, "stratified": bool(strat)}, {"pi0": pi0 / 1e6}


def _inputs(y, p, where, dev):
    if where == "numpy":
        return y, p
    return torch.from_numpy(y).to(dev).reshape(-1, 1), torch.from_numpy(p).to(dev)      # targets as the loaders give them: (n, 1)


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("where", ("device", "numpy"))
@pytest.mark.parametrize("c", CASES)
def test_calc_metrics_v2_plain(F, dev, c, where):
    from oaprogressionmmf_amd.various import _metrics as M, calc_metrics_v2
    y, p, _, kws_ppv = case(F, c)
    yy, pp = _inputs(y, p, where, dev)
    out = calc_metrics_v2(yy, pp, "prog_kl_72", kws_ppv=kws_ppv)
    assert tuple(out) == HEAD + KEYS_PLAIN
    assert out["sample_size"] == y.shape[0] and isinstance(out["sample_size"], int)
    assert out["num_pos"] == y.sum() and out["num_neg"] == (y == 0).sum() and isinstance(out["num_pos"], np.int64)
    for i, k in enumerate(KEYS_PLAIN):
        assert type(out[k]) is (p.dtype.type if k == "cutoff" else np.float64), k
        assert float(out[k]) == F[f"{c}:plain"][i], f"{k}: {out[k]!r} against the reference's {F[f'{c}:plain'][i]!r}"
    raw = M.calc_metrics_unrounded(yy, pp, "prog_kl_72", kws_ppv=kws_ppv)
    assert raw["cutoff"] == F[f"{c}:plain_raw"][5]
    for i, k in enumerate(KEYS_PLAIN):
        if k != "cutoff":
            assert abs(float(raw[k]) - F[f"{c}:plain_raw"][i]) < TOL, k


@pytest.mark.parametrize("where", ("device", "numpy"))
@pytest.mark.parametrize("c", CASES)
def test_calc_metrics_v2_bootstrap(F, dev, c, where):
    from oaprogressionmmf_amd.various import _metrics as M, calc_metrics_v2
    y, p, kws_bs, kws_ppv = case(F, c)
    yy, pp = _inputs(y, p, where, dev)
    out = calc_metrics_v2(yy, pp, "tiulpin2019_prog_bin", bootstrap=True, kws_ppv=kws_ppv, kws_bs=kws_bs)
    assert tuple(out) == HEAD + KEYS_BS
    assert type(out["prevalence"]) is np.float64 and out["prevalence"] == F[f"{c}:bs"][0, 0]
    for i, k in enumerate(KEYS_BS[1:], 1):
        assert isinstance(out[k], np.ndarray) and out[k].shape == (4,) and out[k].dtype == np.float64, k
        assert np.array_equal(out[k], F[f"{c}:bs"][i]), f"{k}: {out[k]} against the reference's {F[f'{c}:bs'][i]}"
    raw = M.calc_metrics_unrounded(yy, pp, "tiulpin2019_prog_bin", bootstrap=True, kws_ppv=kws_ppv, kws_bs=kws_bs)
    for i, k in enumerate(KEYS_BS[1:], 1):
        assert isinstance(raw[k], tuple) and len(raw[k]) == 4
        assert np.abs(np.array(raw[k]) - F[f"{c}:bs_raw"][i]).max() < TOL, k


def test_calc_bootstrap_by_name(F, dev):
    from oaprogressionmmf_amd.various import calc_bootstrap
    for c in ("a", "g"):
        y, p, kws_bs, kws_ppv = case(F, c)
        for i, metric in enumerate(("roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv"), 1):
            col = p[:, 0] if metric == "avg_npv" else p[:, 1]
            got = calc_bootstrap(metric, y, col, verbose=False, **kws_bs, **kws_ppv)
            assert np.abs(np.array(got) - F[f"{c}:bs_raw"][i]).max() < TOL, (c, metric)
            got_dev = calc_bootstrap(metric, torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)[:, 0 if metric == "avg_npv" else 1],
                                     **kws_bs, **kws_ppv)
            assert got_dev == got
    # ddof reaches the standard error; alpha the percentiles
    y, p, kws_bs, _ = case(F, "a")
    a = calc_bootstrap("roc_auc", y, p[:, 1], **kws_bs)
    b = calc_bootstrap("roc_auc", y, p[:, 1], ddof=1, alpha=90., **kws_bs)
    assert b[1] == pytest.approx(a[1] * np.sqrt(64 / 63), rel=1e-12) and b[2] >= a[2] and b[3] <= a[3]


def test_calc_metrics_v2_device_edge_cases(F, dev):
    from oaprogressionmmf_amd.various import calc_metrics_v2
    y, p = torch.from_numpy(F["h:target"]).to(dev), torch.from_numpy(F["h:proba"]).to(dev)
    out = calc_metrics_v2(y, p, "prog_kl_72")                         # single class, known only after the device pass
    assert list(out) == [str(k) for k in F["h:keys"]]
    assert _same(list(out.values()), F["h:values"])
    y, p, *_ = case(F, "a")
    q = p.copy()
    q[7, 1] = np.nan
    for where in ("device", "numpy"):
        with pytest.raises(ValueError, match="NaN or infinity"):
            calc_metrics_v2(*_inputs(y, q, where, dev), "prog_kl_72")
    with pytest.raises(ValueError, match="Unknown target"):
        calc_metrics_v2(*_inputs(y, p, "device", dev), "kl")


def _batches(cfg, sizes, seed, dev):
    out = []
    for i, B in enumerate(sizes):
        xs = tuple(t(a).to(dev) for a in P.model_inputs(cfg, B, seed + i))
        out.append((xs, t(P.make_target("target", B, seed + i)).to(dev)))
    return out


def test_val_epoch(dev):
    from oaprogressionmmf_amd.run import predict_batch, val_epoch
    from oaprogressionmmf_amd.various import calc_metrics_v2, dict_losses
    cfg = P.cfg_full(xr=(160, 160), mr1=(96, 96, 6), mr2=(96, 96, 5), depth=1)
    batches = _batches(cfg, (3, 2, 3), 77, dev)
    targets = torch.cat([ys.reshape(-1) for _, ys in batches])
    assert 0 < int(targets.sum()) < targets.numel(), "both classes"
    m = build(cfg, dev).eval()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert any("running_mean" in k for k in before)
    pred = [predict_batch(m, xs) for xs, _ in batches]
    want = calc_metrics_v2(targets, torch.cat([pr for _, pr in pred]), "prog_kl_72")
    assert np.isfinite(want["roc_auc"]) and set(want) >= {"b_accuracy", "avg_precision"}
    for name, kw in (("FocalLoss", dict(reduction="mean", gamma=2.0, num_classes=2)), ("CrossEntropyLoss", dict(num_classes=2))):
        loss_fn = dict_losses[name](**kw)
        with torch.no_grad():
            losses = [float(loss_fn(lg.squeeze(1), ys.long().squeeze(1))) for (lg, _), (_, ys) in zip(pred, batches)]
        out = val_epoch(m, loss_fn, iter(batches), target="prog_kl_72")
        assert list(out) == ["batch-w", "epoch-w"] and list(out["batch-w"]) == ["loss_prog"]
        assert out["batch-w"]["loss_prog"] == [np.round(v, 3) for v in losses], name
        assert all(type(v) is np.float64 for v in out["batch-w"]["loss_prog"])
        assert list(out["epoch-w"]) == list(want)
        assert all(_same(out["epoch-w"][k], want[k]) and type(out["epoch-w"][k]) is type(want[k]) for k in want)
    assert all(p.grad is None for p in m.parameters()), "a gradient was allocated"
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before), "the pass changed the model"
    # kws_metrics reach calc_metrics_v2; an unknown target is refused
    bs = val_epoch(m, loss_fn, batches, target="prog_kl_72", kws_metrics={"bootstrap": True, "kws_bs": {"n_bootstrap": 8}})
    assert "cutoff" not in bs["epoch-w"] and bs["epoch-w"]["roc_auc"].shape == (4,)
    with pytest.raises(ValueError, match="Unknown target"):
        val_epoch(m, loss_fn, batches, target="kl")
    with pytest.raises(ValueError, match="no batches"):
        val_epoch(m, loss_fn, [], target="prog_kl_72")
