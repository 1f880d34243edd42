"""GPU: the public calibration interface (various/_calibration.py) end to end against fixture F25 and the numpy twin, and
run.val_epoch's `calibration` keyword.
 * calc_calibration gives the same table for numpy inputs and for device tensors, and scikit-learn's values for the sample;
 * with bootstrap=True its resample rows are those of bootstrap_indices(seed) and its intervals equal the twin's over the same
   matrix (the log-free metrics exactly; log_loss within the kernels' log bound; the fitted ones within 1e-8, far above what
   tol = 1e-10 leaves open on these well-conditioned fits and far below anything a wrong resample would show);
 * Recalibrator("temperature") fitted on a (B, 2) logits tensor lowers the log-loss of the softmax-of-probabilities column and
   leaves its ranking unchanged: equal ROC-AUC from calc_metrics_v2 before and after, b > 0;
 * val_epoch(..., calibration={...}) returns today's dict plus the "calibration" entry; calibration=None returns today's dict."""
import numpy as np
import pytest
import torch

import calib_twin as C
import procedural as P
from test_calibration_cpu import GOLD, TOL, logloss_tol
from test_metrics_run_gpu import _batches, _same
from test_models_gpu import build

pytestmark = pytest.mark.gpu
SCALARS = ("brier", "log_loss", "ece", "mce", "calib_intercept", "calib_slope", "citl")
THR = np.linspace(0.05, 0.5, 10)


@pytest.fixture(scope="module")
def F():
    return np.load(GOLD)


def _inputs(F, n, col, where, dev):
    y, p = F[f"{n}:y"], F[f"{n}:{col}"]
    proba = np.stack([1 - p, p], axis=1)
    if where == "numpy":
        return y, proba
    return torch.from_numpy(y).to(dev).reshape(-1, 1), torch.from_numpy(proba).to(dev)     # targets as the loaders give them: (n, 1)


def _equal_tables(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], dict):
            assert list(a[k]) == list(b[k]) and all(_same(a[k][j], b[k][j]) for j in a[k]), k
        elif isinstance(a[k], tuple):
            assert _same(np.array(a[k]), np.array(b[k])), k
        else:
            assert _same(np.asarray(a[k]), np.asarray(b[k])) and type(a[k]) is type(b[k]), k


@pytest.mark.parametrize("strategy", ("uniform", "quantile"))
@pytest.mark.parametrize("n,col", [(97, "p"), (257, "p32"), (1031, "r2")])
def test_calc_calibration_plain(F, dev, n, col, strategy):
    from oaprogressionmmf_amd.various import calc_calibration
    out = calc_calibration(*_inputs(F, n, col, "device", dev), "prog_kl_72", strategy=strategy, thresholds=THR)
    _equal_tables(out, calc_calibration(*_inputs(F, n, col, "numpy", dev), "prog_kl_72", strategy=strategy, thresholds=THR))
    assert list(out) == ["sample_size", "num_pos", "num_neg", "prevalence", "mean_predicted"] + list(SCALARS) + \
        ["bin_edges", "prob_true", "prob_pred", "bin_count", "net_benefit"]
    y, s = F[f"{n}:y"], F[f"{n}:{col}"]
    assert out["sample_size"] == n and out["num_pos"] == y.sum() and out["prevalence"] == y.sum() / n
    assert abs(out["brier"] - F[f"{n}:{col}:brier"]) <= TOL and abs(out["log_loss"] - F[f"{n}:{col}:log_loss"]) <= logloss_tol(n)
    assert np.array_equal(out["prob_true"], F[f"{n}:{col}:{strategy}:prob_true"])
    assert np.abs(out["prob_pred"] - F[f"{n}:{col}:{strategy}:prob_pred"]).max() <= TOL
    if strategy == "quantile":
        assert np.array_equal(out["bin_edges"], F[f"{n}:{col}:edges"])
    fit = F[f"{n}:{col}:fit"]
    assert np.allclose([out["calib_intercept"], out["calib_slope"], out["citl"]], [fit[0, 0], fit[0, 1], fit[2, 0]], rtol=0, atol=1e-8)
    want, _, nb = C.metrics_row(s, y, out["bin_edges"], THR)
    assert [out[k] for k in ("brier", "ece", "mce")] == [want[2], want[5], want[6]] and out["bin_count"].sum() == n
    assert np.array_equal(out["net_benefit"]["net_benefit"], nb[:, 2]) and np.array_equal(out["net_benefit"]["treat_all"], nb[:, 3])
    assert np.array_equal(out["net_benefit"]["treat_none"], np.zeros(10)) and np.array_equal(out["net_benefit"]["thresholds"], THR)
    assert "n_fit_failed" not in out and "net_benefit" not in calc_calibration(*_inputs(F, n, col, "device", dev), "prog_kl_72")


@pytest.mark.parametrize("n", (97, 257))
def test_calc_calibration_bootstrap_is_the_twin_over_bootstrap_indices(F, dev, n):
    from oaprogressionmmf_amd.various import bootstrap_indices, calc_calibration, summarize_bootstrap
    kws_bs = {"n_bootstrap": 8, "seed": 3, "stratified": True, "ddof": 1, "alpha": 90}
    out = calc_calibration(*_inputs(F, n, "p", "device", dev), "tiulpin2019_prog_bin", bootstrap=True, kws_bs=kws_bs)
    _equal_tables(out, calc_calibration(*_inputs(F, n, "p", "numpy", dev), "tiulpin2019_prog_bin", bootstrap=True, kws_bs=kws_bs))
    y, s = F[f"{n}:y"], F[f"{n}:p"]
    idx = bootstrap_indices(y, 8, 3, True)
    rows, _, _ = C.metrics_rows(s, y, np.linspace(0.0, 1.0, 11), None, idx)
    x = C.x_of(s)
    free, large = C.fit_rows(x, y, "slope_intercept", idx), C.fit_rows(x, y, "intercept", idx)
    assert (free[:, 5] == 0).all() and (large[:, 5] == 0).all() and out["n_fit_failed"] == {"calib_intercept": 0, "calib_slope": 0, "citl": 0}
    cols = {"brier": rows[:, 2], "log_loss": rows[:, 3], "ece": rows[:, 5], "mce": rows[:, 6], "calib_intercept": free[:, 0],
            "calib_slope": free[:, 1], "citl": large[:, 0]}
    for k in SCALARS:
        assert isinstance(out[k], tuple) and len(out[k]) == 4, k
        want = np.array(summarize_bootstrap(cols[k][1:], rows[1:, 0], rows[1:, 1], cols[k][0], 90, 1))
        if k in ("brier", "ece", "mce"):
            assert np.array_equal(np.array(out[k]), want), k
        else:
            assert np.abs(np.array(out[k]) - want).max() <= (logloss_tol(n) if k == "log_loss" else 1e-8), k
    # another seed draws other resamples
    other = calc_calibration(*_inputs(F, n, "p", "device", dev), "tiulpin2019_prog_bin", bootstrap=True, kws_bs=dict(kws_bs, seed=4))
    assert other["brier"][0] == out["brier"][0] and other["brier"][1:] != out["brier"][1:]


def test_single_functions(F, dev):
    from oaprogressionmmf_amd import various as V
    n = 257
    y, p = F[f"{n}:y"], F[f"{n}:p01"]
    yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    for yy, pp in ((y, p), (yd, pd)):
        assert abs(V.brier_score_loss(yy, pp) - F[f"{n}:p01:brier"]) <= TOL and type(V.brier_score_loss(yy, pp)) is np.float64
        assert abs(V.log_loss(yy, pp) - F[f"{n}:p01:log_loss"]) <= logloss_tol(n)
        assert V.log_loss(yy, pp, eps=1e-3) < V.log_loss(yy, pp), "the clip reaches the certain-and-wrong samples"
        for strategy in ("uniform", "quantile"):
            pt, pr = V.calibration_curve(yy, pp, n_bins=10, strategy=strategy)
            assert np.array_equal(pt, F[f"{n}:p01:{strategy}:prob_true"]) and np.abs(pr - F[f"{n}:p01:{strategy}:prob_pred"]).max() <= TOL
            ece, mce = V.expected_calibration_error(yy, pp, strategy=strategy)
            counts = np.bincount(C.bin_of(p, _edges(F, n, strategy)), minlength=10)
            assert abs(ece - (np.abs(pt - pr) * counts[counts > 0]).sum() / n) <= TOL and abs(mce - np.abs(pt - pr).max()) <= TOL
        si = V.calibration_slope_intercept(yy, pp)
        fit = F[f"{n}:p01:fit"]
        assert list(si) == ["intercept", "slope", "citl", "mean_diff"]
        assert np.allclose([si["intercept"], si["slope"], si["citl"]], [fit[0, 0], fit[0, 1], fit[2, 0]], rtol=0, atol=1e-8)
        assert abs(si["mean_diff"] - (p.mean() - y.mean())) <= TOL
        dc = V.decision_curve(yy, pp, THR)
        nb = C.metrics_row(p, y, [0.0, 1.0], THR)[2]
        assert np.array_equal(dc["net_benefit"], nb[:, 2]) and np.array_equal(dc["treat_all"], nb[:, 3]) and not dc["treat_none"].any()
    with pytest.raises(ValueError, match="status 2"):
        V.calibration_slope_intercept(F["sep:y"], F["sep:p"])
    with pytest.raises(ValueError, match="other than 0 / 1"):
        V.brier_score_loss(yd + 1, pd)                                    # device labels are judged by the kernel


def _edges(F, n, strategy):
    return np.linspace(0.0, 1.0, 11) if strategy == "uniform" else F[f"{n}:p01:edges"]


def test_temperature_scaling_repairs_the_ensemble_column(F, dev):
    from oaprogressionmmf_amd import various as V
    n = 1031
    y, ens = F[f"{n}:y"], F[f"{n}:ens"]
    yd = torch.from_numpy(y).to(dev)
    # the reference's ensemble hands on probabilities; as logits of a two-class head they are (log(1 - p), log(p))
    logits = torch.from_numpy(np.stack([np.log1p(-ens), np.log(ens)], axis=1)).to(dev)
    rc = V.Recalibrator("temperature").fit(yd, logits)
    assert rc.b > 1.0 and rc.a == 0.0 and rc.kind == "logit" and rc.report[5] == 0, "the confined column is far too flat: T < 1"
    assert abs(rc.b - F[f"{n}:ens:fit"][1, 1]) <= 1e-8
    assert V.fit_temperature(logits, yd) == 1.0 / rc.b and V.fit_temperature(logits.cpu().numpy(), y) == 1.0 / rc.b
    after = rc.transform(logits)
    assert torch.is_tensor(after) and after.is_cuda and after.dtype == torch.float64 and after.shape == (n,)
    again = V.Recalibrator().load_state_dict(rc.state_dict()).transform(logits.cpu().numpy())
    assert isinstance(again, np.ndarray) and np.array_equal(again, after.cpu().numpy())
    before_ll, after_ll = V.log_loss(yd, torch.from_numpy(ens).to(dev)), V.log_loss(yd, after)
    assert after_ll < before_ll, (before_ll, after_ll)
    m0 = V.calc_metrics_v2(yd, torch.from_numpy(np.stack([1 - ens, ens], axis=1)).to(dev), "prog_kl_72")
    m1 = V.calc_metrics_v2(yd, torch.stack([1 - after, after], dim=1), "prog_kl_72")
    assert m0["roc_auc"] == m1["roc_auc"] and m0["avg_precision"] == m1["avg_precision"], "a monotone map moves no rank"
    # the free fit on the probabilities themselves does the same job
    free = V.Recalibrator().fit(y, ens)
    assert free.kind == "proba" and V.log_loss(y, free.transform(ens)) <= after_ll + 1e-12


def test_val_epoch_calibration(dev):
    from oaprogressionmmf_amd.run import predict_batch, val_epoch
    from oaprogressionmmf_amd.various import calc_calibration, dict_losses
    cfg = P.cfg_full(xr=(160, 160), mr1=(96, 96, 6), mr2=(96, 96, 5), depth=1)
    batches = _batches(cfg, (3, 2, 3), 77, dev)
    m = build(cfg, dev).eval()
    loss_fn = dict_losses["CrossEntropyLoss"](num_classes=2)
    plain = val_epoch(m, loss_fn, batches, target="prog_kl_72")
    none = val_epoch(m, loss_fn, batches, target="prog_kl_72", calibration=None)
    assert list(none["epoch-w"]) == list(plain["epoch-w"]) and "calibration" not in none["epoch-w"]
    assert all(_same(none["epoch-w"][k], plain["epoch-w"][k]) for k in plain["epoch-w"]) and none["batch-w"] == plain["batch-w"]
    kw = {"n_bins": 4, "thresholds": [0.2, 0.4]}
    out = val_epoch(m, loss_fn, batches, target="prog_kl_72", calibration=kw)
    assert list(out["epoch-w"]) == list(plain["epoch-w"]) + ["calibration"] and out["batch-w"] == plain["batch-w"]
    assert all(_same(out["epoch-w"][k], plain["epoch-w"][k]) for k in plain["epoch-w"])
    targets = torch.cat([ys.reshape(-1) for _, ys in batches])
    proba = torch.cat([predict_batch(m, xs)[1] for xs, _ in batches])
    _equal_tables(out["epoch-w"]["calibration"], calc_calibration(targets, proba, "prog_kl_72", **kw))
    assert out["epoch-w"]["calibration"]["sample_size"] == 8 and np.isfinite(out["epoch-w"]["calibration"]["brier"])
    with pytest.raises(ValueError, match="n_bins"):
        val_epoch(m, loss_fn, batches, target="prog_kl_72", calibration={"n_bins": 0})
