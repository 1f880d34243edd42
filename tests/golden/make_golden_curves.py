#!/usr/bin/env python3
"""Generate fixture F22 (tests/golden/f22_curves.npz): the REFERENCE's ROC / PR curves, recall-range average precision and
calibrated F1 scores on small cases.

The reference is loaded as make_golden_metrics.py loads it (by file path, under a stub package); nothing of it is modified or
copied.  Its avg_precision_at_recall_range and calc_metrics_v2(with_curves=True) pass `probas_pred=` to scikit-learn's
precision_recall_curve, a keyword scikit-learn 1.7 removed, so the module's global `precision_recall_curve` is wrapped, while it
runs, by a shim that hands `probas_pred` on as `y_score` (the technique make_golden_metrics.py uses for its recorders).
Needs scikit-learn and scipy; their versions and numpy's are recorded as `versions`.

Cases: a, b, c, d, f, g of make_golden_metrics.case_inputs, and
  k  n = 257, no ties (two bins per thread run, trailing runs empty)      l  n = 5000, quantised logits (the 16384-bin kernels)
  m  perfectly separated (full recall early, a 4-point ROC)                p  the lowest score is a positive (nothing truncated)
  q  n = 2
Per case <c>, with s = proba[:, 1] and pi0 = 0.12:
  <c>:target int64 [n], <c>:proba [n, 2], <c>:par = (R, seed, stratified, pi0 * 1e6) int64
  <c>:roc_fpr / roc_tpr / roc_thr          sklearn's roc_curve(target, s)
  <c>:pr_prec / pr_rec / pr_thr            sklearn's precision_recall_curve(target, s)
  <c>:prc_prec / prc_rec / prc_thr         the reference's precision_recall_curve_calib(target, s, pi0=pi0)
  <c>:prn_prec / prn_rec                   the same with pi0=None
  <c>:keys                                 the key order of calc_metrics_v2(with_curves=True), whose three curves are asserted
                                           equal to the arrays above
  <c>:apr [3]                              avg_precision_at_recall_range over RANGES
  <c>:bf1 [2], <c>:f1c [2]                 bestf1score_calib(target, s) and f1score_calib(target, s > 0.5) with pi0 = 0.12 / None
  <c>:apc                                  average_precision_score_calib(target, s, pi0=pi0)
  <c>:rs_apr [3, kept], <c>:rs_bf1 [kept]  the per-resample values over the case's kept resamples, <c>:kept their number (the
                                           index sets are various.bootstrap_indices': asserted here)
  <c>:bs_apr [3, 4], <c>:bs_bf1 [4]        calc_bootstrap's (value, std_err, ci_l, ci_h) around those
mc:true / mc:pred int64 [n] (K = 4 classes, class 2 absent from mc:true), mc:bacc = mc_bacc(true, pred), mc:cm the counts.
The generator asserts that every case runs through the reference without an exception and with finite values.
Outputs and inputs only -- no reference source, bytecode or pickle.

Usage:  python tests/golden/make_golden_curves.py <path of the reference checkout>
"""
import sys
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_metrics import TARGET, case_inputs, load_reference, proba_from_logit  # noqa: E402

RANGES = ((0.0, 1.0), (0.2, 0.8), (0.75, 1.0))
OLD_CASES = ("a", "b", "c", "d", "f", "g")
NEW_CASES = ("k", "l", "m", "p", "q")
PI0 = 0.12


def new_case_inputs(name):
    """-> (target int64 [n], proba [n, 2], R, seed, stratified)"""
    if name == "k":
        rng = np.random.RandomState(606)
        y = (rng.rand(257) < 0.25).astype(np.int64)
        p = proba_from_logit(rng.randn(257) + 0.9 * y, np.float32)
        assert len(np.unique(p[:, 1])) == 257
        return y, p, 8, 0, True
    if name == "l":
        rng = np.random.RandomState(707)
        y = (rng.rand(5000) < 0.15).astype(np.int64)
        lg = np.round((rng.randn(5000) + 0.8 * y) * 16) / 16
        return y, proba_from_logit(lg, np.float32), 6, 0, True
    if name == "m":
        rng = np.random.RandomState(808)
        y = np.zeros(40, np.int64); y[rng.permutation(40)[:9]] = 1
        lg = 4.0 * y + rng.rand(40) - 0.5
        assert lg[y == 1].min() > lg[y == 0].max()
        return y, proba_from_logit(lg, np.float32), 8, 0, True
    if name == "p":
        rng = np.random.RandomState(909)
        y = (rng.rand(60) < 0.3).astype(np.int64)
        lg = rng.randn(60) + 1.0 * y
        lg[np.flatnonzero(y == 1)[0]] = lg.min() - 1.0
        assert y[np.argmin(lg)] == 1
        return y, proba_from_logit(lg, np.float32), 8, 0, True
    if name == "q":
        return np.array([0, 1], np.int64), proba_from_logit(np.array([-0.8, 0.4]), np.float32), 4, 0, True
    raise KeyError(name)


class shimmed(object):
    """while active, the module's precision_recall_curve takes `probas_pred` for `y_score`"""

    def __init__(self, ref):
        self.ref, self.saved = ref, ref.precision_recall_curve

    def __enter__(self):
        saved = self.saved

        def shim(y_true, y_score=None, *, probas_pred=None, **kw):
            return saved(y_true, y_score if probas_pred is None else probas_pred, **kw)
        self.ref.precision_recall_curve = shim

    def __exit__(self, *exc):
        self.ref.precision_recall_curve = self.saved


def run_case(ref, wis, name, out):
    from oaprogressionmmf_amd.various import bootstrap_indices
    y, proba, R, seed, stratified = case_inputs(name) if name in OLD_CASES else new_case_inputs(name)
    n, s = y.shape[0], proba[:, 1]
    out[f"{name}:target"], out[f"{name}:proba"] = y, proba
    out[f"{name}:par"] = np.array([R, seed, int(stratified), round(PI0 * 1e6)], np.int64)

    fpr, tpr, rthr = ref.roc_curve(y, s)
    with shimmed(ref):
        prec, rec, thr = ref.precision_recall_curve(y, probas_pred=s)
        full = ref.calc_metrics_v2(y, proba, TARGET, with_curves=True)
        apr = [ref.avg_precision_at_recall_range(y, s, recall_range=r) for r in RANGES]
    cprec, crec, cthr = wis.precision_recall_curve_calib(y, s, pi0=PI0)
    nprec, nrec, _ = wis.precision_recall_curve_calib(y, s, pi0=None)
    assert tuple(full)[-3:] == ("roc_curve", "pr_curve", "pr_calib_curve")
    for got, want in zip(full["roc_curve"] + full["pr_curve"] + full["pr_calib_curve"], (fpr, tpr, prec, rec, cprec, crec)):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert rthr.dtype == thr.dtype == cthr.dtype == proba.dtype
    out[f"{name}:keys"] = np.array(list(full))
    for key, v in (("roc_fpr", fpr), ("roc_tpr", tpr), ("roc_thr", rthr), ("pr_prec", prec), ("pr_rec", rec), ("pr_thr", thr),
                   ("prc_prec", cprec), ("prc_rec", crec), ("prc_thr", cthr), ("prn_prec", nprec), ("prn_rec", nrec)):
        out[f"{name}:{key}"] = np.asarray(v)
    out[f"{name}:apr"] = np.array(apr, np.float64)
    pred = (s > 0.5).astype(np.int64)
    out[f"{name}:bf1"] = np.array([wis.bestf1score_calib(y, s, pi0=PI0), wis.bestf1score_calib(y, s, pi0=None)], np.float64)
    out[f"{name}:f1c"] = np.array([wis.f1score_calib(y, pred, pi0=PI0), wis.f1score_calib(y, pred, pi0=None)], np.float64)
    out[f"{name}:apc"] = np.float64(wis.average_precision_score_calib(y, s, pi0=PI0))

    # per-resample values and the bootstrap summaries: recorders around the metric handed to the reference's calc_bootstrap
    idx = bootstrap_indices(y, R, seed, stratified)
    keep = y[idx].sum(axis=1) != 0
    kws = dict(n_bootstrap=R, seed=seed, stratified=stratified, verbose=False)

    def recorded(fn):
        vals, drawn = [], []

        def f(t, p):
            v = fn(t, p[:, 0])
            vals.append(float(v)); drawn.append(p[:, 1].astype(np.int32))
            return v
        both = np.stack([s.astype(np.float64), np.arange(n, dtype=np.float64)], axis=1)      # the scores and which sample they are
        summary = ref.calc_bootstrap(f, y, both, **kws)
        assert len(vals) == int(keep.sum()) + 1 and np.array_equal(np.stack(drawn[:-1]), idx[keep]), "bootstrap_indices replays it"
        return np.array(vals[:-1]), np.array([float(v) for v in summary])
    rs, bs = [], []
    with shimmed(ref):
        for r in RANGES:
            v, b = recorded(lambda t, p, r=r: ref.avg_precision_at_recall_range(t, p.astype(proba.dtype), recall_range=r))
            rs.append(v); bs.append(b)
    out[f"{name}:rs_apr"], out[f"{name}:bs_apr"] = np.array(rs), np.array(bs)
    out[f"{name}:rs_bf1"], out[f"{name}:bs_bf1"] = recorded(lambda t, p: wis.bestf1score_calib(t, p.astype(proba.dtype), pi0=PI0))
    out[f"{name}:kept"] = np.int64(keep.sum())
    if name == "g":
        assert 0 < R - int(keep.sum()) < R
    for key in ("apr", "bf1", "f1c", "apc", "rs_apr", "rs_bf1", "bs_apr", "bs_bf1"):
        assert np.isfinite(out[f"{name}:{key}"]).all(), f"case {name}: {key} is not finite"
    assert np.array_equal(out[f"{name}:bs_apr"][:, 0], out[f"{name}:apr"]) and out[f"{name}:bs_bf1"][0] == out[f"{name}:bf1"][0]
    print(f"  case {name}: n = {n}, thresholds {thr.shape[0]}, roc points {fpr.shape[0]}, calibrated points {cprec.shape[0]}, "
          f"apr {out[f'{name}:apr']}, bf1 {out[f'{name}:bf1']}, f1c {out[f'{name}:f1c']}")


def run_multiclass(ref, out):
    from sklearn.metrics import confusion_matrix
    rng = np.random.RandomState(111)
    t = rng.choice([0, 1, 3], size=90, p=[0.5, 0.3, 0.2]).astype(np.int64)
    p = np.where(rng.rand(90) < 0.6, t, rng.randint(0, 4, size=90)).astype(np.int64)
    assert 2 not in t and 2 in p
    out["mc:true"], out["mc:pred"] = t, p
    out["mc:bacc"] = np.float64(ref.mc_bacc(t, p))
    out["mc:cm"] = confusion_matrix(t, p, labels=[0, 1, 2, 3]).astype(np.int64)
    print(f"  multi-class: mc_bacc {out['mc:bacc']}")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import scipy
    import sklearn
    ref = load_reference(sys.argv[1])
    wis = sys.modules["_ref_various._metrics_wissam"]
    out = {"versions": np.array([f"scikit-learn {sklearn.__version__}", f"scipy {scipy.__version__}", f"numpy {np.__version__}"])}
    for name in OLD_CASES + NEW_CASES:
        run_case(ref, wis, name, out)
    run_multiclass(ref, out)
    path = HERE / "f22_curves.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
