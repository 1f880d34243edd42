"""The clinical-baseline figures of DESIGN 3.23: run.clin_fit for 5 folds x 2 class weights on a synthetic clinical table of
n = 4000 train-validation rows (age, sex, BMI, KL, injury, surgery, WOMAC: D = 14) and 1000 test rows, prevalence about 0.12.
  * device-event time of the one koaf_logreg_fit launch that fits all 10 problems, with its Newton steps, and of
    koaf_clin_design on the table;
  * wall time of a whole run.clin_design + run.clin_fit(params_init="grid_search") call per criterion on numpy arrays (uploads,
    fit, held-out scores, the one read-back, the ensemble);
  * where scikit-learn is importable, the same job there on the CPU: GridSearchCV over class_weight, cross_validate with the
    chosen one, the ensemble's predict_proba (n_jobs=1; the product needs no scikit-learn).
Nothing of the reference is read.
  python scripts/bench_clin.py [n]"""
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

COLS = {"AGE": 0, "P02SEX": 1, "P01BMI": 0, "XRKL": 1, "P01INJ-": 1, "P01KSURG-": 1, "WOMTS-": 0}
VARS = ("kl", "inj", "surg", "womac")
CRITERIA = ("average_precision", "roc_auc", "balanced_accuracy", "neg_log_loss")


def table(n, seed=0):
    rng = np.random.default_rng(seed)
    c = {"AGE": rng.integers(45, 80, n).astype(np.float64), "P02SEX": rng.integers(1, 3, n).astype(np.float64),
         "P01BMI": np.round(rng.normal(28.5, 4.5, n), 1), "XRKL": rng.choice(5, n, p=[0.38, 0.18, 0.26, 0.14, 0.04]).astype(np.float64),
         "P01INJ-": (rng.random(n) < 0.3).astype(np.float64), "P01KSURG-": (rng.random(n) < 0.12).astype(np.float64),
         "WOMTS-": np.round(np.abs(rng.normal(0.0, 14.0, n)), 1)}
    lin = -3.4 + 0.02 * (c["AGE"] - 60) + 0.07 * (c["P01BMI"] - 28.5) + 0.45 * c["XRKL"] + 0.5 * c["P01INJ-"] + 0.4 * c["P01KSURG-"] + 0.03 * c["WOMTS-"]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-lin))).astype(np.int64)
    return c, y


def folds_of(y, F=5, seed=0):
    rng = np.random.default_rng(seed)
    fid = np.zeros(y.shape[0], np.int64)
    for cls in (0, 1):
        idx = rng.permutation(np.flatnonzero(y == cls))
        fid[idx] = np.arange(idx.shape[0]) % F
    return [(np.flatnonzero(fid != f), np.flatnonzero(fid == f)) for f in range(F)]


def wall_ms(fn, runs=7, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def sklearn_side(X, y, Xt, folds):
    from sklearn import linear_model, model_selection
    for crit in CRITERIA:
        def job():
            gs = model_selection.GridSearchCV(linear_model.LogisticRegression(), {"class_weight": [None, "balanced"]}, scoring=crit,
                                              cv=iter(folds), refit=False, n_jobs=1).fit(X, y)
            cv = model_selection.cross_validate(linear_model.LogisticRegression(random_state=0, **gs.best_params_), X, y, scoring=crit,
                                                cv=iter(folds), n_jobs=1, return_estimator=True)
            return np.mean([m.predict_proba(Xt) for m in cv["estimator"]], axis=0)
        med, lo, hi = wall_ms(job, runs=5, warm=1)
        print(f"  scikit-learn, CPU, n_jobs=1, {crit:18s}: {med:8.1f} ms (min {lo:.1f}, max {hi:.1f})")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    m = n // 4
    cols, y_all = table(n + m)
    tv = {k: v[:n] for k, v in cols.items()}
    te = {k: v[n:] for k, v in cols.items()}
    y, yt = y_all[:n], y_all[n:]
    folds = folds_of(y)
    import torch
    from oaprogressionmmf_amd import ops, run
    from oaprogressionmmf_amd.various._logreg import fold_weight_rows
    dev = torch.device("cuda:0")
    X, Xt = run.clin_design(tv, te, VARS)
    print(f"n = {n}, m = {m}, D = {X.shape[1]}, positives {int(y.sum())}, 5 folds x 2 class weights")

    def event_ms(fn, runs=20, warm=3, reps=10):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        return statistics.median(ms), min(ms), max(ms)

    Xd = torch.from_numpy(X).to(dev)
    yd = torch.from_numpy(y.astype(np.int32)).to(dev)
    sw = fold_weight_rows(yd, folds, (None, "balanced"))
    flag = ops.clin_flag(dev)
    W, rep = ops.logreg_fit(Xd, yd, sw, flag=flag)
    rep = rep.cpu().numpy()
    med, lo, hi = event_ms(lambda: ops.logreg_fit(Xd, yd, sw, flag=flag))
    print(f"  koaf_logreg_fit, 10 problems in one launch: {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); Newton steps "
          f"{rep[:, 0].min():.0f}..{rep[:, 0].max():.0f}, |g|_inf <= {rep[:, 1].max():.1e}, halvings {rep[:, 3].sum():.0f}")
    med, lo, hi = event_ms(lambda: ops.logreg_fit(Xd, yd, sw[:1], flag=flag))
    print(f"  koaf_logreg_fit, 1 problem:                  {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    raw = torch.from_numpy(np.stack([tv[k] for k in COLS])).to(dev)
    ncat = [len(np.unique(tv[k])) if COLS[k] else 0 for k in COLS]
    cats = [np.unique(tv[k]) if COLS[k] else None for k in COLS]
    med, lo, hi = event_ms(lambda: ops.clin_design(raw, ncat, cats, flag=flag))
    print(f"  koaf_clin_design, fit + transform:           {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    for crit in CRITERIA:
        def job():
            A, B = run.clin_design(tv, te, VARS)
            return run.clin_fit(A, y, B, yt, folds, crit, params_init="grid_search")
        med, lo, hi = wall_ms(job)
        print(f"  clin_design + clin_fit, wall, {crit:18s}: {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}); chose {job()['params']['LR']}")
    try:
        import sklearn  # noqa: F401
    except ImportError:
        print("  scikit-learn is not importable here: its side was not timed")
        return
    sklearn_side(X, y, Xt, folds)


if __name__ == "__main__":
    main()
