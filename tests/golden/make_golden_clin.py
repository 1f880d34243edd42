"""Fixture F23 (tests/golden/f23_clin.npz): the clinical logistic-regression baseline of koafusion/run/train_prog_clin.py as
scikit-learn computes it, on synthetic tables with the reference's variable kinds.  Needs scikit-learn (1.7.2 wrote the committed
file) and tests/clin_twin.py; reads nothing of the reference.  Run from the repository root:  python tests/golden/make_golden_clin.py

Cases (prevalence 0.12, integer ages so identical rows and exact score ties occur):
  a  n = 257, m = 65, all seven variables (D = 14), 5 stratified folds
  b  n = 64,  m = 1,  age / sex / bmi (D = 4), 5 stratified folds
  c  n = 1031, m = 129, D = 14, 5 folds of which the last holds only 2 positive rows
  d  n = 8,   m = 4,  two continuous columns, linearly separable, 4 folds of one positive and one negative row
  e  n = 300, m = 40, 31 continuous synthetic columns (D = 31, the supported maximum), 5 stratified folds

Per case `c` the file holds, under keys `c:<name>`:
  names, ncat [V] (0: continuous), raw_tv [V][n], raw_te [V][m], X_tv [n][D], X_te [m][D] (StandardScaler / OneHotEncoder fitted on
  the train-validation rows), stats [V][2], y_tv, y_te, fold_id [n] (the fold a row is held out in), and for the two class weights
  w = 0 (None), 1 ("balanced") and the two settings s in ("default", "tight" = tol 1e-12, max_iter 100000):
  dec_val_s [2][n] / proba_val_s [2][n][2] (each row by the model of the fold that holds it out), dec_te_s [2][F][m],
  proba_te_s [2][F][m][2], ens_proba_s [2][m][2], ens_pred_s [2][m], score_<criterion>_s [2][F] (sklearn's scorer on the held-out
  rows, what cross_validate returns as test_score), best_<criterion> (GridSearchCV.best_params_ as the index w), gap_default,
  gap_twin, seed, band (the share of test rows whose tight ensemble probability lies within 10 gap_twin of 0.5).
Top level: `keys`, the key list of the dict the reference's fit() pickles for F folds (what run.clin_fit's layout is held to).

Asserted here, per case (a case that fails is reseeded: the seed search below takes the first seed that passes):
  * within every held-out fold two distinct tight decision values differ by more than 1e-5;
  * the two grid candidates' mean scores differ by more than 10 gap_default for every criterion (not case d: it is separable, so
    both candidates rank every fold perfectly and tie at 1.0 by construction);
  * the default and the tight run choose the same candidate, and GridSearchCV's best_params_ is that candidate;
  * at most 1 % of the test rows lie within 10 gap_twin of 0.5 in the tight ensemble."""
import sys
from pathlib import Path

import numpy as np
from sklearn import linear_model, metrics, model_selection, preprocessing

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import clin_twin as TW  # noqa: E402

CRITERIA = ("average_precision", "roc_auc", "balanced_accuracy", "neg_log_loss")
WEIGHTS = (None, "balanced")
SETTINGS = {"default": {}, "tight": {"tol": 1e-12, "max_iter": 100000}}
VARS = ("age", "sex", "bmi", "kl", "inj", "surg", "womac")
KIND = {"age": 0, "sex": 1, "bmi": 0, "kl": 1, "inj": 1, "surg": 1, "womac": 0}


def table(rng, n, names):
    """the reference's variable kinds; the outcome follows a logistic model of them at prevalence about 0.12"""
    cols = {"age": rng.integers(45, 80, n).astype(np.float64), "sex": rng.integers(1, 3, n).astype(np.float64),
            "bmi": np.round(rng.normal(28.5, 4.5, n) * 2.0) / 2.0, "kl": rng.choice(5, n, p=[0.38, 0.18, 0.26, 0.14, 0.04]).astype(np.float64),
            "inj": (rng.random(n) < 0.3).astype(np.float64), "surg": (rng.random(n) < 0.12).astype(np.float64),
            "womac": np.round(np.abs(rng.normal(0.0, 14.0, n)))}
    # misspecified on purpose (a square and an interaction the design has no column for), so that the weighted and the
    # unweighted fit differ in more than their intercepts; the offset is set by bisection to a mean probability of 0.12
    lin = (0.02 * (cols["age"] - 60) + 0.07 * (cols["bmi"] - 28.5) + 0.03 * (cols["bmi"] - 28.5) ** 2 + 0.004 * (cols["age"] - 60) ** 2 + 0.45 * cols["kl"]
           - 0.9 * (cols["kl"] == 4) + 0.5 * cols["inj"] + 0.4 * cols["surg"] + 0.02 * cols["womac"] + 0.08 * cols["womac"] * cols["inj"] - 0.03 * cols["womac"] * cols["kl"]
           + 0.2 * (cols["sex"] == 2))
    lo, hi = -20.0, 20.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if (1.0 / (1.0 + np.exp(-(lin + mid)))).mean() < 0.12 else (lo, mid)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(lin + lo)))).astype(np.int64)
    return np.stack([cols[v] for v in names]), y


def sk_design(raw_tv, raw_te, ncat):
    tv, te, stats = [], [], np.zeros((raw_tv.shape[0], 2))
    for v in range(raw_tv.shape[0]):
        if ncat[v]:
            enc = preprocessing.OneHotEncoder().fit(raw_tv[v].reshape(-1, 1))
            tv.append(enc.transform(raw_tv[v].reshape(-1, 1)).toarray())
            te.append(enc.transform(raw_te[v].reshape(-1, 1)).toarray())
        else:
            sc = preprocessing.StandardScaler().fit(raw_tv[v].reshape(-1, 1))
            tv.append(sc.transform(raw_tv[v].reshape(-1, 1)))
            te.append(sc.transform(raw_te[v].reshape(-1, 1)))
            stats[v] = sc.mean_[0], np.sqrt(sc.var_[0])
    return np.concatenate(tv, axis=1), np.concatenate(te, axis=1), stats


def make_case(name, seed):
    rng = np.random.default_rng(seed)
    if name in ("a", "b", "c"):
        n, m = {"a": (257, 65), "b": (64, 1), "c": (1031, 129)}[name]
        names = VARS[:3] if name == "b" else VARS
        raw, y = table(rng, n + m, names)
        ncat_flag = [KIND[v] for v in names]
    elif name == "d":
        n, m, names, ncat_flag = 8, 4, ("u", "v"), [0, 0]
        y = np.array([0, 1] * 6)
        raw = np.stack([np.where(y == 1, 1.0, -1.0) * rng.uniform(0.5, 2.0, 12), rng.normal(0.0, 1.0, 12)])
    else:
        n, m, names, ncat_flag = 300, 40, tuple(f"z{j:02d}" for j in range(31)), [0] * 31
        raw = rng.normal(0.0, 1.0, (31, n + m)) * rng.uniform(0.5, 20.0, 31)[:, None] + rng.normal(0.0, 5.0, 31)[:, None]
        lin = -2.6 + (raw - raw.mean(axis=1, keepdims=True)).T @ (rng.normal(0.0, 0.35, 31) / raw.std(axis=1))
        y = (rng.random(n + m) < 1.0 / (1.0 + np.exp(-lin))).astype(np.int64)
    raw_tv, raw_te, y_tv, y_te = raw[:, :n], raw[:, n:], y[:n], y[n:]
    if name == "d":
        F, fold_id = 4, np.array([0, 0, 1, 1, 2, 2, 3, 3])
    else:
        F, fold_id = 5, np.zeros(n, np.int64)
        skf = model_selection.StratifiedKFold(5, shuffle=True, random_state=seed)
        for f, (_, va) in enumerate(skf.split(np.zeros(n), y_tv)):
            fold_id[va] = f
        if name == "c":                                   # the last fold keeps 2 positive rows, the others take the rest
            pos = np.flatnonzero((fold_id == 4) & (y_tv == 1))[2:]
            fold_id[pos] = np.arange(pos.shape[0]) % 4
    folds = [(np.flatnonzero(fold_id != f), np.flatnonzero(fold_id == f)) for f in range(F)]
    for tr, va in folds:
        assert 0 < y_tv[tr].sum() < tr.shape[0] and 0 < y_tv[va].sum() < va.shape[0], "a split with one class"
    cats, _ = TW.design_fit(raw_tv, ncat_flag)
    ncat = np.array([0 if c is None else c.shape[0] for c in cats], np.int32)
    if not all(np.isin(raw_te[v], cats[v]).all() for v in range(len(cats)) if cats[v] is not None):
        raise AssertionError("a test row holds a category the train-validation rows lack")
    X_tv, X_te, stats = sk_design(raw_tv, raw_te, ncat)
    out = {"names": np.array(names), "ncat": ncat, "raw_tv": raw_tv, "raw_te": raw_te, "X_tv": X_tv, "X_te": X_te, "stats": stats,
           "y_tv": y_tv, "y_te": y_te, "fold_id": fold_id, "seed": np.int64(seed)}
    scorers = {c: metrics.get_scorer(c) for c in CRITERIA}
    for s, kw in SETTINGS.items():
        dec_val, proba_val = np.zeros((2, n)), np.zeros((2, n, 2))
        dec_te, proba_te = np.zeros((2, F, m)), np.zeros((2, F, m, 2))
        scores = {c: np.zeros((2, F)) for c in CRITERIA}
        for w, cw in enumerate(WEIGHTS):
            for f, (tr, va) in enumerate(folds):
                est = linear_model.LogisticRegression(random_state=0, class_weight=cw, **kw).fit(X_tv[tr], y_tv[tr])
                assert est.n_iter_[0] < est.max_iter
                dec_val[w, va], proba_val[w, va] = est.decision_function(X_tv[va]), est.predict_proba(X_tv[va])
                dec_te[w, f], proba_te[w, f] = est.decision_function(X_te), est.predict_proba(X_te)
                for c in CRITERIA:
                    scores[c][w, f] = scorers[c](est, X_tv[va], y_tv[va])
        ens = proba_te.mean(axis=1)
        out.update({f"dec_val_{s}": dec_val, f"proba_val_{s}": proba_val, f"dec_te_{s}": dec_te, f"proba_te_{s}": proba_te,
                    f"ens_proba_{s}": ens, f"ens_pred_{s}": np.argmax(ens, axis=2).astype(np.int32)})
        out.update({f"score_{c}_{s}": scores[c] for c in CRITERIA})
    gap_default = max(np.abs(out["proba_val_default"] - out["proba_val_tight"]).max(),
                      np.abs(out["proba_te_default"] - out["proba_te_tight"]).max())
    # the twin
    W, _ = TW.fit_problems(X_tv, y_tv, TW.sample_weights(y_tv, folds, WEIGHTS))
    _, p_tv = TW.predict(W, X_tv)
    _, p_te = TW.predict(W, X_te)
    gap_twin = np.abs(p_te.reshape(2, F, m, 2) - out["proba_te_tight"]).max()
    for w in range(2):
        for f, (_, va) in enumerate(folds):
            gap_twin = max(gap_twin, np.abs(p_tv[w * F + f, va] - out["proba_val_tight"][w, va]).max())
    out["gap_default"], out["gap_twin"] = np.float64(gap_default), np.float64(gap_twin)
    # the assertions
    for c in CRITERIA:
        mt, md = out[f"score_{c}_tight"].mean(axis=1), out[f"score_{c}_default"].mean(axis=1)
        if name != "d":
            assert abs(mt[0] - mt[1]) > 10 * gap_default and abs(md[0] - md[1]) > 10 * gap_default, f"{c}: candidates {mt} (default run {md}) within 10 gap_default = {10 * gap_default:.2e}"
        best = int(np.argmax(mt))
        assert best == int(np.argmax(md))
        gs = model_selection.GridSearchCV(linear_model.LogisticRegression(), {"class_weight": list(WEIGHTS)}, scoring=c,
                                          cv=iter(folds), refit=False).fit(X_tv, y_tv)
        assert gs.best_params_ == {"class_weight": WEIGHTS[best]}, (c, gs.best_params_, mt)
        out[f"best_{c}"] = np.int64(best)
    for w in range(2):
        for _, va in folds:
            d = np.diff(np.unique(out["dec_val_tight"][w, va]))
            assert d.size == 0 or d.min() > 1e-5, f"two held-out decision values {d.min():.2e} apart"
    band = (np.abs(out["ens_proba_tight"][:, :, 1] - 0.5) <= 10 * gap_twin).mean()
    assert band <= 0.01, f"{band:.3f} of the test rows within 10 gap_twin of 0.5"
    out["band"] = np.float64(band)
    return out


# where each case's seed search starts (case c passes about one seed in a hundred: its two candidates rank nearly alike)
START = {"a": 2300, "b": 3300, "c": 4380, "d": 5300, "e": 6300}


def main():
    store = {}
    for i, name in enumerate("abcde"):
        for seed in range(START[name], START[name] + 1000):
            try:
                case = make_case(name, seed)
            except AssertionError as err:
                print(f"case {name} seed {seed}: {err}")
                continue
            break
        else:
            raise SystemExit(f"case {name}: no seed passed")
        print(f"case {name}: seed {seed}, n = {case['X_tv'].shape[0]}, D = {case['X_tv'].shape[1]}, positives {int(case['y_tv'].sum())}, "
              f"gap_default {case['gap_default']:.3e}, gap_twin {case['gap_twin']:.3e}, band {case['band']:.3f}, best "
              + ", ".join(f"{c}: {int(case['best_' + c])}" for c in CRITERIA))
        store.update({f"{name}:{k}": v for k, v in case.items()})
    F = 5
    store["keys"] = np.array([k for f in range(F) for k in (f"predict_proba__{f}", f"predict__{f}")] + ["predict_proba", "predict", "target"])
    np.savez_compressed(HERE / "f23_clin.npz", **store)
    print(f"wrote {HERE / 'f23_clin.npz'}: {(HERE / 'f23_clin.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main()
