"""GPU: run.clin_design / run.clin_fit and various.LogisticRegression / fit_logreg_folds against fixture F23.
 * for each of the conf file's four criteria on cases a and c, the grid search chooses GridSearchCV's best_params_; the held-out
   average_precision, roc_auc and balanced_accuracy of every (class weight, fold) equal scikit-learn's tight scores to 1e-12 (they
   depend on the ranking and on the sign of the decision values alone, and the generator asserted that distinct held-out decision
   values are more than 1e-5 apart, far above gap_twin); neg_log_loss lies within 10 gap_twin;
 * the ensemble's predict equals the fixture's on every test row whose tight ensemble probability is more than 10 gap_twin away
   from 0.5 (the generator asserted that at most 1 % of the rows are not), its predict_proba lies within 10 gap_twin;
 * numpy in -> numpy out, device tensors in -> device tensors out, the reference's key layout;
 * clin_design from a mapping of the reference's column names; the estimator's sklearn-shaped surface."""
import numpy as np
import pytest
import torch

import clin_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _args(c):
    return CC.get(c, "X_tv"), CC.get(c, "y_tv"), CC.get(c, "X_te"), CC.get(c, "y_te"), CC.folds(c)


@pytest.mark.parametrize("criterion", CC.CRITERIA)
@pytest.mark.parametrize("c", ("a", "c"))
def test_clin_fit_grid_search(dev, c, criterion):
    from oaprogressionmmf_amd import run
    X, y, Xt, yt, folds = _args(c)
    F, gap = len(folds), float(CC.get(c, "gap_twin"))
    extra = {"AGE": list(range(Xt.shape[0])), "exam_knee_id": [f"k{i}" for i in range(Xt.shape[0])]}
    res = run.clin_fit(X, y, Xt, yt, folds, criterion, params_init="grid_search", extra=extra)
    best = int(CC.get(c, f"best_{criterion}"))
    assert res["params"]["LR"] == {"class_weight": CC.WEIGHTS[best]}
    want = CC.get(c, f"score_{criterion}_tight")
    err = np.abs(res["grid_scores"]["LR"] - want).max()
    print(f"case {c} {criterion}: held-out scores {err:.2e}, means {res['grid_scores']['LR'].mean(axis=1)}")
    assert err <= (10.0 * gap if criterion == "neg_log_loss" else 1e-12)
    assert np.array_equal(res["test_score"]["LR"], res["grid_scores"]["LR"][best])
    raw = res["raw_ens"]["LR"]
    assert list(raw) == list(extra) + [str(k) for k in CC.golden()["keys"]] and raw["AGE"] is not None
    ens_t = CC.get(c, "ens_proba_tight")[best]
    assert isinstance(raw["predict_proba"], np.ndarray) and raw["predict_proba"].shape == (Xt.shape[0], 2)
    assert np.abs(raw["predict_proba"] - ens_t).max() <= 10.0 * gap
    far = np.abs(ens_t[:, 1] - 0.5) > 10.0 * gap
    assert far.mean() >= 0.99 and np.array_equal(raw["predict"][far], CC.get(c, "ens_pred_tight")[best][far])
    assert np.array_equal(raw["target"], yt)
    for f in range(F):
        assert np.abs(raw[f"predict_proba__{f}"] - CC.get(c, "proba_te_tight")[best, f]).max() <= 10.0 * gap
        assert np.array_equal(raw[f"predict__{f}"], np.argmax(raw[f"predict_proba__{f}"], axis=1))
    assert res["coef"]["LR"].shape == (F, X.shape[1] + 1) and (res["n_iter"]["LR"] < 100).all()


def test_clin_fit_prev_best_on_device_tensors(dev):
    from oaprogressionmmf_amd import run
    c = "a"
    X, y, Xt, yt, folds = _args(c)
    gap = float(CC.get(c, "gap_twin"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = run.clin_fit(t(X), t(y), t(Xt), t(yt), folds, "roc_auc")
    assert res["params"]["LR"] == {"class_weight": "balanced"} and res["grid_scores"]["LR"] is None
    raw = res["raw_ens"]["LR"]
    for k in ("predict_proba", "predict", "target", "predict_proba__0", "predict__4"):
        assert torch.is_tensor(raw[k]) and raw[k].is_cuda, k
    assert torch.is_tensor(res["coef"]["LR"]) and res["coef"]["LR"].is_cuda
    assert np.abs(raw["predict_proba"].cpu().numpy() - CC.get(c, "ens_proba_tight")[1]).max() <= 10.0 * gap
    assert np.abs(res["test_score"]["LR"] - CC.get(c, "score_roc_auc_tight")[1]).max() <= 1e-12
    # the same call on numpy arrays: the same numbers
    res_np = run.clin_fit(X, y, Xt, yt, folds, "roc_auc")
    assert np.array_equal(res_np["raw_ens"]["LR"]["predict_proba"], raw["predict_proba"].cpu().numpy())
    assert np.array_equal(res_np["raw_ens"]["LR"]["predict"], raw["predict"].cpu().numpy())
    with pytest.raises(NotImplementedError):
        run.clin_fit(X, y, Xt, yt, folds, "roc_auc", clfs=("DT",))


@pytest.mark.parametrize("c,vars", (("a", ("kl", "inj", "surg", "womac")), ("b", ())))
def test_clin_design_from_columns(dev, c, vars):
    from oaprogressionmmf_amd import run
    from oaprogressionmmf_amd.run._clin import VAR_TO_COL
    names = [str(v) for v in CC.get(c, "names")]
    assert tuple(names) == run.clin_vars(vars)
    tv = {VAR_TO_COL[v]: CC.get(c, "raw_tv")[i] for i, v in enumerate(names)}
    te = {VAR_TO_COL[v]: CC.get(c, "raw_te")[i] for i, v in enumerate(names)}
    tv["exam_knee_id"] = np.arange(len(tv["AGE"]))                # a column the design does not use
    X, Xt = run.clin_design(tv, te, vars)
    bound, _ = CC.design_bound(c)
    assert isinstance(X, np.ndarray) and np.abs(X - CC.get(c, "X_tv")).max() <= bound and np.abs(Xt - CC.get(c, "X_te")).max() <= bound
    Xd, Xtd = run.clin_design(tv, te, vars, device=dev)
    assert Xd.is_cuda and np.array_equal(Xd.cpu().numpy(), X) and np.array_equal(Xtd.cpu().numpy(), Xt)
    if c == "a":
        te["XRKL"] = te["XRKL"] + 7.0
        with pytest.raises(ValueError, match="unknown categories"):
            run.clin_design(tv, te, vars)


def test_estimator_and_batched_fit(dev):
    from oaprogressionmmf_amd.various import LogisticRegression, fit_logreg_folds
    c = "b"
    X, y, Xt, _, folds = _args(c)
    F, gap = len(folds), float(CC.get(c, "gap_twin"))
    W, report = fit_logreg_folds(X, y, folds, CC.WEIGHTS, tol=CC.TOL, max_iter=CC.MAX_ITER)
    assert tuple(W.shape) == (2 * F, X.shape[1] + 1) and W.is_cuda and (report[:, 1] <= CC.TOL).all().item()
    for w, cw in enumerate(CC.WEIGHTS):
        tr, va = folds[1]
        est = LogisticRegression(random_state=0, class_weight=cw).fit(X[tr], y[tr])
        assert est.coef_.shape == (1, X.shape[1]) and est.intercept_.shape == (1,) and isinstance(est.coef_, np.ndarray)
        assert np.array_equal(est.classes_, [0, 1]) and 0 < est.n_iter_[0] < 100
        p = est.predict_proba(X[va])
        assert np.abs(p - CC.get(c, "proba_val_tight")[w, va]).max() <= 10.0 * gap
        assert np.abs(est.predict_proba(Xt) - CC.get(c, "proba_te_tight")[w, 1]).max() <= 10.0 * gap
        assert np.abs(1.0 / (1.0 + np.exp(-est.decision_function(X[va]))) - p[:, 1]).max() <= 4.0 * CC.U53
        assert np.array_equal(est.predict(X[va]), (est.decision_function(X[va]) > 0).astype(y.dtype))
        dev_in = torch.from_numpy(X[va]).to(dev)
        assert est.predict_proba(dev_in).is_cuda and np.array_equal(est.predict_proba(dev_in).cpu().numpy(), p)
    # other labels than 0 / 1, and explicit sample weights equal to the balanced class weights
    tr = folds[0][0]
    lab = np.where(y[tr] == 1, 5, 2)
    cnt = np.bincount(y[tr], minlength=2)
    est = LogisticRegression().fit(X[tr], lab, sample_weight=(tr.shape[0] / (2.0 * cnt))[y[tr]])
    assert np.array_equal(est.classes_, [2, 5]) and set(np.unique(est.predict(X))) <= {2, 5}
    assert np.abs(est.predict_proba(X[folds[0][1]]) - CC.get(c, "proba_val_tight")[1, folds[0][1]]).max() <= 10.0 * gap
