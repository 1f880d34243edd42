"""GPU: koaf_clin_design, koaf_logreg_fit and koaf_logreg_predict (through ops) against fixture F23 and the numpy twin the CPU
tests pin to it.

The bound of the fit against the twin.  The objective f is strongly convex with modulus lam = lambda_min(H) near its minimiser, so
two points u, v satisfy lam |u - v|^2 <= (grad f(u) - grad f(v)) . (u - v), hence |u - v|_2 <= |grad f(u) - grad f(v)|_2 / lam.  Both
the twin and the device stop at a gradient of |g|_inf <= tol, the twin's being the measured one; with |g|_2 <= sqrt(P) |g|_inf the
distance of two such points is bounded by sqrt(P) |g|_inf / lam, both numbers taken from the twin's final iterate.  A decision
value is z_i . w with z_i = (x_i, 1), so it moves by at most max_i |z_i|_2 times that, and a probability by a quarter of it (the
logistic function's slope is at most 1/4).  The near-null directions of the design (a one-hot group against the intercept) make
lam as small as 1 / (C S) while no row sees them, so the bound is loose by orders of magnitude where it is large and still
above the rounding of a dot product where it is small.

Against scikit-learn: within 10 gap_twin of its run at tol = 1e-12 and within 3 gap_default of its default run; both gaps were
measured by the generator and are stored in the fixture (gap_default is what lbfgs's own stopping rule leaves open, the 3 covers
the device sitting on the other side of the minimiser)."""
import numpy as np
import pytest
import torch

import clin_cases as CC
import clin_twin as TW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: the shared twin arrays are read-only


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64)


def _fit(c, dev, sw=None, X=None, **kw):
    from oaprogressionmmf_amd import ops
    SW, _, _ = CC.twin_fit(c)
    X = _dev(CC.get(c, "X_tv") if X is None else X, dev)
    y = _dev(CC.get(c, "y_tv").astype(np.int32), dev)
    return ops.logreg_fit(X, y, _dev(SW if sw is None else sw, dev), tol=CC.TOL, max_iter=CC.MAX_ITER, **kw)


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("c", CC.CASES)
def test_design_against_the_fixture(dev, c):
    from oaprogressionmmf_amd import ops
    raw_tv, raw_te, ncat = CC.get(c, "raw_tv"), CC.get(c, "raw_te"), [int(k) for k in CC.get(c, "ncat")]
    cats = CC.cats(c)
    bound, cont = CC.design_bound(c)
    X, stats = ops.clin_design(_dev(raw_tv, dev), ncat, cats)
    Xt, stats_t = ops.clin_design(_dev(raw_te, dev), ncat, cats, stats=stats)
    assert stats_t is stats
    hot = np.setdiff1d(np.arange(X.shape[1]), cont)
    for got, want in ((X.cpu().numpy(), CC.get(c, "X_tv")), (Xt.cpu().numpy(), CC.get(c, "X_te"))):
        assert got.shape == want.shape
        assert np.isin(got[:, hot], (0.0, 1.0)).all() and np.array_equal(got[:, hot], want[:, hot])
        err = np.abs(got[:, cont] - want[:, cont]).max() if cont else 0.0
        print(f"case {c}: design {err:.2e} (bound {bound:.2e})")
        assert err <= bound
    # fit = 0 with the stored mean and standard deviation reproduces fit = 1 bit for bit
    again, _ = ops.clin_design(_dev(raw_tv, dev), ncat, cats, stats=stats.clone())
    assert np.array_equal(_bits(again), _bits(X))
    # the fitting rows as an index list: the twin's statistics over the same rows
    idx = np.arange(0, raw_tv.shape[1], 2)
    _, st_idx = ops.clin_design(_dev(raw_tv, dev), ncat, cats, fit_idx=_dev(idx.astype(np.int32), dev))
    _, want = TW.design_fit(raw_tv, ncat, idx)
    assert np.allclose(st_idx.cpu().numpy(), want, rtol=4 * idx.shape[0] * CC.U53, atol=4 * idx.shape[0] * CC.U53 * np.abs(raw_tv).max())


def test_design_refusals(dev):
    from oaprogressionmmf_amd import ops
    raw, ncat, cats = CC.get("a", "raw_tv").copy(), [int(k) for k in CC.get("a", "ncat")], CC.cats("a")
    sex = list(CC.get("a", "names")).index("sex")
    bad = raw.copy()
    bad[sex, 256] = 3.0                                        # the row past the first 256
    with pytest.raises(ValueError, match="unknown categories"):
        ops.clin_design(_dev(bad, dev), ncat, cats)
    for v in (0, sex):
        bad = raw.copy()
        bad[v, 100] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            ops.clin_design(_dev(bad, dev), ncat, cats)
    bad = raw.copy()
    bad[0, 5] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        ops.clin_design(_dev(bad, dev), ncat, cats)
    with pytest.raises(ValueError, match="index outside"):
        ops.clin_design(_dev(raw, dev), ncat, cats, fit_idx=_dev(np.array([0, 1, raw.shape[1]], np.int32), dev))
    const = np.stack([np.full(9, 7.0), np.arange(9.0)])
    X, stats = ops.clin_design(_dev(const, dev), [0, 0], [None, None])
    assert stats[0, 1].item() == 0.0 and np.array_equal(X[:, 0].cpu().numpy(), np.zeros(9))      # a zero std scales by 1


# ---------------------------------------------------------------- fit
@pytest.mark.parametrize("c", CC.CASES)
def test_fit_all_problems_in_one_launch(dev, c):
    SW, Wt, infos = CC.twin_fit(c)
    K, P = Wt.shape
    F = K // 2
    X_tv, X_te = CC.get(c, "X_tv"), CC.get(c, "X_te")
    # NaN-filled with a guard row either side: only W [K][D + 1] is written
    big = torch.full((K + 2, P), float("nan"), dtype=torch.float64, device=dev)
    W, report = _fit(c, dev, out=big[1:K + 1])
    assert W.data_ptr() == big[1].data_ptr()
    host = big.cpu().numpy()
    assert np.isnan(host[0]).all() and np.isnan(host[-1]).all() and np.isfinite(host[1:-1]).all()
    Wd, rep = host[1:-1], report.cpu().numpy()
    print(f"case {c}: device steps {rep[:, 0].min():.0f}..{rep[:, 0].max():.0f}, |g| <= {rep[:, 1].max():.1e}, halvings {rep[:, 3].sum():.0f}")
    assert (rep[:, 1] <= CC.TOL).all() and (rep[:, 0] < CC.MAX_ITER).all()
    assert np.allclose(rep[:, 2], [i["objective"] for i in infos], rtol=1e-12, atol=0.0)
    # against the twin: the strong-convexity bound of the module docstring, per problem
    znorm = max(np.sqrt((X_tv ** 2).sum(axis=1) + 1.0).max(), np.sqrt((X_te ** 2).sum(axis=1) + 1.0).max())
    for X in (X_tv, X_te):
        dec_d, p_d = TW.predict(Wd, X)
        dec_t, p_t = TW.predict(Wt, X)
        for k in range(K):
            bound = infos[k]["gnorm"] * np.sqrt(P) / infos[k]["lam_min"] * znorm
            e_dec, e_p = np.abs(dec_d[k] - dec_t[k]).max(), np.abs(p_d[k] - p_t[k]).max()
            print(f"case {c} problem {k}: decision {e_dec:.2e} proba {e_p:.2e} (bound {bound:.2e})")
            assert e_dec <= bound and e_p <= bound / 4.0
    # against scikit-learn, tight and default
    gap_t, gap_d = float(CC.get(c, "gap_twin")), float(CC.get(c, "gap_default"))
    _, p_tv = TW.predict(Wd, X_tv)
    _, p_te = TW.predict(Wd, X_te)
    for s, lim in (("tight", 10.0 * gap_t), ("default", 3.0 * gap_d)):
        worst = np.abs(p_te.reshape(2, F, -1, 2) - CC.get(c, f"proba_te_{s}")).max()
        for w in range(2):
            for f, (_, va) in enumerate(CC.folds(c)):
                worst = max(worst, np.abs(p_tv[w * F + f, va] - CC.get(c, f"proba_val_{s}")[w, va]).max())
        print(f"case {c}: device vs scikit-learn {s} {worst:.3e} (limit {lim:.3e})")
        assert worst <= lim
    # two launches: the same bits
    W2, rep2 = _fit(c, dev)
    assert np.array_equal(_bits(W2), Wd.view(np.int64)) and np.array_equal(_bits(rep2), rep.view(np.int64))


def test_fit_case_b_as_one_problem(dev):
    SW, Wt, infos = CC.twin_fit("b")
    Wall, _ = _fit("b", dev)
    for k in (0, SW.shape[0] - 1):
        W1, rep = _fit("b", dev, sw=SW[k:k + 1])
        assert tuple(W1.shape) == (1, Wt.shape[1]) and rep[0, 1].item() <= CC.TOL and rep[0, 0].item() < CC.MAX_ITER
        assert np.array_equal(_bits(W1[0]), _bits(Wall[k]))                 # a block's arithmetic does not depend on its neighbours
        X = CC.get("b", "X_tv")
        bound = infos[k]["gnorm"] * np.sqrt(Wt.shape[1]) / infos[k]["lam_min"] * np.sqrt((X ** 2).sum(axis=1) + 1.0).max()
        assert np.abs(TW.predict(W1.cpu().numpy(), X)[0] - TW.predict(Wt[k:k + 1], X)[0]).max() <= bound


def test_fit_rows_of_weight_zero_do_not_count(dev):
    c = "a"
    SW, _, _ = CC.twin_fit(c)
    X = CC.get(c, "X_tv")
    out = np.flatnonzero(SW[0] == 0.0)
    assert out.size > 1
    X2 = X.copy()
    X2[out] = X[out[::-1]] * 3.0 + 1.0                          # other values in the rows the problem leaves out
    X2[out[0]] = np.nan                                          # and one that would poison every sum it entered
    W1, _ = _fit(c, dev, sw=SW[0:1])
    W2, _ = _fit(c, dev, sw=SW[0:1], X=X2)
    assert np.isfinite(W1.cpu().numpy()).all() and np.array_equal(_bits(W1), _bits(W2))


def test_fit_separable_with_a_weak_penalty(dev):
    """case d at C = 1e6: the penalty is all that keeps the separable problem finite; sixteen Newton steps to |w| of about 14"""
    from oaprogressionmmf_amd import ops
    X, y = CC.get("d", "X_tv"), CC.get("d", "y_tv")
    wt, info = TW.newton(X, y, np.ones(8), C=1e6, tol=CC.TOL, max_iter=CC.MAX_ITER)
    W, rep = ops.logreg_fit(_dev(X, dev), _dev(y.astype(np.int32), dev), torch.ones((1, 8), dtype=torch.float64, device=dev), C=1e6,
                            tol=CC.TOL, max_iter=CC.MAX_ITER)
    rep = rep.cpu().numpy()[0]
    print(f"separable: device {rep}, twin {info}")
    assert np.isfinite(W.cpu().numpy()).all() and rep[1] <= CC.TOL and rep[0] < CC.MAX_ITER
    bound = info["gnorm"] * np.sqrt(3.0) / info["lam_min"] * np.sqrt((X ** 2).sum(axis=1) + 1.0).max()
    assert np.abs(TW.predict(W.cpu().numpy(), X)[0] - TW.predict(wt[None], X)[0]).max() <= bound


def test_fit_refusals(dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    c = "b"
    SW, _, _ = CC.twin_fit(c)
    y = CC.get(c, "y_tv")
    one = SW[0:2].copy()
    one[1, y == 1] = 0.0                                        # the second problem keeps negatives only
    with pytest.raises(ValueError, match="2 classes"):
        _fit(c, dev, sw=one)
    flag = ops.clin_flag(dev)
    W, _ = _fit(c, dev, sw=one, flag=flag)
    W = W.cpu().numpy()
    assert flag.item() == 4 and np.isfinite(W[0]).all() and np.isnan(W[1]).all()
    neg = SW[0:1].copy()
    neg[0, 3] = -1.0
    with pytest.raises(ValueError, match="negative sample weight"):
        _fit(c, dev, sw=neg)
    X = _dev(CC.get(c, "X_tv"), dev)
    with pytest.raises(KoafError, match="D \\+ 1 <= 32"):
        ops.logreg_fit(torch.zeros((8, 32), dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                       torch.ones((1, 8), dtype=torch.float64, device=dev))
    with pytest.raises(KoafError, match="sw is"):
        ops.logreg_fit(X, _dev(y.astype(np.int32), dev), torch.ones((1, 5), dtype=torch.float64, device=dev))


# ---------------------------------------------------------------- predict
@pytest.mark.parametrize("c", ("a", "b", "e"))
def test_predict_ensemble_and_log_loss(dev, c):
    from oaprogressionmmf_amd import ops
    SW, _, _ = CC.twin_fit(c)
    K = SW.shape[0]
    F, y = K // 2, CC.get(c, "y_tv")
    W, _ = _fit(c, dev)
    Wh = W.cpu().numpy()
    gap = float(CC.get(c, "gap_twin"))
    # the fold ensemble of each class weight on the test rows, against the twin on the same coefficients
    X_te = CC.get(c, "X_te")
    for w in range(2):
        res = ops.logreg_predict(W[w * F:(w + 1) * F].contiguous(), _dev(X_te, dev), ensemble=True)
        dec_t, p_t = TW.predict(Wh[w * F:(w + 1) * F], X_te)
        mean_t, pred_t = TW.ensemble(p_t)
        # a dot product of D + 1 terms and an exp, log1p-free: (D + 2) 2^-53 sum|x_a w_a| on the decision, a quarter of it and
        # a few ulp on a probability
        mag = (np.abs(X_te)[None] * np.abs(Wh[w * F:(w + 1) * F, None, :-1])).sum(axis=2) + np.abs(Wh[w * F:(w + 1) * F, -1:])
        tol_dec = (X_te.shape[1] + 2) * CC.U53 * mag.max()
        tol_p = tol_dec / 4.0 + 8.0 * CC.U53
        dec, p, ens = res["decision"].cpu().numpy(), res["proba"].cpu().numpy(), res["ens_proba"].cpu().numpy()
        assert np.abs(dec - dec_t).max() <= tol_dec and np.abs(p - p_t).max() <= tol_p and np.abs(ens - mean_t).max() <= tol_p
        assert np.abs(p.sum(axis=2) - 1.0).max() <= 2.0 ** -52                 # [1 - p, p] sums to 1 within one ulp
        assert np.array_equal(p[:, :, 0], 1.0 - p[:, :, 1])
        pred = res["ens_pred"].cpu().numpy()
        assert pred.dtype == np.int32 and np.array_equal(pred, np.argmax(ens, axis=1))
        far = np.abs(mean_t[:, 1] - 0.5) > tol_p
        assert np.array_equal(pred[far], pred_t[far])
        assert np.abs(ens - CC.get(c, "ens_proba_tight")[w]).max() <= 10.0 * gap
    # a tie goes to the first index, as np.argmax
    tie = ops.logreg_predict(torch.zeros((2, X_te.shape[1] + 1), dtype=torch.float64, device=dev), _dev(X_te, dev), ensemble=True)
    assert (tie["ens_proba"] == 0.5).all().item() and (tie["ens_pred"] == 0).all().item()
    # held-out log-loss per problem against sklearn.metrics.log_loss of the tight run
    mask = np.zeros((K, y.shape[0]), np.int32)
    for k in range(K):
        mask[k, CC.folds(c)[k % F][1]] = 1
    res = ops.logreg_predict(W, _dev(CC.get(c, "X_tv"), dev), y=_dev(y.astype(np.int32), dev), mask=_dev(mask, dev))
    ll = res["logloss"].cpu().numpy().reshape(2, F)
    err = np.abs(ll + CC.get(c, "score_neg_log_loss_tight")).max()
    print(f"case {c}: log-loss {err:.2e} (limit {10.0 * gap:.2e})")
    assert err <= 10.0 * gap
    none = ops.logreg_predict(W, _dev(CC.get(c, "X_tv"), dev), y=_dev(y.astype(np.int32), dev), mask=_dev(np.zeros_like(mask), dev))
    assert torch.isnan(none["logloss"]).all().item()
