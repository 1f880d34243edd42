"""CPU: the numpy twin of koaf_clin.hip (tests/clin_twin.py) against fixture F23 (scikit-learn's StandardScaler, OneHotEncoder and
LogisticRegression, written by tests/golden/make_golden_clin.py), and everything of the feature that needs no device.
 * the twin's probabilities lie within 10 gap_twin of scikit-learn at tol = 1e-12 (gap_twin is what the generator measured between
   the two on the machine that wrote the file; the 10 allows for another BLAS or platform behind the same minimiser);
 * the twin's design matrix lies within n 2^-53 max|z| of scikit-learn's, the summation bound of mean and variance; one-hot
   columns are equal;
 * koaf.h declares the three entry points, KOAF_VERSION is 200, REST_SRCS lists koaf_clin.hip, and D + 1 > 32, n < 2, K < 1 and
   null pointers come back as KOAF_EINVAL from host code;
 * "DT" raises NotImplementedError, three classes raise ValueError, and the dict clin_fit returns has the reference's keys."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import clin_cases as CC
import clin_twin as TW

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("c", CC.CASES)
def test_twin_against_scikit_learn_tight(c):
    _, W, infos = CC.twin_fit(c)
    F, gap = len(CC.folds(c)), float(CC.get(c, "gap_twin"))
    _, p_tv = TW.predict(W, CC.get(c, "X_tv"))
    _, p_te = TW.predict(W, CC.get(c, "X_te"))
    worst = np.abs(p_te.reshape(2, F, -1, 2) - CC.get(c, "proba_te_tight")).max()
    for w in range(2):
        for f, (_, va) in enumerate(CC.folds(c)):
            worst = max(worst, np.abs(p_tv[w * F + f, va] - CC.get(c, "proba_val_tight")[w, va]).max())
    its, gn = [i["iterations"] for i in infos], [i["gnorm"] for i in infos]
    print(f"case {c}: twin vs tight {worst:.3e} (gap_twin {gap:.3e}), iterations {min(its)}..{max(its)}, |g| <= {max(gn):.1e}, "
          f"halvings {sum(i['halvings'] for i in infos)}")
    assert worst <= 10.0 * gap
    assert max(its) < CC.MAX_ITER and max(gn) <= CC.TOL
    # and scikit-learn's own default run is gap_default away from its tight one, far more than the twin
    assert float(CC.get(c, "gap_default")) > 10.0 * gap


@pytest.mark.parametrize("c", CC.CASES)
def test_twin_design_against_scikit_learn(c):
    raw_tv, raw_te, ncat = CC.get(c, "raw_tv"), CC.get(c, "raw_te"), CC.get(c, "ncat")
    cats, stats = TW.design_fit(raw_tv, ncat)
    assert [0 if k is None else k.shape[0] for k in cats] == list(ncat)
    bound, cont = CC.design_bound(c)
    hot = np.setdiff1d(np.arange(CC.get(c, "X_tv").shape[1]), cont)
    for raw, want in ((raw_tv, CC.get(c, "X_tv")), (raw_te, CC.get(c, "X_te"))):
        X = TW.design(raw, cats, stats)
        assert X.shape == want.shape
        assert np.array_equal(X[:, hot], want[:, hot]) and np.isin(X[:, hot], (0.0, 1.0)).all()
        err = np.abs(X[:, cont] - want[:, cont]).max() if cont else 0.0
        print(f"case {c}: design {err:.2e} (bound {bound:.2e})")
        assert err <= bound
    want_stats = CC.get(c, "stats")
    assert np.allclose(stats, want_stats, rtol=raw_tv.shape[1] * CC.U53 * 4, atol=0.0)


def test_twin_design_refusals_and_zero_std():
    raw = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 1.0, 0.0, 1.0], [7.0, 7.0, 7.0, 7.0]])
    cats, stats = TW.design_fit(raw, [0, 1, 0], fit_idx=[0, 1, 2])
    assert stats[0, 0] == 2.0 and stats[2, 1] == 0.0
    X = TW.design(raw, cats, stats)
    assert np.array_equal(X[:, 3], np.zeros(4)) and np.array_equal(X[:, 1:3], [[1, 0], [0, 1], [1, 0], [0, 1]])
    bad = raw.copy()
    bad[1, 3] = 2.0
    with pytest.raises(ValueError, match="unknown category"):
        TW.design(bad, cats, stats)
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        TW.design(bad, cats, stats)
    with pytest.raises(ValueError, match="2 classes"):
        TW.newton(np.zeros((4, 1)), np.array([1, 1, 0, 0]), np.array([1.0, 1.0, 0.0, 0.0]))


def test_twin_ensemble_and_log_loss_against_the_fixture():
    c = "a"
    _, W, _ = CC.twin_fit(c)
    F, gap, y = len(CC.folds(c)), float(CC.get(c, "gap_twin")), CC.get(c, "y_tv")
    _, p_tv = TW.predict(W, CC.get(c, "X_tv"))
    _, p_te = TW.predict(W, CC.get(c, "X_te"))
    for w in range(2):
        mean, pred = TW.ensemble(p_te[w * F:(w + 1) * F])
        assert np.abs(mean - CC.get(c, "ens_proba_tight")[w]).max() <= 10.0 * gap
        far = np.abs(CC.get(c, "ens_proba_tight")[w][:, 1] - 0.5) > 10.0 * gap
        assert np.array_equal(pred[far], CC.get(c, "ens_pred_tight")[w][far])
        for f, (_, va) in enumerate(CC.folds(c)):
            mask = np.zeros(y.shape[0], np.int32)
            mask[va] = 1
            assert abs(TW.log_loss(p_tv[w * F + f], y, mask) + CC.get(c, "score_neg_log_loss_tight")[w, f]) <= 10.0 * gap


def test_exports_and_refusals_without_a_device():
    from oaprogressionmmf_amd import ops, run, various
    for name in ("clin_design", "logreg_fit", "logreg_predict", "clin_flag", "clin_raise"):
        assert callable(getattr(ops, name))
    assert callable(various.LogisticRegression) and callable(various.fit_logreg_folds)
    assert callable(run.clin_design) and callable(run.clin_fit)
    with pytest.raises(NotImplementedError, match="per-tree generator stream"):
        run.clin_fit(None, None, None, None, [], "roc_auc", clfs=("LR", "DT"))
    with pytest.raises(ValueError, match="Unknown criterion"):
        run.clin_fit(None, None, None, None, [], "f1")
    with pytest.raises(ValueError, match="params_init"):
        run.clin_fit(None, None, None, None, [], "roc_auc", params_init="best")
    with pytest.raises(ValueError, match="3 classes"):
        various.LogisticRegression().fit(np.zeros((6, 2)), np.array([0, 1, 2, 0, 1, 2]))
    with pytest.raises(ValueError, match="only one class"):
        various.LogisticRegression().fit(np.zeros((4, 2)), np.ones(4))
    assert run.clin_vars(("womac", "kl")) == ("age", "sex", "bmi", "kl", "womac")
    with pytest.raises(ValueError, match="Unknown clinical variables"):
        run.clin_vars(("height",))
    for word, text in ((1, "NaN"), (2, "unknown categories"), (4, "2 classes"), (8, "label")):
        with pytest.raises(ValueError, match=text):
            ops.clin_raise(word)
    ops.clin_raise(0)


def test_clin_fit_key_layout():
    from oaprogressionmmf_amd.run import _clin
    c = "a"
    _, W, _ = CC.twin_fit(c)
    F = len(CC.folds(c))
    _, p_te = TW.predict(W[F:], CC.get(c, "X_te"))
    mean, pred = TW.ensemble(p_te)
    extra = {"AGE": [1, 2], "exam_knee_id": ["x", "y"]}
    out = _clin.pack_result(list(p_te), mean, pred, CC.get(c, "y_te"), extra)
    assert list(out) == list(extra) + [str(k) for k in CC.golden()["keys"]]
    assert np.array_equal(out["predict__3"], np.argmax(p_te[3], axis=1)) and out["predict_proba"] is mean
    assert list(_clin.pack_result(list(p_te), mean, pred, CC.get(c, "y_te"))) == [str(k) for k in CC.golden()["keys"]]
    assert _clin.VAR_TO_COL == {"age": "AGE", "sex": "P02SEX", "bmi": "P01BMI", "kl": "XRKL", "inj": "P01INJ-", "surg": "P01KSURG-",
                                "womac": "WOMTS-"}


def test_header_makefile_and_version():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert protos["koaf_clin_design"] == (ctypes.c_int, [vp, i64, i32, vp, vp, vp, i64, i32, vp, vp, vp, vp])
    assert protos["koaf_logreg_fit"] == (ctypes.c_int, [vp, vp, vp, i64, i32, i32, f64, i32, f64, vp, vp, vp, vp])
    assert protos["koaf_logreg_predict"] == (ctypes.c_int, [vp, vp, i64, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp])
    d = _lib.defines()
    assert d["KOAF_VERSION"] == 200 and d["KOAF_LOGREG_MAX_P"] == 32
    mk = (ROOT / "oaprogressionmmf_amd" / "csrc" / "Makefile").read_text()
    rest = re.findall(r"^REST_SRCS\s*=(.*)$", mk, flags=re.M)
    assert len(rest) == 1 and "koaf_clin.hip" in rest[0].split()
    handle = _lib.lib()
    assert handle.koaf_version() == 200
    for name in ("koaf_clin_design", "koaf_logreg_fit", "koaf_logreg_predict"):
        assert getattr(handle, name).argtypes == protos[name][1]


def test_bad_arguments_are_refused_on_the_host():
    """every refusal comes from host code ahead of any launch: the pointers are host buffers no kernel ever sees"""
    from oaprogressionmmf_amd import _lib
    handle, d = _lib.lib(), _lib.defines()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    nc = (ctypes.c_int32 * 40)(*([0] * 40))
    pn = ctypes.addressof(nc)

    def refused(rc, text):
        assert rc == d["KOAF_EINVAL"], (rc, text)
        assert text in handle.koaf_last_error(), handle.koaf_last_error()

    fit = lambda X=p, y=p, sw=p, n=8, D=4, K=2, C=1.0, it=100, tol=1e-10, W=p, rep=p, flag=p: handle.koaf_logreg_fit(
        X, y, sw, n, D, K, C, it, tol, W, rep, flag, None)
    refused(fit(D=32), b"D + 1 <= 32")
    refused(fit(D=0), b"1 <= D")
    refused(fit(n=1), b"2 <= n")
    refused(fit(n=0), b"2 <= n")
    refused(fit(n=1 << 31), b"2 <= n")
    refused(fit(K=0), b"1..65535 problems")
    refused(fit(K=-1), b"1..65535 problems")
    refused(fit(C=0.0), b"C > 0")
    refused(fit(tol=-1.0), b"tol >= 0")
    for name in ("X", "y", "sw", "W", "rep", "flag"):
        refused(fit(**{name: None}), b"koaf_logreg_fit: null pointer")

    pred = lambda W=p, Xt=p, m=8, D=4, K=2, y=p, mask=p, ens=1, dec=p, pr=p, ll=p, ep=p, ei=p: handle.koaf_logreg_predict(
        W, Xt, m, D, K, y, mask, ens, dec, pr, ll, ep, ei, None)
    refused(pred(D=32), b"D + 1 <= 32")
    refused(pred(m=0), b"1 <= m")
    refused(pred(K=0), b"1..65535 problems")
    refused(pred(ens=2), b"ensemble is 0 or 1")
    refused(pred(y=None), b"needs y and mask")
    refused(pred(ep=None), b"needs ens_proba")
    for name in ("W", "Xt", "dec", "pr"):
        refused(pred(**{name: None}), b"koaf_logreg_predict: null pointer")

    des = lambda raw=p, n=8, V=3, ncat=pn, cats=p, idx=None, nfit=8, fit=1, stats=p, X=p, flag=p: handle.koaf_clin_design(
        raw, n, V, ncat, cats, idx, nfit, fit, stats, X, flag, None)
    refused(des(V=0), b"variables")
    refused(des(V=33), b"variables")
    refused(des(V=32), b"D + 1 <= 32")                       # 32 continuous columns and the intercept
    refused(des(n=0), b"1 <= n")
    refused(des(fit=2), b"fit is 0 or 1")
    refused(des(nfit=0), b"fitting rows")
    refused(des(nfit=5), b"fitting rows")                    # no index list: nfit is n
    for name in ("raw", "ncat", "stats", "X", "flag"):
        refused(des(**{name: None}), b"koaf_clin_design: null pointer")
    nc[1] = 2
    buf[0], buf[1] = 3.0, 3.0
    refused(des(), b"not sorted")
    refused(des(cats=None), b"koaf_clin_design: null pointer")
    nc[1] = 32
    refused(des(), b"categories")
