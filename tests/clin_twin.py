"""numpy fp64 twin of koaf_clin.hip: the design transform (StandardScaler + OneHotEncoder per variable), the damped Newton fit of
the L2-penalised logistic regression, prediction, the fold ensemble and the held-out log-loss.  It is what the device is compared
against where scikit-learn is not the yardstick, and what tests/golden/make_golden_clin.py measures `gap_twin` with.

The objective of one problem (sample weights s, S = sum s, the intercept b = w[D] is not penalised):
    f(w) = (1/S) sum_i s_i [log(1 + e^{r_i}) - y_i r_i] + |w[:D]|^2 / (2 C S),     r_i = x_i . w[:D] + b
Newton: solve H d = -g by Cholesky, then backtrack t = 1, 1/2, ... until f(w + t d) <= f(w) + 1e-4 t g.d + 4 eps |f(w)| (the
last term lets a step pass once the decrease is below what fp64 resolves in f).  Stop at |g|_inf <= tol, when no t >= 2^-30
passes, or at the iteration cap."""
import numpy as np

EPS = np.finfo(np.float64).eps
ARMIJO = 1e-4
MIN_STEP = 2.0 ** -30


# ---------------------------------------------------------------- design
def design_fit(raw, ncat, fit_idx=None):
    """raw [V][n] fp64, ncat [V] (0: continuous) -> (cats: list of sorted category arrays (None for continuous), stats [V][2] of
    (mean, population standard deviation) over the fitting rows; zeros for categorical columns)"""
    raw = np.asarray(raw, np.float64)
    rows = raw if fit_idx is None else raw[:, np.asarray(fit_idx)]
    cats, stats = [], np.zeros((raw.shape[0], 2))
    for v in range(raw.shape[0]):
        if ncat[v]:
            cats.append(np.unique(rows[v]))
        else:
            cats.append(None)
            mean = rows[v].sum() / rows.shape[1]
            stats[v] = mean, np.sqrt(((rows[v] - mean) ** 2).sum() / rows.shape[1])
    return cats, stats


def design(raw, cats, stats):
    """-> X [n][D]: (x - mean) / (std or 1) for a continuous column, one 0 / 1 column per category otherwise, in column order.
    An unknown category or a non-finite value raises ValueError."""
    raw = np.asarray(raw, np.float64)
    if not np.isfinite(raw).all():
        raise ValueError("the table holds NaN or infinity")
    out = []
    for v in range(raw.shape[0]):
        if cats[v] is None:
            scale = stats[v, 1] if stats[v, 1] != 0.0 else 1.0
            out.append(((raw[v] - stats[v, 0]) / scale)[:, None])
        else:
            hot = raw[v][:, None] == np.asarray(cats[v])[None, :]
            if not hot.any(axis=1).all():
                raise ValueError("unknown category")
            out.append(hot.astype(np.float64))
    return np.concatenate(out, axis=1)


# ---------------------------------------------------------------- fit
def sample_weights(y, folds, class_weights):
    """SW [len(class_weights) * len(folds)][n]: problem ci * F + f holds fold f's training rows with class weight ci; None -> 1,
    "balanced" -> n_train / (2 count_train(y_i)); every other row 0"""
    y = np.asarray(y).astype(np.int64)
    sw = np.zeros((len(class_weights) * len(folds), y.shape[0]))
    for ci, cw in enumerate(class_weights):
        for f, (tr, _) in enumerate(folds):
            tr = np.asarray(tr)
            if cw is None:
                sw[ci * len(folds) + f, tr] = 1.0
            elif cw == "balanced":
                cnt = np.bincount(y[tr], minlength=2)
                sw[ci * len(folds) + f, tr] = (tr.shape[0] / (2.0 * cnt))[y[tr]]
            else:
                raise ValueError(f"class_weight {cw!r}")
    return sw


def _terms(Z, y, s, w):
    r = Z @ w
    e = np.exp(-np.abs(r))
    p = np.where(r >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    loss = np.maximum(r, 0.0) + np.log1p(e) - y * r
    return r, p, loss


def objective(Z, y, s, w, C):
    S = s.sum()
    return (s * _terms(Z, y, s, w)[2]).sum() / S + (w[:-1] ** 2).sum() / (2.0 * C * S)


def grad_hess(Z, y, s, w, C):
    S = s.sum()
    _, p, _ = _terms(Z, y, s, w)
    pen = np.ones(w.shape[0])
    pen[-1] = 0.0
    g = Z.T @ (s * (p - y)) / S + pen * w / (C * S)
    H = (Z * (s * p * (1.0 - p))[:, None]).T @ Z / S + np.diag(pen) / (C * S)
    return g, H


def newton(X, y, s, C=1.0, tol=1e-10, max_iter=100):
    """-> (w [D + 1] with the intercept last, info dict: iterations, gnorm = |g|_inf, objective, halvings, lam_min of the final H)"""
    X, y, s = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(s, np.float64)
    keep = s != 0
    if np.unique(y[keep]).shape[0] < 2:
        raise ValueError("This solver needs samples of at least 2 classes in the data")
    Z = np.concatenate([X[keep], np.ones((int(keep.sum()), 1))], axis=1)
    y, s = y[keep], s[keep]
    w = np.zeros(Z.shape[1])
    f = objective(Z, y, s, w, C)
    g, H = grad_hess(Z, y, s, w, C)
    it = halvings = 0
    while it < max_iter and np.abs(g).max() > tol:
        L = np.linalg.cholesky(H)
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        slope, t = g @ d, 1.0
        while t >= MIN_STEP:
            ft = objective(Z, y, s, w + t * d, C)
            if ft <= f + ARMIJO * t * slope + 4.0 * EPS * abs(f):
                break
            t *= 0.5
            halvings += 1
        if t < MIN_STEP:
            break
        w, f = w + t * d, ft
        g, H = grad_hess(Z, y, s, w, C)
        it += 1
    return w, {"iterations": it, "gnorm": float(np.abs(g).max()), "objective": float(f), "halvings": halvings,
               "lam_min": float(np.linalg.eigvalsh(H)[0])}


def fit_problems(X, y, SW, C=1.0, tol=1e-10, max_iter=100):
    """-> (W [K][D + 1], list of the K info dicts)"""
    res = [newton(X, y, s, C, tol, max_iter) for s in np.asarray(SW)]
    return np.stack([r[0] for r in res]), [r[1] for r in res]


# ---------------------------------------------------------------- predict
def predict(W, Xt):
    """-> (decision [K][m], proba [K][m][2] = [1 - p, p])"""
    W, Xt = np.atleast_2d(W), np.asarray(Xt, np.float64)
    dec = Xt @ W[:, :-1].T + W[:, -1]
    e = np.exp(-np.abs(dec))
    p = np.where(dec >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).T
    return dec.T.copy(), np.stack([1.0 - p, p], axis=-1)


def ensemble(proba):
    """np.mean over the K problems and its argmax (first index wins ties)"""
    mean = np.mean(proba, axis=0)
    return mean, np.argmax(mean, axis=1)


def log_loss(proba, y, mask):
    """sklearn.metrics.log_loss of the rows mask selects: -mean(log(clip(p_true, eps, 1 - eps)))"""
    y = np.asarray(y).astype(np.int64)
    p = np.clip(proba[np.arange(y.shape[0]), y], EPS, 1.0 - EPS)
    sel = np.asarray(mask) != 0
    return float(-np.log(p[sel]).sum() / sel.sum())
