"""What the clin tests share: fixture F23 (tests/golden/f23_clin.npz), its folds, and the twin's fit of every (class weight, fold)
problem of a case, computed once per process and left unchanged."""
import functools
from pathlib import Path

import numpy as np

import clin_twin as TW

GOLD = Path(__file__).resolve().parent / "golden" / "f23_clin.npz"
CASES = ("a", "b", "c", "d", "e")
WEIGHTS = (None, "balanced")
CRITERIA = ("average_precision", "roc_auc", "balanced_accuracy", "neg_log_loss")
TOL, MAX_ITER = 1e-10, 100
U53 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def get(c, name):
    return golden()[f"{c}:{name}"]


def folds(c):
    fid = get(c, "fold_id")
    return [(np.flatnonzero(fid != f), np.flatnonzero(fid == f)) for f in range(int(fid.max()) + 1)]


def cats(c):
    raw, ncat = get(c, "raw_tv"), get(c, "ncat")
    return [np.unique(raw[v]) if ncat[v] else None for v in range(raw.shape[0])]


def design_bound(c):
    """n 2^-53 max|z|: the fp64 summation bound of the mean and the variance behind a standardised column"""
    X, ncat = get(c, "X_tv"), get(c, "ncat")
    cont, col = [], 0
    for k in ncat:
        if k == 0:
            cont.append(col)
        col += max(int(k), 1)
    zmax = max(np.abs(X[:, cont]).max(), np.abs(get(c, "X_te")[:, cont]).max()) if cont else 0.0
    return X.shape[0] * U53 * zmax, cont


@functools.lru_cache(maxsize=None)
def twin_fit(c):
    """-> (SW [2 F][n], W [2 F][D + 1], infos) of the twin at the tests' tolerance; arrays are read-only"""
    X, y = get(c, "X_tv"), get(c, "y_tv")
    SW = TW.sample_weights(y, folds(c), WEIGHTS)
    W, infos = TW.fit_problems(X, y, SW, tol=TOL, max_iter=MAX_ITER)
    SW.setflags(write=False), W.setflags(write=False)
    return SW, W, infos
