"""Writes tests/golden/f25_calibration.npz: what scikit-learn (1.7.2) and numpy say about the calibration of seeded synthetic
cohorts -- the oracles of tests/test_calibration_cpu.py and of the GPU tests, which read only this file and tests/calib_twin.py.
The reference has no calibration code, so nothing of it is recorded here.

Cohorts (prevalence 0.12, n = 97 / 257 / 1031, one RandomState(5) stream): y ~ Bernoulli(0.12) redrawn until the count of
positives is round(0.12 n); z = 1.2 N(0, 1) + (1.0 if y else -1.5); p = sigmoid(z).  Columns of each cohort:
  p      the single-model probabilities (fp64)
  ens    softmax((1 - p, p))[1]: the softmax-of-probabilities column of the reference's fold ensemble, confined to [0.269, 0.731]
  r2     p rounded to two decimals: scores on the uniform edges, heavy ties
  p01    p with exact 0.0 and 1.0 planted (two of each, one of them on the wrong class): the clip of log-loss and of the logit
  p32    p narrowed to fp32; its records are those of the fp32 values widened to fp64 (the device's arithmetic is fp64 whatever the
         score dtype; scikit-learn would clip an fp32 column at fp32's eps and numpy would interpolate its percentiles in fp32)
Per cohort and column: brier_score_loss, log_loss, calibration_curve(n_bins=10) for both strategies, np.percentile edges for 10
bins, and the recalibration parameters of the three modes from the twin's Newton run to max|g| / n <= 1e-13.
One perfectly separable set (sep: 58 logits, y = logit > 0.75, with their sigmoid as probabilities) closes the file: no finite
intercept / slope exists, while the slope alone (temperature) and the intercept alone still have an optimum.

Run from the repository root:  python tests/golden/make_golden_calibration.py
"""
import sys
from pathlib import Path

import numpy as np
from sklearn.calibration import calibration_curve
from sklearn.metrics import brier_score_loss, log_loss

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import calib_twin as C  # noqa: E402

SIZES = (97, 257, 1031)
COLUMNS = ("p", "ens", "r2", "p01", "p32")
NBINS = 10
FIT_TOL = 1e-13


def cohorts():
    rs = np.random.RandomState(5)
    out = {}
    for n in SIZES:
        want = int(round(0.12 * n))
        y = rs.rand(n) < 0.12
        while int(y.sum()) != want:
            y = rs.rand(n) < 0.12
        z = 1.2 * rs.randn(n) + np.where(y, 1.0, -1.5)
        p = 1.0 / (1.0 + np.exp(-z))
        e1, e0 = np.exp(p), np.exp(1.0 - p)
        p01 = p.copy()
        pos, neg = np.flatnonzero(y), np.flatnonzero(~y)
        p01[pos[0]], p01[neg[0]] = 1.0, 0.0            # certain and right
        p01[pos[1]], p01[neg[1]] = 0.0, 1.0            # certain and wrong: the clip decides the log-loss
        out[n] = {"y": y.astype(np.int64), "p": p, "ens": e1 / (e1 + e0), "r2": np.round(p, 2), "p01": p01, "p32": p.astype(np.float32)}
    return out


def main():
    rec = {}
    q = np.linspace(0, 1, NBINS + 1)
    for n, c in cohorts().items():
        y = c["y"]
        rec[f"{n}:y"] = y
        for col in COLUMNS:
            s = c[col]
            rec[f"{n}:{col}"] = s
            w = s.astype(np.float64)                   # (exact)
            rec[f"{n}:{col}:brier"] = np.float64(brier_score_loss(y, w))
            rec[f"{n}:{col}:log_loss"] = np.float64(log_loss(y, w))
            for strategy in ("uniform", "quantile"):
                pt, pp = calibration_curve(y, w, n_bins=NBINS, strategy=strategy)
                rec[f"{n}:{col}:{strategy}:prob_true"], rec[f"{n}:{col}:{strategy}:prob_pred"] = pt, pp
            rec[f"{n}:{col}:edges"] = np.percentile(w, q * 100)
            x = C.x_of(w)
            rec[f"{n}:{col}:fit"] = np.stack([C.fit_row(x, y, mode, tol=FIT_TOL, max_iter=100) for mode in C.MODES])
    xs = np.linspace(-3.0, 3.0, 61)
    xs = xs[np.abs(xs) > 0.05]
    rec["sep:logit"] = xs
    rec["sep:p"] = 1.0 / (1.0 + np.exp(-xs))
    rec["sep:y"] = (xs > 0.75).astype(np.int64)        # (not separated by the starting line (0, 1): Newton has to walk there)
    rec["sep:fit"] = np.stack([C.fit_row(xs, rec["sep:y"], mode, tol=FIT_TOL, max_iter=100) for mode in C.MODES])
    np.savez_compressed(HERE / "f25_calibration.npz", **rec)
    print(f"{len(rec)} arrays, {(HERE / 'f25_calibration.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main()
