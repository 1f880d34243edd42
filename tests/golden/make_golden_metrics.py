#!/usr/bin/env python3
"""Generate fixture F18 (tests/golden/f18_metrics.npz): the REFERENCE's calc_metrics_v2 / calc_bootstrap on small cases.

The reference's koafusion/various/_metrics_stat_anlys.py and _metrics_wissam.py are loaded by file path under a stub package
(koafusion/various/__init__.py pulls in cv2).  Needs scikit-learn and scipy (the fixture was written with scikit-learn 1.7.2).
Nothing of the reference is modified: its module globals are wrapped while it runs --
  * roc_auc_score / average_precision_score / average_precision_score_calib by recorders, which gives the PER-RESAMPLE values of
    the four metrics in the order calc_metrics_v2 asks for them (roc_auc, avg_precision, avg_ppv_calib, avg_npv: kept + 1 calls each,
    the last one the point estimate);
  * np.round by the identity for a second run, which gives the UNROUNDED outputs.
Per case <c> (a, b, c, d, f, g: see case_inputs) the file holds
  <c>:target int64 [n], <c>:proba [n, 2] (fp32 or fp64), <c>:par = (R, seed, stratified, pi0 * 1e6) int64
  <c>:plain / <c>:plain_raw     the 8 rounded / unrounded values of KEYS_PLAIN (bootstrap=False); cutoff additionally as <c>:cutoff in
                                the scores' dtype
  <c>:bs / <c>:bs_raw           [5, 4]: prevalence (repeated) and the (value, std_err, ci_l, ci_h) of the four metrics
  <c>:vals [4, kept]            the per-resample values, <c>:kept the number of resamples kept
  <c>:idx_kept [kept, n] int32  the index sets the reference drew for its kept resamples
case e: e:off [401], e:target, e:score (fp32, concatenated), e:cutoff [400] fp32 -- sensitivity_specificity_cutoff only.
case h: h:target, h:proba and the single-class return as h:keys (names) / h:values.
The generator asserts that no unrounded value lies within 1e-8 of a rounding tie at three decimals (so rounded outputs compare
exactly) and that case g skips some but not all of its resamples.  Outputs only -- no reference source, bytecode or pickle.

Usage:  python tests/golden/make_golden_metrics.py <path of the reference checkout>
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
KEYS_PLAIN = ("prevalence", "roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv", "cutoff", "youdens_index", "b_accuracy")
KEYS_BS = ("prevalence", "roc_auc", "avg_precision", "avg_ppv_calib", "avg_npv")
TARGET = "prog_kl_72"


def load_reference(ref):
    various = Path(ref) / "koafusion" / "various"
    pkg = types.ModuleType("_ref_various")
    pkg.__path__ = [str(various)]
    sys.modules["_ref_various"] = pkg
    mods = []
    for name in ("_metrics_wissam", "_metrics_stat_anlys"):
        spec = importlib.util.spec_from_file_location(f"_ref_various.{name}", str(various / f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods[1]


class _NumpyNoRound(object):
    """numpy with round() the identity: the reference's outputs before `np.round(v, 3)`"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def round(v, decimals=0):
        return v


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def proba_from_logit(lg, dtype):
    """two-class probabilities of the logit difference lg: [n, 2], rows sum to one (up to rounding)"""
    z = np.stack([np.zeros_like(lg), lg], axis=1).astype(dtype)
    return softmax(z).astype(dtype)


def case_inputs(name):
    """-> (target int64 [n], proba [n, 2], R, seed, stratified)"""
    if name == "a":
        rng = np.random.RandomState(101)
        y = np.zeros(37, np.int64); y[rng.permutation(37)[:5]] = 1
        lg = np.round((rng.randn(37) + 1.2 * y) * 4) / 4
        return y, proba_from_logit(lg, np.float32), 64, 0, True
    if name == "b":
        rng = np.random.RandomState(202)
        y = (rng.rand(300) < 0.12).astype(np.int64)
        lg = rng.randn(300) + 1.0 * y
        return y, proba_from_logit(lg, np.float32), 64, 0, True
    if name == "c":
        rng = np.random.RandomState(303)
        y = (rng.rand(2503) < 0.2).astype(np.int64)
        lg = np.round((rng.randn(2503) + 0.8 * y) * 8) / 8
        return y, proba_from_logit(lg, np.float32), 32, 0, True
    if name == "d":
        rng = np.random.RandomState(404)
        y = (rng.rand(200) < 0.3).astype(np.int64)
        base = np.repeat(rng.rand(100) * 0.8 + 0.1, 2)
        p1 = base + np.tile([0.0, 1e-12], 100)           # pairs 1e-12 apart: equal in fp32, distinct in fp64
        perm = rng.permutation(200)
        p1 = p1[perm]
        assert len(np.unique(p1)) == 200 and len(np.unique(p1.astype(np.float32))) <= 100
        return y, np.stack([1.0 - p1, p1], axis=1), 16, 0, True
    if name == "f":
        y = np.zeros(20, np.int64); y[[1, 4, 7, 8, 15, 19]] = 1
        return y, np.full((20, 2), 0.5, np.float32), 8, 0, True
    if name == "g":
        rng = np.random.RandomState(0)
        y = np.zeros(30, np.int64); y[[3, 17]] = 1
        lg = rng.randn(30) + 1.0 * y
        return y, proba_from_logit(lg, np.float32), 200, 0, False
    raise KeyError(name)


def tie_free(v, what):
    """no value within 1e-8 of a rounding tie at three decimals"""
    v = np.asarray(v, np.float64).ravel()
    v = v[np.isfinite(v)]
    frac = np.abs(v * 1000.0 - np.floor(v * 1000.0) - 0.5)
    assert (frac > 1e-5).all(), f"{what}: a value sits on a rounding tie, change the case's seed: {v[frac <= 1e-5]}"


def run_case(ref, name, out):
    y, proba, R, seed, stratified = case_inputs(name)
    n = y.shape[0]
    pi0 = 0.12
    kws_bs = {"n_bootstrap": R, "seed": seed, "stratified": stratified, "verbose": False}
    out[f"{name}:target"], out[f"{name}:proba"] = y, proba
    out[f"{name}:par"] = np.array([R, seed, int(stratified), round(pi0 * 1e6)], np.int64)

    plain = ref.calc_metrics_v2(y, proba, TARGET)
    assert tuple(plain)[:4] == ("sample_size", "num_pos", "num_neg", "prevalence") and tuple(plain)[4:] == KEYS_PLAIN[1:]
    assert plain["sample_size"] == n and plain["num_pos"] == y.sum()
    assert plain["cutoff"].dtype == proba.dtype
    out[f"{name}:cutoff"] = np.asarray(plain["cutoff"])
    out[f"{name}:plain"] = np.array([float(plain[k]) for k in KEYS_PLAIN])

    # per-resample values: recorders around the metric callables the module looks up at call time
    rec = {"roc": [], "ap": [], "calib": []}
    saved = (ref.roc_auc_score, ref.average_precision_score, ref.average_precision_score_calib)

    def wrap(fn, key):
        def f(*a, **k):
            v = fn(*a, **k)
            rec[key].append(float(v))
            return v
        return f
    ref.roc_auc_score, ref.average_precision_score, ref.average_precision_score_calib = (
        wrap(saved[0], "roc"), wrap(saved[1], "ap"), wrap(saved[2], "calib"))
    try:
        bs = ref.calc_metrics_v2(y, proba, TARGET, bootstrap=True, kws_bs=kws_bs)
    finally:
        ref.roc_auc_score, ref.average_precision_score, ref.average_precision_score_calib = saved
    assert tuple(bs) == ("sample_size", "num_pos", "num_neg") + KEYS_BS
    kept = len(rec["roc"]) - 1
    assert len(rec["calib"]) == kept + 1 and len(rec["ap"]) == 2 * (kept + 1)
    vals = np.array([rec["roc"][:kept], rec["ap"][:kept], rec["calib"][:kept], rec["ap"][kept + 1:2 * kept + 1]])
    out[f"{name}:vals"], out[f"{name}:kept"] = vals, np.int64(kept)
    out[f"{name}:bs"] = np.array([np.broadcast_to(np.asarray(bs[k], np.float64), (4,)) for k in KEYS_BS])
    if name == "g":
        assert 0 < R - kept < R, f"case g keeps {kept} of {R}"
        print(f"  case g keeps {kept} of {R} resamples")
    else:
        assert kept == R

    # the index sets: a metric that returns nothing but records the `y_pred` it is handed, with y_pred = arange(n)
    drawn = []

    def keep_idx(t, p):
        drawn.append(np.asarray(p, np.int32).copy())
        return 0.0
    ref.calc_bootstrap(keep_idx, y, np.arange(n), n_bootstrap=R, seed=seed, stratified=stratified, verbose=False)
    assert len(drawn) == kept + 1 and (drawn[-1] == np.arange(n)).all()
    out[f"{name}:idx_kept"] = np.stack(drawn[:kept])

    # unrounded outputs
    np_saved = ref.np
    ref.np = _NumpyNoRound()
    try:
        plain_raw = ref.calc_metrics_v2(y, proba, TARGET)
        bs_raw = ref.calc_metrics_v2(y, proba, TARGET, bootstrap=True, kws_bs=kws_bs)
    finally:
        ref.np = np_saved
    out[f"{name}:plain_raw"] = np.array([float(plain_raw[k]) for k in KEYS_PLAIN])
    out[f"{name}:bs_raw"] = np.array([np.broadcast_to(np.asarray(bs_raw[k], np.float64), (4,)) for k in KEYS_BS])
    tie_free(out[f"{name}:plain_raw"], f"case {name} plain")
    tie_free(out[f"{name}:bs_raw"], f"case {name} bootstrap")
    nocut = [i for i, k in enumerate(KEYS_PLAIN) if k != "cutoff"]             # (the cutoff is rounded in the scores' dtype)
    assert np.array_equal(np.round(out[f"{name}:plain_raw"], 3)[nocut], out[f"{name}:plain"][nocut])
    assert np.round(plain_raw["cutoff"], 3) == plain["cutoff"] and np.asarray(plain_raw["cutoff"]).dtype == proba.dtype
    assert np.array_equal(np.round(out[f"{name}:bs_raw"], 3), out[f"{name}:bs"])
    print(f"  case {name}: n = {n}, R = {R}, plain {dict(zip(KEYS_PLAIN, out[f'{name}:plain']))}")


def run_case_e(ref, out):
    rng = np.random.RandomState(505)
    off, ys, ss, cut = [0], [], [], []
    for _ in range(400):
        n = int(rng.randint(8, 60))
        y = np.zeros(n, np.int64); y[rng.permutation(n)[:n // 2]] = 1          # balanced
        s = (np.round((rng.randn(n) + 0.7 * y) * 2) / 2).astype(np.float32)      # quantised: tie groups
        s = (1.0 / (1.0 + np.exp(-s))).astype(np.float32)
        c = ref.sensitivity_specificity_cutoff(y, s)
        assert np.asarray(c).dtype == np.float32
        ys.append(y); ss.append(s); cut.append(c); off.append(off[-1] + n)
    out["e:off"], out["e:target"], out["e:score"] = np.array(off, np.int64), np.concatenate(ys), np.concatenate(ss)
    out["e:cutoff"] = np.array(cut, np.float32)
    print(f"  case e: 400 sets, {off[-1]} samples, {int(np.isinf(out['e:cutoff']).sum())} infinite cutoffs")


def run_case_h(ref, out):
    y = np.ones(12, np.int64)
    proba = proba_from_logit(np.linspace(-1, 1, 12), np.float32)
    r = ref.calc_metrics_v2(y, proba, TARGET)
    out["h:target"], out["h:proba"] = y, proba
    out["h:keys"] = np.array(list(r))
    out["h:values"] = np.array([float(v) for v in r.values()])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    out = {}
    for name in ("a", "b", "c", "d", "f", "g"):
        run_case(ref, name, out)
    run_case_e(ref, out)
    run_case_h(ref, out)
    path = HERE / "f18_metrics.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
