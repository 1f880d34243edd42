"""The permutation-test figures of DESIGN 3.18 at the size of an OAI test set: N = 3000 knees, R = 1000 permutations.
  * device-event time of the two launches: koaf_pair_ranks (fp32 and fp64 scores, read through the probability tensors'
    stride) and koaf_perm_metrics with the identity row and all R rows -- warm-up, then the median of RUNS runs of REPS
    back-to-back calls;
  * wall time of a whole various.compare_predictions call on device tensors (the mask draw on the host, its upload, two launches,
    the one copy back and the p-value arithmetic), and of the mask draw alone.
Synthetic scores of two correlated models (prevalence 0.12, logits quantised to 1/64: tie groups, within and across the models);
nothing of the reference is read.
  python scripts/bench_permtest.py [N] [R]
  python scripts/bench_permtest.py --scipy [N] [R]     the same inputs through scipy.stats.permutation_test around scikit-learn's
                                                       metrics, on the CPU (needs both; the product needs neither)"""
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

RUNS, WARM, REPS = 20, 3, 20


def inputs(N):
    rng = np.random.RandomState(0)
    y = (rng.rand(N) < 0.12).astype(np.int64)
    base = rng.randn(N) + 1.0 * y
    p = []
    for sd in (0.8, 0.7):
        lg = np.round((base + sd * rng.randn(N)) * 64) / 64
        p1 = 1.0 / (1.0 + np.exp(-lg))
        p.append(np.stack([1.0 - p1, p1], axis=1))
    return y, p[0], p[1]


def scipy_side(N, R):
    from functools import partial
    from scipy import stats
    from sklearn.metrics import average_precision_score, roc_auc_score
    y, pa, pb = inputs(N)

    def statistic(x0, x1, fn):
        return fn(y, x1) - fn(y, x0)
    t0 = time.perf_counter()
    out = {}
    for name, fn in (("roc_auc", roc_auc_score), ("ap", average_precision_score)):
        ret = stats.permutation_test(data=(pa[:, 1].astype(np.float32), pb[:, 1].astype(np.float32)), permutation_type="samples",
                                     n_resamples=R, alternative="two-sided", statistic=partial(statistic, fn=fn))
        out[f"pvalue__{name}"], out[f"statistic__{name}"] = ret.pvalue, ret.statistic
    print(f"N = {N}, R = {R}: scipy.stats.permutation_test x 2 around scikit-learn, CPU: {(time.perf_counter() - t0) * 1e3:.0f} ms")
    print(out)


def main():
    args = [a for a in sys.argv[1:] if a != "--scipy"]
    N = int(args[0]) if len(args) > 0 else 3000
    R = int(args[1]) if len(args) > 1 else 1000
    if "--scipy" in sys.argv[1:]:
        return scipy_side(N, R)
    import torch
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.various import compare_predictions, swap_masks
    dev = torch.device("cuda:0")

    def event_ms(fn, runs=RUNS, warm=WARM, reps=REPS):
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

    def wall_ms(fn, runs=7, warm=2):
        for _ in range(warm):
            fn()
        ms = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms), max(ms)

    y, pa, pb = inputs(N)
    masks, exact = swap_masks(N, R, 0)
    a32, b32 = torch.from_numpy(pa.astype(np.float32)).to(dev), torch.from_numpy(pb.astype(np.float32)).to(dev)
    a64, b64 = torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev)
    yd, y32 = torch.from_numpy(y).to(dev), torch.from_numpy(y.astype(np.int32)).to(dev)
    md = torch.from_numpy(masks.view(np.int32)).to(dev)
    flag = ops.metrics_flag(dev)
    _, packed = ops.pair_ranks(a32[:, 1], b32[:, 1], y32, flag=flag)
    out = torch.empty((R + 1, 8), dtype=torch.float64, device=dev)
    rows = [("koaf_pair_ranks fp32", lambda: ops.pair_ranks(a32[:, 1], b32[:, 1], y32, flag=flag)),
            ("koaf_pair_ranks fp64", lambda: ops.pair_ranks(a64[:, 1], b64[:, 1], y32, flag=flag)),
            (f"koaf_perm_metrics 1 + {R} rows", lambda: ops.perm_metrics(packed, md, True, out=out, flag=flag)),
            ("koaf_perm_metrics identity only", lambda: ops.perm_metrics(packed, None, True, out=out[:1], flag=flag))]
    print(f"N = {N}, R = {R}: device-event time per launch (median of {RUNS} x {REPS} back-to-back calls, wrapper included)")
    for name, fn in rows:
        med, lo, hi = event_ms(fn)
        print(f"  {name:36s} {med * 1e3:9.1f} us  (min {lo * 1e3:.1f} max {hi * 1e3:.1f})")
    assert int(flag.item()) == 0 and not exact
    print("wall time per call, device tensors in, the row out (median of 7)")
    for name, fn in (("compare_predictions fp32", lambda: compare_predictions(yd, a32, b32, n_resamples=R)),
                     ("compare_predictions fp64", lambda: compare_predictions(yd, a64, b64, n_resamples=R)),
                     ("swap_masks alone (host)", lambda: swap_masks(N, R, 0))):
        med, lo, hi = wall_ms(fn)
        print(f"  {name:40s} {med:9.2f} ms  (min {lo:.2f} max {hi:.2f})")
    print(compare_predictions(yd, a32, b32, n_resamples=R))


if __name__ == "__main__":
    main()
