"""The calibration figures of DESIGN 3.30 at the size of an OAI test set: n = 4000 knees, 10 bins, 32 thresholds, R = 1000
resamples.
  * device-event time per launch: koaf_calib_edges, koaf_calib_metrics (identity row + all R rows, with the bin table and the
    threshold table; and the identity row alone), koaf_recalib_fit (free fit and intercept-only, 1 + R rows) -- warm-up, then
    the median of RUNS runs of REPS back-to-back calls;
  * wall time of a whole various.calc_calibration(bootstrap=True) call on device tensors (the index draw on the host, its upload,
    four launches, the one copy back, the percentile summary) and, in the same run, of various.calc_metrics_v2(bootstrap=True) at
    the same n and R; of the index draw alone; of both tables without the bootstrap.
Synthetic scores (prevalence 0.12, the cohort of the tests' fixture at n = 4000); nothing of the reference is read.
  python scripts/bench_calibration.py [N] [R]"""
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

RUNS, WARM, REPS = 10, 2, 5
NBINS, NTHR = 10, 32


def inputs(N):
    rng = np.random.RandomState(5)
    y = (rng.rand(N) < 0.12).astype(np.int64)
    z = 1.2 * rng.randn(N) + np.where(y == 1, 1.0, -1.5)
    p1 = 1.0 / (1.0 + np.exp(-z))
    return y, np.stack([1.0 - p1, p1], axis=1)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    import torch
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.various import bootstrap_indices, calc_calibration, calc_metrics_v2
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

    def wall_ms(fn, runs=5, warm=1):
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

    y, proba = inputs(N)
    thr = np.linspace(0.01, 0.6, NTHR)
    idx = bootstrap_indices(y, R, 0, True)
    pd, yd = torch.from_numpy(proba).to(dev), torch.from_numpy(y).to(dev)
    p32 = pd.to(torch.float32)
    y32, idx_d, thr_d = yd.to(torch.int32), torch.from_numpy(idx).to(dev), torch.from_numpy(thr).to(dev)
    q = torch.from_numpy(np.linspace(0, 1, NBINS + 1) * 100 / 100).to(dev)
    edges = torch.from_numpy(np.linspace(0.0, 1.0, NBINS + 1)).to(dev)
    flag = ops.calib_flag(dev)
    out = torch.empty((R + 1, 8), dtype=torch.float64, device=dev)
    bins = torch.empty((R + 1, NBINS, 3), dtype=torch.float64, device=dev)
    nb = torch.empty((R + 1, NTHR, 4), dtype=torch.float64, device=dev)
    rep = torch.empty((R + 1, 8), dtype=torch.float64, device=dev)
    rows = [("koaf_calib_edges fp64", lambda: ops.calib_edges(pd[:, 1], q, flag=flag)),
            ("koaf_calib_edges fp32", lambda: ops.calib_edges(p32[:, 1], q, flag=flag)),
            (f"koaf_calib_metrics 1 + {R} rows", lambda: ops.calib_metrics(pd[:, 1], y32, edges, thr_d, idx_d, True, out=out, bins=bins, nb=nb, flag=flag)),
            ("koaf_calib_metrics identity only", lambda: ops.calib_metrics(pd[:, 1], y32, edges, thr_d, None, True, out=out[:1], bins=bins[:1], nb=nb[:1], flag=flag)),
            (f"koaf_recalib_fit free, 1 + {R} rows", lambda: ops.recalib_fit(pd[:, 1], y32, "proba", "slope_intercept", idx=idx_d, out=rep, flag=flag)),
            (f"koaf_recalib_fit intercept, 1 + {R} rows", lambda: ops.recalib_fit(pd[:, 1], y32, "proba", "intercept", idx=idx_d, out=rep, flag=flag))]
    print(f"n = {N}, R = {R}, {NBINS} bins, {NTHR} thresholds on {torch.cuda.get_device_name(0)}: device-event time per launch "
          f"(median of {RUNS} x {REPS} back-to-back calls, wrapper included)")
    for name, fn in rows:
        med, lo, hi = event_ms(fn)
        print(f"  {name:44s} {med * 1e3:9.1f} us  (min {lo * 1e3:.1f} max {hi * 1e3:.1f})")
    steps = rep[:, 2].cpu().numpy()
    print(f"  Newton steps per row of the last fit: median {np.median(steps):.0f}, max {steps.max():.0f}; flag word {int(flag.item())}")
    print("wall time per call, device tensors in, the table out (median of 5)")
    kws = {"n_bootstrap": R}
    for name, fn in (("calc_calibration(bootstrap=True)", lambda: calc_calibration(yd, pd, "prog_kl_72", NBINS, "uniform", thr, True, kws)),
                     ("calc_calibration(bootstrap=True), quantile", lambda: calc_calibration(yd, pd, "prog_kl_72", NBINS, "quantile", thr, True, kws)),
                     ("calc_metrics_v2(bootstrap=True)", lambda: calc_metrics_v2(yd, pd, "prog_kl_72", bootstrap=True, kws_bs=kws)),
                     ("bootstrap_indices alone (host)", lambda: bootstrap_indices(y, R, 0, True)),
                     ("calc_calibration plain", lambda: calc_calibration(yd, pd, "prog_kl_72", NBINS, "uniform", thr)),
                     ("calc_metrics_v2 plain", lambda: calc_metrics_v2(yd, pd, "prog_kl_72"))):
        med, lo, hi = wall_ms(fn)
        print(f"  {name:44s} {med:9.2f} ms  (min {lo:.2f} max {hi:.2f})")
    t = calc_calibration(yd, pd, "prog_kl_72", NBINS, "uniform", thr, True, kws)
    print({k: t[k] for k in ("brier", "log_loss", "ece", "calib_intercept", "calib_slope", "citl", "n_fit_failed")})


if __name__ == "__main__":
    main()
