"""The metrics figures of DESIGN 3.17 at the size of an OAI test set: N = 3000 knees, R = 1000 stratified resamples.
  * device-event time of the launches: koaf_score_ranks (fp32 and fp64 scores, read through the probability tensor's stride),
    koaf_curve_metrics with the identity row and all R resamples, koaf_point_metrics -- warm-up, then the median of RUNS runs
    of REPS back-to-back calls;
  * wall time of a whole various.calc_metrics_v2 call on device tensors, plain and bootstrap=True (the index draw on the host, its
    upload, five launches, the one copy back and the numpy summary), and of the index draw alone.
Synthetic scores (prevalence 0.12, logits quantised to 1/64: tie groups); nothing of the reference is read.
  python scripts/bench_metrics.py [N] [R]"""
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from oaprogressionmmf_amd import ops
from oaprogressionmmf_amd.various import bootstrap_indices, calc_metrics_v2

RUNS, WARM, REPS = 20, 3, 20
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


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    rng = np.random.RandomState(0)
    y = (rng.rand(N) < 0.12).astype(np.int64)
    lg = np.round((rng.randn(N) + 1.0 * y) * 64) / 64
    p1 = 1.0 / (1.0 + np.exp(-lg))
    proba = np.stack([1.0 - p1, p1], axis=1)
    idx = bootstrap_indices(y, R, 0, True)
    p32, p64 = torch.from_numpy(proba.astype(np.float32)).to(dev), torch.from_numpy(proba).to(dev)
    yd, y32, idxd = torch.from_numpy(y).to(dev), torch.from_numpy(y.astype(np.int32)).to(dev), torch.from_numpy(idx).to(dev)
    flag = ops.metrics_flag(dev)
    _, packed = ops.score_ranks(p32[:, 1], y32, flag=flag)
    out = torch.empty((R + 1, 8), dtype=torch.float64, device=dev)
    pt = torch.empty(9, dtype=torch.float64, device=dev)
    rows = [("koaf_score_ranks fp32", lambda: ops.score_ranks(p32[:, 1], y32, flag=flag)),
            ("koaf_score_ranks fp64", lambda: ops.score_ranks(p64[:, 1], y32, flag=flag)),
            (f"koaf_curve_metrics 1 + {R} rows", lambda: ops.curve_metrics(packed, idxd, True, 0.12, out=out, flag=flag)),
            ("koaf_curve_metrics identity only", lambda: ops.curve_metrics(packed, None, True, 0.12, out=out[:1], flag=flag)),
            ("koaf_point_metrics", lambda: ops.point_metrics(p32[:, 1], packed, out=pt, flag=flag))]
    print(f"N = {N}, R = {R}: device-event time per launch (median of {RUNS} x {REPS} back-to-back calls, wrapper included)")
    for name, fn in rows:
        med, lo, hi = event_ms(fn)
        print(f"  {name:36s} {med * 1e3:9.1f} us  (min {lo * 1e3:.1f} max {hi * 1e3:.1f})")
    assert int(flag.item()) == 0
    kws_bs = {"n_bootstrap": R}
    print("wall time per call, device tensors in, the dict out (median of 7)")
    for name, fn in (("calc_metrics_v2 plain", lambda: calc_metrics_v2(yd, p32, "prog_kl_72")),
                     ("calc_metrics_v2 bootstrap=True", lambda: calc_metrics_v2(yd, p32, "prog_kl_72", bootstrap=True, kws_bs=kws_bs)),
                     ("calc_metrics_v2 bootstrap=True, fp64", lambda: calc_metrics_v2(yd, p64, "prog_kl_72", bootstrap=True, kws_bs=kws_bs)),
                     ("bootstrap_indices alone (host)", lambda: bootstrap_indices(y, R, 0, True))):
        med, lo, hi = wall_ms(fn)
        print(f"  {name:40s} {med:9.2f} ms  (min {lo:.2f} max {hi:.2f})")
    print(calc_metrics_v2(yd, p32, "prog_kl_72", bootstrap=True, kws_bs=kws_bs))


if __name__ == "__main__":
    main()
