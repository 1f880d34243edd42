"""The curve figures of DESIGN 3.21 at the size of an OAI test set: N = 3000 knees, prevalence 0.12, R = 1000 stratified resamples.
  * device-event time of the launches: koaf_curve_points (fp32 scores read through the probability tensor's stride),
    koaf_range_metrics with the identity row and all R resamples and with the identity row alone, koaf_confusion (K = 2 and
    K = 32) -- warm-up, then the median of RUNS runs of REPS back-to-back calls;
  * wall time of whole calls on device tensors: various.calc_metrics_v2 plain and bootstrap=True and calc_metrics_curves (the first
    two run the kernels they ran before this script existed: compare them across commits), a bootstrapped
    avg_precision_at_recall_range and best_f1_calib, and roc_curve.
Synthetic scores (logits quantised to 1/64: tie groups); nothing of the reference is read.
  python scripts/bench_curves.py [N] [R]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np
import torch
from bench_metrics import RUNS, REPS, dev, event_ms, wall_ms
from oaprogressionmmf_amd import ops
from oaprogressionmmf_amd.various import bootstrap_indices, calc_bootstrap, calc_metrics_curves, calc_metrics_v2, roc_curve


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    rng = np.random.RandomState(0)
    y = (rng.rand(N) < 0.12).astype(np.int64)
    lg = np.round((rng.randn(N) + 1.0 * y) * 64) / 64
    p1 = 1.0 / (1.0 + np.exp(-lg))
    proba = np.stack([1.0 - p1, p1], axis=1)
    idx = bootstrap_indices(y, R, 0, True)
    p32 = torch.from_numpy(proba.astype(np.float32)).to(dev)
    yd, y32, idxd = torch.from_numpy(y).to(dev), torch.from_numpy(y.astype(np.int32)).to(dev), torch.from_numpy(idx).to(dev)
    pred = (p32[:, 1] > 0.5).to(torch.int32)
    wide = torch.from_numpy(rng.randint(0, 32, N).astype(np.int32)).to(dev)
    flag = ops.metrics_flag(dev)
    _, packed = ops.score_ranks(p32[:, 1], y32, flag=flag)
    pts = torch.empty(ops.curve_points_len(N), dtype=torch.float64, device=dev)
    out = torch.empty((R + 1, 8), dtype=torch.float64, device=dev)
    cm2, cm32 = torch.zeros((2, 2), dtype=torch.int64, device=dev), torch.zeros((32, 32), dtype=torch.int64, device=dev)
    rows = [("koaf_curve_points", lambda: ops.curve_points(p32[:, 1], packed, 0.12, out=pts, flag=flag)),
            (f"koaf_range_metrics 1 + {R} rows", lambda: ops.range_metrics(packed, idxd, True, 0.12, (0.2, 0.8), out=out, flag=flag)),
            ("koaf_range_metrics identity only", lambda: ops.range_metrics(packed, None, True, 0.12, (0.2, 0.8), out=out[:1], flag=flag)),
            (f"koaf_curve_metrics 1 + {R} rows", lambda: ops.curve_metrics(packed, idxd, True, 0.12, out=out, flag=flag)),
            ("koaf_confusion K = 2", lambda: ops.confusion(y32, pred, 2, out=cm2, flag=flag)),
            ("koaf_confusion K = 32", lambda: ops.confusion(wide, wide, 32, out=cm32, flag=flag))]
    print(f"N = {N}, R = {R}: device-event time per launch (median of {RUNS} x {REPS} back-to-back calls, wrapper included)")
    for name, fn in rows:
        med, lo, hi = event_ms(fn)
        print(f"  {name:36s} {med * 1e3:9.1f} us  (min {lo * 1e3:.1f} max {hi * 1e3:.1f})")
    assert int(flag.item()) == 0
    kws_bs = {"n_bootstrap": R}
    kw = dict(n_bootstrap=R, verbose=False)
    print("wall time per call, device tensors in (median of 7)")
    for name, fn in (("calc_metrics_v2 plain", lambda: calc_metrics_v2(yd, p32, "prog_kl_72")),
                     ("calc_metrics_curves", lambda: calc_metrics_curves(yd, p32, "prog_kl_72")),
                     ("calc_metrics_v2 bootstrap=True", lambda: calc_metrics_v2(yd, p32, "prog_kl_72", bootstrap=True, kws_bs=kws_bs)),
                     ("calc_bootstrap range AP (0.2, 0.8)", lambda: calc_bootstrap("avg_precision_at_recall_range", yd, p32[:, 1],
                                                                                   recall_range=(0.2, 0.8), **kw)),
                     ("calc_bootstrap best_f1_calib", lambda: calc_bootstrap("best_f1_calib", yd, p32[:, 1], **kw)),
                     ("roc_curve", lambda: roc_curve(yd, p32[:, 1]))):
        med, lo, hi = wall_ms(fn)
        print(f"  {name:40s} {med:9.2f} ms  (min {lo:.2f} max {hi:.2f})")
    c = calc_metrics_curves(yd, p32, "prog_kl_72")
    print({k: (v if not isinstance(v, tuple) else tuple(a.shape for a in v)) for k, v in c.items()})
    print(calc_bootstrap("avg_precision_at_recall_range", yd, p32[:, 1], recall_range=(0.2, 0.8), **kw))


if __name__ == "__main__":
    main()
