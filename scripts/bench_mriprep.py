"""The MRI-preparation figures of DESIGN 3.20 at the sizes the reference prepares: a MESE series (27, 384, 384, 7) and a DESS
volume (384, 384, 160).
  * device-event time of koaf_t2_fit: both layouts, uint16 and fp64 input, with and without the rounding and the 16-voxel margin;
  * device-event time of koaf_series_hist, koaf_series_quantiles, koaf_series_pack and of the three together;
  * each beside its read-once / write-once byte count at 6.3 TB/s -- warm-up, then the median of RUNS runs of REPS
    back-to-back calls, wrapper included;
  * wall time of preproc.fit_t2_map / compress_series on device tensors, and of the numpy twin's fit_t2_map on the host, whole and
    split by slices over 16 threads.
Synthetic series from a seed; nothing of the reference is read.
  python scripts/bench_mriprep.py            the table
  python scripts/bench_mriprep.py --pmc      a few launches of each kernel variant and nothing else, for a counter-collection run"""
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

RUNS, WARM, REPS = 15, 3, 10
HBM = 6.3e12


def inputs():
    rng = np.random.default_rng(0)
    S, R, C, E = 27, 384, 384, 7
    tes = np.tile(0.010 * np.arange(1, E + 1), (S, 1))
    A = rng.uniform(0.0, 3500.0, (S, R, C, 1)).astype(np.float32)
    A[:, :, :96] = 0.0                          # a quarter of every slice is background, as around a knee
    T2 = rng.uniform(0.010, 0.120, (S, R, C, 1)).astype(np.float32)
    sig = A * np.exp(-tes[:, None, None, :].astype(np.float32) / T2) + rng.normal(0.0, 15.0, (S, R, C, E)).astype(np.float32)
    vol = np.clip(np.rint(sig), 0, 4095).astype(np.uint16)
    # an image that varies slowly along the slice axis (the fastest one in memory), as anatomy does, under a little noise
    base = rng.gamma(1.2, 120.0, (384, 384, 1)).astype(np.float32)
    prof = (0.8 + 0.4 * np.sin(np.linspace(0.0, np.pi, 160))).astype(np.float32)
    dess = np.clip(base * prof + rng.normal(0.0, 3.0, (384, 384, 160)).astype(np.float32), 0, 65535).astype(np.uint16)
    dess[:, :96, :] = 0
    return vol, tes, dess


def main():
    import torch
    import mriprep_twin as TW
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.preproc import compress_series, fit_t2_map
    dev = torch.device("cuda:0")
    pmc = "--pmc" in sys.argv[1:]

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

    vol, tes, dess = inputs()
    S, R, C, E = vol.shape
    v16, v64, td = torch.from_numpy(vol).to(dev), torch.from_numpy(vol.astype(np.float64)).to(dev), torch.from_numpy(tes).to(dev)
    dd = torch.from_numpy(dess).to(dev)
    rng = np.random.default_rng(1)
    flat = torch.from_numpy(rng.integers(0, 65536, dess.size).astype(np.uint16)).to(dev)      # no two lanes on one bin, mostly
    const = torch.from_numpy(np.full(dess.size, 4321, np.uint16)).to(dev)                     # every lane on one bin
    n = dess.size
    out0 = torch.empty((S, R, C), dtype=torch.float64, device=dev)
    out1 = torch.empty((R, C, S), dtype=torch.float64, device=dev)
    flag = ops.series_flag(dev)
    bins = torch.zeros(8192, dtype=torch.int32, device=dev)
    lim = ops.series_quantiles(ops.series_hist(dd, 3, flag=flag), n)
    vox = S * R * C
    cvox = S * (R - 32) * (C - 32)

    def three():
        bins.zero_()
        ops.series_hist(dd, 3, bins=bins, flag=flag)
        return ops.series_pack(dd, ops.series_quantiles(bins, n, out=lim), 3, 16, torch.uint8)

    rows = [("koaf_t2_fit uint16 -> [S][R][C]", lambda: ops.t2_fit(v16, td, out=out0), vox * (2 * E + 8)),
            ("koaf_t2_fit uint16 -> [R][C][S]", lambda: ops.t2_fit(v16, td, layout=1, out=out1), vox * (2 * E + 8)),
            ("koaf_t2_fit fp64   -> [S][R][C]", lambda: ops.t2_fit(v64, td, out=out0), vox * (8 * E + 8)),
            ("koaf_t2_fit fp64   -> [R][C][S]", lambda: ops.t2_fit(v64, td, layout=1, out=out1), vox * (8 * E + 8)),
            ("koaf_t2_fit uint16 -> [R'][C'][S], 6 decimals, margin 16", lambda: ops.t2_fit(v16, td, decimals=6, margin=16, layout=1),
             cvox * (2 * E + 8)),
            ("koaf_series_hist uint16, shift 3", lambda: ops.series_hist(dd, 3, bins=bins, flag=flag), n * 2),
            ("koaf_series_hist, values uniform over uint16", lambda: ops.series_hist(flat, 3, bins=bins, flag=flag), n * 2),
            ("koaf_series_hist, a constant volume", lambda: ops.series_hist(const, 3, bins=bins, flag=flag), n * 2),
            ("koaf_series_quantiles, 2 percentiles", lambda: ops.series_quantiles(bins, n, out=lim), 8192 * 4),
            ("koaf_series_pack uint16 -> uint8, margin 16", lambda: ops.series_pack(dd, lim, 3, 16, torch.uint8), 352 * 352 * 160 * 3),
            ("hist + quantiles + pack (bins zeroed)", three, n * 2 + 352 * 352 * 160 * 3)]
    if pmc:
        for _, fn, _ in rows[:-1]:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return
    print(f"MESE {vol.shape} ({(vol > 0).all(-1).mean() * 100:.0f} % of the voxels fitted), DESS {dess.shape}: device-event time per "
          f"call (median of {RUNS} x {REPS} back-to-back calls, wrapper included); floor = bytes once at 6.3 TB/s")
    for name, fn, nbytes in rows:
        med, lo, hi = event_ms(fn)
        print(f"  {name:58s} {med * 1e3:9.1f} us  (min {lo * 1e3:.1f} max {hi * 1e3:.1f})  {nbytes / 1e6:7.1f} MB  floor "
              f"{nbytes / HBM * 1e6:6.1f} us  {nbytes / (med * 1e-3) / 1e12:5.2f} TB/s")
    print("wall time per call (median of 5)")
    for name, fn in (("preproc.fit_t2_map, uint16 device tensor in", lambda: fit_t2_map(v16, td)),
                     ("preproc.fit_t2_map, uint16 numpy in / numpy out", lambda: fit_t2_map(vol, tes)),
                     ("preproc.compress_series DESS, device tensor in", lambda: compress_series(dd, "SAG_3D_DESS")),
                     ("preproc.compress_series DESS, numpy in / numpy out", lambda: compress_series(dess, "SAG_3D_DESS"))):
        med, lo, hi = wall_ms(fn)
        print(f"  {name:58s} {med:9.2f} ms  (min {lo:.2f} max {hi:.2f})")
    pool = ThreadPoolExecutor(16)

    def twin16():
        return np.concatenate(list(pool.map(lambda s: TW.t2_fit(vol[s:s + 1], tes[s:s + 1]), range(S))))

    for name, fn in (("numpy twin fit_t2_map, host, one thread", lambda: TW.t2_fit(vol, tes)),
                     ("numpy twin fit_t2_map, host, slices over 16 threads", twin16),
                     ("numpy twin compress_series DESS, host", lambda: TW.compress_series(dess, "SAG_3D_DESS"))):
        med, lo, hi = wall_ms(fn, runs=3)
        print(f"  {name:58s} {med:9.2f} ms  (min {lo:.2f} max {hi:.2f})")
    assert np.array_equal(twin16(), TW.t2_fit(vol, tes)) and int(flag.item()) == 0


if __name__ == "__main__":
    main()
