"""(GPU) A/B timing of the stride-2 forward convolutions at the pixel counts of the headline step (syn3, batch 8: 1280 slices), one
library against another on ONE box, alternating:

    python scripts/bench_fwd_s2.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 2

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each shape as the model calls it --
ops.conv2d_fwd with the weights' plane images and shifted statistics; the 3x3 calls behind their BatchNorm prologue, the 1x1 shortcuts
plain -- over --launches launches between two device events after a warm-up, and reports the variant / tile the launch record shows.
The table gives, per shape and library, the median over the rounds with the spread (max - min) of the rounds, the ratio of the medians
(first library / last), and the rates of the faster library's median: TB/s over the bytes the call must move (the input pixels it
touches once, y once) and TFLOP/s over 2 M Cout K.  Checksums of y and of the statistics rows must agree between the libraries."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
# (Cin, Cout, input side H = W, filter, pad) of the stride-2 forward convolutions of layer2-4
SHAPES = [(256, 512, 96, 1, 0), (512, 1024, 48, 1, 0), (1024, 2048, 24, 1, 0), (128, 128, 96, 3, 1), (256, 256, 48, 3, 1), (512, 512, 24, 3, 1)]
SLICES = 1280


def worker(launches):
    sys.path.insert(0, str(ROOT))
    import torch
    from oaprogressionmmf_amd import ops
    dev = torch.device("cuda:0")
    g_ = torch.Generator(device=dev).manual_seed(78)
    N = SLICES
    for Cin, Cout, H, k, pad in SHAPES:
        x = torch.randn(N, H, H, Cin, generator=g_, device=dev) * 1.5 + 0.3
        w = torch.randn(Cout, k, k, Cin, generator=g_, device=dev) * (k * k * Cin) ** -0.5
        sc, sh = torch.rand(Cin, generator=g_, device=dev) * 0.4 + 0.8, torch.randn(Cin, generator=g_, device=dev) * 0.1
        shift = torch.randn(Cout, generator=g_, device=dev) * 0.1
        img = ops.build_weight_planes(w, Cout, k * k, Cin)
        prol = k == 3

        def call():
            return ops.conv2d_fwd(x, w, N, H, H, Cin, Cout, k, k, 2, pad, sc if prol else None, sh if prol else None, stats=True, shift=shift,
                                  wimg=img)
        ops.launch_log(True)
        y, part = call()
        rec = ops.launch_log_read()[0]
        ops.launch_log(False)
        sums = (float(y.double().sum()), float(part.double().sum()), int(part.shape[0]))
        del y, part
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(shape=[Cin, Cout, H, k], ms=e0.elapsed_time(e1) / launches, variant=rec["variant"], bm=rec["bm"], bn=rec["bn"],
                              checksum=sums)), flush=True)
        del x, w, img
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.launches)
    libs = [s.split("=", 1) for s in a.lib]
    assert len(libs) >= 1 and a.launches >= 200
    res = {n: {s: [] for s in SHAPES} for n, _ in libs}
    info = {}
    for rnd in range(a.rounds):
        for name, path in libs:
            env = dict(os.environ, KOAF_LIB=str(Path(path).resolve()))
            out = subprocess.run([sys.executable, __file__, "--worker", "--launches", str(a.launches)], env=env, check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            for ln in out.splitlines():
                if ln.startswith("{"):
                    r = json.loads(ln)
                    s = tuple(r["shape"])
                    s = next(q for q in SHAPES if (q[0], q[1], q[2], q[3]) == s)
                    res[name][s].append(r["ms"])
                    info[(name, s)] = r
            print(f"round {rnd} {name}: done", flush=True)
    print(f"{'call, output pixels':30s} " + " ".join(f"{n + ' ms (spread)':>22s} {'kernel':>20s}" for n, _ in libs) + "   ratio   TB/s  TFLOP/s")
    for s in SHAPES:
        Cin, Cout, H, k, pad = s
        M = SLICES * ((H + 2 * pad - k) // 2 + 1) ** 2
        med = {n: statistics.median(res[n][s]) for n, _ in libs}
        cols = []
        for n, _ in libs:
            v, r = res[n][s], info[(n, s)]
            cols.append(f"{med[n]:12.3f} ({max(v) - min(v):6.3f}) {r['variant'] + ' ' + str(r['bm']) + 'x' + str(r['bn']):>20s}")
        best = min(med.values())
        # (a 1x1 filter reads one input pixel per output pixel, a 3x3 filter every input pixel -- 4 M -- counted once)
        byts = 4.0 * (M * Cout + (M if k == 1 else 4 * M) * Cin)
        ratio = med[libs[0][0]] / med[libs[-1][0]]
        same = len({tuple(info[(n, s)]["checksum"]) for n, _ in libs}) == 1
        print(f"k{k}s2 {Cin:5d}->{Cout:<5d} {M:9d}     " + " ".join(cols) + f"  {ratio:6.3f} {byts / best / 1e9:6.2f} {2.0 * M * Cout * k * k * Cin / best / 1e9:8.1f}"
              + ("" if same else "   CHECKSUMS DIFFER"))


if __name__ == "__main__":
    main()
