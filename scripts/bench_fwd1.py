"""(GPU) A/B timing of the dense 1x1 / stride-1 forward convolutions without a bottleneck tail at the pixel counts of the headline step
(syn3, batch 8: 1280 slices), one library against others on ONE box, alternating:

    python scripts/bench_fwd1.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 2

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each call as the model makes it --
ops.conv2d_fwd with the weights' plane images and shifted statistics; conv3 of the Bottlenecks behind its BatchNorm prologue, block-0
conv1 and the layer1 shortcut plain -- over --launches launches between two device events after a warm-up, and reports the variant /
tile / grid the launch record shows.  Both forms of koaf_fwd1 are timed from two builds of the library that differ in
-DKOAF_FWD1_FORCE=0 | 1 (koaf_fwd1.hip: every admitted shape in that form; benchmark builds only).
The table gives, per call and library, the median over the rounds with the spread (max - min) of the rounds, the ratio of the FIRST
library's median to this one's, whether the call passes the ship rule against the first library (its median below the first's by at
least ten times the larger of the two spreads), and the rates of the median: TB/s over the bytes the call must move (x once, y once)
and TFLOP/s over 2 M Cout Cin.  Checksums of y and of the statistics rows must agree between the libraries."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
# (Cin, Cout, side H = W, prologue) of the calls: conv3 of layer1-4, block-0 conv1 of layer2-3, the layer1 shortcut
SHAPES = [(64, 256, 96, True), (128, 512, 48, True), (256, 1024, 24, True), (512, 2048, 12, True), (256, 128, 96, False),
          (512, 256, 48, False), (64, 256, 96, False)]
SLICES = 1280


def worker(launches):
    sys.path.insert(0, str(ROOT))
    import torch
    from oaprogressionmmf_amd import ops
    dev = torch.device("cuda:0")
    g_ = torch.Generator(device=dev).manual_seed(79)
    N = SLICES
    for Cin, Cout, H, prol in SHAPES:
        x = torch.randn(N, H, H, Cin, generator=g_, device=dev) * 1.5 + 0.3
        w = torch.randn(Cout, 1, 1, Cin, generator=g_, device=dev) * Cin ** -0.5
        sc, sh = torch.rand(Cin, generator=g_, device=dev) * 0.4 + 0.8, torch.randn(Cin, generator=g_, device=dev) * 0.1
        shift = torch.randn(Cout, generator=g_, device=dev) * 0.1
        img = ops.build_weight_planes(w, Cout, 1, Cin)

        def call():
            return ops.conv2d_fwd(x, w, N, H, H, Cin, Cout, 1, 1, 1, 0, sc if prol else None, sh if prol else None, stats=True, shift=shift,
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
        print(json.dumps(dict(shape=[Cin, Cout, H, prol], ms=e0.elapsed_time(e1) / launches, variant=rec["variant"], bm=rec["bm"],
                              bn=rec["bn"], grid_x=rec["grid_x"], checksum=sums)), flush=True)
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
                    res[name][s].append(r["ms"])
                    info[(name, s)] = r
            print(f"round {rnd} {name}: done", flush=True)
    first = libs[0][0]
    print("call, output pixels; per library: median ms (spread) kernel tile grid.x | ratio first/this | ship rule | TB/s TFLOP/s")
    for s in SHAPES:
        Cin, Cout, H, prol = s
        M = SLICES * H * H
        med = {n: statistics.median(res[n][s]) for n, _ in libs}
        spread = {n: max(res[n][s]) - min(res[n][s]) for n, _ in libs}
        same = len({tuple(info[(n, s)]["checksum"]) for n, _ in libs}) == 1
        print(f"k1s1 {Cin:5d}->{Cout:<5d} {'prologue' if prol else 'plain':8s} {M:9d}" + ("" if same else "   CHECKSUMS DIFFER"))
        byts = 4.0 * M * (Cout + Cin)
        for n, _ in libs:
            r = info[(n, s)]
            rule = "" if n == first else ("ships" if med[first] - med[n] >= 10.0 * max(spread[first], spread[n]) else "stays")
            print(f"    {n:10s} {med[n]:9.3f} ({spread[n]:6.3f})  {r['variant']:17s} {r['bm']:3d}x{r['bn']:<3d} grid.x {r['grid_x']:6d} | "
                  f"{med[first] / med[n]:6.3f} | {rule:5s} | {byts / med[n] / 1e9:5.2f} {2.0 * M * Cout * Cin / med[n] / 1e9:7.1f}")


if __name__ == "__main__":
    main()
