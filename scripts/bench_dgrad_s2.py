"""(GPU) A/B timing of the stride-2 data gradients at the pixel counts of the headline step (syn3, batch 8: 1280 slices), one library
against another on ONE box, alternating:

    python scripts/bench_dgrad_s2.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 2

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each shape as the model calls it --
ops.conv2d_dgrad with the weights' plane images and dy as a BnApply; the 3x3 calls through dy's plane images (the pre-pass that cuts them
is inside the timed call, as it is in the step) with the fused BatchNorm-backward reduction mode 2 and max |dz|, the 1x1 shortcuts with
the apply formed on load and no reduction -- over --launches launches between two device events after a warm-up, and reports the variant
/ tile the launch record shows.  The table gives, per shape and library, the median over the rounds with the spread (max - min) of the
rounds, the ratio of the medians (first library / last), and the rates of the faster library's median: TB/s over the bytes the call must
move (dz and c once, dx once, the reduction's c once) and TFLOP/s over 2 M_out Cout k k Cin.  Checksums of dx, the partial rows and
max |dz| must agree between the libraries."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
# (Cin, Cout, input side H = W, filter, pad) of the stride-2 data gradients of layer2-4
SHAPES = [(256, 512, 96, 1, 0), (512, 1024, 48, 1, 0), (1024, 2048, 24, 1, 0), (128, 128, 96, 3, 1), (256, 256, 48, 3, 1), (512, 512, 24, 3, 1)]
SLICES = 1280


def worker(launches):
    sys.path.insert(0, str(ROOT))
    import torch
    from oaprogressionmmf_amd import ops
    dev = torch.device("cuda:0")
    g_ = torch.Generator(device=dev).manual_seed(79)
    N = SLICES
    for Cin, Cout, H, k, pad in SHAPES:
        OH = (H + 2 * pad - k) // 2 + 1
        orow = N * OH * OH

        def rnd(*s):
            return torch.randn(*s, generator=g_, device=dev)
        w = rnd(Cout, k, k, Cin) * (k * k * Cin) ** -0.5
        img = ops.build_weight_planes(w, Cout, k * k, Cin)
        c = rnd(N, OH, OH, Cout) * 1.5 + 0.3
        svc = ops.bn_finalize(ops.colstats(c, orow, Cout), Cout, orow, rnd(Cout) * 0.2 + 1, rnd(Cout) * 0.1, torch.zeros(Cout, device=dev),
                              torch.ones(Cout, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)
        dgm, dbt = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
        ap = ops.bn_bwd(rnd(N, OH, OH, Cout) * 1e-3, c, svc, orow, Cout, orow, dgm, dbt, 2, fused=True)
        bnb = None
        if k == 3:
            sv = torch.stack([rnd(Cin) * 0.3, torch.rand(Cin, generator=g_, device=dev) + 0.5, (rnd(Cin) * 0.5 + 1).abs().clamp(min=0.25), rnd(Cin) * 0.2])
            bnb = dict(mode=2, c=rnd(N, H, H, Cin) * 1.5 + 0.3, saved=sv, dz_amax=True)

        def call():
            ap._koaf_planes = None          # (the step cuts dy's plane images once per convolution: the pre-pass is part of the call)
            return ops.conv2d_dgrad(ap, w, N, H, H, Cin, Cout, k, k, 2, pad, bnb=bnb, wimg=img)
        ops.launch_log(True)
        out = call()
        rec = [r for r in ops.launch_log_read() if r["K"] > 0][0]
        ops.launch_log(False)
        out = out if isinstance(out, tuple) else (out,)
        sums = [float(o.double().sum()) for o in out] + [int(out[1].shape[0]) if len(out) > 1 else 0]
        del out
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
        del w, img, c, ap, bnb
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
    print(f"{'call, input pixels':30s} " + " ".join(f"{n + ' ms (spread)':>22s} {'kernel':>20s}" for n, _ in libs) + "   ratio   TB/s  TFLOP/s")
    for s in SHAPES:
        Cin, Cout, H, k, pad = s
        M, Mo = SLICES * H * H, SLICES * ((H + 2 * pad - k) // 2 + 1) ** 2
        med = {n: statistics.median(res[n][s]) for n, _ in libs}
        cols = []
        for n, _ in libs:
            v, r = res[n][s], info[(n, s)]
            cols.append(f"{med[n]:12.3f} ({max(v) - min(v):6.3f}) {r['variant'] + ' ' + str(r['bm']) + 'x' + str(r['bn']):>20s}")
        best = min(med.values())
        byts = 4.0 * (2 * Mo * Cout + M * Cin * (2 if k == 3 else 1))
        ratio = med[libs[0][0]] / med[libs[-1][0]]
        same = len({tuple(info[(n, s)]["checksum"]) for n, _ in libs}) == 1
        print(f"k{k}s2 {Cin:5d}<-{Cout:<5d} {M:9d}     " + " ".join(cols) + f"  {ratio:6.3f} {byts / best / 1e9:6.2f} {2.0 * Mo * Cout * k * k * Cin / best / 1e9:8.1f}"
              + ("" if same else "   CHECKSUMS DIFFER"))


if __name__ == "__main__":
    main()
