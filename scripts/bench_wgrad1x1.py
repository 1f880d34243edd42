"""(GPU) A/B timing of the 1x1 / stride-1 weight gradients at the pixel counts of the headline step (syn3, batch 8), one library
against another on ONE box, alternating:

    python scripts/bench_wgrad1x1.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 3

--family s2: the stride-2 weight gradients of the downsampling blocks instead (1x1 shortcuts: apply on dy, plain x; 3x3 conv2: apply +
prologue), at 1280 slices.

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each shape as the model calls it --
ops.conv2d_wgrad with dy a BatchNorm-backward apply and x behind its BatchNorm prologue -- over --launches launches between two
device events after a warm-up, and reports the variant / tile the launch record shows.  The table gives, per shape and library, the
median over the rounds with the spread (max - min) of the rounds, the ratio of the medians, and the rates of the faster library's
median: TB/s over the bytes the call must read (dz, c, x once; the slabs it writes) and TFLOP/s over 2 P Cout Cin."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
# (Cin, Cout, pixels) of the layer2-4 1x1 / stride-1 convolutions of the slice-wise encoders at batch 8
SHAPES = [(256, 1024, 737280), (128, 512, 2949120), (1024, 256, 737280), (512, 2048, 184320), (512, 128, 2949120), (512, 256, 2949120),
          (1024, 512, 737280), (2048, 512, 184320)]
# (Cin, Cout, input side H = W, filter, pad) of the stride-2 convolutions of layer2-4 at 1280 slices (the table's pixel column: output pixels)
SHAPES_S2 = [(256, 512, 96, 1, 0), (512, 1024, 48, 1, 0), (1024, 2048, 24, 1, 0), (256, 256, 48, 3, 1), (512, 512, 24, 3, 1)]
SLICES = 1280


def family(name):
    """(Cin, Cout, output pixels, N, H, filter, stride, pad, prologue on x) per shape"""
    if name == "s1":
        return [(Cin, Cout, P, P // (64 * 64), 64, 1, 1, 0, True) for Cin, Cout, P in SHAPES]
    return [(Cin, Cout, SLICES * ((H + 2 * pad - k) // 2 + 1) ** 2, SLICES, H, k, 2, pad, k == 3) for Cin, Cout, H, k, pad in SHAPES_S2]


def worker(launches, fam):
    sys.path.insert(0, str(ROOT))
    import torch
    from oaprogressionmmf_amd import _lib, ops
    dev = torch.device("cuda:0")
    g_ = torch.Generator(device=dev).manual_seed(77)
    for Cin, Cout, P, N, H, k, stride, pad, prol in family(fam):
        x = torch.randn(N * H * H, Cin, generator=g_, device=dev) * 1.5 + 0.3
        dz = torch.randn(P, Cout, generator=g_, device=dev) * 1e-3
        c = torch.randn(P, Cout, generator=g_, device=dev) * 1.5 + 0.3
        sc, sh = torch.rand(Cin, generator=g_, device=dev) * 0.4 + 0.8, torch.randn(Cin, generator=g_, device=dev) * 0.1
        coef = torch.stack([torch.rand(Cout, generator=g_, device=dev) + 0.5, torch.zeros(Cout, device=dev),
                            torch.randn(Cout, generator=g_, device=dev) * 1e-5, torch.randn(Cout, generator=g_, device=dev) * 1e-5]).contiguous()
        amax = (coef[0] * dz + coef[3] - coef[2] * c).abs().max().reshape(1).float()
        ap = ops.BnApply(dz, c, coef, amax, torch.zeros(Cout, device=dev), P, Cout)
        ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, H, Cin, Cout, k, k, stride, pad)
        slabs, dw = torch.empty(ws, device=dev), torch.empty(Cout, k, k, Cin, device=dev)

        def call():
            ops.conv2d_wgrad(ap, x, dw, N, H, H, Cin, Cout, k, k, stride, pad, sc if prol else None, sh if prol else None, aplanes=False,
                             slabs=slabs)
        ops.launch_log(True)
        call()
        rec = ops.launch_log_read()[0]
        ops.launch_log(False)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(shape=[Cin, Cout, P, k], ms=e0.elapsed_time(e1) / launches, variant=rec["variant"], bm=rec["bm"], bn=rec["bn"],
                              splitk=rec["splitk"], checksum=float(dw.double().sum()))), flush=True)
        del x, dz, c, ap, slabs, dw
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--family", choices=("s1", "s2"), default="s1")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.launches, a.family)
    shapes = [(Cin, Cout, P, k) for Cin, Cout, P, _, _, k, _, _, _ in family(a.family)]
    libs = [s.split("=", 1) for s in a.lib]
    assert len(libs) >= 1 and a.launches >= 200
    res = {n: {tuple(s): [] for s in shapes} for n, _ in libs}
    info = {}
    for rnd in range(a.rounds):
        for name, path in libs:
            env = dict(os.environ, KOAF_LIB=str(Path(path).resolve()))
            out = subprocess.run([sys.executable, __file__, "--worker", "--launches", str(a.launches), "--family", a.family], env=env, check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            for ln in out.splitlines():
                if ln.startswith("{"):
                    r = json.loads(ln)
                    res[name][tuple(r["shape"])].append(r["ms"])
                    info[(name, tuple(r["shape"]))] = r
            print(f"round {rnd} {name}: done", flush=True)
    print(f"{'Cin->Cout, pixels':26s} " + " ".join(f"{n + ' ms (spread)':>22s} {'kernel':>20s}" for n, _ in libs) + "   ratio   TB/s  TFLOP/s")
    for s in shapes:
        Cin, Cout, P, k = s
        med = {n: statistics.median(res[n][tuple(s)]) for n, _ in libs}
        cols = []
        for n, _ in libs:
            v, r = res[n][tuple(s)], info[(n, tuple(s))]
            cols.append(f"{med[n]:12.3f} ({max(v) - min(v):6.3f}) {r['variant'] + ' ' + str(r['bm']) + 'x' + str(r['bn']):>20s}")
        best = min(med.values())
        sk = info[(libs[0][0], tuple(s))]["splitk"]
        # (stride 2: a 1x1 filter reads one input pixel per output pixel, a 3x3 filter every input pixel -- 4 P -- counted once)
        px_in = P if a.family == "s1" else (P if k == 1 else 4 * P)
        byts = 4.0 * (2 * P * Cout + px_in * Cin + (sk + 1) * Cout * k * k * Cin)
        ratio = med[libs[0][0]] / med[libs[-1][0]]
        same = len({info[(n, tuple(s))]["checksum"] for n, _ in libs}) == 1
        print(f"{Cin:5d}->{Cout:<5d} k{k} {P:9d} " + " ".join(cols) + f"  {ratio:6.3f} {byts / best / 1e9:6.2f} {2.0 * P * Cout * k * k * Cin / best / 1e9:8.1f}"
              + ("" if same else "   CHECKSUMS DIFFER"))


if __name__ == "__main__":
    main()
