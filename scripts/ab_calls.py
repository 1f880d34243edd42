"""(GPU) The A/B driver of the per-call benchmarks of the 256-row convolution units (bench_wgrad1x1.py, bench_fwd_s2.py,
bench_dgrad_s2.py, bench_fwd1.py): one library against others on ONE box, alternating.

A script brings its shape table, a function build(shape, dev) -> (call, checksum) that forms the operands and returns the timed
closure and what to checksum of its result, and the bytes / FLOP formulas of a shape; run() does the rest.  Every (round, library)
is a fresh child process (KOAF_LIB is read at import) that, per shape: makes the call once with the launch log on and keeps the first
record with work (variant, tile, grid, split count) and the checksums; warms up; times --launches launches between two device events.
The table gives, per shape and library, the median over the rounds with the spread (max - min) of the rounds and the kernel of the
launch record; then either the ratio of the medians (first library / last) and the rates of the faster library's median (TB/s,
TFLOP/s), or -- ship_rule -- one line per library with the ratio to the FIRST library, whether the call passes the ship rule against
it (its median below the first's by at least ten times the larger of the two spreads) and the rates of its own median.  Checksums must
agree between the libraries."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
WARMUP = 10


def generator(dev, seed, _made={}):
    """the one generator a child process draws all its shapes' operands from"""
    import torch
    if seed not in _made:
        _made[seed] = torch.Generator(device=dev).manual_seed(seed)
    return _made[seed]


def worker(shapes, build, launches):
    sys.path.insert(0, str(ROOT))
    import torch
    from oaprogressionmmf_amd import ops
    dev = torch.device("cuda:0")
    for i, shape in enumerate(shapes):
        call, checksum = build(shape, dev)
        ops.launch_log(True)
        out = call()
        rec = [r for r in ops.launch_log_read() if r["K"] > 0][0]
        ops.launch_log(False)
        sums = checksum(out)
        del out
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(index=i, ms=e0.elapsed_time(e1) / launches, checksum=sums,
                              **{f: rec[f] for f in ("variant", "bm", "bn", "grid_x", "splitk")})), flush=True)
        del call, checksum
        torch.cuda.empty_cache()


def run(script, shapes, build, header, label, rates, rounds=2, families=None, ship_rule=False):
    """script: the calling file (the child runs it again with --worker); shapes: the table, or with families = (names) a function
    family name -> table behind a --family option; header / label(shape): the table's head and a row's first column;
    rates(shape, record) -> (bytes, FLOP) of one call"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--launches", type=int, default=200)
    if families:
        ap.add_argument("--family", choices=families, default=families[0])
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    fam = ["--family", a.family] if families else []
    if families:
        shapes = shapes(a.family)
    if a.worker:
        return worker(shapes, build, a.launches)
    libs = [s.split("=", 1) for s in a.lib]
    assert len(libs) >= 1 and a.launches >= 200
    names = [n for n, _ in libs]
    res = {n: [[] for _ in shapes] for n in names}
    info = {}
    for rnd in range(a.rounds):
        for name, path in libs:
            env = dict(os.environ, KOAF_LIB=str(Path(path).resolve()))
            out = subprocess.run([sys.executable, script, "--worker", "--launches", str(a.launches)] + fam, env=env, check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            for ln in out.splitlines():
                if ln.startswith("{"):
                    r = json.loads(ln)
                    res[name][r["index"]].append(r["ms"])
                    info[(name, r["index"])] = r
            print(f"round {rnd} {name}: done", flush=True)
    first, last = names[0], names[-1]
    if ship_rule:
        print(header)
    else:
        print(header + " " + " ".join(f"{n + ' ms (spread)':>22s} {'kernel':>20s}" for n in names) + "   ratio   TB/s  TFLOP/s")
    for i, s in enumerate(shapes):
        med = {n: statistics.median(res[n][i]) for n in names}
        spread = {n: max(res[n][i]) - min(res[n][i]) for n in names}
        differ = "" if len({json.dumps(info[(n, i)]["checksum"]) for n in names}) == 1 else "   CHECKSUMS DIFFER"
        byts, flop = rates(s, info[(first, i)])
        if ship_rule:
            print(label(s) + differ)
            for n in names:
                r = info[(n, i)]
                rule = "" if n == first else ("ships" if med[first] - med[n] >= 10.0 * max(spread[first], spread[n]) else "stays")
                print(f"    {n:10s} {med[n]:9.3f} ({spread[n]:6.3f})  {r['variant']:17s} {r['bm']:3d}x{r['bn']:<3d} grid.x {r['grid_x']:6d} | "
                      f"{med[first] / med[n]:6.3f} | {rule:5s} | {byts / med[n] / 1e9:5.2f} {flop / med[n] / 1e9:7.1f}")
            continue
        cols = [f"{med[n]:12.3f} ({spread[n]:6.3f}) {info[(n, i)]['variant'] + ' ' + str(info[(n, i)]['bm']) + 'x' + str(info[(n, i)]['bn']):>20s}"
                for n in names]
        best = min(med.values())
        print(label(s) + " ".join(cols) + f"  {med[first] / med[last]:6.3f} {byts / best / 1e9:6.2f} {flop / best / 1e9:8.1f}" + differ)
