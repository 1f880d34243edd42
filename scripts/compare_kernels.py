#!/usr/bin/env python3
"""compare_kernels.py OLD_CSRC NEW_CSRC [--work DIR] [-j N] [--diff SUBSTR] -- has a refactor changed any device kernel?  (host only)

Compiles every .hip that each tree's own Makefile builds into libkoaf.so (`make -n -B`: that tree's files and flags) to gfx950
assembly, cuts it per kernel symbol and sorts every kernel into: identical text (comments, directives and the numbering of local
labels aside) / same resources and same work / changed.  "Same" = equal VGPRs, accumulator offset, LDS and scratch bytes in the
kernel descriptor, equal counts of matrix, global / buffer, LDS, scratch, barrier, s_waitcnt and lane-spill instructions, and a
total instruction count within LIMIT (hipcc's schedule of one kernel depends slightly on what else is in the file: recompositions of
an unchanged source moved kernels by up to 4 instructions; LIMIT is ten times that).  The streamed kernels (M_KS) may lose one
s_waitcnt: OLD may still read KoafGemm.prec there.  Exit status 0 iff both sides hold the same kernels, each once, none changed.
--work keeps the assembly (an existing DIR/old|new/FILE.s is reused); --diff prints the text diff of the kernels whose name has SUBSTR."""
import argparse, collections, concurrent.futures as cf, difflib, re, shlex, subprocess, sys, tempfile
from pathlib import Path

LIMIT = 40
DESC = ("next_free_vgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
CLASSES = {"mfma": r"v_mfma", "global": r"(global|buffer)_", "lds": r"ds_", "scratch": r"scratch_", "barrier": r"s_barrier",
           "waitcnt": r"s_waitcnt", "lane": r"v_(write|read)lane"}
STREAMED = re.compile(r"koaf_gemm_kernelILi128ELi(128|64)ELi13ELi6E")


def compile_commands(csrc):
    """-> [(source, hipcc command line up to -c)] of every .hip the tree's Makefile compiles into libkoaf.so (its files, its flags)"""
    dry = subprocess.run(["make", "-n", "-B", "-C", str(csrc)], check=True, capture_output=True, text=True).stdout
    lines = [shlex.split(ln) for ln in dry.splitlines() if " -c " in ln and ".hip" in ln]
    return [(a[a.index("-c") + 1], a[:a.index("-c")]) for a in lines]


def run_all(cmds, cwd, jobs=8):
    """run the command lines in cwd, at most 16 at a time; -> their stderr texts"""
    with cf.ThreadPoolExecutor(max_workers=min(jobs, 16)) as ex:
        done = list(ex.map(lambda c: subprocess.run(c, cwd=cwd, capture_output=True, text=True), cmds))
    for r in done:
        if r.returncode:
            sys.exit(r.stderr[-2000:])
    return [r.stderr for r in done]


def compile_tree(csrc, out, jobs):
    """-> the assembly files of the tree, one per source"""
    out.mkdir(parents=True, exist_ok=True)
    cmds = compile_commands(csrc)
    dst = [out / (Path(src).stem + ".s") for src, _ in cmds]
    assert len(set(dst)) == len(dst), "a source is compiled twice"
    run_all([c + ["--cuda-device-only", "-S", src, "-o", str(d)] for (src, c), d in zip(cmds, dst) if not d.exists()], csrc, jobs)
    return dst


def kernels(files):
    """-> {symbol: (descriptor dict, normalised body lines)}, and the symbols seen more than once"""
    found, twice = {}, []
    for f in files:
        name, body, desc = None, [], None        # body: from the label NAME: to .amdhsa_kernel NAME; desc: from there to .end_amdhsa_kernel
        for raw in f.read_text().splitlines():
            line = raw.split(";")[0].strip()
            if name is None:
                m = re.match(r"\.type\s+(\S+),@function", line)
                name, body, desc = (m.group(1), None, None) if m else (None, [], None)
            elif body is None:
                body = [] if line == name + ":" else None
            elif desc is None:
                if line.startswith(".amdhsa_kernel "):
                    desc = {}
                elif line and not (line.startswith(".") and not line.endswith(":")):
                    body.append(re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", line))
            elif line == ".end_amdhsa_kernel":
                if name in found:
                    twice.append(name)
                found[name] = (desc, body)
                name = None
            else:
                k, _, v = line.partition(" ")
                desc[k.replace(".amdhsa_", "")] = v
    return found, twice


def counts(body):
    ins = [ln for ln in body if not ln.endswith(":")]
    c = {k: sum(1 for ln in ins if re.match(p, ln)) for k, p in CLASSES.items()}
    c["total"] = len(ins)
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old"), ap.add_argument("new"), ap.add_argument("--work"), ap.add_argument("--diff")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    work = Path(a.work or tempfile.mkdtemp(prefix="koaf_cmp_"))
    (old, old2), (new, new2) = (kernels(compile_tree(Path(t).resolve(), work / side, a.j)) for t, side in ((a.old, "old"), (a.new, "new")))
    bad = [f"only in OLD: {k}" for k in old.keys() - new.keys()] + [f"only in NEW: {k}" for k in new.keys() - old.keys()]
    bad += [f"twice in OLD: {k}" for k in old2] + [f"twice in NEW: {k}" for k in new2]
    tally, worst = collections.Counter(), 0
    for k in sorted(old.keys() & new.keys()):
        (d0, b0), (d1, b1) = old[k], new[k]
        if a.diff and a.diff in k:
            print("\n".join(difflib.unified_diff(b0, b1, "old " + k, "new " + k, lineterm="", n=2)))
        same_desc = all(d0.get(f) == d1.get(f) for f in DESC)
        if same_desc and b0 == b1:
            tally["identical"] += 1
            continue
        c0, c1 = counts(b0), counts(b1)
        diffs = {f: (c0[f], c1[f]) for f in CLASSES if c0[f] != c1[f]}
        if STREAMED.search(k) and diffs.get("waitcnt") == (c1["waitcnt"] + 1, c1["waitcnt"]):
            del diffs["waitcnt"]
        dt = c1["total"] - c0["total"]
        ok = same_desc and not diffs and abs(dt) <= LIMIT
        tally["same" if ok else "changed"] += 1
        worst = max(worst, abs(dt)) if ok else worst
        sg = "" if d0.get("next_free_sgpr") == d1.get("next_free_sgpr") else f" sgpr {d0.get('next_free_sgpr')}->{d1.get('next_free_sgpr')}"
        print(f"{'same   ' if ok else 'CHANGED'} {k}: instructions {c0['total']} -> {c1['total']} ({dt:+d}){sg}"
              + ("" if ok else f" descriptor {[(f, d0.get(f), d1.get(f)) for f in DESC if d0.get(f) != d1.get(f)]} counts {diffs}"))
    print("\n".join(bad))
    print(f"kernels compared {len(old.keys() & new.keys())}: identical text {tally['identical']}; same resources and work {tally['same']} "
          f"(largest instruction-count difference {worst}); changed {tally['changed']}; symbol-set problems {len(bad)}")
    sys.exit(1 if bad or tally["changed"] else 0)


if __name__ == "__main__":
    main()
