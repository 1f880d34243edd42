"""Has a change to the encoder schedule (models/_encoder.py) changed what it computes, launches or allocates?

    python scripts/encoder_parity.py dump OUT.json          every case of tests/encoder_schedule.py, from the tree this file is in
    python scripts/encoder_parity.py compare A.json B.json  A = before, B = after; exit status 0 iff nothing differs

Run `dump` once per source tree on ONE box (`KOAF_LIB=<the one built library>` for the tree that has none).  Equal are required:
the launch records (every field, in order), the SHA-256 of the output / input gradient / parameter gradients / buffers (also of
the pass with the side stream on), the number of allocations and the bytes allocated; the peak of B may not exceed A's.
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def dump(out):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import torch
    import encoder_schedule as ES
    dev = torch.device("cuda:0")
    res = {name: ES.run_case(name, dev, side_pass=True) for name in ES.CASES}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res))
    for name, r in res.items():
        print(f"{name:12s} launches {len(r['launches']):4d}  allocs {r['mem']['allocs']:5d}  bytes {r['mem']['bytes']:11d}  "
              f"peak {r['mem']['peak']:10d}")


def compare(fa, fb):
    A, B = json.loads(Path(fa).read_text()), json.loads(Path(fb).read_text())
    bad = 0
    if A.keys() != B.keys():
        print("cases differ:", sorted(set(A) ^ set(B)))
        bad += 1
    print("| case | launches | hashes | allocations | bytes allocated | peak A | peak B |")
    print("|---|---|---|---|---|---|---|")
    for name in A:
        if name not in B:
            continue
        a, b = A[name], B[name]
        msgs = []
        la, lb = a["launches"], b["launches"]
        if la != lb:
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            msgs.append(f"launch {i} of {len(la)} / {len(lb)}: {la[i] if i < len(la) else None} != {lb[i] if i < len(lb) else None}")
        for key in ("hashes", "hashes_side"):
            ha, hb = a[key], b[key]
            diff = sorted(k for k in set(ha) | set(hb) if ha.get(k) != hb.get(k))
            if diff:
                msgs.append(f"{key}: {len(diff)} differ, first {diff[0]}")
        ma, mb = a["mem"], b["mem"]
        for k in ("allocs", "bytes"):
            if ma[k] != mb[k]:
                msgs.append(f"{k}: {ma[k]} != {mb[k]}")
        if mb["peak"] > ma["peak"]:
            msgs.append(f"peak rose: {ma['peak']} -> {mb['peak']}")
        nh = len(a["hashes"]) + len(a["hashes_side"])
        print(f"| {name} | {len(la)} {'=' if la == lb else '!='} {len(lb)} | {nh} {'equal' if not any('hashes' in m for m in msgs) else 'DIFFER'} "
              f"| {ma['allocs']} / {mb['allocs']} | {ma['bytes']} / {mb['bytes']} | {ma['peak']} | {mb['peak']} |")
        for m in msgs:
            print(f"  DIFFERENT {name}: {m}")
        bad += len(msgs)
    print("identical" if not bad else f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
