"""Fixture F19 (tests/golden/f19_encoder_schedule.json): the koaf_gemm launch sequence of every case of tests/encoder_schedule.py,
cut down to the fields the encoder schedule decides (encoder_schedule.SCHEDULE_FIELDS).  Run on the GPU box, at the commit whose
schedule is to be pinned:

    python tests/golden/make_golden_encoder_schedule.py [OUT.json]

Stored compactly: `rows` holds each distinct row once, `cases[name]` the launch order as indices into it.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]


def main(out):
    import torch
    import encoder_schedule as ES
    dev = torch.device("cuda:0")
    rows, index, cases = [], {}, {}
    for name in ES.CASES:
        seq = []
        for row in ES.schedule_rows(ES.run_case(name, dev)["launches"]):
            k = tuple(row)
            if k not in index:
                index[k] = len(rows)
                rows.append(row)
            seq.append(index[k])
        cases[name] = seq
        print(f"{name}: {len(seq)} launches")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(dict(fields=list(ES.SCHEDULE_FIELDS), rows=rows, cases=cases), separators=(",", ":")) + "\n")
    print(f"{out}: {len(rows)} distinct rows, {Path(out).stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "f19_encoder_schedule.json")
