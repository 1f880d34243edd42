"""GPU: which fusions of the encoder schedule are active where.  One forward and backward of each small trunk of
tests/encoder_schedule.py; the koaf_gemm launches, in order, are compared with fixture F19 on the fields the schedule decides
(M, N, K, nbatch, fmt, a_tf, b_tf, act16, emit) -- not on the tile, grid or kernel variant, which the library's planner picks, so a
kernel-tuning change does not have to regenerate the fixture.  Equality, no tolerance: these are integers.

What this pins that the value tests do not (every fused path has an element-wise twin that computes the same numbers): the
bottleneck tail formed on load behind plain and downsample blocks (a_tf 3), plane images emitted by conv1 in eval mode and in
rebuilt stages (emit 1), the BatchNorm-backward apply formed on load in the data and weight gradients (a_tf 2; a gradient that
was written out instead arrives as a plain operand, a_tf 0), the fp16 scheme of every contraction that has plane images (fmt 1:
a data gradient whose epilogue reduction did not leave max |dz| falls off it).  The record has no field for the epilogue
reductions themselves, and the stem's kernels are not koaf_gemm launches: a fall-back there shows here only through its consumers;
scripts/encoder_parity.py, which also compares allocator traffic between two source trees, is the tool for those."""
import json

import pytest

import encoder_schedule as ES
from common import GOLDEN

pytestmark = pytest.mark.gpu

_F19 = {}


def _fixture():
    if not _F19:
        _F19.update(json.loads((GOLDEN / "f19_encoder_schedule.json").read_text()))
    return _F19


@pytest.mark.parametrize("name", list(ES.CASES))
def test_launch_sequence_matches_the_pinned_schedule(dev, name):
    g = _fixture()
    assert tuple(g["fields"]) == ES.SCHEDULE_FIELDS
    want = [g["rows"][i] for i in g["cases"][name]]
    got = ES.schedule_rows(ES.run_case(name, dev)["launches"])
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{name}: launch {first} of {len(got)} (pinned: {len(want)}) is "
                         f"{dict(zip(ES.SCHEDULE_FIELDS, got[first])) if first < len(got) else None}, pinned "
                         f"{dict(zip(ES.SCHEDULE_FIELDS, want[first])) if first < len(want) else None}")
