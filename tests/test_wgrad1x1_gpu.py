"""The 256-wide-tile kernel of the 1x1 / stride-1 weight gradients (koaf_wgrad1.hip) against the generic path it replaces.

koaf_conv2d_wgrad hands a 1x1 / stride-1 weight gradient to koaf_wgrad1 when the call runs the fp16 scheme on fp32 tensors, both
channel counts are whole multiples of 128 with at least one of them >= 256, and the split-K plan (wgrad_plan, unchanged) leaves
k-ranges of at least 1024 pixels (koaf_wgrad1.hip koaf_wgrad1_ok).  Every row of CASES is the smallest shape of its kind that the rule
engages; it goes through ops.conv2d_wgrad as the model calls it and ASSERTS FROM THE LAUNCH RECORD the variant, tile, tile count
and split count.  dw and the slab workspace are pre-filled with NaN.

Held per case:
  * dw is torch.equal to the generic path on the same inputs: ops.gemm with the descriptor koaf_conv2d_wgrad builds for
    koaf_gemm_kernel (128 x 128 tiles, the same splitk, slabs) followed by koaf_slab_reduce.  The kernel keeps koaf_gemm_kernel's
    arithmetic, pieces and order of piece products per accumulator, so nothing may move.
  * against float64 on the CPU for eight sampled 64 x 64 blocks of dw (corners and interior, both halves of every tile along both
    dimensions): relative L2 < BWD per block and the componentwise bar of test_wgrad_gpu.py (8 x torch's fp32 product of the same
    operands); BWD and the bar's function are imported from test_tiles_gpu, not restated.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: the generic kernel at 128-wide tiles keeps the bf16 scheme, bf16 storage, k-ranges
under 1024 pixels and channel counts that are no multiple of 128.

Inputs are drawn on the device (one set per shape, shared by its calls); only the sampled columns travel to the CPU."""
from collections import namedtuple

import pytest

import tile256_refs as R

pytestmark = pytest.mark.gpu

W1K = "koaf_wgrad1"
Case = namedtuple("Case", "name shape call bm bn splitk empty last")
# shape (N, H, W, Cin, Cout); call: plain (dy + its amax) | apply_prologue (dy an ops.BnApply -- tf 2 on A --, x behind its BatchNorm
# prologue -- tf 1 on B: the production combination); splitk / empty trailing splits / rows of the last live split: wgrad_plan's,
# as koaf_conv2d_wgrad_ws reports them (test_the_table_against_the_library_plan)
S1 = (17, 62, 63, 256, 1024)      # P = 66 402 = 2 mod 32: 64 splits of 1056 rows, the last live one 930, one empty; 4 tiles 256 x 256
S2 = (5, 57, 61, 512, 2048)       # P = 17 385 = 9 mod 32: 16 splits of 1088 rows, 16 tiles per split
S3 = (65, 63, 65, 256, 256)       # P = 266 175 = 31 mod 32: 256 splits of one tile, the last live one 63 rows, 3 empty; two-level slab reduce
S4 = (65, 63, 65, 128, 512)       # the same 256 splits on 256 x 128 tiles (two per split)
S5 = (65, 63, 65, 512, 128)       # 128 x 256 tiles
S6 = (9, 61, 62, 1024, 512)       # P = 34 038 = 22 mod 32: 32 splits, 8 tiles per split
SHAPES = [S1, S2, S3, S4, S5, S6]
CASES = [
    Case("256to1024-plain", S1, "plain", 256, 256, 64, 1, 930),
    Case("256to1024-apply_prologue", S1, "apply_prologue", 256, 256, 64, 1, 930),
    Case("512to2048-apply_prologue", S2, "apply_prologue", 256, 256, 16, 0, 1065),
    Case("256to256-apply_prologue", S3, "apply_prologue", 256, 256, 256, 3, 63),
    Case("128to512-apply_prologue", S4, "apply_prologue", 256, 128, 256, 3, 63),
    Case("512to128-apply_prologue", S5, "apply_prologue", 128, 256, 256, 3, 63),
    Case("1024to512-plain", S6, "plain", 256, 256, 32, 0, 310),
]
Refusal = namedtuple("Refusal", "name shape call store")
R1 = (9, 20, 20, 512, 2048)       # P = 3600: k-ranges of 480 pixels
R2 = (17, 62, 63, 256, 192)       # Cout no multiple of 128
REFUSALS = [
    Refusal("bf16scheme", S1, "bf16scheme", "fp32"),      # dy_amax withheld
    Refusal("bf16storage", S1, "apply_prologue", "bf16"),      # x and the apply's c stored as bf16 (act16 3)
    Refusal("kchunk480", R1, "plain", "fp32"),
    Refusal("cout192", R2, "plain", "fp32"),
]


def inputs(shape, dev, store16=False):
    # (the apply only where a case calls with it: colstats serves no Cout = 192)
    return R.wgrad_inputs(shape, 1, dev, 9100 + (SHAPES + [R1, R2]).index(shape), store16,
                          apply=any(c.shape == shape and c.call == "apply_prologue" for c in CASES))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_table_against_the_library_plan(case):
    P, splitk, kchunk, empty, last = R.plan_of(case.shape, 1)
    assert (splitk, empty, last) == (case.splitk, case.empty, case.last), (case.name, P, splitk, kchunk, empty, last)
    assert kchunk >= 1024, (case.name, kchunk)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_wide_tile_kernel_equals_the_generic_path(dev, case):
    R.check_wgrad(dev, case, W1K, 1, inputs(case.shape, dev), f"[wgrad1x1] {case.name:28s}", show_tap=False)


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernel(dev, case):
    R.check_wgrad_refusal(dev, case, W1K, 1, inputs(case.shape, dev, case.store == "bf16"))
