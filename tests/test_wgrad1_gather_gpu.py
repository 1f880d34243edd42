"""The stride-2 weight gradients on the 256-wide-tile kernel (koaf_wgrad1.hip, gathered B) against the generic path they leave.

koaf_conv2d_wgrad hands a stride-2 weight gradient -- the 1x1 / pad 0 shortcuts and the 3x3 / pad 1 conv2 of a downsampling block -- to
koaf_wgrad1 when the call runs the fp16 scheme on fp32 tensors without plane images, Cout and KH KW Cin are whole multiples of the tile
(256, or 128 on ONE side), Cin is a whole number of column tiles (a block works on one filter tap) and the split-K plan (wgrad_plan,
unchanged) leaves k-ranges of at least 1024 pixels (koaf_wgrad1.hip koaf_wgrad1_ok).  B is then x gathered on the k index: k-row p = output
pixel (n, oy, ox), column (tap, ci), element x[n][2 oy - pad + kh][2 ox - pad + kw][ci] behind its transform, 0 outside the image.
Every row of CASES is the smallest shape of its kind that the rule engages, with P no multiple of 32; it goes through ops.conv2d_wgrad as
the model calls it and ASSERTS FROM THE LAUNCH RECORD the variant, tile, tile count and split count.  dw and the slab workspace are
pre-filled with NaN.

Held per case:
  * dw is torch.equal to the generic path on the same inputs: ops.gemm with the descriptor koaf_conv2d_wgrad builds for
    koaf_gemm_kernel (128 x 128 tiles, the same splitk, the same gather on B, slabs) followed by koaf_slab_reduce.  The zero
    contributions of border taps and of the rows behind a k-range enter the accumulators where the generic kernel's do, so nothing
    may move.
  * against float64 on the CPU for sampled 64 x 64 blocks of dw -- the eight of test_wgrad1x1_gpu.py, and for the 3x3 cases one more
    per filter tap the eight miss, so that all nine taps are met: relative L2 < BWD per block and the componentwise bar of
    test_wgrad_gpu.py (8 x torch's fp32 product of the same operands); BWD and the bar's function are imported from test_tiles_gpu,
    not restated.  The CPU reference gathers the RAW x, applies the prologue and THEN zeroes the padding rows.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: the generic kernel at 128-wide tiles keeps layer2's 3x3 / stride 2 at 128 -> 128 (1152
columns are no whole number of 256-wide tiles beside 128 rows), the bf16 scheme, bf16 storage, k-ranges under 1024 pixels and a 3x3 /
stride-1 call without plane images.

(61 x 61 -> 31 x 31 and 30 x 31 -> 15 x 16 at 1x1; 61 x 62 -> 31 x 31 at 3x3: odd H reaches the bottom border tap, even W does not reach
the right one, top and left are reached in every image; 45 x 47 -> 23 x 24 reaches all four; 9 x 10 -> 5 x 5: a 32-row k-tile crosses
pixel rows and image boundaries several times, and a thread's four units, 8 rows apart, each wrap.)

Inputs are drawn on the device (one set per shape, shared by its calls); only the sampled, gathered columns travel to the CPU."""
from collections import namedtuple

import pytest

import tile256_refs as R

pytestmark = pytest.mark.gpu

W1K = "koaf_wgrad1"
Case = namedtuple("Case", "name shape call bm bn splitk empty last")
# shape (N, H, W, Cin, Cout, k, pad), stride 2; call: plain (dy + its amax) | apply (dy an ops.BnApply -- tf 2 on A --, plain x: the
# shortcuts' production call) | apply_prologue (and x behind its BatchNorm prologue -- tf 1 on B: conv2's); splitk / empty trailing
# splits / rows of the last live split: wgrad_plan's, as koaf_conv2d_wgrad_ws reports them (test_the_table_against_the_library_plan)
S1 = (133, 61, 61, 256, 512, 1, 0)        # P = 127 813: 128 splits of 1024 rows, the last live one 837, 3 empty; 2 tiles 256 x 256
S2 = (529, 61, 61, 128, 256, 1, 0)        # P = 508 369: 512 splits, 15 empty, one 256 x 128 tile
S3 = (529, 61, 61, 256, 128, 1, 0)        # the same plan, one 128 x 256 tile
S4 = (133, 30, 31, 1024, 512, 1, 0)       # P = 31 920: 32 splits; Cin / bn = 4 column tiles in the one tap
S5 = (58, 61, 62, 256, 256, 3, 1)         # P = 55 738: 56 splits, one empty; 9 column tiles = 9 taps
S6 = (13, 45, 47, 512, 512, 3, 1)         # P = 7 176: 7 splits of 1056 rows (no XCD remap); 18 column tiles, two per tap
S7 = (2223, 9, 10, 256, 256, 3, 1)        # P = 55 575: 5 x 5 output pixels per image
SHAPES = [S1, S2, S3, S4, S5, S6, S7]
CASES = [
    Case("k1-256to512-plain", S1, "plain", 256, 256, 128, 3, 837),
    Case("k1-256to512-apply", S1, "apply", 256, 256, 128, 3, 837),
    Case("k1-128to256-apply", S2, "apply", 256, 128, 512, 15, 465),
    Case("k1-256to128-apply", S3, "apply", 128, 256, 512, 15, 465),
    Case("k1-1024to512-plain", S4, "plain", 256, 256, 32, 0, 176),
    Case("k3-256to256-apply_prologue", S5, "apply_prologue", 256, 256, 56, 1, 442),
    Case("k3-512to512-apply_prologue", S6, "apply_prologue", 256, 256, 7, 0, 840),
    Case("k3-256to256-5x5-apply_prologue", S7, "apply_prologue", 256, 256, 56, 1, 279),
]
Refusal = namedtuple("Refusal", "name shape stride call store long_k")
R1 = (241, 61, 62, 128, 128, 3, 1)        # layer2's conv2: M = 128, N = 1152; k-ranges of 2080 pixels
R2 = (3, 40, 40, 512, 1024, 1, 0)         # P = 1200: k-ranges of 416 pixels
R3 = (80, 30, 31, 256, 256, 3, 1)         # 3x3 / stride 1 on the fp32 tensors (aplanes=False)
REFUSALS = [
    Refusal("k3s2-128to128", R1, 2, "apply_prologue", "fp32", True),
    Refusal("bf16scheme", S1, 2, "bf16scheme", "fp32", True),      # dy_amax withheld
    Refusal("bf16storage", S1, 2, "apply", "bf16", True),           # x and the apply's c stored as bf16 (act16 3)
    Refusal("kchunk416", R2, 2, "plain", "fp32", False),
    Refusal("k3s1-no-planes", R3, 1, "apply_prologue", "fp32", True),
]


def inputs(shape, stride, dev, store16=False):
    return R.wgrad_inputs(shape, stride, dev, 9300 + (SHAPES + [R1, R2, R3]).index(shape), store16)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_table_against_the_library_plan(case):
    P, splitk, kchunk, empty, last = R.plan_of(case.shape)
    assert (splitk, empty, last) == (case.splitk, case.empty, case.last), (case.name, P, splitk, kchunk, empty, last)
    assert kchunk >= 1024 and P % 32 != 0, (case.name, P, kchunk)


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_the_refusals_against_the_library_plan(case):
    """a refusal that is not about the k-range has k-ranges the rule would take"""
    P, splitk, kchunk, empty, last = R.plan_of(case.shape, case.stride)
    assert (kchunk >= 1024) == case.long_k, (case.name, P, splitk, kchunk)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gathered_wide_tile_kernel_equals_the_generic_path(dev, case):
    R.check_wgrad(dev, case, W1K, 2, inputs(case.shape, 2, dev), f"[wgrad1 gather] {case.name:32s}", show_tap=True)


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernel(dev, case):
    R.check_wgrad_refusal(dev, case, W1K, case.stride, inputs(case.shape, case.stride, dev, case.store == "bf16"))
