"""The dense 1x1 / stride-1 forward convolutions on the 256-row kernel (koaf_fwd1.hip) against the streamed kernel they leave.

koaf_conv2d_fwd hands a pointwise forward convolution to koaf_fwd1 when the call runs the fp16 scheme on fp32 tensors with the weights'
F plane image, without tail or emission, Cin % 32 == 0 with at least two k-tiles, Cout % 128 == 0, the streamed kernels switched on and
M a whole number of 256-row tiles, at least one per CU (M >= 65536) -- koaf_fwd1.hip koaf_fwd1_ok.  koaf_fwd1_form's table names, per
production (Cin, Cout), the form that passed the per-call rule: one tile per block (grid_x = tiles; 512 -> 2048), the persistent walk
(grid_x = min(tiles, 256); 128 -> 512, 256 -> 1024, 256 -> 128, 512 -> 256) or neither (64 -> 256 stays on the streamed kernel: the
first REFUSAL; K = 64 is therefore reached at 64 -> 512); a shape the table does not know runs the walk.  Every row of CASES is the smallest shape of its
kind (all have M >= 65536, none more than 70000 rows); it goes through ops.conv2d_fwd as the model calls it, with y and the statistics
buffer pre-filled with NaN, and ASSERTS FROM THE LAUNCH RECORD the variant, tile, tile count and grid_x.

Held per case:
  * y, the returned row count and part[:rows] are torch.equal to ops.gemm on the descriptor koaf_conv2d_fwd builds, at 128 x 128 tiles
    (ops.gemm bypasses the new rule and runs koaf_gemm/stream), and once more with ops.set_stream(False) around the reference call (the
    block-wide loader).  The new kernel writes two partial rows per 256-row tile where the 128-row tiling puts them.
  * against float64 on the CPU for sampled 64-column blocks of y over ALL rows: relative L2 < FWD per 128-row band and the componentwise
    bar of test_tiles_gpu (8 x torch's fp32 product of the same operands); FWD and the bar's function are imported, not restated.  The
    statistics of the sampled columns are held against the float64 column sums of (y - shift) and (y - shift)^2 at run_forward's bars
    (1e-4 / 1e-5 relative L2 over the columns); the shift is a generic vector, not the mean.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: no koaf_fwd1 record, and the last GEMM record is koaf_gemm or koaf_gemm/stream on 128-row
tiles (stride 2 at the same shape: koaf_fwd_s2).  K-8224: the rule admits at most 8192 channels; the call stays on the generic kernel
and must not come back KOAF_EINVAL from the unit's entry.

(K = 64: two k-steps, the next tile's prefetch is issued in the first; 66304 rows = 259 row tiles x 2 = 518 tiles: blocks walk 2 and 3
tiles and a row-tile change falls inside a block's run; 256 -> 768 and 128 -> 384: three column tiles per row tile at either width; Cin = 1024 fills the coefficient table; Cin = 2048
plain runs past it.)"""
from collections import namedtuple

import pytest
import torch

import tile256_refs as R
from tile256_refs import GEN, STREAM

pytestmark = pytest.mark.gpu

F1, FS2 = "koaf_fwd1", "koaf_fwd_s2"
Case = namedtuple("Case", "name shape call stats bn walk")
# shape (N, H, W, Cin, Cout); call: plain | prologue (tf 1); stats: False | True | "shift"; walk: the form koaf_fwd1_form ships the shape in
CASES = [
    Case("64to512-prologue-shift", (64, 32, 32, 64, 512), "prologue", "shift", 256, 1),
    Case("128to512-prologue-259-row-tiles", (37, 32, 56, 128, 512), "prologue", True, 256, 1),
    Case("256to768-prologue-nostats", (64, 32, 32, 256, 768), "prologue", False, 256, 1),
    Case("1024to256-prologue", (64, 32, 32, 1024, 256), "prologue", True, 256, 1),
    Case("2048to256-plain", (64, 32, 32, 2048, 256), "plain", True, 256, 1),
    Case("256to128-plain-shift", (64, 32, 32, 256, 128), "plain", "shift", 128, 1),
    Case("128to384-prologue", (64, 32, 32, 128, 384), "prologue", True, 128, 1),
    Case("512to2048-prologue-one-tile-form", (64, 32, 32, 512, 2048), "prologue", True, 256, 0),
]
Refusal = namedtuple("Refusal", "name shape stride how")
BASE = (64, 32, 32, 128, 256)
REFUSALS = [
    Refusal("64to256-kept-by-the-per-call-rule", (64, 32, 32, 64, 256), 1, "prologue"),
    Refusal("M-65664", (513, 16, 8, 128, 256), 1, "plain"),
    Refusal("M-12288", (48, 16, 16, 256, 512), 1, "plain"),
    Refusal("stream-off", BASE, 1, "nostream"),
    Refusal("tail", BASE, 1, "tail"),
    Refusal("emit", BASE, 1, "emit"),
    Refusal("bf16storage", BASE, 1, "bf16"),
    Refusal("bf16scheme", BASE, 1, "noimg"),
    Refusal("Cout-64", (64, 32, 32, 128, 64), 1, "plain"),
    Refusal("K-32", (64, 32, 32, 32, 256), 1, "plain"),
    Refusal("prologue-Cin-2048", (64, 32, 32, 2048, 128), 1, "prologue"),
    Refusal("K-8224", (64, 32, 32, 8224, 128), 1, "plain"),      # (more channels than the unit takes, at the smallest M its rule engages)
    Refusal("stride-2", BASE, 2, "plain"),
]


def inputs(shape, dev):
    return R.forward_inputs(shape, dev, 10100 + sum(shape))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_256_row_kernel_equals_the_streamed_kernel(dev, case):
    N, H, W, Cin, Cout = case.shape
    M = N * H * W
    assert M % 256 == 0 and 65536 <= M <= 70000
    # the reference twice: the streamed kernel, and with ops.set_stream(False) the block-wide loader.  float64: both halves of a column
    # tile, the first and the last tile; at K >= 1024 the first and the last block (34 GFLOP in float64)
    R.check_forward(dev, case, F1, 1, inputs(case.shape, dev), f"[fwd1] {case.name:32s}", grid_x=lambda tiles: min(tiles, 256) if case.walk else tiles,
                    legs=((True, STREAM), (False, GEN)), few=Cin >= 1024)


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernels(dev, case):
    from oaprogressionmmf_amd import ops
    N, H, W, Cin, Cout = case.shape
    was = ops.set_stream(case.how != "nostream")
    try:
        t = dict(inputs(case.shape, dev))
        kw = {}
        call = "prologue" if case.how in ("prologue", "tail") else "plain"
        if case.how == "noimg":
            kw["wimg"] = None
        if case.how == "bf16":
            t["x"] = t["x"].bfloat16()
        if case.how == "tail":
            kw["tail_idt"] = torch.randn(N, H, W, Cin, device=dev)
        if case.how == "emit":
            kw["emit"] = (t["sc"].new_ones(Cout), t["sc"].new_zeros(Cout))
        y, part, launches = R.conv_fwd(case.shape, case.stride, t, call, True, **kw)
        last = R.hold_refusal(case.name, launches, F1, [y], 0 if case.how == "noimg" else 1, 1 if case.how == "bf16" else 0,
                              kept=(FS2,) if case.stride == 2 else (GEN, STREAM))[-1]
        assert last["bm"] == (256 if case.stride == 2 else 128), (case.name, launches)
        assert case.how != "nostream" or last["variant"] == GEN, (case.name, launches)
        assert bool(last["emit"]) == (case.how == "emit") and last["a_tf"] == {"tail": 3, "prologue": 1}.get(case.how, 0), (case.name, last)
    finally:
        ops.set_stream(was)
        torch.cuda.empty_cache()
