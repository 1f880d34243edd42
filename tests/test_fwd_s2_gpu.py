"""The stride-2 forward convolutions on the 256-row gathered kernel (koaf_fwd_s2.hip) against the generic path they leave.

koaf_conv2d_fwd hands a stride-2 forward convolution -- the 1x1 / pad 0 shortcuts and the 3x3 / pad 1 conv2 of a downsampling block -- to
koaf_fwd_s2 when the call runs the fp16 scheme on fp32 tensors with the weights' F plane image, Cin % 32 == 0, Cout % 128 == 0 and
M = N OH OW is a whole number of 256-row tiles (koaf_fwd_s2.hip koaf_fwd_s2_ok).  Row m = output pixel (n, oy, ox), k = (tap, ci), element
x[n][2 oy - pad + kh][2 ox - pad + kw][ci] behind its transform, 0 outside the image.  Every row of CASES is the smallest shape of its
kind; it goes through ops.conv2d_fwd as the model calls it, with y and the statistics buffer pre-filled with NaN, and ASSERTS FROM THE
LAUNCH RECORD the variant, tile and tile count.

Held per case:
  * y, the returned row count and part[:rows] are torch.equal to the generic path on the same inputs: ops.gemm with the descriptor
    koaf_conv2d_fwd builds for koaf_gemm_kernel on 128 x 128 tiles (the tile the production sizes of these calls run on), which bypasses
    the new rule.  The new kernel writes two partial rows per 256-row tile where the 128-row tiling puts them, so nothing may move.
  * against float64 on the CPU for sampled 64-column blocks of y over ALL rows: relative L2 < FWD per 128-row band and the componentwise
    bar of test_tiles_gpu (8 x torch's fp32 product of the same operands); FWD and the bar's function are imported, not restated.  The
    CPU reference gathers the RAW x, applies the prologue and THEN zeroes the padding.  The statistics of the sampled columns are held
    against the float64 column sums of (y - shift) and (y - shift)^2 at run_forward's bars for the same sums (1e-4 / 1e-5 relative L2
    over the columns); the shift is a generic vector, not the mean, so the first sum is not a cancellation.
  * the same call twice gives equal results.
REFUSALS are asserted from the launch record: M no multiple of 256, the bf16 scheme (no plane images), bf16 activation storage,
caller-supplied x_planes, an emission request (the library serves none for a gathered call: it must not reach the new kernel either), Cout = 64
and stride 1.

(23 x 31 -> 12 x 16 at 3x3 / pad 1: odd H and W reach all four border taps and the 256-row tiles cross image boundaries; 9 x 10 -> 5 x 5:
a tile spans ten images and each of a thread's four rows, 64 apart, wraps rows and images; Cin = 32: the tap changes every k-step, nine
steps; 1x1 at Cin = 32 is ONE k-tile: the pipeline's prologue meets its drain.)"""
from collections import namedtuple

import pytest
import torch

import tile256_refs as R

pytestmark = pytest.mark.gpu

FS2 = "koaf_fwd_s2"
Case = namedtuple("Case", "name shape call stats bn")
# shape (N, H, W, Cin, Cout, k, pad), stride 2; call: plain | prologue (tf 1); stats: False | True | "shift"
CASES = [
    Case("k3-128to128-prologue-shift", (4, 23, 31, 128, 128, 3, 1), "prologue", "shift", 128),
    Case("k3-256to256-5x5-prologue", (256, 9, 10, 256, 256, 3, 1), "prologue", True, 256),
    Case("k3-32to128-prologue", (4, 23, 31, 32, 128, 3, 1), "prologue", True, 128),
    Case("k1-256to512-plain", (4, 23, 31, 256, 512, 1, 0), "plain", True, 256),
    Case("k1-1024to2048-plain", (2, 31, 31, 1024, 2048, 1, 0), "plain", True, 256),
    Case("k1-32to128-one-ktile", (4, 23, 31, 32, 128, 1, 0), "plain", True, 128),
    Case("k3-128to128-prologue-nostats", (4, 23, 31, 128, 128, 3, 1), "prologue", False, 128),
]
Refusal = namedtuple("Refusal", "name shape stride how")
REFUSALS = [
    Refusal("M-960", (5, 23, 31, 128, 128, 3, 1), 2, "plain"),
    Refusal("bf16scheme", (4, 23, 31, 128, 128, 3, 1), 2, "noimg"),
    Refusal("bf16storage", (4, 23, 31, 128, 128, 3, 1), 2, "bf16"),
    Refusal("x_planes", (4, 23, 31, 128, 128, 3, 1), 2, "xplanes"),
    Refusal("emit", (4, 23, 31, 128, 128, 3, 1), 2, "emit"),
    Refusal("Cout-64", (4, 23, 31, 128, 64, 3, 1), 2, "plain"),
    Refusal("stride-1", (4, 16, 16, 128, 128, 3, 1), 1, "plain"),
]


def inputs(shape, dev):
    return R.forward_inputs(shape, dev, 9800 + sum(shape))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gathered_256_row_kernel_equals_the_generic_path(dev, case):
    R.check_forward(dev, case, FS2, 2, inputs(case.shape, dev), f"[fwd_s2] {case.name:30s}")


@pytest.mark.parametrize("case", REFUSALS, ids=[c.name for c in REFUSALS])
def test_refused_calls_stay_on_the_generic_kernel(dev, case):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    N, H, W, Cin, Cout, k, pad = case.shape
    try:
        t = dict(inputs(case.shape, dev))
        kw = {}
        if case.how == "noimg":
            kw["wimg"] = None
        if case.how == "bf16":
            t["x"] = t["x"].bfloat16()
        if case.how == "xplanes":
            kw["aplanes"] = ops.act_planes(t["x"], N * H * W, Cin, 0, None, None, fscale=ops.ACT_SCALE)
        if case.how == "emit":
            kw["emit"] = (t["sc"].new_ones(Cout), t["sc"].new_zeros(Cout))
        if case.stride == 1:
            kw["aplanes"] = False
        try:
            y, part, launches = R.conv_fwd(case.shape, case.stride, t, "plain", case.how != "emit", **kw)
        except KoafError:
            # (an emission request on a gathered call: the generic path serves none and says so -- the new kernel must not have taken it)
            assert case.how == "emit", case.name
            ops.launch_log(False)
            return
        R.hold_refusal(case.name, launches, FS2, [y], 0 if case.how == "noimg" else 1, 1 if case.how == "bf16" else 0)
    finally:
        torch.cuda.empty_cache()
