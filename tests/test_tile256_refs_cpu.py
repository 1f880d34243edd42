"""The float64 references of the 256-row units' tests (tile256_refs.py), checked without a GPU against torch's own conv2d and its autograd.

Geometries (N, H, W, ., ., k, pad), tiny channel counts, each with and without the ReLU prologue, at stride 2 and stride 1: an odd and
an even image under a 3x3 / pad 1 filter, two images under a 1x1 / pad 0 one.  Held:
  * the gathered operand (raw x gathered, the prologue applied, THEN the padding zeroed) times the packed weight is conv2d of the
    transformed image, and dy^T times it is autograd's weight gradient of that conv2d;
  * the four parity classes of classes() are the row blocks test_tiles_gpu._class_rows cuts, and cover every input pixel exactly once;
  * the dense column block is the one-tap case of the gathered one, bit for bit; sampled_blocks gives the dense eight with one tap;
  * a reference with the pad shifted by one, with kh / kw swapped, or with the padding zeroed BEFORE the prologue fails the comparison
    on the non-square images.
Bar: the unmutated differences are 0 (forward) and at most 1.5e-14 (weight gradient) in float64 at these sizes -- sums of a few hundred
terms of magnitude ~1; 1e-12 leaves two orders of magnitude.  A mutation moves whole terms: it must exceed 1e-3."""
import pytest
import torch
import torch.nn.functional as F

import tile256_refs as R
from test_tiles_gpu import _class_rows

BAR, CAUGHT = 1e-12, 1e-3
CIN, COUT = 5, 4
GEOMS = [(2, 7, 9, CIN, COUT, 3, 1), (2, 8, 6, CIN, COUT, 3, 1), (3, 7, 8, CIN, COUT, 1, 0), (1, 6, 6, CIN, COUT, 1, 0)]
NON_SQUARE = GEOMS[:3]
ids = lambda s: f"{s[0]}x{s[1]}x{s[2]}-k{s[5]}"      # noqa: E731


def draw(shape, stride):
    """x [N H W, Cin] float32, a prologue with shifts of both signs, a packed weight and a gradient in float64"""
    N, H, W, Cin, Cout, k, pad = shape
    OH, OW = R.out_hw(shape, stride)
    g_ = torch.Generator().manual_seed(77 + sum(shape) + stride)
    x = torch.randn(N * H * W, Cin, generator=g_) * 1.5 + 0.3
    sc, sh = torch.randn(Cin, generator=g_) * 0.2 + 1.0, torch.randn(Cin, generator=g_) * 0.5
    sh[0], sh[1] = 0.4, -0.4
    w = torch.randn(Cout, k, k, Cin, generator=g_, dtype=torch.float64) * (k * k * Cin) ** -0.5
    dy = torch.randn(N * OH * OW, Cout, generator=g_, dtype=torch.float64)
    return x, sc, sh, w, dy


def errors(shape, stride, prol, ref_shape=None):
    """(forward, weight gradient) largest absolute difference between the harness's operand and torch, both in float64; ref_shape: the
    geometry torch computes, where the harness is handed a mutated one"""
    N, H, W, Cin, Cout, k, pad = ref_shape or shape
    x, sc, sh, w, dy = draw(ref_shape or shape, stride)
    a64 = R.all_cols(shape, stride, x, sc if prol else None, sh if prol else None)[2]
    img = R.transform(x, sc if prol else None, sh if prol else None)[1].reshape(N, H, W, Cin).permute(0, 3, 1, 2)
    wt = w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(img, wt, stride=stride, padding=pad)
    y.backward(dy.reshape(N, *R.out_hw(ref_shape or shape, stride), Cout).permute(0, 3, 1, 2))
    fwd = (a64 @ w.reshape(Cout, -1).t() - y.detach().permute(0, 2, 3, 1).reshape(-1, Cout)).abs().max().item()
    wg = (dy.t() @ a64 - wt.grad.permute(0, 2, 3, 1).reshape(Cout, -1)).abs().max().item()
    return fwd, wg


@pytest.mark.parametrize("prol", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("stride", [2, 1])
@pytest.mark.parametrize("shape", GEOMS, ids=ids)
def test_gathered_operand_against_conv2d_and_its_autograd(shape, stride, prol):
    fwd, wg = errors(shape, stride, prol)
    assert fwd <= BAR and wg <= BAR, (fwd, wg)


@pytest.mark.parametrize("prol", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("stride", [2, 1])
@pytest.mark.parametrize("shape", NON_SQUARE, ids=ids)
def test_mutated_references_are_caught(shape, stride, prol, monkeypatch):
    N, H, W, Cin, Cout, k, pad = shape
    true_hw = R.out_hw(shape, stride)
    with monkeypatch.context() as m:            # the pad shifted by one (the output grid kept)
        m.setattr(R, "out_hw", lambda s, stride=2: true_hw)
        fwd, wg = errors((N, H, W, Cin, Cout, k, pad + 1), stride, prol, ref_shape=shape)
        assert fwd > CAUGHT and wg > CAUGHT, ("pad + 1", fwd, wg)
    if k == 1:
        return          # (one tap, no padding: nothing to swap, nothing to zero)
    with monkeypatch.context() as m:            # kh / kw swapped
        m.setattr(R, "tap_hw", lambda tap, k: (tap % k, tap // k))
        fwd, wg = errors(shape, stride, prol)
        assert fwd > CAUGHT and wg > CAUGHT, ("kh / kw", fwd, wg)
    if prol:
        with monkeypatch.context() as m:        # the padding zeroed before the prologue: relu(sh) where 0 belongs
            m.setattr(R, "masked", lambda x, ok, sc, sh: R.transform(x * ok, sc, sh))
            fwd, wg = errors(shape, stride, prol)
            assert fwd > CAUGHT and wg > CAUGHT, ("zeroed first", fwd, wg)


@pytest.mark.parametrize("shape", GEOMS, ids=ids)
def test_parity_classes_cover_every_input_pixel_once(shape):
    N, H, W, Cin, Cout, k, pad = shape
    pix = torch.arange(N * H * W).reshape(N, H, W, 1)
    rows = _class_rows(pix, (N, H, W, Cin, Cout, k, 2, pad))
    cls = R.classes(shape)
    assert len(rows) == len(cls) == 4
    for (py, px, Hc, Wc, khs, kws, nkh, nkw, offy, offx), r in zip(cls, rows):
        assert r.shape[0] == N * Hc * Wc, (py, px)
        assert torch.equal(r.reshape(N, Hc, Wc), pix[:, py::2, px::2, 0])
        # the taps of the class: kh = khs, khs + 2, ... < k reads dy row (y + pad - kh) / 2 = yy + offy - i
        assert nkh == len(range(khs, k, 2)) and nkw == len(range(kws, k, 2))
        assert (py + pad - khs) % 2 == 0 and offy == (py + pad - khs) // 2 and offx == (px + pad - kws) // 2
    assert torch.equal(torch.cat(rows).flatten().sort().values, torch.arange(N * H * W))


@pytest.mark.parametrize("prol", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", [g for g in GEOMS if g[5] == 1], ids=ids)
def test_dense_column_block_is_the_one_tap_gathered_one(shape, prol):
    x, sc, sh, w, dy = draw(shape, 1)
    assert R.pointwise(shape, 1) and R.pointwise(shape[:5], 1) and not R.pointwise(shape, 2)
    for ci in (slice(None), slice(1, 4)):
        dense = R.dense_cols(x, ci, sc if prol else None, sh if prol else None)
        gathered = R.gathered_cols(shape, 1, x, 0, ci, sc if prol else None, sh if prol else None)
        assert dense[:2] == gathered[:2] == (0, 0)
        assert torch.equal(dense[2], gathered[2]) and torch.equal(dense[3], gathered[3])


def test_sampled_blocks_with_one_tap_are_the_dense_eight():
    for Cout, Cin in ((1024, 256), (2048, 512), (256, 256), (512, 128), (128, 512), (512, 1024)):
        one = R.sampled_blocks(Cout, Cin, Cin)
        assert len(one) == len(set(one)) == min(8, (Cout // 64) * (Cin // 64))
        nine = R.sampled_blocks(Cout, 9 * Cin, Cin)
        assert {bj // (Cin // 64) for _, bj in nine} == set(range(9)) and len(nine) >= 8
