"""GPU: the two class-activation-map kernels (koaf_cam.hip) on their own.

koaf_cam against float64 numpy.  The summation order built: a lane multiplies its 4-channel vectors into four fmaf chains of
ceil(C / 256) links, adds them pairwise (2 roundings) and the wave adds its 64 lanes in a 6-level butterfly; the store rounds
nothing.  ceil(C / 256) + 8 roundings on the longest path -- and where fewer than 64 lanes hold a vector (C < 256) the
butterfly levels that add zeros are exact: 1 + 2 + ceil(log2(C / 4)) -- which is never more than the C / 64 + 7 the bar
below counts (C = 4: 3 vs 7.06; 68: 8 vs 8.06; 512: 10 vs 15; 2048: 16 vs 39).  Per element: (C / 64 + 7) * 2^-24 * sum_c |a_c w_c|.
img_sum: the per-element bounds of the row's pixels added up, plus (log2 HW + 1) * 2^-24 * sum |cam| for the sum itself (built:
each of the 4 waves deals its row results to its lanes, a butterfly per wave, (w0 + w1) + (w2 + w3): for HW = 1 / 9 / 25 / 121
that is 0 / 4 / 5 / 7 roundings against 1 / 4.2 / 5.6 / 7.9).  img_max: the bits of the largest magnitude of the returned map.

koaf_cam_upsample against F.interpolate(mode="bilinear", align_corners=False) in float64 on the CPU, within 2e-6 * max|map| (the
bar test_interpolate_any_scale_vs_reference holds koaf_resize to), through every row of the stride table of run.cam_strides."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = 3


def _case(HW, C, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, HW, C)).astype(np.float32)
    w = (rng.standard_normal((N, C)) / C).astype(np.float32)
    return torch.from_numpy(A), torch.from_numpy(w)


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("C", [4, 68, 512, 2048])
@pytest.mark.parametrize("HW", [1, 9, 25, 121])
def test_cam_vs_float64(dev, HW, C):
    from oaprogressionmmf_amd import ops
    A32, w = _case(HW, C, 1000 * HW + C)
    for store in (torch.float32, torch.bfloat16):
        A = A32.to(store)
        Aw = A.float()                                    # (the values the kernel computes on: bf16 widens exactly)
        prod = Aw.double().numpy() * w.double().numpy()[:, None, :]
        truth, mag = prod.sum(-1), np.abs(prod).sum(-1)
        bar = (C / 64 + 7) * U * mag
        for relu in (True, False):
            cam, isum, imax = ops.cam(A.to(dev), w.to(dev), N, HW, C, relu=relu)
            assert cam.shape == (N, HW) and isum.shape == imax.shape == (N,) and cam.dtype == isum.dtype == imax.dtype == torch.float32
            want = np.maximum(truth, 0.0) if relu else truth
            got = cam.cpu().double().numpy()
            err = np.abs(got - want)
            print(f"\n[cam HW={HW} C={C} {store} relu={relu}] worst error / bar {float((err / bar).max()):.3f}")
            assert (err <= bar).all(), (HW, C, store, relu, float((err / bar).max()))
            sum_bar = bar.sum(-1) + (math.log2(HW) + 1) * U * np.abs(want).sum(-1)
            serr = np.abs(isum.cpu().double().numpy() - want.sum(-1))
            assert (serr <= sum_bar).all(), (HW, C, store, relu, serr, sum_bar)
            assert torch.equal(_bits(imax), _bits(cam.abs().max(dim=1).values)), "img_max: the bits of the largest magnitude"
            again = ops.cam(A.to(dev), w.to(dev), N, HW, C, relu=relu)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((cam, isum, imax), again)), "two runs, the same bits"
            if store == torch.bfloat16:
                wide = ops.cam(Aw.to(dev), w.to(dev), N, HW, C, relu=relu)
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((cam, isum, imax), wide)), "bf16 == fp32 on the widened values"
            if relu:
                assert float(cam.min()) >= 0.0 and (HW * N < 8 or float(cam.max()) > 0.0)


@pytest.mark.parametrize("store", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cam_nan_reaches_its_pixel_and_its_image_maximum(dev, store):
    from oaprogressionmmf_amd import ops
    HW, C = 25, 512
    A, w = _case(HW, C, 5)
    A[1, 7, 300] = float("nan")
    for relu in (True, False):
        cam, isum, imax = ops.cam(A.to(store).to(dev), w.to(dev), N, HW, C, relu=relu)
        bad = torch.isnan(cam).cpu()
        want = torch.zeros(N, HW, dtype=torch.bool)
        want[1, 7] = True
        assert torch.equal(bad, want), "exactly that pixel"
        assert torch.isnan(imax[1]) and torch.isfinite(imax[[0, 2]]).all() and torch.isfinite(isum[[0, 2]]).all()


def test_cam_refuses_bad_arguments(dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    A, w = _case(9, 6, 3)
    with pytest.raises(KoafError):
        ops.cam(A.to(dev), w.to(dev), N, 9, 6)                     # C % 4
    A, w = _case(9, 8, 3)
    with pytest.raises(KoafError):
        ops.cam(A.to(dev), w.to(dev), N, 25, 8)                    # shape mismatch
    with pytest.raises(KoafError):
        ops.cam_upsample(torch.zeros(2, 3, 3, device=dev), None, torch.zeros(2, 1, 8, 8, device=dev), 2, 1, 3, 3, 8, 8, (64, 64, 8, 2))


# ---- koaf_cam_upsample ---------------------------------------------------------------------------------------------------
# layout -> (shape of out for (B, K, H, W), permutation of the (B, K, H, W) truth into it)
LAYOUTS = {
    None: (lambda B, K, H, W: (B, 1, H, W), None),
    "rc": (lambda B, K, H, W: (B, 1, H, W, K), (0, 2, 3, 1)),
    "src": (lambda B, K, H, W: (B, 1, K, H, W), (0, 1, 2, 3)),
    "cs": (lambda B, K, H, W: (B, 1, K, H, W), (0, 1, 2, 3)),
    "rs": (lambda B, K, H, W: (B, 1, H, K, W), (0, 2, 1, 3)),
}
SENTINEL = -12345.0


def _upsample_case(dev, view, B, K, h, w, H, W, normalize, maxima=None):
    """run the kernel into a sentinel-filled tensor; -> (out on the CPU as float64, float64 truth in the same layout)"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.run import cam_strides
    rng = np.random.default_rng(h * 1000 + H + K)
    cam = torch.from_numpy(rng.standard_normal((B * K, h, w)).astype(np.float32))
    imax = cam.abs().reshape(B * K, -1).max(dim=1).values if maxima is None else maxima
    shape_of, perm = LAYOUTS[view]
    shape = shape_of(B, K, H, W)
    Kc, sb, sk, si, sj = cam_strides(view, shape)
    assert Kc == K
    out = torch.full(shape, SENTINEL, device=dev)
    ops.cam_upsample(cam.to(dev), imax.to(dev) if normalize is not None or maxima is not None else None, out, B, K, h, w, H, W,
                     (sb, sk, si, sj), normalize)
    up = F.interpolate(cam.double().view(B, K, h, w), size=(H, W), mode="bilinear", align_corners=False)
    with np.errstate(all="ignore"):
        if normalize == "sample":
            m = imax.double().view(B, K).max(dim=1).values.view(B, 1, 1, 1)
            m = torch.where(torch.isnan(imax.view(B, K)).any(dim=1).view(B, 1, 1, 1), torch.full_like(m, float("nan")), m)
        elif normalize == "image":
            m = imax.double().view(B, K, 1, 1)
        else:
            m = torch.ones(1, 1, 1, 1, dtype=torch.float64)
        m = m.expand(B, K, 1, 1)
        want = torch.where(m == 0, torch.zeros_like(up), torch.where(torch.isfinite(m), up / m, torch.full_like(up, float("nan"))))
    if perm is not None:
        want = want.permute(*perm)
    return out.cpu().double().reshape(want.shape), want.contiguous()


def _check(got, want, what):
    assert not (got == SENTINEL).any(), f"{what}: an element was not written"
    tol = 2e-6 * float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= tol, f"{what}: off by {err:.3e} (bar {tol:.3e})"


SIZES = [((3, 3), (96, 96)), ((5, 5), (160, 160)), ((11, 11), (350, 350)), ((1, 1), (32, 32)), ((3, 5), (90, 150))]


@pytest.mark.parametrize("normalize", [None, "sample", "image"], ids=str)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_cam_upsample_radiograph_and_rc_volume(dev, size, normalize):
    """every size, for the (B,1,H,W) radiograph and the (B,1,R,C,S) volume with a slice count that takes the 16-byte stores (8)
    and one that takes the scalar ones (5); (3,5)->(90,150) has a column count that is no multiple of 4 either"""
    (h, w), (H, W) = size
    for view, K in ((None, 1), ("rc", 8), ("rc", 5)):
        got, want = _upsample_case(dev, view, 2, K, h, w, H, W, normalize)
        _check(got, want, f"{view} K={K} {size} {normalize}")


@pytest.mark.parametrize("normalize", [None, "sample", "image"], ids=str)
@pytest.mark.parametrize("view", list(LAYOUTS), ids=str)
def test_cam_upsample_every_layout(dev, view, normalize):
    (h, w), (H, W) = SIZES[0]
    got, want = _upsample_case(dev, view, 2, 1 if view is None else 6, h, w, H, W, normalize)
    _check(got, want, f"{view} {normalize}")


def test_cam_upsample_rc_volume_whose_source_row_exceeds_lds(dev):
    """slices on the unit-stride axis are written from a source row staged in LDS (w * K floats); where that row does not fit
    (64 columns x 300 slices: 75 KiB) the element-wise kernel takes the same strides"""
    got, want = _upsample_case(dev, "rc", 1, 300, 2, 64, 4, 128, "sample")
    _check(got, want, "rc, wide source")


@pytest.mark.parametrize("view", [None, "rc", "rs"], ids=str)
def test_cam_upsample_zero_and_non_finite_maxima(dev, view):
    """a zero maximum writes zeros; a non-finite one NaN for everything it scales: the sample ("sample") or the image ("image")"""
    (h, w), (H, W) = SIZES[0]
    B, K = 3, 1 if view is None else 4
    for normalize in ("sample", "image"):
        for poison in (float("nan"), float("inf")):
            maxima = torch.full((B * K,), 2.0)
            maxima[0:K] = 0.0                                  # sample 0: all maxima zero
            maxima[2 * K + K // 2] = poison                    # sample 2: one image's maximum is not finite
            got, want = _upsample_case(dev, view, B, K, h, w, H, W, normalize, maxima=maxima)
            assert not (got == SENTINEL).any()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (view, normalize, poison)
            b_axis = got.reshape(B, -1)
            assert (b_axis[0] == 0).all(), "a zero maximum writes zeros"
            assert torch.isfinite(b_axis[1]).all() and torch.isnan(b_axis[2]).any()
            if normalize == "sample":
                assert torch.isnan(b_axis[2]).all(), "the whole sample"
            ok = ~torch.isnan(want)
            assert float((got[ok] - want[ok]).abs().max()) <= 2e-6 * float(want[ok].abs().max())
