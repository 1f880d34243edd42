"""koaf_window_minmax / koaf_input_pipeline (koaf_inpipe.hip) and preproc.PTBatchPipeline: from the stored integer volumes to the
model's input in two library calls (three kernels).

The float64 reference is composed as the reference composes it: np.flip -> crop slice -> elem_refs.augment_ref (unit range,
affine_grid + grid_sample, gamma, normalise) -> float64 F.interpolate(scale_factor, recompute_scale_factor=True,
align_corners=False).  Bars are the ones the project already holds koaf_augment to (test_augment_both_vector_widths): 2e-5
absolute where the exponent is 0 or 2, the 4x-yardstick rule against the same chain in torch fp32 (floor 2e-5) where it is 0.5;
a mean of 4 or 8 values that each meet such a bar meets it too.

Every stored voxel OUTSIDE the window is 60000 (the type's maximum where that does not fit) while the window holds [5, 310] with
its extremes in its first and last voxel: a read outside the window -- in the reduction or as a bilinear neighbour -- is a
gross error, not a rounding-level one.  Shapes are a few thousand voxels; one case has a million voxels per sample, several
thousand blocks in each sample's block column."""
import functools
import math
import random
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elem_refs as ER
from test_elem_edges_gpu import yardstick

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
MEAN, STD = 0.4, 0.2
NP_DT = {"uint8": np.uint8, "uint16": np.uint16, "int16": np.int16, "float32": np.float32}
OUTSIDE = {"uint8": 255, "uint16": 60000, "int16": 32767, "float32": 60000}
SHAPES3 = {"s6": ((11, 13, 9), (8, 10, 6)), "s8": ((14, 12, 11), (8, 8, 8))}       # s8: S % 4 == 0, four slices per thread
SHAPE2 = ((13, 11), (10, 8))
FLIPS = {"none": None, "C": 2, "S": -1}
POOLS = {"p111": None, "p221": (0.5, 0.5, 1.0), "p222": (0.5, 0.5, 0.5)}
ROTS = [None, 0.0, 7.0, 45.0, 90.0]
GAMMAS = [(1.0, 1.0), (0.0, 2.0), (0.0, 0.5)]                                       # exponent 0 (off), 0.5, 2 across the batch


def _flipped_dim(flip_axis, nd):
    return None if flip_axis is None else (flip_axis - 1 if flip_axis >= 0 else nd + flip_axis)


@functools.lru_cache(maxsize=None)
def make_case(in_shape, out, flip_axis, end, dtype="uint16", seed=0, lo=5, hi=310, B=3):
    """-> (stored [B, *in_shape] of `dtype`, window [B, *out] int64, ratios): the window the reference's flip + crop cuts out of
    `stored` is `window`; everything else in `stored` is OUTSIDE[dtype]"""
    nd = len(out)
    rng = np.random.default_rng(4100 + seed + 7 * nd + sum(in_shape))
    ratios = (0.0,) * nd if end == 0 else (0.999999,) * nd
    start = [math.floor(r * (i - o)) for r, i, o in zip(ratios, in_shape, out)]
    win = rng.integers(lo, hi + 1, size=(B,) + tuple(out)).astype(np.int64)
    win.reshape(B, -1)[:, 0], win.reshape(B, -1)[:, -1] = lo, hi
    vol = np.full((B,) + tuple(in_shape), OUTSIDE[dtype], dtype=np.int64)
    vol[(slice(None),) + tuple(slice(s, s + o) for s, o in zip(start, out))] = win
    fd = _flipped_dim(flip_axis, nd)
    if fd is not None:
        vol = np.flip(vol, axis=1 + fd)            # stored = un-flipped: the reference's np.flip brings the window back
    stored = np.ascontiguousarray(vol).astype(NP_DT[dtype])
    # the reference's own composition on `stored`: np.flip (axis counted on the (ch, d0, ...) array of ONE sample) -> crop slice
    for b in range(B):
        img = stored[b][None]
        img = img if flip_axis is None else np.flip(img, axis=flip_axis)
        crop = img[(slice(None),) + tuple(slice(s, s + o) for s, o in zip(start, out))][0]
        assert np.array_equal(crop.astype(np.int64), win[b])
    stored.setflags(write=False)
    win.setflags(write=False)
    return stored, win, ratios


def states_of(ratios, rot_deg, gammas):
    return [(ratios, 1.0 if rot_deg is None else 0.0, 0.0 if rot_deg is None else math.radians(rot_deg), pg, g) for pg, g in gammas]


def prm_of(states):
    """(cos, sin, exponent or 0, rotated) as PTBatchPipeline builds them (rotate_prob = gamma_prob = 0.5)"""
    return torch.tensor([[math.cos(th) if pr < 0.5 else 1.0, math.sin(th) if pr < 0.5 else 0.0, 1.0 / g if pg < 0.5 else 0.0,
                          1.0 if pr < 0.5 else 0.0] for _, pr, th, pg, g in states], dtype=torch.float32)


def chain_ref(win, prm, sf, dtype=torch.float64, mean=MEAN, std=STD):
    """augment_ref on the cropped window, then F.interpolate as PTInterpolate calls it -> [B, R', C'[, S']]"""
    B, nd = win.shape[0], win.ndim - 1
    raw = torch.from_numpy(np.asarray(win, dtype=np.float32)).reshape((B,) + tuple(win.shape[1:]) + (1,) * (3 - nd))
    a = ER.augment_ref(raw, prm, mean, std, dtype=dtype)
    a = a[..., 0] if nd == 2 else a
    if sf is None:
        return a
    return F.interpolate(a[:, None], scale_factor=sf, recompute_scale_factor=True, align_corners=False,
                         mode={2: "bilinear", 3: "trilinear"}[nd])[:, 0]


def dev_vol(stored, dev):
    return torch.from_numpy(np.array(stored)).unsqueeze(1).to(dev)              # (B, 1, R0, C0[, S0])


def hold(got, win, states, sf, what):
    """every sample of the batch to its bar (the exponent decides which)"""
    prm = prm_of(states)
    ref, ref32 = chain_ref(win, prm, sf), chain_ref(win, prm, sf, dtype=torch.float32)
    got = got.cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for b in range(got.shape[0]):
        ex = float(prm[b, 2])
        if ex == 0.5:
            yardstick(got[b], ref[b], ref32[b], f"{what} b{b} ex=0.5", floor=2e-5)
        else:
            assert torch.isfinite(got[b]).all(), f"{what} b{b}: non-finite output"
            e = float((got[b].double() - ref[b]).abs().max())
            print(f"ABS {what} b{b} ex={ex}: {e:.3e}")
            assert e < 2e-5, f"{what} b{b} ex={ex}: off by {e:.3e}"


# =================================================================================================
# window_minmax
# =================================================================================================
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32"])
@pytest.mark.parametrize("in_shape,out", [((11, 13, 9), (8, 10, 6)), ((14, 12, 11), (8, 8, 8)), ((13, 11), (10, 8)), ((13, 10), (10, 7)),
                                          ((20, 21, 19), (18, 18, 16)), ((35, 37, 12), (32, 32, 8))])
def test_window_minmax_is_exact(dev, in_shape, out, dtype):
    """bit-equal to torch's amin / amax of the window, with flips on and odd origins; (18, 18, 16) and (32, 32, 8) reach a second
    block of the first stage, (10, 8) walks a radiograph's columns four at a time, (10, 7) one at a time"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.preproc import crop_geometry
    nd = len(out)
    hi = 250 if dtype == "uint8" else 310
    for flip_axis in (None, 2, -1):
        for end in (0, 1):
            stored, win, ratios = make_case(in_shape, out, flip_axis, end, dtype, hi=hi)
            vols = list(dev_vol(stored, dev).unbind(0))
            geo = [crop_geometry(in_shape, out, ratios, flip_axis) for _ in vols]
            table, code, w3 = ops.window_table(vols, [g[0] for g in geo], [g[1] for g in geo], out)
            mm = ops.window_minmax(table, code, w3).cpu()
            w = torch.from_numpy(np.asarray(win, dtype=np.float32)).reshape(len(vols), -1)
            assert torch.equal(mm[:, 0], w.amin(1)) and torch.equal(mm[:, 1], w.amax(1)), (flip_axis, end, mm)
            assert torch.equal(mm, torch.tensor([[5.0, float(hi)]] * len(vols)))
    if dtype == "int16":                                        # negative stored values keep their sign
        v = torch.tensor([[-300, 7], [12, -32768]], dtype=torch.int16).reshape(1, 2, 2, 1).to(dev)
        table, code, w3 = ops.window_table([v], [(0, 0, 0)], [0], (2, 2, 1))
        assert torch.equal(ops.window_minmax(table, code, w3).cpu(), torch.tensor([[-32768.0, 12.0]]))


def test_window_table_refuses_what_leaves_the_volume(dev):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    v = torch.zeros(1, 11, 13, 9, dtype=torch.uint8, device=dev)
    ops.window_table([v], [(3, 3, 3)], [0], (8, 10, 6))
    ops.window_table([v], [(10, 12, 8)], [7], (8, 10, 6))
    for org, back in (((4, 3, 3), 0), ((3, 3, 4), 0), ((3, 3, 4), 4), ((6, 12, 8), 7), ((-1, 0, 0), 0), ((3, 13, 3), 2)):
        with pytest.raises(KoafError, match="leaves the stored volume"):
            ops.window_table([v], [org], [back], (8, 10, 6))
    with pytest.raises(KoafError):
        ops.window_table([v.double()], [(0, 0, 0)], [0], (8, 10, 6))
    with pytest.raises(KoafError):
        ops.window_table([v.cpu()], [(0, 0, 0)], [0], (8, 10, 6))
    with pytest.raises(KoafError):
        ops.window_table([v.permute(0, 2, 1, 3)], [(0, 0, 0)], [0], (8, 10, 6))


# =================================================================================================
# pipeline parity: pools x rotation x exponent x flip x origin
# =================================================================================================
@pytest.mark.parametrize("end", [0, 1])
@pytest.mark.parametrize("flip", ["none", "C", "S"])
@pytest.mark.parametrize("pool", ["p111", "p221", "p222"])
@pytest.mark.parametrize("shape", ["s6", "s8"])
def test_pipeline_parity_3d(dev, shape, pool, flip, end):
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = SHAPES3[shape]
    stored, win, ratios = make_case(in_shape, out, FLIPS[flip], end)
    x = dev_vol(stored, dev)
    pipe = PTBatchPipeline(out, MEAN, STD, flip_axis=FLIPS[flip], scale_factor=POOLS[pool])
    for rot in ROTS:
        states = states_of(ratios, rot, GAMMAS)
        got = pipe(x, flip=None if flip == "none" else [True] * 3, states=states)
        assert got.shape[:2] == (3, 1) and got.dtype == torch.float32
        hold(got[:, 0], win, states, POOLS[pool], f"inpipe {shape} {pool} flip={flip} end={end} rot={rot}")


@pytest.mark.parametrize("end", [0, 1])
@pytest.mark.parametrize("flip_axis", [None, 2, -1])
@pytest.mark.parametrize("sf", [None, (0.5, 0.5)])
def test_pipeline_parity_2d(dev, sf, flip_axis, end):
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = SHAPE2
    stored, win, ratios = make_case(in_shape, out, flip_axis, end)
    x = dev_vol(stored, dev)
    pipe = PTBatchPipeline(out, MEAN, STD, flip_axis=flip_axis, scale_factor=sf)
    for rot in ROTS:
        states = states_of(ratios, rot, GAMMAS)
        got = pipe(x, flip=None if flip_axis is None else [True] * 3, states=states)
        assert got.ndim == 4 and got.shape[:2] == (3, 1)
        hold(got[:, 0], win, states, sf, f"inpipe 2d sf={sf} flip={flip_axis} end={end} rot={rot}")


def test_pipeline_centre_crop_and_partial_flips(dev):
    """validation settings (centre crop with an odd difference, nothing random) and a batch in which only some knees are RIGHT"""
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = (11, 14, 9), (8, 10, 6)            # differences 3, 4, 3
    rng = np.random.default_rng(4200)
    stored = rng.integers(5, 311, size=(3,) + in_shape).astype(np.uint16)
    flips = [True, False, True]
    wins = []
    for b in range(3):
        img = stored[b][None]
        img = np.flip(img, axis=-1) if flips[b] else img
        wins.append(img[:, 1:9, 2:12, 1:7][0])
    win = np.stack(wins).astype(np.int64)
    pipe = PTBatchPipeline(out, MEAN, STD, flip_axis=-1, random_crop=False, rotate_prob=0.0, gamma_prob=0.0, scale_factor=(0.5, 0.5, 0.5))
    s0 = random.getstate()
    got = pipe(dev_vol(stored, dev), flip=flips)
    assert random.getstate() == s0                      # validation draws nothing
    hold(got[:, 0], win, [(None, 1.0, 0.0, 1.0, 1.0)] * 3, (0.5, 0.5, 0.5), "inpipe centre crop")


def test_validation_table_is_reused_with_new_addresses(dev):
    """with nothing random the checked host table is kept per (stored shapes, flip pattern) and only the addresses change: a
    second batch of the same shapes in other memory, another flip pattern, and a ragged list must each give their own result"""
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = (11, 14, 9), (8, 10, 6)
    pipe = PTBatchPipeline(out, MEAN, STD, flip_axis=2, random_crop=False, rotate_prob=0.0, gamma_prob=0.0, scale_factor=(0.5, 0.5, 1.0))
    rng = np.random.default_rng(4250)
    keep = []
    for k, flips in enumerate(([True, False, True], [True, False, True], [False, False, True], None)):
        stored = rng.integers(5, 311, size=(3,) + in_shape).astype(np.uint16)
        fl = flips or [False] * 3
        win = np.stack([(np.flip(stored[b], axis=1) if fl[b] else stored[b])[1:9, 2:12, 1:7] for b in range(3)]).astype(np.int64)
        x = dev_vol(stored, dev)
        keep.append(x)                                  # (earlier batches stay allocated: the new one lies elsewhere)
        hold(pipe(x, flip=flips)[:, 0], win, [(None, 1.0, 0.0, 1.0, 1.0)] * 3, (0.5, 0.5, 1.0), f"inpipe reuse {k}")
        ragged = list(x.unbind(0))
        assert torch.equal(pipe(ragged, flip=flips).cpu(), pipe(x, flip=flips).cpu())
    assert len(pipe._tables) == 6                       # three flip patterns, dense and as a list
    with pytest.raises(ValueError, match="Invalid crop size"):
        pipe(torch.zeros(3, 1, 11, 9, 9, dtype=torch.uint16).to(dev))


def test_pipeline_large_window(dev):
    """2 x 96 x 96 x 114 voxels (S % 4 != 0: one slice per thread): 4104 blocks per sample, two samples side by side in the grid,
    flat indices past 2^20.  Not rotated: at 96 x 96 the fp32 sample coordinates of a rotation cost torch's own fp32 op 9e-5 on
    such data, which is the parity tests' subject at sizes where the bar holds"""
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = (99, 97, 117), (96, 96, 114)
    stored, win, ratios = make_case(in_shape, out, -1, 1, "uint8", hi=250, B=2)
    pipe = PTBatchPipeline(out, MEAN, STD, flip_axis=-1)
    states = states_of(ratios, None, [(0.0, 0.5), (1.0, 1.0)])
    got = pipe(dev_vol(stored, dev), flip=[True, True], states=states)
    hold(got[:, 0], win, states, None, "inpipe large window")


def test_constant_window_is_nan_like_the_reference(dev):
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    x = torch.full((1, 1, 11, 13, 9), 60000, dtype=torch.uint16)
    x[:, :, 1:9, 1:11, 1:7] = 77
    pipe = PTBatchPipeline((8, 10, 6), MEAN, STD, random_crop=False, rotate_prob=0.0, gamma_prob=0.0)
    assert torch.isnan(pipe(x.to(dev))).all()           # 0 / 0, as PTToUnitRange


# =================================================================================================
# bit-for-bit invariants
# =================================================================================================
@pytest.mark.parametrize("shape", ["s6", "s8"])
def test_stored_dtype_does_not_change_a_bit(dev, shape):
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = SHAPES3[shape]
    pipe = PTBatchPipeline(out, MEAN, STD, flip_axis=-1, scale_factor=(0.5, 0.5, 0.5))
    outs = {}
    for dtype in ("uint8", "uint16", "int16", "float32"):
        stored, win, ratios = make_case(in_shape, out, -1, 1, dtype, hi=250)      # same seed: the same window in every type
        states = states_of(ratios, 7.0, GAMMAS)
        outs[dtype] = pipe(dev_vol(stored, dev), flip=[True] * 3, states=states).cpu()
    hold(outs["uint8"][:, 0], win, states, (0.5, 0.5, 0.5), f"inpipe dtypes {shape}")
    for dtype in ("uint16", "int16", "float32"):
        assert torch.equal(outs[dtype], outs["uint8"]), f"{dtype} volumes give other bits than uint8 volumes of the same values"
    # negative values: int16 against fp32
    neg = {}
    for dtype in ("int16", "float32"):
        stored, win, ratios = make_case(in_shape, out, 2, 0, dtype, seed=1, lo=-300, hi=310)
        states = states_of(ratios, 45.0, GAMMAS)
        neg[dtype] = PTBatchPipeline(out, MEAN, STD, flip_axis=2, scale_factor=(0.5, 0.5, 0.5))(dev_vol(stored, dev), flip=[True] * 3, states=states)
        assert torch.isfinite(neg[dtype]).all()
    assert torch.equal(neg["int16"].cpu(), neg["float32"].cpu())


@pytest.mark.parametrize("pool", ["p111", "p221", "p222"])
@pytest.mark.parametrize("shape", ["s6", "s8"])
def test_ncdhw_is_the_permuted_rcs(dev, shape, pool):
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = SHAPES3[shape]
    stored, win, ratios = make_case(in_shape, out, 2, 1)
    x = dev_vol(stored, dev)
    states = states_of(ratios, 7.0, GAMMAS)
    a = PTBatchPipeline(out, MEAN, STD, flip_axis=2, scale_factor=POOLS[pool])(x, flip=[True] * 3, states=states)
    b = PTBatchPipeline(out, MEAN, STD, flip_axis=2, scale_factor=POOLS[pool], layout="ncdhw")(x, flip=[True] * 3, states=states)
    assert b.shape == (3, 1, a.shape[4], a.shape[2], a.shape[3])
    assert torch.equal(b.cpu(), a.permute(0, 1, 4, 2, 3).contiguous().cpu())


@pytest.mark.parametrize("flip_axis", [None, -1])
@pytest.mark.parametrize("pool,pool_s", [(1, 1), (2, 1), (2, 2)])
def test_four_slice_path_equals_each_slice_pair(dev, pool, pool_s, flip_axis):
    """S % 4 == 0 takes the four-slices-per-thread instantiation with its vector loads; its output must be, bit for bit, that of
    every slice pair run on its own as a two-slice window (the one- / two-slice instantiations) with the whole window's range"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.preproc import crop_geometry
    in_shape, out = SHAPES3["s8"]
    stored, win, ratios = make_case(in_shape, out, flip_axis, 1)
    vols = list(dev_vol(stored, dev).unbind(0))
    org, back = crop_geometry(in_shape, out, ratios, flip_axis)
    table, code, w3 = ops.window_table(vols, [org] * 3, [back] * 3, out)
    mm = ops.window_minmax(table, code, w3)
    prm = prm_of(states_of(ratios, 7.0, GAMMAS)).to(dev)
    full = ops.input_pipeline(table, code, w3, mm, prm, MEAN, STD, pool, pool_s).cpu()
    for k in range(4):
        o2 = (org[0], org[1], org[2] + (-2 * k if back & 4 else 2 * k))
        t2, _, w2 = ops.window_table(vols, [o2] * 3, [back] * 3, (out[0], out[1], 2))
        pair = ops.input_pipeline(t2, code, w2, mm, prm, MEAN, STD, pool, pool_s).cpu()
        n = 2 // pool_s
        assert torch.equal(pair, full[..., n * k:n * (k + 1)]), f"slices {2 * k}, {2 * k + 1} differ from their own two-slice run"


def test_ragged_list_equals_each_sample_alone(dev):
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    out = (8, 10, 6)
    shapes = [(11, 13, 9), (9, 10, 7), (14, 12, 11)]
    cases = [make_case(s, out, -1, 1, "uint8", seed=10 + i, hi=250, B=1) for i, s in enumerate(shapes)]
    pipe = PTBatchPipeline(out, MEAN, STD, flip_axis=-1, scale_factor=(0.5, 0.5, 0.5))
    states = states_of(cases[0][2], 7.0, GAMMAS)
    flips = [True, True, True]
    ragged = [torch.from_numpy(np.array(c[0])).to(dev) for c in cases]             # each (1, R0, C0, S0)
    got = pipe(ragged, flip=flips, states=states)
    assert got.shape == (3, 1, 4, 5, 3)
    for b in range(3):
        alone = pipe(ragged[b].unsqueeze(0), flip=[flips[b]], states=[states[b]])
        assert torch.equal(alone[0].cpu(), got[b].cpu()), f"sample {b} of the ragged list differs from its own dense run"
    hold(got[:, 0], np.concatenate([c[1] for c in cases]), states, (0.5, 0.5, 0.5), "inpipe ragged")


# =================================================================================================
# the unfused fallback, the prefetcher
# =================================================================================================
@pytest.mark.parametrize("sf", [(0.5, 0.5, 0.5), (0.75, 0.75, 0.75)])
@pytest.mark.parametrize("layout", ["rcs", "ncdhw"])
def test_unfused_fallback(dev, sf, layout):
    """an odd crop size, or a factor that is not 0.5: the fused pass unpooled, then koaf_resize.  The unpooled pass is held to the
    pipeline's own bar; the resize on top of it to test_resize_edges's: 2e-6 of the largest magnitude against float64 F.interpolate
    of the very tensor it resized"""
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    in_shape, out = (11, 13, 9), (9, 10, 6)
    stored, win, ratios = make_case(in_shape, out, -1, 1)
    x = dev_vol(stored, dev)
    states = states_of(ratios, 7.0, [(1.0, 1.0), (0.0, 0.5), (0.0, 0.5)])
    unpooled = PTBatchPipeline(out, MEAN, STD, flip_axis=-1)(x, flip=[True] * 3, states=states)
    hold(unpooled[:, 0], win, states, None, "inpipe unpooled (9, 10, 6)")
    got = PTBatchPipeline(out, MEAN, STD, flip_axis=-1, scale_factor=sf, layout=layout)(x, flip=[True] * 3, states=states).cpu()
    ref = F.interpolate(unpooled.cpu().double(), scale_factor=sf, recompute_scale_factor=True, align_corners=False, mode="trilinear")
    assert ref.shape == (3, 1) + tuple(int(math.floor(n * s)) for n, s in zip(out, sf))
    if layout == "ncdhw":
        ref = ref.permute(0, 1, 4, 2, 3)
    assert got.shape == ref.shape
    bar = 2e-6 * float(ref.abs().max())
    e = float((got.double() - ref).abs().max())
    print(f"FALLBACK sf={sf} {layout}: {e:.3e} bar {bar:.3e}")
    assert e < bar, f"fallback sf={sf}: off the float64 op by {e:.3e} (bar {bar:.3e})"


def test_prefetcher_uploads_ragged_lists(dev):
    from oaprogressionmmf_amd.preproc import PinnedPrefetcher
    g = torch.Generator().manual_seed(4300)
    batches = []
    for i in range(3):
        vols = [torch.randint(0, 256, (1, 9 + b + i, 10, 7 + b), generator=g, dtype=torch.uint8) for b in range(3)]
        batches.append({"image": vols, "pair": (vols[0].float(), vols[1].float()), "target": torch.arange(3) + i, "ids": ["a", "b", "c"],
                        "n": 3, "empty": []})
    n = 0
    for cur, src in zip(PinnedPrefetcher(batches, dev), batches):
        assert isinstance(cur["image"], list) and isinstance(cur["pair"], tuple) and len(cur["image"]) == 3
        for t, s in zip(list(cur["image"]) + list(cur["pair"]) + [cur["target"]], list(src["image"]) + list(src["pair"]) + [src["target"]]):
            assert t.is_cuda and t.dtype == s.dtype and torch.equal(t.cpu(), s)
        assert cur["ids"] is src["ids"] and cur["n"] == 3 and cur["empty"] == []
        n += 1
    assert n == 3


# =================================================================================================
# fixture F13: the reference's own transform objects
# =================================================================================================
@pytest.mark.parametrize("group", ["mr", "cc", "xr"])
def test_pipeline_vs_reference_objects_f13(dev, group):
    """tests/golden/inpipe_f13.npz (make_golden_inpipe.py): after the same seed PTBatchPipeline.draw reproduces every state the
    reference's transforms recorded, and the pipeline's output is held to the yardstick rule between the float64 restatement
    and the reference's own float32 output"""
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    z = np.load(GOLDEN / "inpipe_f13.npz")
    vol, flips, rec = z[group + ":vol"], [bool(f) for f in z[group + ":flip"]], z[group + ":states"]
    mean, std = (float(v) for v in z[group + ":norm"])
    nd = vol.ndim - 1
    kw = {"mr": dict(crop_size=(24, 20, 6), flip_axis=-1, scale_factor=(0.5, 0.5, 0.5)),
          "cc": dict(crop_size=(24, 20, 6), flip_axis=-1, scale_factor=(0.5, 0.5, 1.0), random_crop=False, rotate_prob=0.0, gamma_prob=0.0),
          "xr": dict(crop_size=(24, 20), flip_axis=2, scale_factor=(0.5, 0.5))}[group]
    pipe = PTBatchPipeline(mean=mean, std=std, **kw)
    states = []
    for seed in range(len(vol)):
        random.seed(seed)
        (st,) = pipe.draw(1)
        if group == "cc":
            assert st == (None, 1.0, 0.0, 1.0, 1.0)
        else:
            assert list(st[0]) + list(st[1:]) == list(rec[seed]), (seed, st, rec[seed])
        states.append(st)
    got = pipe(torch.from_numpy(vol).unsqueeze(1).to(dev), flip=flips, states=states).cpu()
    ref, ref32 = torch.from_numpy(z[group + ":out64"]), torch.from_numpy(z[group + ":out32"])
    assert got.shape == ref.shape and nd in (2, 3)
    yardstick(got, ref, ref32, f"inpipe F13 {group}", floor=2e-5)
