"""Host side of the stored-volume input pipeline (preproc.crop_geometry, preproc.PTBatchPipeline.draw, the header and build):
 * crop_geometry against numpy: an index volume is flipped and cropped with the reference's own formulas (np.flip, then
   floor(ratio * (in - out)) of preproc/_np_nd.py:91 or (in - out) // 2 of :133) and must equal the gather that the returned
   (origin, backwards mask) describe -- the walk the kernels make through the table;
 * the order of the draws from Python's `random`: crop ratios, rotation (p, theta), gamma (p, gamma); absent transforms draw
   nothing.  theta is drawn as the reference's transforms draw it: between float32 bounds, in float32 (preproc/_pt.py:259, :307);
 * koaf.h declares the two kernels, the library exports them, KOAF_VERSION is still 200, the Makefile builds koaf_inpipe.hip."""
import ctypes
import math
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _reference_crop(vol, out, ratios, flip_axis):
    """the reference's chain on a (ch, d0, ...) array: np.flip -> RandomCrop (ratios) | CenterCrop (None)"""
    img = vol if flip_axis is None else np.flip(vol, axis=flip_axis)
    ds_in = img.shape[1:]
    if ratios is None:
        start = [(ds_in[i] - out[i]) // 2 for i in range(len(out))]
    else:
        start = [math.floor(ratios[i] * (ds_in[i] - out[i])) for i in range(len(out))]
    sel = (slice(None),) + tuple(slice(s, s + o) for s, o in zip(start, out))
    return np.ascontiguousarray(img[sel])


def _gather(vol, out, origin, back):
    """window voxel i along an axis is stored index origin + i, or origin - i on a backwards axis"""
    idx = [origin[a] + (-1 if back >> a & 1 else 1) * np.arange(out[a]) for a in range(len(out))]
    return vol[(slice(None),) + np.ix_(*idx)]


@pytest.mark.parametrize("in_shape,out", [((11, 13, 9), (8, 10, 6)), ((13, 11), (10, 8)), ((11, 10, 9), (8, 10, 6))])
@pytest.mark.parametrize("flip_axis", [None, 2, -1])
def test_crop_geometry_against_numpy(in_shape, out, flip_axis):
    from oaprogressionmmf_amd.preproc import crop_geometry
    nd = len(in_shape)
    vol = np.arange(int(np.prod(in_shape)), dtype=np.int64).reshape((1,) + in_shape)
    rs = [None, (0.0,) * nd, (0.999999,) * nd, (0.999999, 0.0, 0.5)[:nd], (0.31, 0.77, 0.5)[:nd]]    # None: the centre crop (odd differences)
    for ratios in rs:
        origin, back = crop_geometry(in_shape, out, ratios, flip_axis)
        assert len(origin) == nd
        want_back = 0 if flip_axis is None else 1 << ((flip_axis - 1) if flip_axis >= 0 else nd + flip_axis)
        assert back == want_back
        got, ref = _gather(vol, out, origin, back), _reference_crop(vol, out, ratios, flip_axis)
        assert np.array_equal(got, ref), (in_shape, out, ratios, flip_axis, origin, back)


def test_batch_geometry_is_crop_geometry_per_sample():
    """PTBatchPipeline.geometry, the numpy form the transform uses for a whole (ragged) batch, against crop_geometry sample by
    sample: random and centre crops, some knees flipped"""
    from oaprogressionmmf_amd.preproc import PTBatchPipeline, crop_geometry
    rng = random.Random(3)
    for out, flip_axis in (((8, 10, 6), -1), ((8, 10, 6), 2), ((10, 8), 2), ((10, 8), -1)):
        nd = len(out)
        shapes = [tuple(o + rng.randrange(0, 9) for o in out) for _ in range(7)]
        ratios = [tuple(rng.choice([0.0, 0.999999, rng.random()]) for _ in range(nd)) for _ in shapes]
        flips = [rng.random() < 0.5 for _ in shapes]
        for random_crop in (True, False):
            pipe = PTBatchPipeline(out, 0.5, 0.2, flip_axis=flip_axis, random_crop=random_crop)
            org, back = pipe.geometry(shapes, ratios, flips)
            for b, sp in enumerate(shapes):
                want = crop_geometry(sp, out, ratios[b] if random_crop else None, flip_axis if flips[b] else None)
                assert (tuple(int(v) for v in org[b]), int(back[b])) == want, (sp, out, ratios[b], flips[b])
            org, back = pipe.geometry(shapes, ratios, None)
            assert not back.any() and (org >= 0).all()
    with pytest.raises(ValueError, match=r"Invalid crop size \(8, 10, 6\) for input \(11, 9, 9\)"):
        PTBatchPipeline((8, 10, 6), 0.5, 0.2).geometry([(11, 13, 9), (11, 9, 9)], [(0.5,) * 3] * 2)


def test_crop_geometry_refuses_like_the_reference():
    from oaprogressionmmf_amd.preproc import crop_geometry
    with pytest.raises(ValueError, match=r"Invalid crop size \(8, 10, 6\) for input \(11, 9, 9\)"):
        crop_geometry((11, 9, 9), (8, 10, 6), None, None)
    with pytest.raises(ValueError, match="Invalid crop size"):
        crop_geometry((9, 9), 10, (0.5, 0.5), -1)
    with pytest.raises(ValueError, match="not a spatial axis"):
        crop_geometry((9, 9), 8, None, 0)                       # (axis 0 of the reference's array is the channel)
    assert crop_geometry((9, 12), 8, None, None) == ((0, 2), 0)     # an int crop size is every axis


def _theta(u):
    """random.uniform(*torch.deg2rad(torch.Tensor([-15, 15]))) as the reference's randomize() evaluates it: float32 throughout"""
    lo, hi = (np.float32(v) for v in torch.deg2rad(torch.Tensor([-15., 15.])).tolist())
    return float(lo + (hi - lo) * np.float32(u))


def test_draw_order_and_absent_transforms():
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    full = PTBatchPipeline((8, 10, 6), mean=0.257, std=0.235, flip_axis=-1)
    for k in (0, 7):
        random.seed(k)
        got = full.draw(3)
        random.seed(k)
        want = []
        for _ in range(3):
            ratios = (random.random(), random.random(), random.random())
            p1 = random.random(); th = _theta(random.random()); p2 = random.random(); g = random.uniform(0.5, 2.0)
            want.append((ratios, p1, th, p2, g))
        assert got == want
        assert all(abs(s[2]) <= math.radians(15.0) * (1 + 1e-6) for s in got)
    t2 = PTBatchPipeline((8, 10, 6), mean=0.259, std=0.345, gamma_prob=0.0)          # T2 maps: no gamma correction
    random.seed(7)
    a = t2.draw(2)
    random.seed(7)
    b = [((random.random(), random.random(), random.random()), random.random(), _theta(random.random()), 1.0, 1.0) for _ in range(2)]
    assert a == b
    xr = PTBatchPipeline((10, 8), mean=0.5, std=0.3, flip_axis=2, random_crop=False)    # two ratios fewer in the stream
    random.seed(7)
    a = xr.draw(2)
    random.seed(7)
    b = [(None, random.random(), _theta(random.random()), random.random(), random.uniform(0.5, 2.0)) for _ in range(2)]
    assert a == b
    random.seed(7)
    s0 = random.getstate()
    ev = PTBatchPipeline((8, 10, 6), mean=0., std=1., random_crop=False, rotate_prob=0.0, gamma_prob=0.0)   # validation / test
    assert ev.draw(4) == [(None, 1.0, 0.0, 1.0, 1.0)] * 4
    assert random.getstate() == s0
    with pytest.raises(NotImplementedError):
        PTBatchPipeline((8, 10, 6), mean=0., std=1., clip_to_unit=True)
    with pytest.raises(ValueError):
        PTBatchPipeline((8, 10, 6), mean=0., std=1., scale_factor=(0.5, 0.5))
    with pytest.raises(ValueError):
        PTBatchPipeline((8, 10, 6), mean=0., std=1., layout="nhwc")


def test_header_makefile_and_version():
    from oaprogressionmmf_amd import _lib, ops, preproc
    protos = _lib.parse_header()
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert protos["koaf_window_minmax_ws"] == (i64, [i64])
    assert protos["koaf_window_minmax"] == (ctypes.c_int, [vp, i32, i32, i32, i32, i32, vp, vp, vp])
    assert protos["koaf_input_pipeline"] == (ctypes.c_int, [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, vp])
    assert _lib.defines()["KOAF_VERSION"] == 200
    mk = (ROOT / "oaprogressionmmf_amd" / "csrc" / "Makefile").read_text()
    rest = re.findall(r"^REST_SRCS\s*=(.*)$", mk, flags=re.M)
    assert len(rest) == 1 and "koaf_inpipe.hip" in rest[0].split()
    handle = _lib.lib()
    assert handle.koaf_version() == 200
    for name in ("koaf_window_minmax_ws", "koaf_window_minmax", "koaf_input_pipeline"):
        assert getattr(handle, name).argtypes == protos[name][1]
    assert handle.koaf_window_minmax_ws(1) == 2 and handle.koaf_window_minmax_ws(4097) == 4
    assert handle.koaf_window_minmax_ws(320 * 320 * 128) == 512                    # capped at 256 blocks per sample
    for name in ("window_table", "window_minmax", "input_pipeline"):
        assert callable(getattr(ops, name))
    assert preproc.PTBatchPipeline is not None and preproc.crop_geometry is not None


def test_bad_arguments_are_refused_on_the_host():
    """every refusal comes from host code ahead of any launch: the pointers are host buffers no kernel ever sees"""
    from oaprogressionmmf_amd import _lib
    handle, d = _lib.lib(), _lib.defines()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def refused(rc):
        assert rc == d["KOAF_EINVAL"], rc

    refused(handle.koaf_window_minmax(None, 1, 1, 8, 8, 4, p, p, None))
    refused(handle.koaf_window_minmax(p, 4, 1, 8, 8, 4, p, p, None))               # dtype codes are 0 .. 3
    refused(handle.koaf_window_minmax(p, 1, 1, 0, 8, 4, p, p, None))
    refused(handle.koaf_window_minmax(p, 1, 1, 2048, 2048, 512, p, p, None))        # a window of 2^31 voxels
    refused(handle.koaf_input_pipeline(p, 1, p, p, p, 1, 8, 8, 4, 3, 1, 0, 0.5, 0.2, None))      # pool 3
    refused(handle.koaf_input_pipeline(p, 1, p, p, p, 1, 9, 8, 4, 2, 1, 0, 0.5, 0.2, None))      # odd R under pool 2
    refused(handle.koaf_input_pipeline(p, 1, p, p, p, 1, 8, 8, 5, 2, 2, 0, 0.5, 0.2, None))      # odd S under slice pool 2
    refused(handle.koaf_input_pipeline(p, 1, p, p, p, 1, 8, 8, 4, 2, 2, 2, 0.5, 0.2, None))      # layout 2
    refused(handle.koaf_input_pipeline(p, 1, None, p, p, 1, 8, 8, 4, 2, 2, 0, 0.5, 0.2, None))
