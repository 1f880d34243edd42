#!/usr/bin/env python3
"""Generate fixture F13 of the input pipeline (tests/golden/inpipe_f13.npz): the reference's OWN transform objects, run the
way its dataset runs them (datasets/oai/_dataset.py:298-321: np.flip of RIGHT knees, then per transform `randomize()` and the
call) and followed by the step's PTInterpolate (run/train_prog_fus.py:111-116), on stored uint8 volumes.

The reference's preproc/_np_nd.py, _various.py and _pt.py are loaded by path (its package __init__ pulls in what is not
installed here).  Only arrays are stored.  Three groups, transforms constructed once, `random.seed(seed)` before each sample:
  mr  seeds 0..11, stored (29, 26, 9): [np.flip(axis=-1) for odd seeds, RandomCrop([24, 20, 6]), NumpyToTensor, PTToUnitRange,
      PTRotate3DInSlice(+-15 degrees, 0.5), PTGammaCorrection(), PTNormalize(0.257, 0.235)], PTInterpolate((0.5, 0.5, 0.5))
  cc  two samples (the second flipped), stored (29, 26, 9): [np.flip, CenterCrop([24, 20, 6]), NumpyToTensor, PTToUnitRange,
      PTNormalize(0.257, 0.235)], PTInterpolate((0.5, 0.5, 1.0)) -- validation: nothing random
  xr  seeds 0..3, stored (29, 26): [np.flip(axis=2) for odd seeds, RandomCrop([24, 20]), NumpyToTensor, PTToUnitRange,
      PTRotate2D(+-15 degrees, 0.5), PTGammaCorrection(), PTNormalize(0.543, 0.296)], PTInterpolate((0.5, 0.5))
Per group <g>: <g>:vol the stored volumes, <g>:flip, <g>:states float64 rows (crop ratios..., p_rot, theta, p_gamma, gamma) as the
transforms' .state held them after the sample (theta: the float32 value the reference drew), <g>:out32 the reference's float32
output, <g>:out64 the float64 restatement np.flip -> crop slice -> tests/elem_refs.augment_ref -> float64 F.interpolate,
<g>:norm (mean, std).  Asserted here: the two outputs agree within 2e-5, PTBatchPipeline.draw reproduces the recorded states
after the same seed, and all four rotate / gamma combinations occur among the mr seeds.

Usage:  python tests/golden/make_golden_inpipe.py /path/to/reference
"""
import importlib.util
import math
import random
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
import elem_refs as ER  # noqa: E402

SEED = 1313


def load_reference(root):
    mods = {}
    for name in ("_np_nd", "_various", "_pt"):
        spec = importlib.util.spec_from_file_location("ref_preproc" + name, Path(root) / "koafusion" / "preproc" / (name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods["_np_nd"], mods["_various"], mods["_pt"]


def run_group(vols, flips, seeds, flip_axis, transforms, interp, crop, mean, std, sf):
    """-> states [n, nd + 4], out32, out64"""
    nd = len(crop)
    states, out32, out64 = [], [], []
    for vol, fl, seed in zip(vols, flips, seeds):
        if seed is not None:
            random.seed(seed)
        img = vol[None]                                           # (ch, d0, ...)
        if fl:
            img = np.flip(img, axis=flip_axis)
        x = img
        for fn in transforms:                                     # _dataset.py:316-321
            if hasattr(fn, "randomize"):
                fn.randomize()
            x = fn(x)
        out32.append(interp(x[None])[0].numpy())
        st = {}
        for fn in transforms:
            for k, v in getattr(fn, "state", {}).items():
                st[type(fn).__name__ + ":" + k] = float(v)
        rot = [k for k in st if k.startswith("PTRotate")]
        ratios = [st[f"RandomCrop:ratio_d{i}"] for i in range(nd)] if "RandomCrop:ratio_d0" in st else None
        p_rot, theta = (st[[k for k in rot if k.endswith(":p")][0]], st[[k for k in rot if k.endswith(":theta")][0]]) if rot else (1.0, 0.0)
        p_gam, gamma = (st["PTGammaCorrection:p"], st["PTGammaCorrection:gamma"]) if "PTGammaCorrection:p" in st else (1.0, 1.0)
        states.append((ratios if ratios is not None else [0.0] * nd) + [p_rot, theta, p_gam, gamma])
        # the float64 restatement
        start = [math.floor(ratios[i] * (img.shape[1 + i] - crop[i])) if ratios is not None else (img.shape[1 + i] - crop[i]) // 2
                 for i in range(nd)]
        win = np.ascontiguousarray(img[(slice(None),) + tuple(slice(s, s + o) for s, o in zip(start, crop))])[0]
        raw = torch.from_numpy(win.astype(np.float32)).reshape((1,) + tuple(crop) + (1,) * (3 - nd))
        is_rot, is_gam = p_rot < 0.5, p_gam < 0.5
        prm = torch.tensor([[math.cos(theta) if is_rot else 1.0, math.sin(theta) if is_rot else 0.0,
                             (1.0 / gamma) if is_gam else 0.0, 1.0 if is_rot else 0.0]], dtype=torch.float32)
        a64 = ER.augment_ref(raw, prm, mean, std).reshape((1, 1) + tuple(crop))
        mode = {2: "bilinear", 3: "trilinear"}[nd]
        out64.append(F.interpolate(a64, scale_factor=sf, recompute_scale_factor=True, align_corners=False, mode=mode)[0].numpy())
    return np.asarray(states, dtype=np.float64), np.stack(out32), np.stack(out64)


def main(root):
    NP, VA, PT = load_reference(root)
    from oaprogressionmmf_amd.preproc import PTBatchPipeline
    rng = np.random.default_rng(SEED)
    out = {}

    def finish(tag, vols, flips, res, mean, std):
        states, o32, o64 = res
        err = float(np.abs(o32.astype(np.float64) - o64).max())
        print(f"  {tag}: {len(vols)} samples, worst |fp32 - fp64| = {err:.2e}")
        assert err < 2e-5, (tag, err)
        out.update({tag + ":vol": vols, tag + ":flip": np.asarray(flips), tag + ":states": states, tag + ":out32": o32,
                    tag + ":out64": o64, tag + ":norm": np.array([mean, std])})
        return states

    # mr: the train pipeline of a DESS-like volume
    vols = rng.integers(5, 251, size=(12, 29, 26, 9), dtype=np.uint8)
    flips = [s % 2 == 1 for s in range(12)]
    tf = [NP.RandomCrop([24, 20, 6], ndim=3), VA.NumpyToTensor(), PT.PTToUnitRange(), PT.PTRotate3DInSlice(degree_range=[-15., 15.], prob=0.5),
          PT.PTGammaCorrection(gamma_range=(0.5, 2.0), prob=0.5, clip_to_unit=False), PT.PTNormalize(mean=[0.257, ], std=[0.235, ])]
    st = finish("mr", vols, flips, run_group(vols, flips, range(12), -1, tf, PT.PTInterpolate((0.5, 0.5, 0.5)), (24, 20, 6), 0.257,
                                            0.235, (0.5, 0.5, 0.5)), 0.257, 0.235)
    assert {(bool(s[3] < 0.5), bool(s[5] < 0.5)) for s in st} == {(False, False), (False, True), (True, False), (True, True)}
    pipe = PTBatchPipeline((24, 20, 6), 0.257, 0.235, flip_axis=-1, scale_factor=(0.5, 0.5, 0.5))
    for seed in range(12):
        random.seed(seed)
        (ratios, *rest), = pipe.draw(1)
        assert list(ratios) + rest == list(st[seed]), (seed, ratios, rest, st[seed])

    # cc: validation, centre crop, in-plane pool only
    vols = rng.integers(5, 251, size=(2, 29, 26, 9), dtype=np.uint8)
    tf = [NP.CenterCrop([24, 20, 6], ndim=3), VA.NumpyToTensor(), PT.PTToUnitRange(), PT.PTNormalize(mean=[0.257, ], std=[0.235, ])]
    finish("cc", vols, [False, True], run_group(vols, [False, True], [None, None], -1, tf, PT.PTInterpolate((0.5, 0.5, 1.0)),
                                                 (24, 20, 6), 0.257, 0.235, (0.5, 0.5, 1.0)), 0.257, 0.235)

    # xr: the train pipeline of a radiograph
    vols = rng.integers(5, 251, size=(4, 29, 26), dtype=np.uint8)
    flips = [s % 2 == 1 for s in range(4)]
    tf = [NP.RandomCrop([24, 20], ndim=2), VA.NumpyToTensor(), PT.PTToUnitRange(), PT.PTRotate2D(degree_range=[-15., 15.], prob=0.5),
          PT.PTGammaCorrection(gamma_range=(0.5, 2.0), prob=0.5, clip_to_unit=False), PT.PTNormalize(mean=[0.543, ], std=[0.296, ])]
    st = finish("xr", vols, flips, run_group(vols, flips, range(4), 2, tf, PT.PTInterpolate((0.5, 0.5)), (24, 20), 0.543, 0.296,
                                            (0.5, 0.5)), 0.543, 0.296)
    pipe = PTBatchPipeline((24, 20), 0.543, 0.296, flip_axis=2, scale_factor=(0.5, 0.5))
    for seed in range(4):
        random.seed(seed)
        (ratios, *rest), = pipe.draw(1)
        assert list(ratios) + rest == list(st[seed]), (seed, ratios, rest, st[seed])

    np.savez_compressed(HERE / "inpipe_f13.npz", **out)
    print(f"  wrote inpipe_f13.npz ({(HERE / 'inpipe_f13.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
