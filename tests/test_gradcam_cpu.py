"""CPU: the host side of the Grad-CAM interface.  run.cam_strides against numpy restatements of the five slice folds of
models/_common.fold_slices (a labelled slice batch scattered through the strides gives back the input tensor, every element
written once); argument validation of run.gradcam / explain_epoch(explain_fn="gradcam") before anything touches a device; the two
entry points declared in koaf.h with the documented prototypes, built into the library, at the unchanged ABI version."""
import ctypes

import numpy as np
import pytest
import torch

# view -> (input shape for B = 2, fold: array -> slice images [B*K, H, W]); fold_slices' definitions restated
B, R, C, S = 2, 4, 5, 3
FOLDS = {
    None: ((B, 1, R, C), lambda x: x.reshape(B, R, C)),
    "rc": ((B, 1, R, C, S), lambda x: x.transpose(0, 4, 1, 2, 3).reshape(B * S, R, C)),          # "b ch r c s -> (b s) ch r c"
    "src": ((B, 1, S, R, C), lambda x: x.reshape(B * S, R, C)),
    "cs": ((B, 1, R, C, S), lambda x: x.reshape(B * R, C, S)),
    "rs": ((B, 1, R, C, S), lambda x: x.reshape(B, R, C, S).transpose(0, 2, 1, 3).reshape(B * C, R, S)),
}


@pytest.mark.parametrize("view", list(FOLDS), ids=str)
def test_cam_strides_invert_the_slice_folds(view):
    from oaprogressionmmf_amd.models._common import fold_slices
    from oaprogressionmmf_amd.run import cam_strides
    shape, fold = FOLDS[view]
    x = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 1.0
    imgs = fold(x)
    if view in ("src", "cs", "rs"):               # (these folds are views / copies in torch: the definition itself runs here)
        assert np.array_equal(fold_slices(torch.from_numpy(x), view).numpy()[:, 0], imgs)
    K, sb, sk, si, sj = cam_strides(view, shape)
    N, H, W = imgs.shape
    assert N == B * K and sb == K * H * W == x.size // B
    out, hits = np.zeros(x.size, dtype=np.float32), np.zeros(x.size, dtype=np.int64)
    b, k, i, j = np.meshgrid(np.arange(B), np.arange(K), np.arange(H), np.arange(W), indexing="ij")
    off = b * sb + k * sk + i * si + j * sj
    np.add.at(hits, off.reshape(-1), 1)
    out[off.reshape(-1)] = imgs.reshape(-1)
    assert (hits == 1).all(), "every element of the input is reached exactly once"
    assert np.array_equal(out.reshape(shape), x)
    assert 1 in ((sj,) if view is None else (sk, sj)), "one of the axes the kernel walks has unit stride"


def test_cam_strides_table():
    from oaprogressionmmf_amd.run import cam_strides
    assert cam_strides(None, (7, 1, 350, 310))[3:] == (310, 1)
    assert cam_strides("rc", (8, 1, 384, 380, 160)) == (160, 384 * 380 * 160, 1, 380 * 160, 160)
    assert cam_strides("src", (8, 1, 160, 384, 380)) == (160, 384 * 380 * 160, 384 * 380, 380, 1)
    assert cam_strides("cs", (8, 1, 384, 380, 160)) == (384, 384 * 380 * 160, 380 * 160, 160, 1)
    assert cam_strides("rs", (8, 1, 384, 380, 160)) == (380, 384 * 380 * 160, 160, 380 * 160, 1)
    with pytest.raises(ValueError):
        cam_strides("sr", (2, 1, 4, 5, 3))
    with pytest.raises(ValueError):
        cam_strides("rc", (2, 1, 4, 5))
    with pytest.raises(ValueError):
        cam_strides(None, (2, 3, 4, 5))


def test_gradcam_argument_validation():
    from oaprogressionmmf_amd.run import explain_epoch, gradcam
    with pytest.raises(ValueError, match="Unknown normalize: max"):
        gradcam(None, (), 0, normalize="max")
    with pytest.raises(ValueError, match="no encoder trunk"):
        gradcam(torch.nn.Linear(2, 2), (torch.zeros(1, 2),), 0)
    with pytest.raises(TypeError):
        gradcam(None, (), 0, False)                # relu / normalize / upsample are keyword-only
    assert explain_epoch(None, [], ("xr_pa",), explain_fn="gradcam") == {}
    with pytest.raises(ValueError, match="Unknown explain_fn: grad_cam"):
        explain_epoch(None, [], ("xr_pa",), explain_fn="grad_cam")


def test_gradcam_refuses_a_trunk_it_cannot_map_to_an_input():
    """every KoafTrunk of the model gets a hook or the call is refused: a trunk that is not a `_fe` / `_fe{i}` child (nested, or
    named otherwise) has no input to return a map for, and leaving it out would leave its graph uncut"""
    from oaprogressionmmf_amd.models import KoafTrunk
    from oaprogressionmmf_amd.run import _gradcam, gradcam

    class Model(torch.nn.Module):
        def __init__(self, **children):
            super().__init__()
            for name, mod in children.items():
                setattr(self, name, mod)
    a, b = KoafTrunk(), KoafTrunk()
    assert _gradcam._trunks(Model(_fe=a)) == {0: a}
    assert _gradcam._trunks(Model(_fe0=a, _fe2=b, _fe1=torch.nn.Identity())) == {0: a, 2: b}
    x = (torch.zeros(1, 1, 32, 32),)
    with pytest.raises(ValueError, match="trunk `encoder` is not"):
        gradcam(Model(_fe0=a, encoder=b), x, 0)
    with pytest.raises(ValueError, match="trunk `_fe1.body` is not"):
        gradcam(Model(_fe0=a, _fe1=Model(body=b)), x, 0)
    with pytest.raises(ValueError, match="one trunk serves several inputs"):
        gradcam(Model(_fe0=a, _fe1=a), x + x, 0)


def test_gradcam_trunk_stash_is_off_by_default():
    from oaprogressionmmf_amd.models import KoafTrunk
    assert KoafTrunk.keep_features is False and KoafTrunk.features is None


def test_cam_entry_points_are_declared_and_built():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    P, I, L = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # koaf_cam(A, w, cam, img_sum, img_max, N, HW, C, relu, act16, stream)
    assert protos["koaf_cam"] == (ctypes.c_int, [P, P, P, P, P, I, I, I, I, I, P])
    # koaf_cam_upsample(cam, img_max, out, B, K, h, w, H, W, sb, sk, si, sj, normalize, stream)
    assert protos["koaf_cam_upsample"] == (ctypes.c_int, [P, P, P, I, I, I, I, I, I, L, L, L, L, I, P])
    assert _lib.defines()["KOAF_VERSION"] == 200
    handle = _lib.lib()                            # (binds every declared symbol: a library without the two fails here)
    assert handle.koaf_cam.argtypes == protos["koaf_cam"][1]
    mk = (_lib.LIB_PATH.parent / "Makefile").read_text()
    rest = [ln for ln in mk.splitlines() if ln.startswith("REST_SRCS")]
    assert len(rest) == 1 and "koaf_cam.hip" in rest[0].split()
