"""CPU: the host side of the attention relevance (run.attention_relevance, koaf_attnrel.hip).  The numpy twin (attn_twin.py) against
closed forms and against fixture F24's stored results; models/_common.token_layout for every registry class; the argument checks of
ops.attn_* and of the three entry points ahead of any launch; the entry points declared, built and exported at the unchanged ABI
version; explain_epoch's two new keys on a stub."""
import ctypes

import numpy as np
import pytest
import torch

import attn_twin as T
import procedural as P
from common import load


# ---- the twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", list(T.FUSE))
def test_twin_identity_attention_gives_the_identity(fuse):
    B, h, n, L = 2, 3, 5, 4
    A = np.broadcast_to(np.eye(n), (B, h, n, n))
    R = T.chain([T.rollout_layer(A, fuse) for _ in range(L)])
    assert np.array_equal(R, np.broadcast_to(np.eye(n), (B, n, n)))


@pytest.mark.parametrize("L", (1, 2, 5))
def test_twin_uniform_attention_closed_form(L):
    """A = J / n, mean fusion: A^ = (I + J/n) / 2 and, J/n being idempotent, A^^L = 2^-L I + (1 - 2^-L) J/n"""
    B, h, n = 1, 2, 7
    A = np.full((B, h, n, n), 1.0 / n)
    R = T.chain([T.rollout_layer(A, "mean")] * L)
    want = 2.0 ** -L * np.eye(n) + (1 - 2.0 ** -L) * np.full((n, n), 1.0 / n)
    assert np.abs(R[0] - want).max() <= 1e-15
    assert np.abs(R.sum(axis=-1) - 1.0).max() <= 1e-15


def _random_layer(rng, B, h, n, d):
    s = rng.standard_normal((B, h, n, n))
    a = np.exp(s - s.max(axis=-1, keepdims=True))
    return a / a.sum(axis=-1, keepdims=True), rng.standard_normal((B, n, h * d)), rng.standard_normal((B, n, 3 * h * d))


def test_twin_gradient_rule_one_layer_and_its_definition():
    rng = np.random.default_rng(3)
    B, h, n, d = 2, 3, 6, 4
    a, do, qkv = _random_layer(rng, B, h, n, d)
    abar = T.grad_layer(a, do, qkv)
    assert np.abs(T.chain([abar], add_identity=True) - (np.eye(n) + abar)).max() == 0.0
    # the definition, element by element: dA[b,h,i,j] = sum_k dout[b,i,h d + k] V[b,j,h,k], V the third part of '(qkv h d)'
    want = np.zeros((B, n, n))
    for b in range(B):
        for i in range(n):
            for j in range(n):
                for hh in range(h):
                    dA = sum(do[b, i, hh * d + k] * qkv[b, j, 2 * h * d + hh * d + k] for k in range(d))
                    want[b, i, j] += max(dA * a[b, hh, i, j], 0.0) / h
    assert np.abs(abar - want).max() <= 1e-14
    assert (T.grad_layer_bar(a, do, qkv) >= (d + h + 4) * T.EPS * abar - 1e-18).all(), "the bar's magnitude dominates the value"
    # two layers: R_2 = R_1 + Abar_2 R_1
    a2, do2, qkv2 = _random_layer(rng, B, h, n, d)
    ab2 = T.grad_layer(a2, do2, qkv2)
    R1 = np.eye(n) + abar
    assert np.abs(T.chain([abar, ab2], add_identity=True) - (R1 + ab2 @ R1)).max() <= 1e-14


def test_twin_rows_from_the_left_and_the_hierarchy():
    """carry() is the CLS row of chain(); relevance() is the explicit block composition: the final chain's CLS row, its segment
    of an aggregated input multiplied into that aggregator's chain"""
    rng = np.random.default_rng(5)
    B, h, ncls = 2, 2, 1
    lens = (1, 4, 6, 1)                                    # [xr | agg_1 states | agg_2 states | clin]
    n = ncls + sum(lens)
    fin = [T.rollout_layer(_random_layer(rng, B, h, n, 2)[0]) for _ in range(3)]
    agg = {k: [T.rollout_layer(_random_layer(rng, B, h, lens[k], 2)[0]) for _ in range(2)] for k in (1, 2)}
    zero = lambda ms: [np.zeros_like(m) for m in ms]          # noqa: E731
    segs = [(0, 0, 1, 1, None), (1, 1, 4, 2, 1), (2, 5, 6, 1, 2), (3, 11, 1, 1, None)]
    out = T.relevance(fin, zero(fin), ncls, segs, agg, {k: zero(v) for k, v in agg.items()}, 4)
    R = T.chain(fin)
    assert np.abs(out["final"] - R[:, 0]).max() <= 1e-15
    assert np.abs(out["tokens"][0] - R[:, 0, 1:2]).max() <= 1e-15 and np.abs(out["tokens"][3] - R[:, 0, 12:13]).max() <= 1e-15
    for k, (lo, hi) in ((1, (2, 6)), (2, (6, 12))):
        want = np.einsum("bs,bst->bt", R[:, 0, lo:hi], T.chain(agg[k]))
        assert np.abs(out["tokens"][k] - want).max() <= 1e-15
    assert out["slices"][1].shape == (B, 2) and out["slices"][2].shape == (B, 6) and out["slices"][0].shape == (B, 1)
    assert np.abs(out["slices"][1] - out["tokens"][1].reshape(B, 2, 2).sum(-1)).max() <= 1e-15
    # rollout conserves: every chain is row-stochastic
    assert np.abs(out["totals"].sum(axis=1) + out["cls_self"] - 1.0).max() <= 1e-14
    assert np.abs(out["totals"][:, 1] - R[:, 0, 2:6].sum(-1)).max() <= 1e-14
    assert all(np.abs(b).max() < 1e-4 for b in out["tokens_bar"]), "the bars stay at rounding level"


def test_twin_reproduces_the_fixture():
    g = load("f24_attn_relevance.npz")
    L = 3
    a64, d64 = [g[f"attn64:{l}"] for l in range(L)], [g[f"dattn64:{l}"] for l in range(L)]
    assert a64[0].shape == (2, 2, 9, 9) and a64[0].dtype == np.float64 and g["attn32:0"].dtype == np.float32
    assert g["features"].shape == (2, 8, 32) and g["target"].tolist() == [[1], [0]] and int(g["heads"]) == 2
    abar = [np.maximum(d * a, 0.0).mean(axis=1) for a, d in zip(a64, d64)]
    for l in range(L):
        assert np.array_equal(abar[l], g[f"abar64:{l}"])
    for fuse in T.FUSE:
        assert np.array_equal(T.chain([T.rollout_layer(a, fuse) for a in a64]), g[f"rollout64:{fuse}"])
        assert np.abs(g[f"rollout64:{fuse}"].sum(axis=-1) - 1.0).max() <= 1e-14
    assert np.array_equal(T.chain(abar, add_identity=True), g["gradrel64"])
    # the gradient rule separates the classes: the two samples gather different logits
    assert np.abs(g["gradrel64"][0] - g["gradrel64"][1]).max() > 1e-4
    # the reference's own float32 run stays at float32 distance from the float64 one (what the GPU test measures against)
    a32, d32 = [g[f"attn32:{l}"] for l in range(L)], [g[f"dattn32:{l}"] for l in range(L)]
    r32 = T.chain([np.maximum(d.astype(np.float64) * a, 0.0).mean(axis=1) for a, d in zip(a32, d32)], add_identity=True)
    assert 0 < np.abs(r32 - g["gradrel64"]).max() < 1e-5


# ---- token_layout --------------------------------------------------------------------------------------------------------------
def _model(cfg, monkeypatch):
    """the registry class built from its config on the CPU, its trunks left empty: the layout reads `vs` and the FeaTs only"""
    from oaprogressionmmf_amd.config import ConfigDict
    from oaprogressionmmf_amd.models import KoafTrunk, _common, dict_models
    monkeypatch.setattr(_common, "build_trunk", lambda arch, pretrained, with_gap: KoafTrunk())
    return dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)


LAYOUTS = {
    "MR1CnnTrf-rc-gap": (lambda: P.cfg_mr1(shape=(64, 96, 32), depth=1), [(0, 0, 32, 1, None)]),
    "MR1CnnTrf-rc": (lambda: P.cfg_mr1(shape=(64, 96, 32), with_gap=False, depth=1), [(0, 0, 192, 6, None)]),
    "MR1CnnTrf-cs": (lambda: P.cfg_mr1(shape=(64, 96, 32), dims_view="cs", with_gap=False, depth=1), [(0, 0, 192, 3, None)]),
    "MR1CnnTrf-rs": (lambda: P.cfg_mr1(shape=(64, 96, 32), dims_view="rs", with_gap=False, depth=1), [(0, 0, 192, 2, None)]),
    "MR2CnnTrf": (lambda: P.cfg_mr2(shape0=(160, 160, 4), shape1=(160, 160, 3)), [(0, 0, 4, 1, None), (1, 4, 3, 1, None)]),
    "XR1MR1CnnTrf": (lambda: P.cfg_xr1mr1(xr=(96, 96), mr=(64, 64, 3)), [(0, 0, 1, 1, None), (1, 1, 3, 1, None)]),
    "XR1MR1CnnTrf-nogap": (lambda: P.cfg_xr1mr1(xr=(96, 96), mr=(64, 64, 3), with_gap=False), [(0, 0, 9, 9, None), (1, 9, 12, 4, None)]),
    "XR1MR2CnnTrf": (lambda: P.cfg_xr1mr2(xr=(96, 96), mr1=(64, 64, 6), mr2=(64, 64, 5)),
                     [(0, 0, 1, 1, None), (1, 1, 6, 1, "_agg_1"), (2, 7, 5, 1, "_agg_2")]),
    "XR1MR2C1CnnTrf": (lambda: P.cfg_full(xr=(96, 96), mr1=(64, 64, 6), mr2=(64, 64, 5), depth=1),
                       [(0, 0, 1, 1, None), (1, 1, 6, 1, "_agg_1"), (2, 7, 5, 1, "_agg_2"), (3, 12, 1, 1, None)]),
    "MR1C1CnnTrf": (lambda: P.cfg_mr1c1(mr=(96, 96, 6), depth=1), [(0, 0, 6, 1, "_agg_0"), (1, 6, 1, 1, None)]),
    "XR1MR3C1CnnTrf": (lambda: P.cfg_xr1mr3c1(xr=(96, 96), mr1=(64, 64, 6), mr2=(64, 64, 5), mr3=(64, 64, 4), depth=1),
                       [(0, 0, 1, 1, None), (1, 1, 6, 1, "_agg_1"), (2, 7, 5, 1, "_agg_2"), (3, 12, 4, 1, "_agg_3"), (4, 16, 1, 1, None)]),
}


@pytest.mark.parametrize("which", list(LAYOUTS))
def test_token_layout(which, monkeypatch):
    from oaprogressionmmf_amd.models import FeaT
    from oaprogressionmmf_amd.models._common import token_layout
    make, want = LAYOUTS[which]
    m = _model(make(), monkeypatch)
    lay = token_layout(m)
    segs, ncls, feat = lay
    assert ncls == 1 and isinstance(feat, FeaT) and feat is getattr(m, "_agg_final", getattr(m, "_agg", None))
    got = [(s.input, s.offset, s.length, s.per_slice, s.agg) for s in segs]
    assert [g[:4] for g in got] == [w[:4] for w in want]
    for g, w in zip(got, want):
        assert g[4] is (getattr(m, w[4]) if w[4] else None)
        if g[4] is not None:
            assert not g[4].with_cls and g[4].pos_embedding.shape[1] == g[2], "an aggregator's states are its segment"
        assert g[2] % g[3] == 0
    assert feat.pos_embedding.shape[1] == ncls + sum(g[2] for g in got), "the segments tile the final sequence behind the CLS token"
    assert [g[1] for g in got] == list(np.cumsum([0] + [g[2] for g in got[:-1]]))


@pytest.mark.parametrize("make", (lambda: P.cfg_xr1cnn(arch="resnet18", size=160), lambda: P.cfg_xr1c1(arch="resnet18", size=160)),
                         ids=("XR1Cnn", "XR1C1Cnn"))
def test_token_layout_refuses_a_model_without_a_feat(make, monkeypatch):
    from oaprogressionmmf_amd.models._common import token_layout
    from oaprogressionmmf_amd.run import attention_relevance
    m = _model(make(), monkeypatch)
    with pytest.raises(ValueError, match="has no FeaT"):
        token_layout(m)
    with pytest.raises(ValueError, match="has no FeaT"):
        attention_relevance(m, (torch.zeros(1, 1, 160, 160),))
    with pytest.raises(ValueError, match="has no FeaT"):
        token_layout(torch.nn.Linear(2, 2))


def test_attention_relevance_argument_validation(monkeypatch):
    from oaprogressionmmf_amd import functional as KF
    from oaprogressionmmf_amd.models import FeaT
    from oaprogressionmmf_amd.run import attention_relevance
    with pytest.raises(ValueError, match="Unknown method: rollup"):
        attention_relevance(None, (), method="rollup")
    with pytest.raises(ValueError, match="Unknown fuse: median"):
        attention_relevance(None, (), fuse="median")
    with pytest.raises(ValueError, match="fuse stays"):
        attention_relevance(None, (), 0, method="grad", fuse="max")
    with pytest.raises(ValueError, match="needs a target"):
        attention_relevance(None, (), method="grad")
    with pytest.raises(TypeError):
        attention_relevance(None, (), 0, "grad")              # method / fuse are keyword-only
    m = _model(P.cfg_mr2(shape0=(160, 160, 4), shape1=(160, 160, 3)), monkeypatch)
    with pytest.raises(ValueError, match="takes 2 inputs, got 1"):
        attention_relevance(m, (torch.zeros(1),))
    m._agg = FeaT(num_patches=7, patch_dim=8, emb_dim=8, depth=1, heads=2, mlp_dim=8, num_classes=2, with_cls=False)
    with pytest.raises(ValueError, match="no CLS token"):
        attention_relevance(m, (torch.zeros(1), torch.zeros(1)))
    assert KF.ATTN_TAPE is None, "the tape is off unless a call installs it"


# ---- ops and entry points ------------------------------------------------------------------------------------------------------
def test_attn_entry_points_are_declared_and_built():
    from oaprogressionmmf_amd import _lib, ops
    protos = _lib.parse_header()
    P_, I = ctypes.c_void_p, ctypes.c_int32
    # koaf_attn_layer(attn, dout, qkv, abar, B, n, h, d, mode, stream)
    assert protos["koaf_attn_layer"] == (ctypes.c_int, [P_, P_, P_, P_, I, I, I, I, I, P_])
    # koaf_attn_apply(r_in, abar, r_out, B, q, n, add_identity, stream)
    assert protos["koaf_attn_apply"] == (ctypes.c_int, [P_, P_, P_, I, I, I, I, P_])
    # koaf_attn_segsum(r, out, B, n, off, K, t, stream)
    assert protos["koaf_attn_segsum"] == (ctypes.c_int, [P_, P_, I, I, I, I, I, P_])
    assert _lib.defines()["KOAF_VERSION"] == 200
    handle = _lib.lib()                            # (binds every declared symbol: a library without the three fails here)
    assert handle.koaf_version() == 200
    for name in ("koaf_attn_layer", "koaf_attn_apply", "koaf_attn_segsum"):
        assert getattr(handle, name).argtypes == protos[name][1]
    mk = (_lib.LIB_PATH.parent / "Makefile").read_text()
    rest = [ln for ln in mk.splitlines() if ln.startswith("REST_SRCS")]
    assert len(rest) == 1 and "koaf_attnrel.hip" in rest[0].split()
    assert ops.ATTN_MODES == ("mean", "max", "min", "grad")


def test_attn_kernels_refuse_bad_arguments_without_a_device():
    """KOAF_REQUIRE runs ahead of any launch: sizes below 1, an unknown mode, missing or surplus pointers, aliasing, a segment that
    leaves its row"""
    from oaprogressionmmf_amd import _lib
    L, EINVAL = _lib.lib(), _lib.defines()["KOAF_EINVAL"]
    p, q, r = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)     # (never dereferenced)
    o = ctypes.c_void_p(4 << 20)
    bad_layer = [(p, None, None, o, 0, 4, 2, 1, 0), (p, None, None, o, 1, 0, 2, 1, 0), (p, None, None, o, 1, 4, 0, 1, 0),
                 (p, None, None, o, 1, 4, 2, 0, 0), (p, None, None, o, 1, 4, 2, 1, 4), (p, None, None, o, 1, 4, 2, 1, -1),
                 (None, None, None, o, 1, 4, 2, 1, 0), (p, None, None, None, 1, 4, 2, 1, 0),
                 (p, q, None, o, 1, 4, 2, 1, 0), (p, None, r, o, 1, 4, 2, 1, 1),               # rollout takes no dout / qkv
                 (p, None, r, o, 1, 4, 2, 1, 3), (p, q, None, o, 1, 4, 2, 1, 3),               # the gradient rule needs both
                 (p, None, None, p, 1, 4, 2, 1, 0), (p, q, r, q, 1, 4, 2, 1, 3), (p, q, r, r, 1, 4, 2, 1, 3),   # abar aliases an input
                 (p, q, r, o, 65536, 4, 2, 1, 3)]
    for args in bad_layer:
        assert L.koaf_attn_layer(*args, None) == EINVAL, args
        assert b"koaf_attn_layer" in L.koaf_last_error()
    bad_apply = [(p, q, o, 0, 1, 4, 0), (p, q, o, 1, 0, 4, 0), (p, q, o, 1, 1, 0, 0), (p, None, o, 1, 1, 4, 0), (p, q, None, 1, 1, 4, 0),
                 (p, q, o, 1, 1, 4, 2), (None, q, o, 1, 3, 4, 0),                              # r_in NULL needs q == n
                 (p, q, p, 1, 1, 4, 0), (p, q, q, 1, 1, 4, 1), (None, q, q, 1, 4, 4, 0), (p, q, o, 65536, 1, 4, 0)]
    for args in bad_apply:
        assert L.koaf_attn_apply(*args, None) == EINVAL, args
        assert b"koaf_attn_apply" in L.koaf_last_error()
    assert L.koaf_attn_apply(p, q, p, 1, 1, 4, 0, None) == EINVAL and b"aliases" in L.koaf_last_error()
    bad_seg = [(None, o, 1, 8, 0, 1, 1), (p, None, 1, 8, 0, 1, 1), (p, o, 0, 8, 0, 1, 1), (p, o, 1, 0, 0, 1, 1), (p, o, 1, 8, -1, 1, 1),
               (p, o, 1, 8, 0, 0, 1), (p, o, 1, 8, 0, 1, 0), (p, o, 1, 8, 0, 3, 3), (p, o, 1, 8, 8, 1, 1), (p, o, 1, 8, 2, 1, 7),
               (p, o, 1, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 16, 2 ** 16), (p, p, 1, 8, 0, 1, 1)]
    for args in bad_seg:
        assert L.koaf_attn_segsum(*args, None) == EINVAL, args
        assert b"koaf_attn_segsum" in L.koaf_last_error()


def test_ops_attn_argument_checks_raise_before_a_launch(monkeypatch):
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    a, do, qkv = torch.zeros(2, 2, 4, 4), torch.zeros(2, 4, 6), torch.zeros(2, 4, 18)
    with pytest.raises(ValueError, match="Unknown attention mode: median"):
        ops.attn_layer(a, "median")
    for bad in (a, a.double(), a[:, :, :, :3], "x"):                       # (a CPU tensor is refused: there is no fallback)
        with pytest.raises(KoafError, match="attn_layer: attn is"):
            ops.attn_layer(bad, "mean")
    with pytest.raises(KoafError, match="attn_apply: abar is"):
        ops.attn_apply(torch.zeros(2, 4, 4))
    with pytest.raises(KoafError, match="attn_segsum: r is"):
        ops.attn_segsum(torch.zeros(2, 8), 0, 1, 8)
    # the checks behind the device test, on CPU tensors: check_tensor is handed the tensor itself as the device to be on
    import oaprogressionmmf_amd.ops.explain as E
    real = E.check_tensor
    monkeypatch.setattr(E, "check_tensor", lambda what, name, t, dtype, shape=None, like=None, nonempty=False, where="":
                        real(what, name, t, dtype, shape, t if torch.is_tensor(t) else like, nonempty, where))
    with pytest.raises(KoafError, match=r"attn is \[B, h, n, n\]"):
        ops.attn_layer(torch.zeros(2, 2, 4, 5), "mean")
    with pytest.raises(KoafError, match="mode grad needs dout"):
        ops.attn_layer(a, "grad", dout=do)
    with pytest.raises(KoafError, match=r"dout is \[2, 4, 2 \* d\]"):
        ops.attn_layer(a, "grad", dout=torch.zeros(2, 4, 5), qkv=qkv)
    with pytest.raises(KoafError, match="qkv is"):
        ops.attn_layer(a, "grad", dout=do, qkv=torch.zeros(2, 4, 12))
    with pytest.raises(KoafError, match="mode max takes no dout / qkv"):
        ops.attn_layer(a, "max", dout=do, qkv=qkv)
    with pytest.raises(KoafError, match=r"abar is \[B, n, n\]"):
        ops.attn_apply(torch.zeros(2, 4, 5))
    with pytest.raises(KoafError, match=r"r_in is \[2, q, 4\]"):
        ops.attn_apply(torch.zeros(2, 4, 4), r_in=torch.zeros(2, 1, 5))
    with pytest.raises(KoafError, match=r"r is \[B, n\]"):
        ops.attn_segsum(torch.zeros(2, 8, 1), 0, 1, 8)
    for off, K, t in ((-1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 3, 3), (8, 1, 1), (1, 1, 8)):
        with pytest.raises(KoafError, match="leaves the row of n = 8"):
            ops.attn_segsum(torch.zeros(2, 8), off, K, t)


# ---- explain_epoch -------------------------------------------------------------------------------------------------------------
def test_explain_epoch_attention_keys_on_a_stub(monkeypatch):
    from oaprogressionmmf_amd.run import AttnRelevance, _attnrel, ensemble_explain_foldw, explain_epoch
    calls = []

    def fake(model, xs, target=None, *, method="rollout", fuse="mean"):
        calls.append((method, fuse, tuple(int(v) for v in torch.as_tensor(target).reshape(-1))))
        B = xs[0].shape[0]
        rel = (AttnRelevance(torch.full((B, 1), 0.25), torch.full((B, 1), 0.25)),
               AttnRelevance(torch.arange(6.).repeat(B, 1) / 30, (torch.arange(6.).repeat(B, 1) / 30).reshape(B, 3, 2).sum(-1)))
        return rel, torch.stack([r.tokens.sum(1) for r in rel], dim=1), torch.full((B,), 0.25)
    monkeypatch.setattr(_attnrel, "attention_relevance", fake)
    modals = ("xr_pa", "sag_3d_dess")
    xs, y = (torch.zeros(3, 1, 4, 4), torch.zeros(3, 1, 4, 4, 3)), torch.tensor([[1], [0], [1]])
    loader = [{"image__xr_pa": xs[0][lo:hi], "image__sag_3d_dess": xs[1][lo:hi], "target": y[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in ((0, 2), (2, 3))]
    seen = []
    acc = explain_epoch(None, loader, modals, device="cpu", explain_fn="attn_rollout", explain_kwargs=dict(fuse="max"),
                        sink=lambda ids, mods, rel: seen.append((list(ids), list(mods), rel)))
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "attn_attrs", "attn_percent", "attn_slice_scores"]
    assert calls == [("rollout", "max", (1, 0)), ("rollout", "max", (1,))]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and acc["modal_names"] == [list(modals)] * 3 and acc["target"] == y.tolist()
    np.testing.assert_allclose(acc["attn_attrs"], [[0.25, 0.5]] * 3, rtol=1e-6)
    np.testing.assert_allclose(acc["attn_percent"], [[33.333, 66.667]] * 3, atol=2e-3)
    np.testing.assert_allclose(acc["attn_slice_scores"][2][1], [1 / 30, 5 / 30, 9 / 30], rtol=1e-6)
    assert [len(r) for r in acc["attn_slice_scores"][0]] == [1, 3]
    assert [ids for ids, _, _ in seen] == [["k0", "k1"], ["k2"]] and all(isinstance(r, AttnRelevance) for _, _, rel in seen for r in rel)
    assert not any(torch.is_tensor(v) for vals in acc.values() for v in vals), "the returned lists hold no tensors"
    calls.clear()
    acc2 = explain_epoch(None, loader, modals, device="cpu", explain_fn="attn_grad")
    assert acc2.keys() == acc.keys() and [c[:2] for c in calls] == [("grad", "mean")] * 2
    ens = ensemble_explain_foldw({0: acc, 1: acc2}, prefix="attn")
    np.testing.assert_allclose(np.asarray(ens["attn_percent"]) * 100.0, acc["attn_percent"], atol=2e-3)
    assert "attn_attrs__0" in ens and "attn_percent__1" in ens
    # refusals keep their words
    with pytest.raises(ValueError, match="Unknown explain_fn: grad_cam"):
        explain_epoch(None, [], modals, explain_fn="grad_cam")
    with pytest.raises(ValueError, match="takes no explain_kwargs"):
        explain_epoch(None, loader, modals, device="cpu", explain_fn="attn_rollout", explain_kwargs=dict(n_steps=3))
    with pytest.raises(ValueError, match="takes no explain_kwargs"):
        explain_epoch(None, loader, modals, device="cpu", explain_fn="gradcam", explain_kwargs=dict(fuse="max"))
    with pytest.raises(ValueError, match="takes no explain_kwargs"):
        explain_epoch(None, loader, modals, device="cpu", explain_kwargs=dict(fuse="max"))
    assert explain_epoch(None, [], modals, explain_fn="attn_rollout") == {} and explain_epoch(None, [], modals, explain_fn="attn_grad") == {}
