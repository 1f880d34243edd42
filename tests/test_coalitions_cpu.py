"""CPU: the host side of the modality coalitions (run.modal_coalitions / run.modal_shapley, koaf_coal.hip).  The brute force of
coal_twin.py against the axioms that define the Shapley value; the two entry points as koaf.h declares them, bound by the library
at the unchanged ABI version; the refusals that need no device; the registration of the explain_epoch key; and the Python route --
the coalition masks, chunking through the batch dimension, the explain_epoch plumbing -- on a stub with the fold replaced by the
twin."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import coal_twin as T


def _game(P, B=2, seed=0):
    return np.random.default_rng(100 * P + seed).uniform(-1.0, 1.0, size=(1 << P, B)).astype(np.float32)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_twin_axioms(P):
    """efficiency, the dummy player, symmetry, additivity: what singles the Shapley value out -- and the brute force has them"""
    v = _game(P).astype(np.float64)
    S = 1 << P
    phi, inter, loo, solo = T.shapley(v)
    tol = 1e-14
    np.testing.assert_allclose(phi.sum(1), v[S - 1] - v[0], atol=tol)                          # efficiency
    for i in range(P):
        assert (inter[:, i, i] == 0).all()
        np.testing.assert_allclose(loo[:, i], v[S - 1] - v[(S - 1) ^ (1 << i)], atol=0)
        np.testing.assert_allclose(solo[:, i], v[1 << i] - v[0], atol=0)
    np.testing.assert_allclose(inter, inter.transpose(0, 2, 1), atol=tol)
    if P == 1:
        assert (inter == 0).all()
        return
    # a dummy: player 0 never changes the value
    d = v.copy()
    for s in range(S):
        d[s | 1] = d[s & ~1]
    pd, idd, _, _ = T.shapley(d)
    np.testing.assert_allclose(pd[:, 0], 0.0, atol=tol)
    np.testing.assert_allclose(idd[:, 0, :], 0.0, atol=tol)
    # symmetric players 0 and 1: the value depends on how many of the two are present only
    sym = v.copy()
    for s in range(S):
        if s & 3 == 2:
            sym[s] = sym[s ^ 3]
    ps = T.shapley(sym)[0]
    np.testing.assert_allclose(ps[:, 0], ps[:, 1], atol=tol)
    # an additive game: phi = a, no interaction, loo = solo = a
    a = np.random.default_rng(P).uniform(-1, 1, size=(2, P))
    add = np.stack([sum((a[:, i] for i in range(P) if s >> i & 1), np.full(2, 0.25)) for s in range(S)])
    pa, ia, la, sa = T.shapley(add)
    for got in (pa, la, sa):
        np.testing.assert_allclose(got, a, atol=tol)
    np.testing.assert_allclose(ia, 0.0, atol=tol)


def test_twin_known_values():
    """the glove game (players 0, 1 hold a left glove, 2 a right one; a pair is worth 1): phi = (1/6, 1/6, 2/3); and a pure pair
    interaction v = [0 and 1 present]: phi = (1/2, 1/2), I_01 = 1"""
    v = np.array([[float(bool(s & 4) and bool(s & 3))] for s in range(8)])
    phi, inter, loo, solo = T.shapley(v)
    np.testing.assert_allclose(phi[0], [1 / 6, 1 / 6, 2 / 3], atol=1e-15)
    np.testing.assert_allclose(loo[0], [0, 0, 1], atol=0)
    np.testing.assert_allclose(solo[0], [0, 0, 0], atol=0)
    np.testing.assert_allclose(inter[0, 0, 1], -0.5, atol=1e-15)       # the two left gloves are substitutes
    np.testing.assert_allclose(inter[0, 0, 2], 0.5, atol=1e-15)
    v = np.array([[float(s & 3 == 3)] for s in range(4)])
    phi, inter, _, _ = T.shapley(v)
    np.testing.assert_allclose(phi[0], [0.5, 0.5], atol=0)
    np.testing.assert_allclose(inter[0], [[0, 1], [1, 0]], atol=0)


def test_weights_are_the_orderings_counted():
    """ops.shapley_weights -- the table the kernel is handed -- against the counted orderings of the twin"""
    from oaprogressionmmf_amd import ops
    assert ops.COAL_MAX_M == 8
    for M in range(1, 9):
        wp, wi = ops.shapley_weights(M)
        assert len(wp) == M and len(wi) == M - 1
        cnt = T._prefix_counts(M)
        for mask, c in cnt.items():
            assert wp[bin(mask).count("1")] == c / math.factorial(M), (M, mask)
        assert abs(sum(wp[t] * math.comb(M - 1, t) for t in range(M)) - 1) < 1e-15
        if M > 1:
            assert wi == ops.shapley_weights(M - 1)[0], "the pair's weights are the Shapley weights of the reduced game"


def test_twin_tokens():
    tx = np.arange(2 * 5 * 3, dtype=np.float32).reshape(2, 5, 3)
    t0 = -np.ones((1, 5, 3), dtype=np.float32)
    out = T.tokens(tx, t0, [0, 1, 4, 5], [0, 7, 2, 5])
    assert out.shape == (4, 2, 5, 3) and (out[0] == -1).all() and (out[1] == tx).all()
    assert (out[2][:, 1:4] == tx[:, 1:4]).all() and (out[2][:, [0, 4]] == -1).all()
    assert (out[3][:, [0, 4]] == tx[:, [0, 4]]).all() and (out[3][:, 1:4] == -1).all()


def test_coal_entry_points_are_declared_and_built():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    P, I = ctypes.c_void_p, ctypes.c_int32
    # koaf_coal_tokens(tx, t0, seg_off, masks, out, J, B, B0, L, D, M, stream)
    assert protos["koaf_coal_tokens"] == (ctypes.c_int, [P, P, P, P, P, I, I, I, I, I, I, P])
    # koaf_shapley_fold(v, w_phi, w_int, phi, inter, loo, solo, S, B, M, stream)
    assert protos["koaf_shapley_fold"] == (ctypes.c_int, [P, P, P, P, P, P, P, I, I, I, P])
    assert _lib.defines()["KOAF_VERSION"] == 200 and _lib.defines()["KOAF_COAL_MAX_M"] == 8
    handle = _lib.lib()                            # (binds every declared symbol: a library without the two fails here)
    for name in ("koaf_coal_tokens", "koaf_shapley_fold"):
        assert getattr(handle, name).argtypes == protos[name][1]
    mk = (_lib.LIB_PATH.parent / "Makefile").read_text()
    rest = [ln for ln in mk.splitlines() if ln.startswith("REST_SRCS")]
    assert len(rest) == 1 and "koaf_coal.hip" in rest[0].split()


def test_coal_kernels_refuse_bad_arguments_without_a_device():
    """the argument checks run ahead of any launch; the tables are host arrays, so that they can"""
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    EINVAL = _lib.defines()["KOAF_EINVAL"]
    p = ctypes.c_void_p(256)                       # (never dereferenced: every call below is refused first)
    I32, U32, F64 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_double
    seg, msk = (I32 * 4)(0, 1, 4, 6), (U32 * 2)(5, 2)

    def tokens(seg=seg, msk=msk, J=2, B=2, B0=1, Lt=6, D=4, M=3, tx=p, out=p):
        return L.koaf_coal_tokens(tx, p, seg, msk, out, J, B, B0, Lt, D, M, None)
    for M in (0, 9, -1):
        assert tokens(M=M) == EINVAL and b"koaf_coal_tokens" in L.koaf_last_error() and b"M" in L.koaf_last_error()
    assert tokens(msk=(U32 * 2)(5, 8)) == EINVAL and b"masks[1]" in L.koaf_last_error()          # bit 3 at M = 3
    assert tokens(seg=(I32 * 4)(0, 4, 4, 6)) == EINVAL and b"ascends" in L.koaf_last_error()
    assert tokens(seg=(I32 * 4)(0, 4, 3, 6)) == EINVAL and b"ascends" in L.koaf_last_error()
    assert tokens(seg=(I32 * 4)(0, 1, 4, 5)) == EINVAL and b"seg_off" in L.koaf_last_error()     # seg_off[M] != L
    assert tokens(seg=(I32 * 4)(1, 2, 4, 6)) == EINVAL
    assert tokens(B=3, B0=2) == EINVAL and b"B0" in L.koaf_last_error()
    assert tokens(B=3, B0=0) == EINVAL
    assert tokens(J=0) == EINVAL and tokens(D=0) == EINVAL and tokens(B=0, B0=0) == EINVAL and tokens(B=65536, B0=1) == EINVAL
    assert tokens(tx=None) == EINVAL and tokens(out=None) == EINVAL and tokens(seg=None) == EINVAL and tokens(msk=None) == EINVAL
    assert L.koaf_coal_tokens(p, p, (I32 * 2)(0, 1 << 20), msk, p, 1, 1, 1, 1 << 20, 1 << 11, 1, None) == EINVAL   # L * D = 2^31

    wp, wi = (F64 * 3)(1 / 3, 1 / 6, 1 / 3), (F64 * 2)(0.5, 0.5)

    def fold(S=8, B=2, M=3, v=p, wp=wp, wi=wi, phi=p):
        return L.koaf_shapley_fold(v, wp, wi, phi, p, p, p, S, B, M, None)
    for M in (0, 9):
        assert fold(S=1 << M, M=M) == EINVAL and b"koaf_shapley_fold" in L.koaf_last_error()
    for S in (7, 9, 16, 0):
        assert fold(S=S) == EINVAL and b"2^M" in L.koaf_last_error()
    assert fold(B=0) == EINVAL and fold(v=None) == EINVAL and fold(wp=None) == EINVAL and fold(wi=None) == EINVAL
    assert fold(phi=None) == EINVAL


def test_wrappers_refuse_host_tensors_and_bad_tables():
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    tx, t0 = torch.zeros(2, 6, 4), torch.zeros(1, 6, 4)
    with pytest.raises(KoafError, match="tx"):
        ops.coal_tokens(tx, t0, [0, 1, 4, 6], [5, 2])                  # no CPU fallback
    with pytest.raises(KoafError, match="shapley_fold"):
        ops.shapley_fold(torch.zeros(8, 2), 3)
    with pytest.raises(KoafError, match="1 <= M <= 8"):
        ops.shapley_fold(torch.zeros(1, 2), 0)
    with pytest.raises(KoafError, match="1 <= M <= 8"):
        ops.shapley_fold(torch.zeros(512, 2), 9)


# ---- the Python route on a stub ------------------------------------------------------------------------------------------------
def _stub():
    """a three-input stub with the product models' calling convention: (B, 2) logits, with a pair interaction of inputs 0 and 2"""
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 16).reshape(1, 1, 4, 4))
            self.c = torch.nn.Parameter(torch.linspace(0.5, -0.25, 9).reshape(1, 9))
            self.calls = []

        def forward(self, img, vec, clin):
            self.calls.append(int(img.shape[0]))
            u = (img * self.a).flatten(1).sum(1)
            w = (clin.flatten(1) * self.c).sum(1)
            q = vec.flatten(1).sum(1)
            return torch.stack([torch.tanh(u) + 0.3 * u * w + q, w - 0.1 * q * q], dim=1)
    return Stub().eval()


def _inputs(B=3):
    g = torch.Generator().manual_seed(5)
    xs = (torch.randn(B, 1, 4, 4, generator=g), torch.randn(B, 1, 5, generator=g), torch.randn(B, 1, 9, generator=g))
    return xs, torch.tensor([[0], [1], [0]][:B])


@pytest.fixture
def twin_fold(monkeypatch):
    from oaprogressionmmf_amd import ops

    def fold(v, M):
        assert v.shape[0] == 1 << M and v.dtype == torch.float32
        return tuple(torch.from_numpy(a) for a in T.shapley(v.numpy()))
    monkeypatch.setattr(ops, "shapley_fold", fold)
    return ops


def test_players_and_masks():
    from oaprogressionmmf_amd.run import coalition_masks, player_masks
    assert player_masks(None, 4) == [1, 2, 4, 8]
    assert player_masks([[0, 1, 2, 3], [4]], 5) == [15, 16]
    assert coalition_masks([15, 16]) == [0, 15, 16, 31]
    assert coalition_masks([1, 2, 4]) == list(range(8))
    assert coalition_masks(player_masks([[2], [0, 1]], 3)) == [0, 4, 3, 7]


def test_refusals():
    from oaprogressionmmf_amd.run import modal_coalitions, modal_shapley
    m, (xs, y) = _stub(), _inputs()
    for bad in ([[0, 1]], [[0, 1], [1, 2]], [[0], [1], [2], [3]], [[0, 1, 2], []], [[0], [1], [2, 2]], 3, [0, 1, 2]):
        with pytest.raises(ValueError, match="partition"):
            modal_coalitions(m, xs, y, players=bad, sparse=False)
    with pytest.raises(ValueError, match="players <= 8"):
        modal_coalitions(m, [xs[1]] * 9, y, sparse=False)
    m.train()
    with pytest.raises(ValueError, match="sparse=True keeps encoder features .* eval\\(\\)"):
        modal_coalitions(m, xs, y, sparse=True)
    with pytest.raises(ValueError, match="sparse=True keeps encoder features .* eval\\(\\)"):
        modal_shapley(m, xs, y, sparse=True, chunk=1)
    with pytest.raises(ValueError, match="eval\\(\\)"):
        modal_coalitions(m, xs, y, sparse=False, chunk=2)                          # _check_chunk's rule
    m.eval()
    with pytest.raises(ValueError, match="sparse=False"):
        modal_coalitions(m, xs, y)                                                 # no token layout to splice
    with pytest.raises(ValueError, match="chunk"):
        modal_coalitions(m, xs, y, sparse=False, chunk=65)
    with pytest.raises(ValueError, match="baselines"):
        modal_coalitions(m, xs, y, baselines=(0, 0), sparse=False)
    assert m.calls == [], "every refusal comes ahead of the first model pass"


def test_models_without_a_token_layout_name_sparse_false():
    from oaprogressionmmf_amd.models import dict_models
    from oaprogressionmmf_amd.run._coalitions import _layout
    for name in ("XR1Cnn", "XR1C1Cnn"):
        assert name in dict_models
        fake = object.__new__(dict_models[name])                       # (token_layout looks at the class and `vs` only)
        with pytest.raises(ValueError, match=f"{name} has no token layout .* sparse=False"):
            _layout(fake, 1)


def test_dense_route_on_a_stub(twin_fold):
    """sparse=False: ceil(S / chunk) passes at batch J * B; every value is the plain forward of the copy; the fold of the values
    satisfies efficiency; players merge inputs"""
    from oaprogressionmmf_amd.run import ModalShapley, modal_coalitions, modal_shapley
    m, (xs, y) = _stub(), _inputs()
    bases = (-0.5, None, torch.full((3, 1, 9), 0.25))
    vals, masks = modal_coalitions(m, xs, y, baselines=bases, chunk=3, sparse=False)
    assert masks == list(range(8)) and vals.shape == (8, 3) and vals.dtype == torch.float32
    assert m.calls == [9, 9, 6], "8 coalitions as 3 + 3 + 2 at B = 3"
    bt = (torch.full_like(xs[0], -0.5), torch.zeros_like(xs[1]), bases[2])
    with torch.no_grad():
        for s in range(8):
            want = m(*[x if s >> i & 1 else b for i, (x, b) in enumerate(zip(xs, bt))]).gather(1, y)[:, 0]
            assert torch.allclose(vals[s], want, rtol=1e-5, atol=1e-6), s
    m.calls.clear()
    one, _ = modal_coalitions(m, xs, y, baselines=bases, chunk=1, sparse=False)
    assert m.calls == [3] * 8 and torch.allclose(one, vals, rtol=1e-5, atol=1e-6)
    ms = modal_shapley(m, xs, y, baselines=bases, chunk=8, sparse=False)
    assert isinstance(ms, ModalShapley) and ms.phi.shape == (3, 3) and ms.interaction.shape == (3, 3, 3)
    assert ms.phi.dtype == ms.interaction.dtype == ms.loo.dtype == ms.solo.dtype == torch.float64
    assert torch.equal(ms.v_full, ms.values[-1]) and torch.equal(ms.v_empty, ms.values[0])
    np.testing.assert_allclose(ms.phi.sum(1).numpy(), (ms.v_full.double() - ms.v_empty.double()).numpy(), atol=1e-14)
    tgt0 = (y[:, 0] == 0).numpy()
    assert np.abs(ms.interaction.numpy()[tgt0, 0, 2]).min() > 1e-3, "logit 0 couples inputs 0 and 2"
    np.testing.assert_allclose(ms.interaction.numpy()[:, 0, 1], 0.0, atol=1e-6)
    m.calls.clear()
    grp = modal_shapley(m, xs, y, baselines=bases, players=[[0, 2], [1]], chunk=8, sparse=False)
    assert m.calls == [12] and grp.phi.shape == (3, 2) and grp.values.shape == (4, 3)
    assert torch.allclose(grp.values, ms.values[[0, 5, 2, 7]], rtol=1e-5, atol=1e-6)
    assert all(p.requires_grad and p.grad is None for p in m.parameters())


def test_registration():
    from oaprogressionmmf_amd.run import explain_epoch
    from oaprogressionmmf_amd.run._explain import EXPLAIN_FNS
    assert "modal_shapley" in EXPLAIN_FNS and len(set(EXPLAIN_FNS)) == len(EXPLAIN_FNS)
    with pytest.raises(ValueError, match="Unknown explain_fn"):
        explain_epoch(None, [], ("a",), explain_fn="shapley")
    with pytest.raises(ValueError, match="takes no explain_kwargs"):
        explain_epoch(None, [], ("a",), explain_fn="modal_abl", explain_kwargs={"players": None})
    assert explain_epoch(None, [], ("a",), explain_fn="modal_shapley", explain_kwargs={"sparse": False}) == {}


def test_explain_epoch_plumbing_on_a_stub(twin_fold):
    from oaprogressionmmf_amd.run import ModalShapley, ensemble_explain_foldw, explain_epoch, modal_shapley
    m, (xs, y) = _stub(), _inputs()
    modals = ("xr_pa", "cor_iw_tse", "clin")             # (names the loader convention knows; the stub does not care)
    loader = [{**{f"image__{mm}": x[lo:hi] for mm, x in zip(modals, xs)}, "target": y[lo:hi],
               ("-", "exam_knee_id"): [f"k{j}" for j in range(lo, hi)]} for lo, hi in ((0, 2), (2, 3))]
    seen = []

    def sink(ids, mods, ms):
        assert list(mods) == list(modals) and isinstance(ms, ModalShapley)
        seen.append((list(ids), ms))
    kw = dict(baselines=0.5, chunk=4, sparse=False)
    acc = explain_epoch(m, loader, modals, device="cpu", explain_fn="modal_shapley", sink=sink, explain_kwargs=kw)
    assert list(acc.keys()) == ["exam_knee_id", "target", "modal_names", "shap_attrs", "shap_percent", "shap_interactions", "shap_loo",
                                "shap_solo", "shap_delta"]
    assert acc["exam_knee_id"] == ["k0", "k1", "k2"] and [i for ids, _ in seen for i in ids] == ["k0", "k1", "k2"]
    assert m.calls == [8, 8, 4, 4], "per batch 8 coalitions in chunks of 4 (B = 2, then 1)"
    want = modal_shapley(m, xs, y, **kw)
    np.testing.assert_allclose(np.asarray(acc["shap_attrs"]), want.phi.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(np.asarray(acc["shap_interactions"]), want.interaction.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(np.asarray(acc["shap_loo"]), want.loo.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(np.asarray(acc["shap_solo"]), want.solo.numpy(), rtol=1e-4, atol=1e-6)
    assert np.asarray(acc["shap_interactions"]).shape == (3, 3, 3) and np.abs(np.asarray(acc["shap_delta"])).max() < 1e-14
    np.testing.assert_allclose(np.asarray(acc["shap_percent"]).sum(1), 100.0, atol=2e-3)
    assert not any(torch.is_tensor(v) for vals in acc.values() for v in vals), "the returned lists hold no tensors"
    ens = ensemble_explain_foldw({0: acc, 1: acc}, prefix="shap")
    np.testing.assert_allclose(np.asarray(ens["shap_percent"]) * 100.0, acc["shap_percent"], atol=2e-3)
    m.calls.clear()
    grp = explain_epoch(m, loader, modals, device="cpu", explain_fn="modal_shapley", explain_kwargs=dict(kw, players=[[0, 1], [2]]))
    assert np.asarray(grp["shap_attrs"]).shape == (3, 2) and m.calls == [8, 4], "explain_kwargs reach the function"
