"""CPU: fixture F15 (the imported reference's float64 input gradients, tests/golden/make_golden_input_grads.py) pins the oracle:
the oracle's float64 gradients of sum_b logit[b, y_b] with respect to its four inputs, in eval mode and in train mode, equal the
reference's to 1e-9 relative (float64 summation-order slack).  Plus the host side of the input-gradient interface: the four
entry points are declared where the binding reads them, and the fold ensemble merges the "ixg" field family like the
reference's "modal_abl" one."""
import json

import numpy as np
import pytest
import torch

import procedural as P
from common import rel
from input_grads_fixture import load_f15
from oracle import koafusion_cpu as O


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_oracle_input_gradients_match_reference_fixture(mode):
    g = load_f15()
    cfg, B, seed = json.loads(str(g["cfg_json"])), int(g["B"]), int(g["seed"])
    torch.set_num_threads(8)
    y = torch.from_numpy(P.make_target("target", B, seed)).long()
    assert np.array_equal(y.numpy(), g["target"])
    om = O.OracleModel(cfg, fill=P.fill_value, dtype=torch.float64)
    xs = [torch.from_numpy(a).double().requires_grad_(True) for a in P.model_inputs(cfg, B, seed)]
    out = om(*xs, train=mode == "train")
    out = out["main"] if isinstance(out, dict) else out
    assert rel(out.detach().numpy(), g[f"{mode}:logits64"]) < 1e-9
    out.reshape(B, -1).gather(1, y).sum().backward()
    for i, x in enumerate(xs):
        assert x.grad.shape == g[f"g64:{mode}:{i}"].shape
        assert rel(x.grad.numpy(), g[f"g64:{mode}:{i}"]) < 1e-9, (mode, i)
    # the table the GPU bar is stated against: the reference's own float32 distance from these gradients
    assert g[f"e32:{mode}"].shape == (4,) and (g[f"e32:{mode}"] > 0).all()
    assert len(g["eval:e32_keys"]) == len(g["eval:e32_vals"]) > 100


def test_input_gradient_entry_points_are_declared():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    for name in ("koaf_stem_dgrad", "koaf_bn_bwd_finalize_eval", "koaf_slice_unfold", "koaf_rowdot", "koaf_rowdot_ws"):
        assert name in protos, name
    assert _lib.STRUCTS["KoafBnApply"] in [getattr(a, "_type_", None) for a in protos["koaf_stem_dgrad"][1]]


def test_fold_ensemble_takes_a_field_prefix():
    from oaprogressionmmf_amd.run import ensemble_explain_foldw, explain_epoch, saliency_maps
    raw = {0: dict(exam_knee_id=["a", "b"], target=[[1], [0]], modal_names=[["x", "c"]] * 2,
                   ixg_attrs=[[0.3, -0.1], [0.0, 0.2]], ixg_percent=[[75.0, 25.0], [0.0, 100.0]]),
           2: dict(exam_knee_id=["b", "a"], target=[[0], [1]], modal_names=[["x", "c"]] * 2,
                   ixg_attrs=[[0.1, 0.1], [-0.2, 0.2]], ixg_percent=[[50.0, 50.0], [50.0, 50.0]])}
    ens = ensemble_explain_foldw(raw, prefix="ixg")
    assert ens["exam_knee_id"] == ["a", "b"] and ens["ixg_attrs__2"] == [[-0.2, 0.2], [0.1, 0.1]]
    np.testing.assert_allclose(ens["ixg_percent"], [[0.625, 0.375], [0.25, 0.75]], rtol=1e-15)
    renamed = {k: {kk.replace("ixg", "modal_abl"): v for kk, v in d.items()} for k, d in raw.items()}
    assert ensemble_explain_foldw(renamed)["modal_abl_percent"] == ens["ixg_percent"]
    assert explain_epoch(None, [], ("xr_pa",), explain_fn="input_x_grad") == {}
    with pytest.raises(ValueError, match="Unknown explain_fn: grad_cam"):
        explain_epoch(None, [], ("xr_pa",), explain_fn="grad_cam")
    with pytest.raises(ValueError):
        saliency_maps(None, (), 0, kind="integrated_gradients")
