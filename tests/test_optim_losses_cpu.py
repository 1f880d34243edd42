"""No GPU: host side of the native SGD / RMSprop / BCE registry entries -- the C ABI is declared, exported and checks its
arguments; the classes validate their constructor arguments like torch's, refuse CPU tensors, and keep torch's state_dict
layout (torch.optim's own state loads and comes back unchanged)."""
import ctypes
import subprocess

import pytest
import torch

NEW_ENTRY_POINTS = ("koaf_sgd_step", "koaf_rmsprop_step", "koaf_optim_hyper", "koaf_bce_loss", "koaf_bce_ws")


def test_registry_classes_are_native():
    from oaprogressionmmf_amd.various import dict_losses, dict_optimizers
    for reg, keys in ((dict_optimizers, ("SGD", "RMSprop")), (dict_losses, ("bce_loss", "bce_wlogits_loss"))):
        for k in keys:
            assert reg[k].__module__.startswith("oaprogressionmmf_amd"), (k, reg[k].__module__)


def test_entry_points_declared_exported_and_versioned():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW_ENTRY_POINTS:
        assert hasattr(handle, name), name
    assert _lib.lib().koaf_version() >= 200


def test_library_exports_exactly_the_declared_symbols():
    from oaprogressionmmf_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("koaf_") and " T " in ln}
    assert exported == set(_lib.parse_header())


def test_null_arguments_come_back_as_errors():
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    assert L.koaf_sgd_step(None, None, None, 16, 0.1, 0.9, 0.0, 0.0, 0, 0, 0, None, None) != 0
    assert b"koaf_sgd_step" in L.koaf_last_error()
    assert L.koaf_rmsprop_step(None, None, None, None, None, 16, 0.01, 0.99, 1e-8, 0.0, 0.0, 0, None, None) != 0
    assert b"koaf_rmsprop_step" in L.koaf_last_error()
    assert L.koaf_optim_hyper(None, None, None, None) != 0
    assert b"koaf_optim_hyper" in L.koaf_last_error()
    assert L.koaf_bce_loss(None, None, None, None, None, None, 16, 1, 0, 1, None, None) != 0
    assert b"koaf_bce_loss" in L.koaf_last_error()
    assert L.koaf_bce_ws(64) == 0 and L.koaf_bce_ws(2 * 3 * 70 * 71) > 0


def test_constructor_validation_matches_torch():
    from oaprogressionmmf_amd.various import dict_optimizers
    p = [torch.nn.Parameter(torch.zeros(3))]
    for name, ref in (("SGD", torch.optim.SGD), ("RMSprop", torch.optim.RMSprop)):
        for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4)):
            for cls in (ref, dict_optimizers[name]):
                with pytest.raises(ValueError):
                    cls(p, **kw)
    for kw in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        for cls in (torch.optim.SGD, dict_optimizers["SGD"]):
            with pytest.raises(ValueError):
                cls(p, lr=0.1, **kw)
    for name in ("SGD", "RMSprop"):
        with pytest.raises(ValueError):
            dict_optimizers[name](p, differentiable=True)
        opt = dict_optimizers[name](p, foreach=True, maximize=True)          # accepted; foreach ignored
        assert opt.param_groups[0]["maximize"] is True and opt.capturable is False
        assert dict_optimizers[name](p, capturable=True).capturable is True
    # torch's defaults
    g = dict_optimizers["SGD"](p).param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) == (1e-3, 0, 0, 0, False)
    g = dict_optimizers["RMSprop"](p).param_groups[0]
    assert (g["lr"], g["alpha"], g["eps"], g["weight_decay"], g["momentum"], g["centered"]) == (1e-2, 0.99, 1e-8, 0, 0, False)


@pytest.mark.parametrize("name", ["SGD", "Adam", "AdamW", "RMSprop"])
def test_cpu_parameter_raises(name):
    from oaprogressionmmf_amd.various import dict_optimizers
    p = torch.nn.Parameter(torch.zeros(5))
    opt = dict_optimizers[name]([p], lr=0.1)
    opt.step()                                   # no gradient: nothing to do, like torch
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(5))
    with pytest.raises(RuntimeError, match="arena parameters only"):
        dict_optimizers[name]([p], lr=0.1, capturable=True).step()


def test_bce_losses_refuse_cpu_tensors_and_mismatched_shapes():
    from oaprogressionmmf_amd._lib import KoafError
    from oaprogressionmmf_amd.various import dict_losses
    x, t = torch.full((4, 3), 0.5), torch.ones(4, 3)
    for key in ("bce_loss", "bce_wlogits_loss"):
        with pytest.raises(KoafError):
            dict_losses[key]()(x, t)
        with pytest.raises(ValueError):
            dict_losses[key]()(x, torch.ones(4))
        with pytest.raises(ValueError):
            dict_losses[key](reduction="median")
    # weight / pos_weight are buffers: they follow .to(device) and show in the state dict, as in torch
    m = dict_losses["bce_wlogits_loss"](weight=torch.ones(3), pos_weight=[1.0, 2.0, 3.0])
    assert set(dict(m.named_buffers())) == {"weight", "pos_weight"} and m.pos_weight.dtype == torch.float32
    assert set(dict(dict_losses["bce_loss"](weight=[0.5]).named_buffers())) == {"weight"}


def _two_cpu_steps(opt, params):
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()


@pytest.mark.parametrize("name,kw", [("SGD", dict(lr=0.1, momentum=0.9)),
                                     ("RMSprop", dict(lr=0.01, centered=True, momentum=0.5))])
def test_torch_state_dict_round_trip(name, kw):
    """torch.optim's state after two CPU steps loads into the native class and comes back with the same keys, shapes and
    values -- host logic only, no step taken (the state is parked until the parameters' placement is known)"""
    from oaprogressionmmf_amd.various import dict_optimizers
    shapes = [(4, 3, 3, 3), (7,), (2, 5)]
    params = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i))) for i, s in enumerate(shapes)]
    ref = getattr(torch.optim, name)(params[:2], **kw)               # (the third parameter is never updated: no entry)
    ref.add_param_group(dict(params=[params[2]]))
    params[2].requires_grad_(False)
    _two_cpu_steps(ref, params[:2])
    sd = ref.state_dict()
    assert sorted(sd["state"]) == [0, 1]
    opt = dict_optimizers[name]([dict(params=params[:2]), dict(params=[params[2]])], **kw)
    opt.load_state_dict(sd)
    back = opt.state_dict()
    assert sorted(back["state"]) == [0, 1]
    want = {"SGD": {"momentum_buffer"}, "RMSprop": {"step", "square_avg", "momentum_buffer", "grad_avg"}}[name]
    for i in (0, 1):
        assert set(back["state"][i]) == set(sd["state"][i]) == want
        for k in want:
            a, b = torch.as_tensor(back["state"][i][k]), torch.as_tensor(sd["state"][i][k])
            assert a.shape == b.shape and torch.equal(a.float(), b.float()), (i, k)
    assert [g["params"] for g in back["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    for k, v in kw.items():
        assert back["param_groups"][0][k] == v
    # ... and the way back: torch's class takes the native class's export
    ref2 = getattr(torch.optim, name)([dict(params=params[:2]), dict(params=[params[2]])], **kw)
    ref2.load_state_dict(back)
    _two_cpu_steps(ref2, params[:2])


def test_sgd_without_momentum_keeps_no_state():
    from oaprogressionmmf_amd.various import dict_optimizers
    p = torch.nn.Parameter(torch.zeros(3))
    ref = torch.optim.SGD([p], lr=0.1)
    _two_cpu_steps(ref, [p])
    opt = dict_optimizers["SGD"]([p], lr=0.1)
    opt.load_state_dict(ref.state_dict())
    assert opt.state_dict()["state"] == {}
