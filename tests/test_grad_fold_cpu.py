"""No GPU: host side of gradient accumulation and global-norm clipping -- the C ABI is declared, exported and checks its
arguments; the workspace function sizes like every other reduction's; the Python layers refuse CPU tensors (there is no
fallback) and unknown norm types; the micro-batch weights are the sample shares."""
import ctypes
import math

import pytest
import torch

NEW_ENTRY_POINTS = ("koaf_grad_fold", "koaf_grad_norm_part", "koaf_grad_norm_final", "koaf_grad_scale", "koaf_grad_norm_ws")


def test_entry_points_declared_and_exported():
    from oaprogressionmmf_amd import _lib
    protos = _lib.parse_header()
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
        assert hasattr(handle, name), name
    assert protos["koaf_grad_norm_ws"][0] is ctypes.c_int64
    assert _lib.lib().koaf_version() == _lib.defines()["KOAF_VERSION"]


def test_null_arguments_come_back_as_errors():
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    assert L.koaf_grad_fold(None, None, 16, 1.0, 0, 0, None, None) != 0
    assert b"koaf_grad_fold" in L.koaf_last_error()
    assert L.koaf_grad_norm_part(None, 16, 0, None, None) != 0
    assert b"koaf_grad_norm_part" in L.koaf_last_error()
    assert L.koaf_grad_norm_final(None, 2, 0, 1.0, None, None, None) != 0
    assert b"koaf_grad_norm_final" in L.koaf_last_error()
    assert L.koaf_grad_scale(None, 16, None, None) != 0
    assert b"koaf_grad_scale" in L.koaf_last_error()


def test_workspace_size():
    from oaprogressionmmf_amd import _lib
    L = _lib.lib()
    assert L.koaf_grad_norm_ws(0) == 0 and L.koaf_grad_norm_ws(-5) == 0
    sizes = [L.koaf_grad_norm_ws(n) for n in (1, 1000, 10 ** 6, 389 * 10 ** 6)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[1]
    assert all(s % 2 == 0 for s in sizes)                      # whole 8-byte slots, counted in floats


def test_cpu_parameters_are_refused():
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd._lib import KoafError
    from oaprogressionmmf_amd.run import GradientFold
    from oaprogressionmmf_amd.various import clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(5))
    p.grad = torch.full((5,), 2.0)
    with pytest.raises(KoafError):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(KoafError):
        clip_grad_norm_(p, 1.0, norm_type=float("inf"))
    assert torch.equal(p.grad, torch.full((5,), 2.0))
    with pytest.raises(RuntimeError):
        GradientFold(torch.nn.Linear(3, 2))
    x = torch.zeros(8)
    for call in (lambda: ops.grad_fold(x, x.clone(), 1.0, 1), lambda: ops.grad_scale(x, x[:1]),
                 lambda: ops.grad_norm_part(x, torch.zeros(1, dtype=torch.float64))):
        with pytest.raises(KoafError):
            call()


def test_unknown_norm_type_raises():
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.various import clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(5))
    p.grad = torch.ones(5)
    for nt in (3, 1.0, 0):
        with pytest.raises(ValueError):
            clip_grad_norm_([p], 1.0, norm_type=nt)
    assert ops.norm_kind(2) == 0 and ops.norm_kind(2.0) == 0 and ops.norm_kind(math.inf) == 1 and ops.norm_kind("inf") == 1


def test_micro_batch_weights():
    from oaprogressionmmf_amd.run import micro_batch_weights
    assert micro_batch_weights([3, 3, 2]) == [0.375, 0.375, 0.25]
    assert micro_batch_weights([8]) == [1.0]
    for sizes in ([5, 3, 3], [7, 7, 7, 1], [1] * 13):
        w = micro_batch_weights(sizes)
        assert abs(math.fsum(w) - 1.0) <= 2 ** -52 * len(w), (sizes, w)
        assert all(abs(wi - b / sum(sizes)) == 0.0 for wi, b in zip(w, sizes))
    for bad in ([], [4, 0], [0], [2, -1]):
        with pytest.raises(ValueError):
            micro_batch_weights(bad)


def test_train_step_signature_keeps_its_defaults():
    import inspect
    from oaprogressionmmf_amd.run import GraphedTrainStep, train_step, train_step_accum
    for fn in (train_step, GraphedTrainStep.__init__):
        par = inspect.signature(fn).parameters["max_grad_norm"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    sig = inspect.signature(train_step_accum).parameters
    assert list(sig)[:6] == ["model", "loss_fn", "optimizer", "micro_batches", "downscale", "max_grad_norm"]
