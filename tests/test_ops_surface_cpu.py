"""The surface of `oaprogressionmmf_amd.ops` after its split into a package: every name the single-file module had is still
reachable as `ops.<name>` with the signature it had, the live profiler still logs into the list installed on the package, and
the argument checks the families now share refuse in the words the per-family copies used.

golden/ops_surface.json is the sorted {name: str(inspect.signature) or null} of the single-file module's non-dunder attributes
(functions and classes carry a signature; constants, ctypes structures and cached functions null), written once from the last
commit that had ops.py.  Left out of it: the modules ops.py happened to import (torch, np, ...) and its two private checkers
_metric_i32 / _clin_f64, which ops/_base.py's check_tensor replaces.  Names added later are not constrained."""
import inspect
import json
from pathlib import Path

import pytest
import torch

from oaprogressionmmf_amd import ops

SURFACE = json.loads((Path(__file__).parent / "golden" / "ops_surface.json").read_text())


def test_every_name_and_signature_is_still_on_ops():
    assert len(SURFACE) == 159 and list(SURFACE) == sorted(SURFACE)
    missing = [name for name in SURFACE if not hasattr(ops, name)]
    assert not missing, missing
    moved = {name: (sig, str(inspect.signature(getattr(ops, name)))) for name, sig in SURFACE.items()
             if sig is not None and str(inspect.signature(getattr(ops, name))) != sig}
    assert not moved, moved


def test_private_names_import_and_state_exists_once():
    from oaprogressionmmf_amd.ops import _ptr, _stream
    assert _stream is ops._stream is ops._base._stream and _ptr is ops._base._ptr
    assert ops._dy_planes is ops.conv._dy_planes and ops.check is ops._base.check
    assert ops._STATUS_BY_DEV is ops._base._STATUS_BY_DEV and ops._window_ws is ops.inputs._window_ws
    assert ops.CONV_F16 is ops.conv.CONV_F16 and not hasattr(ops._base, "PROFILE")
    for fam in (ops.conv, ops.dense):                   # the families that profile share _base's hooks
        assert fam._prof_begin is ops._base._prof_begin and fam._prof_end is ops._base._prof_end
    assert ops._STATUS is ops._base._STATUS and ops._STATUS_DEV is ops._base._STATUS_DEV      # (read through, not copied)


def test_shared_argument_checks_keep_the_families_words():
    """the checks need no device to refuse: texts as the per-family copies worded them, masks from the tables' keys"""
    from oaprogressionmmf_amd.ops._base import FlagWord, check_tensor, out_buffer
    like = torch.zeros(1)
    with pytest.raises(ops.KoafError, match=r"^f: idx is a contiguous int32 tensor \[2, 3\] on the scores' device, got \(\(3,\), torch.float32"):
        check_tensor("f", "idx", torch.zeros(3), torch.int32, (2, 3), like, where="the scores' device")
    with pytest.raises(ops.KoafError, match=r"^f: sw is a non-empty contiguous fp64 tensor on the HIP device, got <class 'list'>"):
        check_tensor("f", "sw", [], torch.float64, nonempty=True)
    with pytest.raises(ops.KoafError, match="non-empty"):
        check_tensor("f", "sw", torch.zeros(0, dtype=torch.float64), torch.float64, None, like, nonempty=True)
    with pytest.raises(ops.KoafError, match="on the HIP device"):             # no `like`: a HIP device is asked for
        check_tensor("f", "x", torch.zeros(2, dtype=torch.int32), torch.int32)
    check_tensor("f", "x", torch.zeros(2, dtype=torch.int32), torch.int32, (2,), like)
    with pytest.raises(ops.KoafError, match=r"^f: out is contiguous fp64 \[80\] on the scores' device, got \(79,\) torch.float64"):
        out_buffer("f", torch.zeros(79, dtype=torch.float64), (80,), torch.float64, like, "the scores' device")
    mine = torch.zeros(80, dtype=torch.float64)
    assert out_buffer("f", mine, (80,), torch.float64, like, "x") is mine
    fresh = out_buffer("f", None, (2, 2), torch.int64, like, "x", fresh=torch.zeros)
    assert fresh.dtype == torch.int64 and fresh.shape == (2, 2) and not fresh.any()
    for table, mask in ((ops.METRICS_FLAG_TEXT, 7), (ops.SERIES_FLAG_TEXT, 3), (ops.CLIN_FLAG_TEXT, 15)):
        assert FlagWord(table).mask == mask
    ops.metrics_raise(0), ops.metrics_raise(8), ops.series_raise(4), ops.clin_raise(16)      # bits outside a table pass
    with pytest.raises(ValueError, match=r"^Input contains NaN or infinity\.; an index of the resampling matrix lies outside \[0, n\)$"):
        ops.metrics_raise(5)
    fw = FlagWord({1: "one", 2: "two"}, "the scores' device")
    word = fw.new(like.device)
    assert word.dtype == torch.int32 and word.shape == (1,) and int(word) == 0
    with fw.own("f", word, like) as flag:               # the caller's word: handed through, never read back
        assert flag is word
        flag[0] = 3
    with pytest.raises(ValueError, match="^two$"):      # an own word: read back and raised from when the block is done
        with fw.own("f", None, like) as flag:
            flag[0] = 2
    with pytest.raises(ops.KoafError, match=r"flag is a contiguous int32 tensor \[1\] on the scores' device"):
        with fw.own("f", torch.zeros(2, dtype=torch.int32), like):
            pass


def test_profile_installed_on_the_package_is_the_one_logged_into(monkeypatch):

    made = []

    class Event(object):
        def __init__(self, enable_timing=False):
            made.append(self)

        def record(self):
            pass

    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(ops, "PROFILE", None)
    assert ops.conv._prof_begin() is None
    ops.conv._prof_end(None, "gemm", 1.0)
    assert made == []
    log = []
    ops.PROFILE = log                                   # as bench.py installs it: on the package
    e0 = ops.conv._prof_begin()
    ops.conv._prof_end(e0, "gemm", 2.0, "tag", elems=3, mpp=3)
    assert len(log) == 1 and len(made) == 2
    assert log[0] == ("gemm", 2.0, made[0], made[1], "tag", 12.0, 3) and len(log[0]) == 7
    ops.PROFILE = None
    assert ops.dense._prof_begin() is None and len(made) == 2
