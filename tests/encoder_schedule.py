"""One forward and backward of a small KoafTrunk with everything the encoder schedule decides written down -- a test helper:
tests/test_encoder_schedule_gpu.py compares the launch sequence with fixture F19, scripts/encoder_parity.py compares two source
trees over the whole record (launches, bits, allocator traffic).

The trunks are the ones tests/test_models_gpu.py::_recompute_cases builds (procedural weights, seeded input), at the smallest
shapes the trunk tests use, and -- but for one case -- with a parameter arena, so that the weight plane images exist and the
tail-on-load, emit and apply-on-load paths are the ones that run.  Each case runs with lane=None and the side stream off: the
caching allocator then sees one stream and its figures are a function of the schedule alone.
"""
import hashlib

import numpy as np
import torch

import procedural as P

# name -> (arch, input shape, KoafTrunk.recompute, act_dtype, mode, arena?)
# mode "train": train-mode step; "eval_dx": eval(), every parameter frozen, the input asks for its gradient
CASES = {
    "r50_keep": ("resnet50", (2, 1, 96, 112), False, torch.float32, "train", True),
    "r50_rc01": ("resnet50", (2, 1, 96, 112), (0, 1), torch.float32, "train", True),
    "r50_block": ("resnet50", (2, 1, 96, 112), "block", torch.float32, "train", True),
    "rx50_keep": ("resnext50_32x4d", (2, 1, 96, 96), False, torch.float32, "train", True),
    "rx50_rc": ("resnext50_32x4d", (2, 1, 96, 96), True, torch.float32, "train", True),
    "r18_keep": ("resnet18", (2, 1, 64, 96), False, torch.float32, "train", True),
    "r50_bf16": ("resnet50", (2, 1, 96, 112), False, torch.bfloat16, "train", True),
    "r50_eval_dx": ("resnet50", (2, 1, 96, 112), False, torch.float32, "eval_dx", True),
    "r50_noarena": ("resnet50", (2, 1, 96, 112), False, torch.float32, "train", False),
}

# what the schedule decides about a koaf_gemm launch (the tile, the grid and the kernel variant are the library planner's)
SCHEDULE_FIELDS = ("M", "N", "K", "nbatch", "fmt", "a_tf", "b_tf", "act16", "emit")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def _step(name, dev, side):
    """build the case's trunk, run one forward and backward; -> (hashes, launch records, allocator figures)"""
    from oaprogressionmmf_amd import ops
    from oaprogressionmmf_amd.arena import get_arena
    from oaprogressionmmf_amd.models import _encoder
    from oaprogressionmmf_amd.models._core_fes import dict_fes
    arch, shape, rc, adt, mode, arena = CASES[name]
    trunk = _encoder.KoafTrunk(*list(dict_fes[arch](pretrained=False).children())[:-1])
    P.fill_state_dict(trunk.state_dict())
    trunk = trunk.to(dev)
    trunk.recompute, trunk.act_dtype = rc, adt
    x = _t(P.make_input("trunk", shape)).to(dev)
    if mode == "eval_dx":
        trunk.eval()
        for p in trunk.parameters():
            p.requires_grad_(False)
        x.requires_grad_(True)
    else:
        trunk.train()
    if arena:
        get_arena(trunk)
    # (the output's shape does not depend on the schedule: the upstream gradient is made before the measured region)
    C = 512 if arch == "resnet18" else 2048
    gy = _t(P.make_input("trunkg", (shape[0], C, 1, 1))).to(dev)
    was = _encoder.USE_SIDE_STREAM
    _encoder.USE_SIDE_STREAM = side
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_stats()
    ops.launch_log(True)
    try:
        y = trunk(x)
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        launches = ops.launch_log_read()
    finally:
        ops.launch_log(False)
        _encoder.USE_SIDE_STREAM = was
    m1 = torch.cuda.memory_stats()
    mem = dict(allocs=m1["allocation.all.allocated"] - m0["allocation.all.allocated"],
               bytes=m1["allocated_bytes.all.allocated"] - m0["allocated_bytes.all.allocated"],
               peak=m1["allocated_bytes.all.peak"] - m0["allocated_bytes.all.current"])
    hashes = {"y": _sha(y)}
    if x.grad is not None:
        hashes["dx"] = _sha(x.grad)
    for k, p in trunk.named_parameters():
        if p.grad is not None:
            hashes["grad:" + k] = _sha(p.grad)
    for k, b in trunk.named_buffers():
        hashes["buf:" + k] = _sha(b)
    return hashes, launches, mem


def run_case(name, dev, side_pass=False):
    """-> dict(launches = the full ops.launch_log_read() records, hashes = SHA-256 of the output, dx, every parameter gradient and
    every buffer, mem = allocations / bytes allocated / peak bytes allocated over the step); side_pass: a second, fresh trunk
    with the weight gradients on the side stream adds its hashes (hashes_side)"""
    hashes, launches, mem = _step(name, dev, False)
    out = dict(launches=launches, hashes=hashes, mem=mem)
    if side_pass:
        out["hashes_side"] = _step(name, dev, True)[0]
    return out


def schedule_rows(launches):
    """the launch records cut down to SCHEDULE_FIELDS, as lists in launch order"""
    return [[int(r[f]) for f in SCHEDULE_FIELDS] for r in launches]
