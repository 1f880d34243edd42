#!/usr/bin/env python3
"""Generate fixture F15 (tests/golden/f15_input_grads*.npz): the REFERENCE model's input gradients.

F13's configuration (XR1MR2C1CnnTrf, XR 160 x 160, MRI 96 x 96 x 6 and 96 x 96 x 5, depth 1, output_type "main", B = 3, seed 77);
the differentiated scalar is sum_b logit[b, y_b], in eval mode and in train mode.  Written:
  * g64:<mode>:<i>        the reference's float64 gradient with respect to input i (mode = eval | train);
  * e32:<mode>            per input, the relative L2 distance of the reference's own float32 gradient from that float64 one;
  * eval:e32_keys / eval:e32_vals   the same distance per PARAMETER for the eval-mode pass (make_golden.fp64_twin's table);
  * <mode>:logits64       the float64 logits.
Outputs only -- no reference source, bytecode or pickle.  The float64 image gradients are 6 MB, more than one committed file
may hold: f15_input_grads.npz keeps the small entries and the layout of the large ones, whose concatenated values follow in
f15_input_grads.partNN.npz slices of PART elements (tests/input_grads_fixture.py reads them back).

Usage:  python tests/golden/make_golden_input_grads.py
"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from make_golden import Cfg, P, _rel, import_reference, t  # noqa: E402

PART = 120000          # float64 elements per part file (960 kB)


def main():
    t0 = time.time()
    km = import_reference()[0]
    cfg = P.cfg_full(xr=(160, 160), mr1=(96, 96, 6), mr2=(96, 96, 5), depth=1)
    cfg["output_type"] = "main"
    B, seed = 3, 77
    y = t(P.make_target("target", B, seed)).long()

    def build(dt):
        torch.manual_seed(0)
        m = km.dict_models[cfg["name"]](config=Cfg(cfg), path_weights=None)
        P.fill_state_dict(m.state_dict())
        return m.to(dt)

    def run(dt, train):
        m = build(dt)
        m.train(train)
        xs = [t(a).to(dt).requires_grad_(True) for a in P.model_inputs(cfg, B, seed)]
        logits = m(*xs).reshape(B, -1)
        logits.gather(1, y).sum().backward()
        return (logits.detach(), [x.grad.detach() for x in xs],
                {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None})

    small = {"B": np.int64(B), "seed": np.int64(seed), "cfg_json": np.array(json.dumps(cfg)),
             "torch_version": np.array(torch.__version__), "target": y.numpy()}
    big = {}
    for mode, train in (("eval", False), ("train", True)):
        lg32, gx32, gp32 = run(torch.float32, train)
        lg64, gx64, gp64 = run(torch.float64, train)
        small[f"{mode}:logits64"] = lg64.numpy()
        small[f"e32:{mode}"] = np.array([_rel(a, b) for a, b in zip(gx32, gx64)])
        for i, g in enumerate(gx64):
            big[f"g64:{mode}:{i}"] = g.numpy()
        if mode == "eval":
            keys = [k for k in gp32 if k in gp64]
            small["eval:e32_keys"] = np.array(keys)
            small["eval:e32_vals"] = np.array([_rel(gp32[k], gp64[k]) for k in keys])
        print(f"  {mode}: e32 per input = {small[f'e32:{mode}']}  ({time.time() - t0:.0f}s)")
    names = list(big)
    small["big_names"] = np.array(names)
    small["big_shapes_json"] = np.array(json.dumps([list(big[k].shape) for k in names]))
    flat = np.concatenate([big[k].reshape(-1) for k in names])
    nparts = (flat.size + PART - 1) // PART
    small["nparts"] = np.int64(nparts)
    for old in HERE.glob("f15_input_grads*.npz"):
        old.unlink()
    np.savez_compressed(HERE / "f15_input_grads.npz", **small)
    for k in range(nparts):
        np.savez_compressed(HERE / f"f15_input_grads.part{k:02d}.npz", data=flat[k * PART:(k + 1) * PART])
    sizes = [f.stat().st_size for f in sorted(HERE.glob("f15_input_grads*.npz"))]
    print(f"  wrote f15_input_grads.npz + {nparts} parts ({sum(sizes) / 2 ** 20:.1f} MiB, largest {max(sizes) / 1024:.0f} KiB) "
          f"in {time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
