#!/usr/bin/env python3
"""Generate fixture F16 (tests/golden/f16_gradcam.npz): Grad-CAM maps of the REFERENCE model.

F13 / F15's configuration (XR1MR2C1CnnTrf, XR 160 x 160, MRI 96 x 96 x 6 and 96 x 96 x 5, depth 1, output_type "main", B = 3,
seed 77, procedural weights, eval mode), with the target classes set to (1, 0, 1): the seed's own draw is one class for all three
samples, and the comparison should gather a different logit per sample.  A forward hook on child 7 (layer4) of _fe0 / _fe1 / _fe2 keeps the last feature map A
and its gradient dA (retain_grad) of the scalar sum_b logit[b, y_b].  Written:
  * cam64:<i>   the float64 signed low-resolution maps  sum_c mean_yx(dA)_c * A_c  of input i: (3, 5, 5), (18, 3, 3), (15, 3, 3),
                slice image n = b * S + s as the reference folds the volumes ("b ch r c s -> (b s) ch r c");
  * e32         per input, the relative L2 distance of the reference's own float32 maps from those;
  * pos_max     (3, B): the largest value of every (input, sample)'s maps -- asserted positive here, so the ReLU'd maps of the
                tests are not empty;
  * pos_frac    per input, the fraction of positive map values.
Outputs only -- no reference source, bytecode or pickle.

Usage:  python tests/golden/make_golden_gradcam.py
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


def main():
    t0 = time.time()
    km = import_reference()[0]
    cfg = P.cfg_full(xr=(160, 160), mr1=(96, 96, 6), mr2=(96, 96, 5), depth=1)
    cfg["output_type"] = "main"
    B, seed = 3, 77
    y = torch.tensor([[1], [0], [1]])           # mixed classes (the seed's own draw is class 0 three times)
    assert y.shape == (B, 1) and len(set(y.flatten().tolist())) > 1

    def run(dt):
        torch.manual_seed(0)
        m = km.dict_models[cfg["name"]](config=Cfg(cfg), path_weights=None)
        P.fill_state_dict(m.state_dict())
        m = m.to(dt).eval()
        kept = {}

        def keep(i):
            def hook(mod, args, out):
                out.retain_grad()
                kept[i] = out
            return hook
        handles = [getattr(m, f"_fe{i}")[7].register_forward_hook(keep(i)) for i in range(3)]
        xs = [t(a).to(dt) for a in P.model_inputs(cfg, B, seed)]
        logits = m(*xs).reshape(B, -1)
        logits.gather(1, y).sum().backward()
        for h in handles:
            h.remove()
        cams = []
        for i in range(3):
            A, dA = kept[i].detach(), kept[i].grad.detach()
            cams.append((A * dA.mean(dim=(2, 3), keepdim=True)).sum(dim=1))
        return logits.detach(), cams

    lg32, cam32 = run(torch.float32)
    lg64, cam64 = run(torch.float64)
    out = {"B": np.int64(B), "seed": np.int64(seed), "cfg_json": np.array(json.dumps(cfg)),
           "torch_version": np.array(torch.__version__), "target": y.numpy(), "logits64": lg64.numpy(),
           "e32": np.array([_rel(a, b) for a, b in zip(cam32, cam64)])}
    pos_max = np.stack([c.reshape(B, -1).max(dim=1).values.numpy() for c in cam64])
    assert (pos_max > 0).all(), f"a (input, sample) without a positive Grad-CAM value -- choose another seed: {pos_max}"
    out["pos_max"] = pos_max
    out["pos_frac"] = np.array([float((c > 0).double().mean()) for c in cam64])
    for i, c in enumerate(cam64):
        out[f"cam64:{i}"] = c.numpy()
    np.savez_compressed(HERE / "f16_gradcam.npz", **out)
    print(f"  shapes {[tuple(c.shape) for c in cam64]}  e32 {out['e32']}  positive {out['pos_frac']}")
    print(f"  wrote f16_gradcam.npz ({(HERE / 'f16_gradcam.npz').stat().st_size / 1024:.1f} KiB) in {time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
