#!/usr/bin/env python3
"""Generate fixture F24 (tests/golden/f24_attn_relevance.npz): the attentions of the REFERENCE FeaT and their gradients.

The reference's FeaT, imported by path, on the CPU: B = 2, 8 patches + CLS (n = 9), emb_dim = patch_dim = 32, heads 2 (d = 16), depth 3,
mlp_dim 32, 2 classes, dropout 0, eval mode; default initialisation under torch.manual_seed(24) with the to_qkv weights scaled by 3
(attention rows away from uniform).  The returned attentions get retain_grad() and sum_b logit[b, target_b] is backpropagated, once
in float32 and once in float64 from the same state_dict.  Written:
  * features, target, heads         the input, the classes (1, 0) and the head count
  * sd:<key>                        the float32 state_dict
  * attn32:<l>, dattn32:<l>         the reference's float32 attentions and their gradients, layer l
  * attn64:<l>, dattn64:<l>         the same of the float64 run
  * abar64:<l>                      the float64 twin's mean_h relu(dattn64 * attn64)              (tests/attn_twin.py)
  * rollout64:<fuse>                the twin's A^_L ... A^_1 on attn64, fuse in mean / max / min
  * gradrel64                       the twin's (I + Abar_L) ... (I + Abar_1)
Arrays only -- no reference source, bytecode or pickle.

Usage:  python tests/golden/make_golden_attn_relevance.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
from make_golden import REF, _load_by_path  # noqa: E402
import attn_twin as T  # noqa: E402

B, NP, DIM, HEADS, DEPTH, MLP, NCLS = 2, 8, 32, 2, 3, 32, 2


def main():
    ref = _load_by_path("_ref_core_trf", REF / "koafusion/models/_core_trf.py")
    torch.manual_seed(24)
    kw = dict(num_patches=NP, patch_dim=DIM, emb_dim=DIM, depth=DEPTH, heads=HEADS, mlp_dim=MLP, num_classes=NCLS, emb_dropout=0.,
              mlp_dropout=0.)
    m = ref.FeaT(**kw).eval()
    with torch.no_grad():
        for l in range(DEPTH):
            getattr(m.transformer, f"attn_{l}").to_qkv.weight.mul_(3.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    feats = torch.randn(B, NP, DIM)
    y = torch.tensor([[1], [0]])

    def run(dt):
        mm = ref.FeaT(**kw).to(dt).eval()
        mm.load_state_dict({k: v.to(dt) for k, v in sd.items()})
        out, _, attns = mm(feats.to(dt))
        for a in attns:
            a.retain_grad()
        out.reshape(B, -1).gather(1, y).sum().backward()
        return [a.detach().numpy() for a in attns], [a.grad.numpy() for a in attns]

    a32, g32 = run(torch.float32)
    a64, g64 = run(torch.float64)
    out = {"features": feats.numpy(), "target": y.numpy(), "heads": np.int64(HEADS)}
    out.update({f"sd:{k}": v.numpy() for k, v in sd.items()})
    abar = []
    for l in range(DEPTH):
        assert a32[l].shape == (B, HEADS, NP + 1, NP + 1) and a32[l].dtype == np.float32 and a64[l].dtype == np.float64
        out[f"attn32:{l}"], out[f"dattn32:{l}"], out[f"attn64:{l}"], out[f"dattn64:{l}"] = a32[l], g32[l], a64[l], g64[l]
        abar.append(np.maximum(g64[l] * a64[l], 0.0).mean(axis=1))
        out[f"abar64:{l}"] = abar[-1]
        assert abar[-1].max() > 0
    for fuse in T.FUSE:
        out[f"rollout64:{fuse}"] = T.chain([T.rollout_layer(a, fuse) for a in a64])
    out["gradrel64"] = T.chain(abar, add_identity=True)
    path = HERE / "f24_attn_relevance.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
