"""The occlusion figures of DESIGN 3.27: one run.occlusion call with sparse=True (only the touched slice images are encoded again)
next to sparse=False (every occluded copy encoded in full) and next to a naive loop of modal_ablation-style forwards over the same
windows (a torch copy of the input with the window overwritten, one forward per window), eval mode, one GPU.  Device-event timing,
5 warm-up and 20 timed calls per side, the sides alternating in one process; the median.
  python scripts/bench_occlusion.py mr1     MR1CnnTrf, one 128 x 128 x 32 volume per sample, 64 x 64 x 8 windows (16 of them)
  python scripts/bench_occlusion.py fusion  XR1MR2C1CnnTrf: XR 160^2, MRI 128 x 128 x 32 and 128 x 128 x 16, the clinical vector
                                            (4 + 16 + 8 + 3 windows)
  python scripts/bench_occlusion.py         both"""
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch
import procedural as P
from oaprogressionmmf_amd.config import ConfigDict
from oaprogressionmmf_amd.models import dict_models
from oaprogressionmmf_amd.run import occlusion, occlusion_windows, touched_images
from oaprogressionmmf_amd.run._explain import _forward_main
from oaprogressionmmf_amd.run._gradcam import _view_of, slice_dims
from oaprogressionmmf_amd.run._occlusion import _window

WARM, RUNS, B, CHUNK = 5, 20, 2, 4
dev = torch.device("cuda:0")


def alternate(fns):
    for _ in range(WARM):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(RUNS):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms], [(min(m), max(m)) for m in ms]


def naive(model, xs, y, wins, base):
    """what a caller had before: per window a copy of the input with the box overwritten, and one plain forward"""
    tgt = y.reshape(-1, 1)
    with torch.no_grad():
        f0 = _forward_main(model, xs).gather(1, tgt)
        out = []
        for m, w in enumerate(wins):
            if w is None:
                continue
            for k in range(occlusion_windows(xs[m].shape, w)[1]):
                pt = xs[m].clone()
                pt[(slice(None),) + tuple(slice(lo, hi) for lo, hi in _window(xs[m].shape, w, None, k))] = base
                out.append(f0 - _forward_main(model, tuple(pt if i == m else x for i, x in enumerate(xs))).gather(1, tgt))
    return out


def run(name, cfg, wins):
    cfg["output_type"] = "main"
    model = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)
    P.fill_state_dict(model.state_dict())
    model = model.to(dev).eval()
    xs = [torch.from_numpy(a).to(dev) for a in P.model_inputs(cfg, B, seed=1234)]
    y = torch.from_numpy(P.make_target("target", B, 1234)).to(dev).long()
    K = [0 if w is None else occlusion_windows(x.shape, w)[1] for x, w in zip(xs, wins)]
    imgs = [slice_dims(_view_of(model, x), x.shape)[0] if x.dim() in (4, 5) else 0 for x in xs]
    dense = sum(K) * sum(imgs)
    sparse = sum(len(touched_images(_view_of(model, x), x.shape, w, None, k)) for x, w, n in zip(xs, wins, K) if x.dim() in (4, 5)
                 for k in range(n))
    (ts, td, tn), sp = alternate([lambda: occlusion(model, xs, y, wins, baselines=-0.5, chunk=CHUNK, sparse=True),
                                  lambda: occlusion(model, xs, y, wins, baselines=-0.5, chunk=CHUNK, sparse=False),
                                  lambda: naive(model, xs, y, wins, -0.5)])
    print(f"{name}: {cfg['name']} batch {B}, {sum(K)} windows {K}, chunk {CHUNK}: sparse {ts:8.1f} ms [{sp[0][0]:.1f}, {sp[0][1]:.1f}]; "
          f"dense {td:8.1f} ms [{sp[1][0]:.1f}, {sp[1][1]:.1f}]; naive loop {tn:8.1f} ms [{sp[2][0]:.1f}, {sp[2][1]:.1f}]; "
          f"dense / sparse {td / ts:.2f}, naive / sparse {tn / ts:.2f}; slice encodes per sample behind the intact forward: dense "
          f"{dense}, sparse {sparse} (ratio {dense / sparse:.2f}); peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


which = sys.argv[1] if len(sys.argv) > 1 else "both"
if which in ("mr1", "both"):
    run("mr1", P.cfg_mr1(shape=(128, 128, 32), depth=1), [(1, 64, 64, 8)])
if which in ("fusion", "both"):
    run("fusion", P.cfg_full(xr=(160, 160), mr1=(128, 128, 32), mr2=(128, 128, 16), depth=1),
        [(1, 80, 80), (1, 64, 64, 8), (1, 64, 64, 8), (1, 3)])
