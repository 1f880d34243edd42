"""time of one explain pass per batch: input gradients (one forward + one backward, parameters frozen, the trunks' data gradient
down to the images) next to the modality ablation (M + 1 forwards), eval mode.
  python scripts/bench_explain.py f15      XR1MR2C1CnnTrf at fixture F15's size (XR 160^2, MRI 96x96x6 / 96x96x5, batch 3)
  python scripts/bench_explain.py syn3     bench.py's headline shapes (XR 310^2 + 3 x MRI 160x384x384, batch 8, its recompute policy)"""
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch
import procedural as P
import bench
from oaprogressionmmf_amd.config import ConfigDict
from oaprogressionmmf_amd.models import dict_models
from oaprogressionmmf_amd.run import input_gradients, modal_ablation

which = sys.argv[1] if len(sys.argv) > 1 else "f15"
dev = torch.device("cuda:0")
if which == "f15":
    cfg, B, policy = P.cfg_full(xr=(160, 160), mr1=(96, 96, 6), mr2=(96, 96, 5), depth=1), 3, "none"
else:
    cfg, B, policy = bench.workload_cfg(which)
shapes = cfg.pop("_tensor_shapes", None)
cfg["output_type"] = "main"
model = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)
P.fill_state_dict(model.state_dict())
model = model.to(dev).eval()
bench.apply_recompute(model, policy)
xs = [torch.from_numpy(a).to(dev) for a in P.model_inputs(dict(cfg, input_size=shapes) if shapes else cfg, B, seed=1234)]
y = torch.from_numpy(P.make_target("target", B, 1234)).to(dev)


def timeit(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


n = 20 if which == "f15" else 3
tg = timeit(lambda: input_gradients(model, xs, y), n)
ta = timeit(lambda: modal_ablation(model, xs, y), n)
print(f"{which}: {cfg['name']} batch {B}, recompute {policy}: input gradients {tg:8.1f} ms per batch; modality ablation ({len(xs)} + 1 forwards) "
      f"{ta:8.1f} ms per batch; peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
