"""optimizer step time of the registry's SGD / RMSprop / Adam on the flagship model's parameter arena (GPU box):
    python scripts/bench_optim_step.py [--steps 200] [--block 25] [--warmup 10] [--out result.json]
Times ONE optimizer.step() -- device events around the step only, no forward / backward -- for XR1MR2C1CnnTrf at its native
sizes (every parameter holds a gradient: views of the arena's flat gradient buffer), for
    native:  dict_optimizers["SGD"](momentum=0.9) / ["RMSprop"]() / ["Adam"]()        (koaf_sgd_step / koaf_rmsprop_step / koaf_adam_step)
    torch:   torch.optim.SGD(momentum=0.9) / torch.optim.RMSprop() / torch.optim.Adam()
on the SAME arena-backed parameters, in alternating blocks of `--block` steps on one device, `--steps` timed steps each.
Prints per optimizer the median step time of both, the spread of the block medians, and the bytes-moved floor (SGD, RMSprop:
5 x 4 B per element -- p, g and one state buffer read, p and the state written; Adam: 7 x 4 B -- p, g, m, v read, p, m, v
written) at the achievable HBM rate, 6.3 TB/s."""
import argparse, json, statistics, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, procedural as P
from oaprogressionmmf_amd.arena import get_arena
from oaprogressionmmf_amd.config import ConfigDict
from oaprogressionmmf_amd.models import dict_models
from oaprogressionmmf_amd.various import dict_optimizers

HBM_ACHIEVABLE = 6.3e12          # B/s (float4 copy)
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--block", type=int, default=25)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_optim_step: no GPU (a step time is measured on the device or not at all)")
dev = torch.device("cuda:0")
cfg = P.cfg_full()
m = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)
P.fill_state_dict(m.state_dict())
m = m.to(dev).train()
a = get_arena(m)
a.G.copy_(torch.randn(a.G.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 1e-3)
params = list(m.parameters())
for p in params:
    p.grad = p._koaf_grad
n_elem = sum(hi - lo for lo, hi in a.active_ranges(params))
# (tiny learning rates: 2 x (warmup + steps) updates must leave the weights where they are, whatever the rule)
CASES = {"SGD": (dict(lr=1e-7, momentum=0.9), 5), "RMSprop": (dict(lr=1e-9), 5),
         "Adam": (dict(lr=1e-9), 7)}      # name -> (arguments, fp32 words moved per element)


def time_block(opt, k):
    out = []
    for _ in range(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        opt.step()
        e1.record()
        out.append((e0, e1))
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in out]


result = dict(model=cfg["name"], arena_elements=int(n_elem), parameter_tensors=len(params), steps=args.steps, block=args.block)
for name, (kw, words) in CASES.items():
    opts = {"native": dict_optimizers[name](params, **kw), "torch": getattr(torch.optim, name)(params, **kw)}
    if not type(opts["native"]).__module__.startswith("oaprogressionmmf_amd"):
        sys.exit(f"bench_optim_step: dict_optimizers[{name!r}] is not the native class")
    times = {k: [] for k in opts}
    for k, o in opts.items():
        time_block(o, args.warmup)
    for _ in range(max(1, args.steps // args.block)):
        for k, o in opts.items():                        # alternating blocks
            times[k].append(time_block(o, args.block))
    floor_ms = words * 4 * n_elem / HBM_ACHIEVABLE * 1e3
    r = dict(floor_ms=floor_ms, bytes_per_element=4 * words)
    for k, blocks in times.items():
        med = [statistics.median(b) for b in blocks]
        r[k] = dict(median_ms=statistics.median([t for b in blocks for t in b]), block_median_min_ms=min(med),
                    block_median_max_ms=max(med))
    r["native_share_of_floor"] = floor_ms / r["native"]["median_ms"]
    result[name] = r
    print(f"{name}: native {r['native']['median_ms']:.3f} ms (block medians {r['native']['block_median_min_ms']:.3f}-"
          f"{r['native']['block_median_max_ms']:.3f}), torch.optim {r['torch']['median_ms']:.3f} ms (block medians "
          f"{r['torch']['block_median_min_ms']:.3f}-{r['torch']['block_median_max_ms']:.3f}); floor {floor_ms:.3f} ms for "
          f"{n_elem / 1e6:.1f} M elements x {4 * words} B at 6.3 TB/s")
    del opts
    torch.cuda.empty_cache()
print(json.dumps(result))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1))
