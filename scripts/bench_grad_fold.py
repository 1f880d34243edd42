"""gradient fold / norm / scale kernels on a flat buffer of the headline arena's size (GPU box):
    python scripts/bench_grad_fold.py [--elements 389000000] [--steps 50] [--warmup 5] [--out result.json]
    python scripts/bench_grad_fold.py --headline [--steps 6] [--warmup 2]
Default: times each pass with device events around the one launch -- fold mode 0 (8 B per element), modes 1 and 2 (12 B), mode 2
emitting the norm partials, the norm partials alone (4 B), the finalize, the scale with a coefficient below 1 (8 B) and of exactly
1 (no traffic) -- and, as the yardstick, koaf_adam_step over the same elements (28 B) on the same box; prints GB/s beside the
6.3 TB/s a float4 copy achieves.
--headline: the bench's default workload (syn3, batch 8, its recompute policy) as a plain train step and as ONE accumulated step
of 2 x batch 8 with the clip on: ms per optimizer step and peak allocated / reserved memory of both."""
import argparse, json, statistics, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch
from oaprogressionmmf_amd import ops

HBM_ACHIEVABLE = 6.3e12          # B/s (float4 copy)
ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=389_000_000)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--headline", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_grad_fold: no GPU (a pass is timed on the device or not at all)")
dev = torch.device("cuda:0")


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in evs]


def flat():
    n = args.elements
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    acc = torch.randn(n, device=dev, generator=gen) * 1e-3
    ws, cuts = ops.grad_norm_ws([n], dev)
    ops.grad_norm_part(g, cuts[0])
    below = ops.grad_norm_final(ws, 1e30)[1].clone()         # exactly 1: nothing is clipped
    # (a coefficient a hair under 1, so that hundreds of scale passes leave the values where they are)
    under = torch.full((), 1.0 - 2.0 ** -24, device=dev)
    p, m, v = (torch.zeros(n, device=dev) for _ in range(3))
    cases = [
        ("fold mode 0: acc = w g", 8, lambda: ops.grad_fold(acc, g, 0.5, 0)),
        ("fold mode 1: acc += w g", 12, lambda: ops.grad_fold(acc, g, 1e-9, 1)),
        ("fold mode 2: g = acc + w g", 12, lambda: ops.grad_fold(acc, g, 0.5, 2)),
        ("fold mode 2 + norm partials", 12, lambda: ops.grad_fold(acc, g, 0.5, 2, ws=cuts[0])),
        ("norm partials (2-norm)", 4, lambda: ops.grad_norm_part(g, cuts[0])),
        ("norm partials (inf-norm)", 4, lambda: ops.grad_norm_part(g, cuts[0], float("inf"))),
        ("finalize", 0, lambda: ops.grad_norm_final(ws, 1.0)),
        ("scale, coef < 1", 8, lambda: ops.grad_scale(g, under)),
        ("scale, coef == 1", 0, lambda: ops.grad_scale(g, below)),
        ("adam_step (yardstick)", 28, lambda: ops.adam_step(p, g, m, v, n, 1e-9, 0.9, 0.999, 1e-8, 0.0, 1)),
    ]
    result = dict(elements=n, steps=args.steps, partials=int(ws.numel()), passes={})
    for name, bpe, fn in cases:
        ms = timed(fn, args.warmup, args.steps)
        med = statistics.median(ms)
        gbs = bpe * n / (med * 1e-3) / 1e9 if bpe else 0.0
        result["passes"][name] = dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), bytes_per_element=bpe, gb_per_s=gbs,
                                      share_of_achievable=gbs * 1e9 / HBM_ACHIEVABLE)
        print(f"{name:32s} {med:8.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"
              + (f"  {gbs:7.0f} GB/s = {gbs * 1e9 / HBM_ACHIEVABLE:.0%} of 6.3 TB/s" if bpe else ""))
    return result


def headline():
    import bench
    import procedural as P
    from oaprogressionmmf_amd.config import ConfigDict
    from oaprogressionmmf_amd.models import dict_models
    from oaprogressionmmf_amd.run import train_step, train_step_accum
    from oaprogressionmmf_amd.various import dict_losses, dict_optimizers
    cfg, B, policy = bench.workload_cfg("syn3")
    shapes = cfg.pop("_tensor_shapes", None)
    model = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None).to(dev)
    bench.apply_recompute(model, policy)
    model.train()
    loss_fn = dict_losses["FocalLoss"](reduction="mean", gamma=2.0, num_classes=2)
    opt = dict_optimizers["Adam"](model.parameters(), lr=1e-4, weight_decay=1e-4)
    xs = [torch.from_numpy(a).to(dev) for a in P.model_inputs(dict(cfg, input_size=shapes) if shapes else cfg, B, seed=1234)]
    y = torch.from_numpy(P.make_target("target", B, seed=1234)).to(dev)
    result = dict(workload="syn3", batch=B, recompute=policy, steps=args.steps)

    def peak():
        return dict(allocated_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
                    reserved_gib=round(torch.cuda.max_memory_reserved() / 2 ** 30, 1))
    for name, fn in (("plain", lambda: train_step(model, loss_fn, opt, xs, y)[1].item()),
                     ("accum_2x_clip", lambda: train_step_accum(model, loss_fn, opt, [(xs, y), (xs, y)], max_grad_norm=1.0)[1].item())):
        torch.cuda.reset_peak_memory_stats()
        ms = timed(fn, args.warmup, args.steps)
        result[name] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), **peak())
        print(f"{name}: {result[name]}")
    return result


out = headline() if args.headline else flat()
print(json.dumps(out))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1))
