"""The attention-relevance figures of DESIGN 3.26.  Device-event timing, warm-up, the median of RUNS runs, the sides of every
comparison alternating in one process.
  python scripts/bench_attnrel.py kernels   the three kernels at the headline fusion shape (B = 8, h = 8, n = 483, d = 256): one layer
                                            of koaf_attn_layer per mode, one koaf_attn_apply of the CLS row and of the whole matrix,
                                            koaf_attn_segsum of the 160-slice totals, each next to its HBM floor (bytes that must be
                                            read / 6.3 TB/s)
  python scripts/bench_attnrel.py e2e [B]   run.attention_relevance (rollout, grad) next to run.predict_batch on the headline model
                                            (bench.py's syn3: XR + three 160-slice MRI + clinical, final sequence 483, depth 4, eval
                                            mode, one GPU), batch B (default 8)
  python scripts/bench_attnrel.py           both"""
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch
from oaprogressionmmf_amd import ops

RUNS, WARM = 20, 3
HBM = 6.3e12            # bytes / s the streaming kernels reach
dev = torch.device("cuda:0")


def alternate(fns, runs=RUNS, warm=WARM):
    """-> the median milliseconds of each of `fns`, run in turn `runs` times after `warm` untimed turns"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms], [(min(m), max(m)) for m in ms]


def kernels():
    B, h, n, d = 8, 8, 483, 256
    attn = torch.softmax(torch.empty(B, h, n, n, device=dev).normal_(), dim=-1)
    dout = torch.empty(B, n, h * d, device=dev).normal_()
    qkv = torch.empty(B, n, 3 * h * d, device=dev).normal_()
    abar = torch.empty(B, n, n, device=dev)
    row = torch.zeros(B, 1, n, device=dev)
    row[:, 0, 0] = 1.0
    out1, outn, seg = torch.empty(B, 1, n, device=dev), torch.empty(B, n, n, device=dev), torch.empty(B, 160, device=dev)
    full = torch.softmax(torch.empty(B, n, n, device=dev).normal_(), dim=-1)
    names = ["attn_layer mean", "attn_layer max", "attn_layer min", "attn_layer grad", "attn_apply q=1", "attn_apply q=n", "attn_segsum K=160 t=3"]
    fns = [lambda: ops.attn_layer(attn, "mean", out=abar), lambda: ops.attn_layer(attn, "max", out=abar),
           lambda: ops.attn_layer(attn, "min", out=abar), lambda: ops.attn_layer(attn, "grad", dout=dout, qkv=qkv, out=abar),
           lambda: ops.attn_apply(full, r_in=row, out=out1), lambda: ops.attn_apply(full, r_in=abar, out=outn),
           lambda: ops.attn_segsum(row.view(B, n), 2, 160, 3, out=seg)]
    read = [attn.numel() * 4] * 3 + [(attn.numel() + dout.numel() + qkv.numel() // 3) * 4, (full.numel() + row.numel()) * 4,
                                     2 * full.numel() * 4, B * 480 * 4]
    flops = {3: 2.0 * B * h * n * n * d, 5: 2.0 * B * n * n * n}
    med, spread = alternate(fns)
    for k, name in enumerate(names):
        floor = read[k] / HBM * 1e3
        extra = f"  {flops[k] / med[k] / 1e9:7.2f} TFLOP/s fp32" if k in flops else ""
        print(f"koaf_{name:24s} {med[k] * 1e3:9.1f} us (min {spread[k][0] * 1e3:.1f} max {spread[k][1] * 1e3:.1f});  reads {read[k] / 1e6:8.2f} MB, "
              f"HBM floor {floor * 1e3:7.2f} us, time / floor {med[k] / floor:7.1f}{extra}")


def e2e(B=8):
    import procedural as P
    import bench
    from oaprogressionmmf_amd.config import ConfigDict
    from oaprogressionmmf_amd.models import dict_models
    from oaprogressionmmf_amd.run import attention_relevance, predict_batch
    cfg, _, _ = bench.workload_cfg("syn3")
    shapes = cfg.pop("_tensor_shapes")
    model = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)
    P.fill_state_dict(model.state_dict())
    model = model.to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(1234)
    xs = [torch.randn((B, 1, *s), generator=g).to(dev) for s in shapes]
    y = torch.randint(0, 2, (B, 1), generator=g).to(dev)
    (t_pred, t_roll, t_grad), spread = alternate([lambda: predict_batch(model, xs), lambda: attention_relevance(model, xs),
                                                  lambda: attention_relevance(model, xs, y, method="grad")], runs=7, warm=2)
    print(f"syn3 ({cfg['name']}, batch {B}, eval, final sequence 483): run.predict_batch {t_pred:8.1f} ms (min {spread[0][0]:.1f} max {spread[0][1]:.1f}); "
          f"attention_relevance rollout {t_roll:8.1f} ms (min {spread[1][0]:.1f} max {spread[1][1]:.1f}) = {t_roll / t_pred:.3f} x; "
          f"grad {t_grad:8.1f} ms (min {spread[2][0]:.1f} max {spread[2][1]:.1f}) = {t_grad / t_pred:.3f} x")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("kernels", "all"):
        kernels()
    if what in ("e2e", "all"):
        e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
