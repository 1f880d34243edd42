"""The path-attribution figures of DESIGN 3.16.  Device-event timing, warm-up, the median of RUNS runs, the sides of every
comparison alternating in one process.
  python scripts/bench_attr.py kernels   koaf_path_points (no noise, then with noise) and koaf_attr_fold at one headline MRI input
                                         (B = 1, n = 160 x 384 x 384, J = 4), each next to koaf_grad_fold mode 1 (the project's
                                         streaming yardstick: two reads and a write per element) on a range sized to move the
                                         same number of bytes
  python scripts/bench_attr.py e2e       run.integrated_gradients at n_steps = 8 on the single-patient headline input (bench.py's
                                         syn3 shapes, batch 1, eval mode, one GPU) next to 8 x one run.input_gradients call
  python scripts/bench_attr.py           both"""
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch
from oaprogressionmmf_amd import ops

RUNS, WARM, REPS = 20, 3, 50     # (REPS: back-to-back calls per timing of the 0.1 ms kernels)
dev = torch.device("cuda:0")


def alternate(fns, runs=RUNS, warm=WARM, reps=1):
    """-> the median milliseconds per call of each of `fns`, timed in turn `runs` times (`reps` back-to-back calls per timing: a
    0.1 ms kernel alone is within reach of the event clock and the launch gap) after `warm` untimed turns"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return [statistics.median(m) for m in ms], [(min(m), max(m)) for m in ms]


def _yardstick(nbytes):
    """koaf_grad_fold mode 1 (acc += w g: 12 bytes per element) on a range that moves `nbytes`"""
    m = nbytes // 12
    acc, g = torch.zeros(m, device=dev), torch.empty(m, device=dev).normal_()
    return lambda: ops.grad_fold(acc, g, 0.5, 1)


def kernels():
    B, n, J = 1, 160 * 384 * 384, 4
    x = torch.empty(B, n, device=dev).normal_()
    alpha = torch.linspace(0.1, 0.9, J, device=dev)
    mm = ops.minmax(x, B)
    out = ops.path_points(x, alpha)                  # (the wrapper allocates its output: the caching allocator hands the same block back)
    del out
    nbytes = (1 + J) * n * 4
    yard = _yardstick(nbytes)
    (t_pp, t_nz, t_y), sp = alternate([lambda: ops.path_points(x, alpha), lambda: ops.path_points(x, alpha, mm=mm, noise_level=0.15, seed=1),
                                       yard], reps=REPS)
    gb = nbytes / 1e9
    print(f"koaf_path_points  B {B} n {n} J {J}, no noise ({gb:.3f} GB: x read once, {J} points written): {t_pp:7.3f} ms {gb / t_pp * 1e3:6.0f} GB/s"
          f"  (min {sp[0][0]:.3f} max {sp[0][1]:.3f})")
    print(f"koaf_grad_fold mode 1, the same bytes:                                    {t_y:7.3f} ms {gb / t_y * 1e3:6.0f} GB/s"
          f"  (min {sp[2][0]:.3f} max {sp[2][1]:.3f})   path_points / grad_fold = {t_pp / t_y:.3f}")
    print(f"koaf_path_points with noise (the same bytes; {J * n / 2 / 1e6:.1f} M Box-Muller pairs):  {t_nz:7.3f} ms {gb / t_nz * 1e3:6.0f} GB/s"
          f"  {J * n / 2 / t_nz / 1e6:6.1f} G pairs/s  (min {sp[1][0]:.3f} max {sp[1][1]:.3f})   noise / no noise = {t_nz / t_pp:.2f}")
    del yard
    g = torch.empty(J, B, n, device=dev).normal_()
    w = torch.tensor([0.25, -0.25, 0.125, -0.125], device=dev)     # (signs alternate: thousands of accumulating calls stay finite)
    acc = torch.zeros(B, n, device=dev)
    nbytes = (J + 2) * n * 4
    yard = _yardstick(nbytes)
    (t_f, t_fin, t_y), sp = alternate([lambda: ops.attr_fold(acc, g, w), lambda: ops.attr_fold(acc, g, w, x=x, base=-0.5), yard], reps=REPS)
    gb = nbytes / 1e9
    print(f"koaf_attr_fold    accumulating ({gb:.3f} GB: {J} gradient planes and acc read, acc written):   {t_f:7.3f} ms {gb / t_f * 1e3:6.0f} GB/s"
          f"  (min {sp[0][0]:.3f} max {sp[0][1]:.3f})")
    print(f"koaf_grad_fold mode 1, the same bytes:                                    {t_y:7.3f} ms {gb / t_y * 1e3:6.0f} GB/s"
          f"  (min {sp[2][0]:.3f} max {sp[2][1]:.3f})   attr_fold / grad_fold = {t_f / t_y:.3f}")
    gbf = (J + 3) * n * 4 / 1e9
    print(f"koaf_attr_fold    finishing ({gbf:.3f} GB: x read as well):                               {t_fin:7.3f} ms {gbf / t_fin * 1e3:6.0f} GB/s"
          f"  (min {sp[1][0]:.3f} max {sp[1][1]:.3f})")


def e2e():
    import procedural as P
    import bench
    from oaprogressionmmf_amd.config import ConfigDict
    from oaprogressionmmf_amd.models import dict_models
    from oaprogressionmmf_amd.run import input_gradients, integrated_gradients
    cfg, _, _ = bench.workload_cfg("syn3")
    shapes = cfg.pop("_tensor_shapes")
    cfg["output_type"] = "main"
    B, steps = 1, 8
    model = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)
    P.fill_state_dict(model.state_dict())
    model = model.to(dev).eval()
    xs = [torch.from_numpy(a).to(dev) for a in P.model_inputs(dict(cfg, input_size=shapes), B, seed=1234)]
    y = torch.from_numpy(P.make_target("target", B, 1234)).to(dev)
    (t_ig, t_g), sp = alternate([lambda: integrated_gradients(model, xs, y, n_steps=steps), lambda: input_gradients(model, xs, y)], runs=7, warm=2)
    own = t_ig - steps * t_g
    print(f"syn3 ({cfg['name']}, batch {B}, eval): run.integrated_gradients n_steps {steps}, chunk 1: {t_ig:8.1f} ms (min {sp[0][0]:.1f} max {sp[0][1]:.1f}); "
          f"run.input_gradients {t_g:8.1f} ms (min {sp[1][0]:.1f} max {sp[1][1]:.1f}); {steps} x = {steps * t_g:8.1f} ms; "
          f"the feature's own share {own:7.1f} ms = {100 * own / t_ig:.1f} % of the call")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("kernels", "all"):
        kernels()
    if what in ("e2e", "all"):
        e2e()
