"""The three Grad-CAM figures of DESIGN 3.15.  Device-event timing, warm-up, the median of RUNS (>= 20) runs, the two sides of
every comparison alternating in one process.
  python scripts/bench_gradcam.py kernels   koaf_cam next to koaf_gap_fwd on the headline MRI feature map (3840 x 144 x 2048 fp32, the
                                            same tensor, 4.5 GB read); koaf_cam_upsample 12x12 -> 384x384 into the (B,1,R,C,S) layout
                                            (2.3 GB written) next to koaf_slice_unfold (the same output, 2.3 GB more read)
  python scripts/bench_gradcam.py e2e       run.gradcam next to run.input_gradients on the native-size three-MRI model (bench.py's
                                            native3 shapes, batch 8, eval mode, one GPU)
  python scripts/bench_gradcam.py           both"""
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch
from oaprogressionmmf_amd import ops

RUNS, WARM = 20, 3
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
    N, HW, C = 3840, 144, 2048
    A = torch.empty(N, HW, C, device=dev).normal_()
    w = torch.empty(N, C, device=dev).normal_()
    (t_cam, t_gap), spread = alternate([lambda: ops.cam(A, w, N, HW, C), lambda: ops.gap_fwd(A, N, HW, C)])
    gb = A.numel() * 4 / 1e9
    print(f"koaf_cam     {N} x {HW} x {C} fp32 ({gb:.2f} GB read): {t_cam:7.3f} ms  {gb / t_cam * 1e3:7.0f} GB/s  (min {spread[0][0]:.3f} max {spread[0][1]:.3f})")
    print(f"koaf_gap_fwd the same tensor:                     {t_gap:7.3f} ms  {gb / t_gap * 1e3:7.0f} GB/s  (min {spread[1][0]:.3f} max {spread[1][1]:.3f})"
          f"   cam / gap_fwd = {t_cam / t_gap:.3f}")
    A16 = A.bfloat16()
    (t16, g16), _ = alternate([lambda: ops.cam(A16, w, N, HW, C), lambda: ops.gap_fwd(A16, N, HW, C)])
    print(f"bf16 storage ({gb / 2:.2f} GB read): koaf_cam {t16:7.3f} ms {gb / 2 / t16 * 1e3:7.0f} GB/s; koaf_gap_fwd {g16:7.3f} ms {gb / 2 / g16 * 1e3:7.0f} GB/s")
    del A, A16, w
    B, S, h, R = 24, 160, 12, 384
    cam = torch.empty(B * S, h, h, device=dev).normal_().abs_()
    imax = cam.reshape(B * S, -1).max(dim=1).values.contiguous()
    out = torch.empty(B, 1, R, R, S, device=dev)
    src = torch.empty(B * S, R, R, device=dev).normal_()
    strides = (R * R * S, 1, R * S, S)
    (t_up, t_un), spread = alternate([lambda: ops.cam_upsample(cam, imax, out, B, S, h, h, R, R, strides, "sample"),
                                      lambda: ops.slice_unfold(src, B, R, R, S)])
    gb = out.numel() * 4 / 1e9
    print(f"koaf_cam_upsample {h}x{h} -> {R}x{R}, {B} x {S} slices into (B,1,R,C,S) ({gb:.2f} GB written): {t_up:7.3f} ms  {gb / t_up * 1e3:7.0f} GB/s written"
          f"  (min {spread[0][0]:.3f} max {spread[0][1]:.3f})")
    print(f"koaf_slice_unfold the same output ({gb:.2f} GB read + {gb:.2f} GB written): {t_un:7.3f} ms  {2 * gb / t_un * 1e3:7.0f} GB/s moved"
          f"  (min {spread[1][0]:.3f} max {spread[1][1]:.3f})")
    out2 = torch.empty(B, 1, S, R, R, device=dev)
    (t_sm,), _ = alternate([lambda: ops.cam_upsample(cam, imax, out2, B, S, h, h, R, R, (R * R * S, R * R, R, 1), "sample")])
    print(f"koaf_cam_upsample into the slice-major (B,1,S,R,C) layout: {t_sm:7.3f} ms  {gb / t_sm * 1e3:7.0f} GB/s written")


def e2e():
    import procedural as P
    import bench
    from oaprogressionmmf_amd.config import ConfigDict
    from oaprogressionmmf_amd.models import dict_models
    from oaprogressionmmf_amd.run import gradcam, input_gradients
    cfg, B, policy = bench.workload_cfg("native3")
    cfg["output_type"] = "main"
    model = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)
    P.fill_state_dict(model.state_dict())
    model = model.to(dev).eval()
    xs = [torch.from_numpy(a).to(dev) for a in P.model_inputs(cfg, B, seed=1234)]
    y = torch.from_numpy(P.make_target("target", B, 1234)).to(dev)
    (t_cam, t_low, t_ig), spread = alternate([lambda: gradcam(model, xs, y), lambda: gradcam(model, xs, y, upsample=False),
                                              lambda: input_gradients(model, xs, y)])
    print(f"native3 ({cfg['name']}, batch {B}, eval): run.gradcam {t_cam:8.1f} ms per batch (min {spread[0][0]:.1f} max {spread[0][1]:.1f}); "
          f"without the upsample {t_low:8.1f} ms; run.input_gradients {t_ig:8.1f} ms (min {spread[2][0]:.1f} max {spread[2][1]:.1f}); "
          f"input_gradients / gradcam = {t_ig / t_cam:.2f}")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("kernels", "all"):
        kernels()
    if what in ("e2e", "all"):
        e2e()
