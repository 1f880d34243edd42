"""The coalition figures of DESIGN 3.29: one run.modal_shapley call with sparse=True (two encoder passes, then the final FeaT over
spliced tokens) next to sparse=False (every coalition's copy encoded in full) and next to the unchanged run.modal_ablation (M + 1
forwards, the leave-one-out number alone), on the hierarchical fusion model XR1MR2C1CnnTrf at mid-size volumes -- XR 160^2, MRI
128 x 128 x 32 and 128 x 128 x 16, the clinical vector: M = 4, 16 coalitions -- eval mode, one GPU.  Device-event timing, 5 warm-up
and 20 timed calls per side, the sides alternating in one process; the median.  Beside the times, the encoder passes each side
costs: (1 + B0 / B) against 2^M and against M + 1.
Then koaf_coal_tokens alone at the headline fusion shape (XR1MR3C1CnnTrf, batch 8: M = 5, 1 + 3 x 160 + 1 = 482 tokens of width
2048) next to the time of moving its bytes once at the 6.3 TB/s a float4 copy reaches on this chip.
  python scripts/bench_coalitions.py model    the three-sided comparison
  python scripts/bench_coalitions.py tokens   the kernel alone
  python scripts/bench_coalitions.py          both"""
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch
import procedural as P
from oaprogressionmmf_amd import ops
from oaprogressionmmf_amd.config import ConfigDict
from oaprogressionmmf_amd.models import dict_models
from oaprogressionmmf_amd.run import modal_ablation, modal_shapley

WARM, RUNS, B, CHUNK = 5, 20, 4, 8
BASES = (-0.5, -0.5, -0.5, None)
HBM_ACHIEVABLE = 6.3e12
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


def model_sides():
    cfg = P.cfg_full(xr=(160, 160), mr1=(128, 128, 32), mr2=(128, 128, 16), depth=1)
    cfg["output_type"] = "main"
    model = dict_models[cfg["name"]](config=ConfigDict(cfg), path_weights=None)
    P.fill_state_dict(model.state_dict())
    model = model.to(dev).eval()
    xs = [torch.from_numpy(a).to(dev) for a in P.model_inputs(cfg, B, seed=1234)]
    y = torch.from_numpy(P.make_target("target", B, 1234)).to(dev).long()
    M = len(xs)
    (ts, td, ta), sp = alternate([lambda: modal_shapley(model, xs, y, baselines=BASES, chunk=CHUNK, sparse=True),
                                  lambda: modal_shapley(model, xs, y, baselines=BASES, chunk=CHUNK, sparse=False),
                                  lambda: modal_ablation(model, xs, y)])
    enc = 1 + 1 / B
    print(f"model: {cfg['name']} batch {B}, M {M}, {1 << M} coalitions, chunk {CHUNK}: modal_shapley sparse {ts:8.1f} ms [{sp[0][0]:.1f}, "
          f"{sp[0][1]:.1f}]; dense {td:8.1f} ms [{sp[1][0]:.1f}, {sp[1][1]:.1f}]; modal_ablation {ta:8.1f} ms [{sp[2][0]:.1f}, {sp[2][1]:.1f}]; "
          f"dense / sparse {td / ts:.2f}, modal_ablation / sparse {ta / ts:.2f}; encoder passes: sparse {enc:.2f} (1 + B0 / B, B0 = 1), dense "
          f"{1 << M} (ratio {(1 << M) / enc:.1f}), modal_ablation {M + 1} (ratio {(M + 1) / enc:.1f}); final FeaT passes behind them: "
          f"sparse {(1 << M) - 2}; peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def tokens_alone():
    Bh, L, D, seg = 8, 482, 2048, [0, 1, 161, 321, 481, 482]
    g = torch.Generator(device="cpu").manual_seed(7)
    tx = torch.randn(Bh, L, D, generator=g).to(dev)
    for B0 in (1, Bh):
        t0 = torch.randn(B0, L, D, generator=g).to(dev)
        for masks in (list(range(1, 9)), list(range(1, 31))):
            J = len(masks)
            out = torch.empty((J, Bh, L, D), device=dev)
            (t,), sp = alternate([lambda: ops.coal_tokens(tx, t0, seg, masks, out=out)])
            nbytes = 4 * L * D * (Bh + B0 + J * Bh)
            floor = nbytes / HBM_ACHIEVABLE * 1e3
            print(f"tokens: koaf_coal_tokens B {Bh} B0 {B0} L {L} D {D} M 5 J {J}: {t * 1e3:8.1f} us [{sp[0][0] * 1e3:.1f}, {sp[0][1] * 1e3:.1f}]; "
                  f"{nbytes / 2 ** 20:.0f} MiB moved once = {nbytes / t / 1e9:.2f} TB/s; floor at 6.3 TB/s {floor * 1e3:.1f} us "
                  f"({floor / t:.0%} of it reached)")


which = sys.argv[1] if len(sys.argv) > 1 else "both"
if which in ("model", "both"):
    model_sides()
if which in ("tokens", "both"):
    tokens_alone()
