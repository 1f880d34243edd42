"""Stored volumes -> model input: preproc.PTBatchPipeline (koaf_window_minmax + koaf_input_pipeline, reading the stored uint8
volumes in place) against the chain it replaces, ops.widen -> ops.minmax -> ops.augment -> ops.downscale2 on a batch that was
cropped, flipped and stacked BEFOREHAND (the crop's cost is left out, in the chain's favour).  One process, the two paths
alternating, native shapes at batch 16, train (rotation + gamma on every sample) and eval (centre crop, nothing random)
settings.  "fused" is the whole PTBatchPipeline call, host table and its upload included -- the figure the comparison is about; "kernels" is
its two calls into the library with the table built ahead of the clock, which shows how much of the call is host work.  Every timed
window lasts at least 0.2 s (median of five per path).  Per row: the times, the ratios, and the share of the byte floor -- 2 x the
stored bytes of the window (range pass + the pass itself) + the fp32 output, at the 6.3 TB/s an HBM stream reaches here (DESIGN
3.3).  The T2 and radiograph inputs (55 MB, 9 MB) fit the 256 MB last-level cache and stay there across iterations for both paths:
for those rows the floor is a cache-warm one.  GPU box."""
import argparse
import json
import math
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from oaprogressionmmf_amd import ops
from oaprogressionmmf_amd.preproc import PTBatchPipeline

dev = torch.device("cuda:0")
HBM_STREAM_GBS = 6300.0
B = 16
ROWS = (("dess 320x320x128", (352, 352, 144), (320, 320, 128), (0.5, 0.5, 0.5), -1, 0.257, 0.235),
        ("t2   320x320x25", (352, 352, 28), (320, 320, 25), (0.5, 0.5, 1.0), -1, 0.259, 0.345),
        ("xr   700x700", (768, 760), (700, 700), (0.5, 0.5), 2, 0.543, 0.296))


def timeit(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main(layout="rcs", window_s=0.2, rounds=5):
    for tag, stored, crop, sf, flip_axis, mean, std in ROWS:
        nd = len(crop)
        g = torch.Generator().manual_seed(5)
        vols = torch.randint(3, 250, (B, 1) + stored, generator=g, dtype=torch.uint8).to(dev)
        flips = [b % 2 == 1 for b in range(B)]
        for mode in ("train", "eval"):
            train = mode == "train"
            pipe = PTBatchPipeline(crop, mean, std, flip_axis=flip_axis, random_crop=train, rotate_prob=0.5 if train else 0.0,
                                   gamma_prob=0.5 if train else 0.0, scale_factor=sf, layout=layout)
            states = [((0.37, 0.61, 0.45)[:nd] if train else None, 0.1 if train else 1.0, 0.2, 0.1 if train else 1.0, 1.4)] * B
            # the chain's input: the same windows, cut and flipped ahead of the clock
            start = [math.floor(r * (i - o)) if train else (i - o) // 2 for r, i, o in zip((0.37, 0.61, 0.45), stored, crop)]
            fd = flip_axis - 1 if flip_axis >= 0 else nd + flip_axis
            sel = (slice(None),) + tuple(slice(s, s + o) for s, o in zip(start, crop))
            cropped = torch.stack([(v.flip(1 + fd) if f else v)[sel] for v, f in zip(vols, flips)]).contiguous()
            R, C = crop[:2]
            S = crop[2] if nd == 3 else 1
            fs = 2 if nd == 3 and sf[2] == 0.5 else 1
            prm = torch.tensor([[math.cos(0.2), math.sin(0.2), 1.0 / 1.4, 1.0] if train else [1.0, 0.0, 0.0, 0.0]] * B).to(dev)

            def chain():
                x = ops.widen(cropped)
                y = ops.augment(x, ops.minmax(x, B), prm, B, R, C, S, mean, std)
                return ops.downscale2(y, B, R, C, S, fs)

            def fused():
                return pipe(vols, flip=flips, states=states)

            # the two library calls alone, table built ahead of the clock as the chain's params and crop are
            org = [[vols.shape[2 + d] - 1 - start[d] if f and d == fd else start[d] for d in range(nd)] for f in flips]
            table, code, win = ops.window_table(vols, org, [(1 << fd) if f else 0 for f in flips], crop)
            pool, pool_s = 2, fs

            def kernels():
                return ops.input_pipeline(table, code, win, ops.window_minmax(table, code, win), prm, mean, std, pool, pool_s, layout)

            a, b = fused(), chain()
            assert torch.equal(kernels().reshape(-1), a.reshape(-1))
            if layout == "ncdhw" and nd == 3:
                b = b.permute(0, 3, 1, 2)
            diff = float((a.reshape(b.shape) - b).abs().max())
            for _ in range(3):
                fused(); chain(); kernels()
            torch.cuda.synchronize()
            # every timed window lasts at least window_s: thousands of calls for the radiograph, a hundred for DESS
            nf, nc, nk = (max(20, math.ceil(window_s * 1e3 / timeit(fn, 20))) for fn in (fused, chain, kernels))
            tf, tc, tk = [], [], []
            for _ in range(rounds):
                tf.append(timeit(fused, nf))
                tc.append(timeit(chain, nc))
                tk.append(timeit(kernels, nk))
            tf.sort(); tc.sort(); tk.sort()
            mf, mc, mk = tf[len(tf) // 2], tc[len(tc) // 2], tk[len(tk) // 2]
            nwin = B * R * C * S
            floor_bytes = 2 * nwin * vols.element_size() + a.numel() * 4
            floor_ms = floor_bytes / (HBM_STREAM_GBS * 1e9) * 1e3
            print(json.dumps({"row": tag.strip(), "mode": mode, "layout": layout, "batch": B, "calls_per_window": [nf, nc, nk], "fused_ms": round(mf, 4), "chain_ms": round(mc, 4),
                              "chain_over_fused": round(mc / mf, 2), "kernels_ms": round(mk, 4), "chain_over_kernels": round(mc / mk, 2), "fused_ms_spread": [round(tf[0], 4), round(tf[-1], 4)],
                              "chain_ms_spread": [round(tc[0], 4), round(tc[-1], 4)], "floor_ms": round(floor_ms, 4),
                              "fused_share_of_floor": round(floor_ms / mf, 3), "kernels_share_of_floor": round(floor_ms / mk, 3), "max_abs_diff": diff}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="rcs", choices=("rcs", "ncdhw"), help="ncdhw: the slice-major output (3-D rows)")
    main(ap.parse_args().layout)
