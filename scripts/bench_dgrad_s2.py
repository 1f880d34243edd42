"""(GPU) A/B timing of the stride-2 data gradients at the pixel counts of the headline step (syn3, batch 8: 1280 slices), one library
against another on ONE box, alternating:

    python scripts/bench_dgrad_s2.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 2

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each shape as the model calls it --
ops.conv2d_dgrad with the weights' plane images and dy as a BnApply; the 3x3 calls through dy's plane images (the pre-pass that cuts them
is inside the timed call, as it is in the step) with the fused BatchNorm-backward reduction mode 2 and max |dz|, the 1x1 shortcuts with
the apply formed on load and no reduction -- over --launches launches between two device events after a warm-up, and reports the variant
/ tile the launch record shows.  The table gives, per shape and library, the median over the rounds with the spread (max - min) of the
rounds, the ratio of the medians (first library / last), and the rates of the faster library's median: TB/s over the bytes the call must
move (dz and c once, dx once, the reduction's c once) and TFLOP/s over 2 M_out Cout k k Cin.  Checksums of dx, the partial rows and
max |dz| must agree between the libraries."""
import ab_calls

# (Cin, Cout, input side H = W, filter, pad) of the stride-2 data gradients of layer2-4
SHAPES = [(256, 512, 96, 1, 0), (512, 1024, 48, 1, 0), (1024, 2048, 24, 1, 0), (128, 128, 96, 3, 1), (256, 256, 48, 3, 1), (512, 512, 24, 3, 1)]
SLICES = 1280


def build(shape, dev):
    import torch
    from oaprogressionmmf_amd import ops
    Cin, Cout, H, k, pad = shape
    N, g_ = SLICES, ab_calls.generator(dev, 79)
    OH = (H + 2 * pad - k) // 2 + 1
    orow = N * OH * OH

    def rnd(*s):
        return torch.randn(*s, generator=g_, device=dev)
    w = rnd(Cout, k, k, Cin) * (k * k * Cin) ** -0.5
    img = ops.build_weight_planes(w, Cout, k * k, Cin)
    c = rnd(N, OH, OH, Cout) * 1.5 + 0.3
    svc = ops.bn_finalize(ops.colstats(c, orow, Cout), Cout, orow, rnd(Cout) * 0.2 + 1, rnd(Cout) * 0.1, torch.zeros(Cout, device=dev),
                          torch.ones(Cout, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), 0.1, 1e-5, True)
    dgm, dbt = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
    ap = ops.bn_bwd(rnd(N, OH, OH, Cout) * 1e-3, c, svc, orow, Cout, orow, dgm, dbt, 2, fused=True)
    bnb = None
    if k == 3:
        sv = torch.stack([rnd(Cin) * 0.3, torch.rand(Cin, generator=g_, device=dev) + 0.5, (rnd(Cin) * 0.5 + 1).abs().clamp(min=0.25), rnd(Cin) * 0.2])
        bnb = dict(mode=2, c=rnd(N, H, H, Cin) * 1.5 + 0.3, saved=sv, dz_amax=True)

    def call():
        ap._koaf_planes = None          # (the step cuts dy's plane images once per convolution: the pre-pass is part of the call)
        out = ops.conv2d_dgrad(ap, w, N, H, H, Cin, Cout, k, k, 2, pad, bnb=bnb, wimg=img)
        return out if isinstance(out, tuple) else (out,)
    return call, lambda out: [float(o.double().sum()) for o in out] + [int(out[1].shape[0]) if len(out) > 1 else 0]


def label(shape):
    Cin, Cout, H, k, pad = shape
    return f"k{k}s2 {Cin:5d}<-{Cout:<5d} {SLICES * H * H:9d}     "


def rates(shape, rec):
    Cin, Cout, H, k, pad = shape
    M, Mo = SLICES * H * H, SLICES * ((H + 2 * pad - k) // 2 + 1) ** 2
    return 4.0 * (2 * Mo * Cout + M * Cin * (2 if k == 3 else 1)), 2.0 * Mo * Cout * k * k * Cin


if __name__ == "__main__":
    ab_calls.run(__file__, SHAPES, build, f"{'call, input pixels':30s}", label, rates, rounds=2)
