"""(GPU) A/B timing of the stride-2 forward convolutions at the pixel counts of the headline step (syn3, batch 8: 1280 slices), one
library against another on ONE box, alternating:

    python scripts/bench_fwd_s2.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 2

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each shape as the model calls it --
ops.conv2d_fwd with the weights' plane images and shifted statistics; the 3x3 calls behind their BatchNorm prologue, the 1x1 shortcuts
plain -- over --launches launches between two device events after a warm-up, and reports the variant / tile the launch record shows.
The table gives, per shape and library, the median over the rounds with the spread (max - min) of the rounds, the ratio of the medians
(first library / last), and the rates of the faster library's median: TB/s over the bytes the call must move (the input pixels it
touches once, y once) and TFLOP/s over 2 M Cout K.  Checksums of y and of the statistics rows must agree between the libraries."""
import ab_calls

# (Cin, Cout, input side H = W, filter, pad) of the stride-2 forward convolutions of layer2-4
SHAPES = [(256, 512, 96, 1, 0), (512, 1024, 48, 1, 0), (1024, 2048, 24, 1, 0), (128, 128, 96, 3, 1), (256, 256, 48, 3, 1), (512, 512, 24, 3, 1)]
SLICES = 1280


def build(shape, dev):
    import torch
    from oaprogressionmmf_amd import ops
    Cin, Cout, H, k, pad = shape
    N, g_ = SLICES, ab_calls.generator(dev, 78)
    x = torch.randn(N, H, H, Cin, generator=g_, device=dev) * 1.5 + 0.3
    w = torch.randn(Cout, k, k, Cin, generator=g_, device=dev) * (k * k * Cin) ** -0.5
    sc, sh = torch.rand(Cin, generator=g_, device=dev) * 0.4 + 0.8, torch.randn(Cin, generator=g_, device=dev) * 0.1
    shift = torch.randn(Cout, generator=g_, device=dev) * 0.1
    img = ops.build_weight_planes(w, Cout, k * k, Cin)
    prol = k == 3

    def call():
        return ops.conv2d_fwd(x, w, N, H, H, Cin, Cout, k, k, 2, pad, sc if prol else None, sh if prol else None, stats=True, shift=shift,
                              wimg=img)
    return call, lambda out: (float(out[0].double().sum()), float(out[1].double().sum()), int(out[1].shape[0]))


def pixels(shape):
    Cin, Cout, H, k, pad = shape
    return SLICES * ((H + 2 * pad - k) // 2 + 1) ** 2


def label(shape):
    Cin, Cout, H, k, pad = shape
    return f"k{k}s2 {Cin:5d}->{Cout:<5d} {pixels(shape):9d}     "


def rates(shape, rec):
    Cin, Cout, H, k, pad = shape
    M = pixels(shape)
    # (a 1x1 filter reads one input pixel per output pixel, a 3x3 filter every input pixel -- 4 M -- counted once)
    return 4.0 * (M * Cout + (M if k == 1 else 4 * M) * Cin), 2.0 * M * Cout * k * k * Cin


if __name__ == "__main__":
    ab_calls.run(__file__, SHAPES, build, f"{'call, output pixels':30s}", label, rates, rounds=2)
