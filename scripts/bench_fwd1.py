"""(GPU) A/B timing of the dense 1x1 / stride-1 forward convolutions without a bottleneck tail at the pixel counts of the headline step
(syn3, batch 8: 1280 slices), one library against others on ONE box, alternating:

    python scripts/bench_fwd1.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 2

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each call as the model makes it --
ops.conv2d_fwd with the weights' plane images and shifted statistics; conv3 of the Bottlenecks behind its BatchNorm prologue, block-0
conv1 and the layer1 shortcut plain -- over --launches launches between two device events after a warm-up, and reports the variant /
tile / grid the launch record shows.  Both forms of koaf_fwd1 are timed from two builds of the library that differ in
-DKOAF_FWD1_FORCE=0 | 1 (koaf_fwd1.hip: every admitted shape in that form; benchmark builds only).
The table gives, per call and library, the median over the rounds with the spread (max - min) of the rounds, the ratio of the FIRST
library's median to this one's, whether the call passes the ship rule against the first library (its median below the first's by at
least ten times the larger of the two spreads), and the rates of the median: TB/s over the bytes the call must move (x once, y once)
and TFLOP/s over 2 M Cout Cin.  Checksums of y and of the statistics rows must agree between the libraries."""
import ab_calls

# (Cin, Cout, side H = W, prologue) of the calls: conv3 of layer1-4, block-0 conv1 of layer2-3, the layer1 shortcut
SHAPES = [(64, 256, 96, True), (128, 512, 48, True), (256, 1024, 24, True), (512, 2048, 12, True), (256, 128, 96, False),
          (512, 256, 48, False), (64, 256, 96, False)]
SLICES = 1280


def build(shape, dev):
    import torch
    from oaprogressionmmf_amd import ops
    Cin, Cout, H, prol = shape
    N, g_ = SLICES, ab_calls.generator(dev, 79)
    x = torch.randn(N, H, H, Cin, generator=g_, device=dev) * 1.5 + 0.3
    w = torch.randn(Cout, 1, 1, Cin, generator=g_, device=dev) * Cin ** -0.5
    sc, sh = torch.rand(Cin, generator=g_, device=dev) * 0.4 + 0.8, torch.randn(Cin, generator=g_, device=dev) * 0.1
    shift = torch.randn(Cout, generator=g_, device=dev) * 0.1
    img = ops.build_weight_planes(w, Cout, 1, Cin)

    def call():
        return ops.conv2d_fwd(x, w, N, H, H, Cin, Cout, 1, 1, 1, 0, sc if prol else None, sh if prol else None, stats=True, shift=shift,
                              wimg=img)
    return call, lambda out: (float(out[0].double().sum()), float(out[1].double().sum()), int(out[1].shape[0]))


def label(shape):
    Cin, Cout, H, prol = shape
    return f"k1s1 {Cin:5d}->{Cout:<5d} {'prologue' if prol else 'plain':8s} {SLICES * H * H:9d}"


def rates(shape, rec):
    Cin, Cout, H, prol = shape
    M = SLICES * H * H
    return 4.0 * M * (Cout + Cin), 2.0 * M * Cout * Cin


if __name__ == "__main__":
    ab_calls.run(__file__, SHAPES, build, "call, output pixels; per library: median ms (spread) kernel tile grid.x | ratio first/this | ship rule | "
                 "TB/s TFLOP/s", label, rates, rounds=2, ship_rule=True)
