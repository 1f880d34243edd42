"""(GPU) A/B timing of the 1x1 / stride-1 weight gradients at the pixel counts of the headline step (syn3, batch 8), one library
against another on ONE box, alternating:

    python scripts/bench_wgrad1x1.py --lib parent=/path/libkoaf_parent.so --lib new=oaprogressionmmf_amd/csrc/libkoaf.so --rounds 3

--family s2: the stride-2 weight gradients of the downsampling blocks instead (1x1 shortcuts: apply on dy, plain x; 3x3 conv2: apply +
prologue), at 1280 slices.

Every (round, library) is a fresh child process (KOAF_LIB is read at import) that times each shape as the model calls it --
ops.conv2d_wgrad with dy a BatchNorm-backward apply and x behind its BatchNorm prologue -- over --launches launches between two
device events after a warm-up, and reports the variant / tile the launch record shows.  The table gives, per shape and library, the
median over the rounds with the spread (max - min) of the rounds, the ratio of the medians, and the rates of the faster library's
median: TB/s over the bytes the call must read (dz, c, x once; the slabs it writes) and TFLOP/s over 2 P Cout Cin."""
import ab_calls

# (Cin, Cout, pixels) of the layer2-4 1x1 / stride-1 convolutions of the slice-wise encoders at batch 8
SHAPES = [(256, 1024, 737280), (128, 512, 2949120), (1024, 256, 737280), (512, 2048, 184320), (512, 128, 2949120), (512, 256, 2949120),
          (1024, 512, 737280), (2048, 512, 184320)]
# (Cin, Cout, input side H = W, filter, pad) of the stride-2 convolutions of layer2-4 at 1280 slices (the table's pixel column: output pixels)
SHAPES_S2 = [(256, 512, 96, 1, 0), (512, 1024, 48, 1, 0), (1024, 2048, 24, 1, 0), (256, 256, 48, 3, 1), (512, 512, 24, 3, 1)]
SLICES = 1280


def family(name):
    """(Cin, Cout, output pixels, N, H, filter, stride, pad, prologue on x) per shape"""
    if name == "s1":
        return [(Cin, Cout, P, P // (64 * 64), 64, 1, 1, 0, True) for Cin, Cout, P in SHAPES]
    return [(Cin, Cout, SLICES * ((H + 2 * pad - k) // 2 + 1) ** 2, SLICES, H, k, 2, pad, k == 3) for Cin, Cout, H, k, pad in SHAPES_S2]


def build(shape, dev):
    import torch
    from oaprogressionmmf_amd import _lib, ops
    Cin, Cout, P, N, H, k, stride, pad, prol = shape
    g_ = ab_calls.generator(dev, 77)
    x = torch.randn(N * H * H, Cin, generator=g_, device=dev) * 1.5 + 0.3
    dz = torch.randn(P, Cout, generator=g_, device=dev) * 1e-3
    c = torch.randn(P, Cout, generator=g_, device=dev) * 1.5 + 0.3
    sc, sh = torch.rand(Cin, generator=g_, device=dev) * 0.4 + 0.8, torch.randn(Cin, generator=g_, device=dev) * 0.1
    coef = torch.stack([torch.rand(Cout, generator=g_, device=dev) + 0.5, torch.zeros(Cout, device=dev),
                        torch.randn(Cout, generator=g_, device=dev) * 1e-5, torch.randn(Cout, generator=g_, device=dev) * 1e-5]).contiguous()
    amax = (coef[0] * dz + coef[3] - coef[2] * c).abs().max().reshape(1).float()
    ap = ops.BnApply(dz, c, coef, amax, torch.zeros(Cout, device=dev), P, Cout)
    ws = _lib.lib().koaf_conv2d_wgrad_ws(N, H, H, Cin, Cout, k, k, stride, pad)
    slabs, dw = torch.empty(ws, device=dev), torch.empty(Cout, k, k, Cin, device=dev)

    def call():
        ops.conv2d_wgrad(ap, x, dw, N, H, H, Cin, Cout, k, k, stride, pad, sc if prol else None, sh if prol else None, aplanes=False,
                         slabs=slabs)
    return call, lambda out: float(dw.double().sum())


def label(shape):
    Cin, Cout, P, N, H, k, stride, pad, prol = shape
    return f"{Cin:5d}->{Cout:<5d} k{k} {P:9d} "


def rates(shape, rec):
    Cin, Cout, P, N, H, k, stride, pad, prol = shape
    # (stride 2: a 1x1 filter reads one input pixel per output pixel, a 3x3 filter every input pixel -- 4 P -- counted once)
    px_in = P if stride == 1 or k == 1 else 4 * P
    return 4.0 * (2 * P * Cout + px_in * Cin + (rec["splitk"] + 1) * Cout * k * k * Cin), 2.0 * P * Cout * k * k * Cin


if __name__ == "__main__":
    ab_calls.run(__file__, family, build, f"{'Cin->Cout, pixels':26s}", label, rates, rounds=3, families=("s1", "s2"))
