"""float64 references and derived error bounds of the element-wise edge-shape tests (test_elem_edges_gpu.py; checked on
the CPU by test_elem_edges_cpu.py).

Bounds.  u = 2^-24 is the unit roundoff of fp32 round-to-nearest.
  * a chain of k roundings applied to terms t_i entering one element errs by at most k * u * sum|t_i| (first order; every
    chain here has k <= 5, and the callers' operands make the second-order part, k^2 u^2, vanish under the slack of
    counting a fused multiply-add as two roundings);
  * an fp32 sum whose longest chain of additions has length m errs by at most gamma(m) * sum|t_i|, gamma(m) = m u / (1 - m u)
    (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4, any order of summation).
The column kernels' m comes from the geometry below, a Python twin of col_geom (koaf_cols.h), itself checked against
koaf_colpart_rows.

bf16 activation storage (test_elem_edges_bf16_gpu.py).  Widening a stored bf16 value is exact, so a kernel fed bf16 activations
owes its fp32-typed outputs exactly the bound of the fp32 case on the widened values; an output STORED as bf16 owes that bound
plus one rounding to 8 significand bits, u16 = 2^-8 (stored16_bound).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EW_CAP = 256 * 32 * 256     # ew_grid: 256 CUs * KOAF_EW_BLOCKS_PER_CU (32) blocks of 256 threads


def gamma(m):
    return m * U / (1.0 - m * U)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# column-reduction geometry (col_geom): max_blk = 1024 for colstats / bn_bwd_reduce[_pool], 256 for layernorm_bwd / colsum
# ------------------------------------------------------------------------------------------------
def col_geom(rows, C, max_blk=1024):
    """-> dict(CW, nchunk, CV, RP, rpb, nblk) or None where the kernels refuse the width"""
    if C <= 0 or C % 4:
        return None
    CW = 1024 if C > 1024 else C
    if C % CW:
        return None
    CV = CW // 4
    if 256 % CV:
        return None
    RP = 256 // CV
    rpb = cdiv(cdiv(rows, max_blk), RP) * RP
    rpb = max(rpb, 4 * RP)
    return dict(CW=CW, nchunk=C // CW, CV=CV, RP=RP, rpb=rpb, nblk=cdiv(rows, rpb))


def col_rp(C):
    return 256 // (min(C, 1024) // 4)


def col_chain(rows, C, max_blk, term_roundings):
    """longest chain of fp32 roundings behind one column sum: rpb / RP sequential rows per thread, RP - 1 additions of the LDS
    fold, the roundings of the term itself, and the one rounding of the fp64 second stage's result to fp32"""
    g = col_geom(rows, C, max_blk)
    return g["rpb"] // g["RP"] + (g["RP"] - 1) + term_roundings + 1


def col_bound(rows, C, max_blk, term_roundings, abs_terms):
    """abs_terms [rows][C] float64 = |t| of every term -> per-column bound [C]"""
    return gamma(col_chain(rows, C, max_blk, term_roundings)) * abs_terms.sum(0)


def case_a_rows(C):
    """the row counts of case A for width C: 1, RP - 1, one block, one block + 1, about 3.5 blocks (ragged)"""
    RP = col_rp(C)
    out = [1, RP - 1, 4 * RP, 4 * RP + 1, 14 * RP + max(1, RP // 3)]
    return sorted({r for r in out if r > 0})


def emulate_colsum(terms32, max_blk=1024, drop_row=None):
    """numpy fp32 emulation of the column kernels' summation order over terms [rows][C] (already rounded to fp32): thread
    (ry) adds rows ry, ry + RP, ... of its block in order, the fold adds ry = 1 .. RP - 1 onto ry = 0 in order, the blocks'
    partials are added in fp64 and rounded once.  drop_row: leave that row out (the `rend - 1` mistake)"""
    rows, C = terms32.shape
    g = col_geom(rows, C, max_blk)
    RP, rpb, nblk = g["RP"], g["rpb"], g["nblk"]
    t = np.zeros((nblk * rpb, C), dtype=np.float32)
    t[:rows] = terms32
    if drop_row is not None:
        t[drop_row] = 0
    t = t.reshape(nblk, rpb // RP, RP, C)
    acc = np.zeros((nblk, RP, C), dtype=np.float32)
    for i in range(rpb // RP):
        acc = (acc + t[:, i]).astype(np.float32)
    part = acc[:, 0].copy()
    for j in range(1, RP):
        part = (part + acc[:, j]).astype(np.float32)
    return part.astype(np.float64).sum(0).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# inputs whose mask / arg-max decisions do not depend on rounding
# ------------------------------------------------------------------------------------------------
def borderline(c, sc, sh):
    """elements of c [..., C] whose pre-activation sc * c + sh lies within its own rounding of zero: the fp32 result (two
    roundings, or one when the compiler fuses) is within 2 u (|sc c| + |sh|) of the exact one, so outside 4 u (...) -- a factor
    two of margin -- the sign is the exact sign whatever the instruction selection"""
    c64, s64, h64 = c.double(), sc.double(), sh.double()
    z = c64 * s64 + h64
    return z.abs() <= 4 * U * ((c64 * s64).abs() + h64.abs())


def stored(t, store):
    """an activation as the storage mode holds it: rounded to `store` (torch.float32: left alone; torch.bfloat16: to nearest even,
    on the CPU) and widened again -- the fp32 values a kernel computes with, and the ones the float64 reference is fed"""
    return t.to(store).float()


def draw_preact(gen, shape, sc, sh, scale=1.0, store=torch.float32):
    """fp32 randn tensor [..., C] with no borderline element (rejected and redrawn, not excluded from the comparison); every draw
    is rounded to `store` BEFORE the borderline test, so the values the kernel widens are the ones that were tested"""
    c = stored(torch.randn(*shape, generator=gen) * scale, store)
    for _ in range(64):
        bad = borderline(c, sc, sh)
        n = int(bad.sum())
        if n == 0:
            return c
        c[bad] = stored(torch.randn(n, generator=gen) * scale, store)
    raise AssertionError("draw_preact: borderline elements survive 64 redraws")


def draw_grid(gen, shape, step=2.0 ** -4, span=4.0):
    """multiples of `step` in [-span, span]: with sc in {0.5, 1, 2} and sh a multiple of `step`, sc * c + sh is exact in fp32
    (fused or not), so max-pool values are bit-equal to the float64 reference and equal maxima are true ties"""
    k = int(span / step)
    return torch.randint(-k, k + 1, shape, generator=gen).float() * step


# ------------------------------------------------------------------------------------------------
# point-wise and row-wise references (float64 of fp32 inputs)
# ------------------------------------------------------------------------------------------------
def gelu_ref(x64):
    return 0.5 * x64 * (1 + torch.erf(x64 / math.sqrt(2.0)))


def gelu_grad_ref(x64):
    return 0.5 * (1 + torch.erf(x64 / math.sqrt(2.0))) + x64 * torch.exp(-0.5 * x64 * x64) / math.sqrt(2.0 * math.pi)


def layernorm_ref(x, g, b, eps):
    """-> (y, mean, rstd) of LayerNorm over the last axis of x [rows][D]"""
    x64 = x.double()
    m = x64.mean(1)
    rs = (x64.var(1, unbiased=False) + eps).rsqrt()
    return (x64 - m[:, None]) * rs[:, None] * g.double() + b.double(), m, rs


# ------------------------------------------------------------------------------------------------
# BatchNorm pieces
# ------------------------------------------------------------------------------------------------
def bn_sums_ref(dz, c, mean, invstd):
    """float64 (sum dz, sum dz * xhat) per channel and the |terms|: dz, c [rows][C]; mean, invstd [C] (fp32 values widened)"""
    xh = (c.double() - mean.double()) * invstd.double()
    t = dz.double() * xh
    return dz.double().sum(0), t.sum(0), dz.double().abs(), t.abs()


def bn_dc_ref(dz, c, mean, invstd, sc, s1, s2, count):
    """dc = k0 (dz - k1) - k2 (c - mean) with k0 = sc, k1 = s1 / count, k2 = sc invstd s2 / count, in float64 -> (dc, A, B):
    A and B are the two products, whose magnitudes enter the rounding bound"""
    k0, k1 = sc.double(), s1 / count
    k2 = sc.double() * invstd.double() * s2 / count
    A = k0 * (dz.double() - k1)
    B = k2 * (c.double() - mean.double())
    return A - B, A, B


# ------------------------------------------------------------------------------------------------
# max-pool 3x3 / stride 2 / pad 1 over relu(sc * c + sh), NHWC
# ------------------------------------------------------------------------------------------------
def pool_out(h):
    return (h + 2 - 3) // 2 + 1


def maxpool_ref(a):
    """a [N][H][W][C] float64 activations (>= 0) -> (y, am): the maximum of each window and the FIRST position reaching it in
    row-major window order, as index kh * 3 + kw of the 3x3 window (positions outside the image do not take part)"""
    N, H, W, C = a.shape
    OH, OW = pool_out(H), pool_out(W)
    y = torch.full((N, OH, OW, C), -float("inf"), dtype=torch.float64)
    am = torch.zeros((N, OH, OW, C), dtype=torch.uint8)
    oy, ox = torch.arange(OH), torch.arange(OW)
    for kh in range(3):
        iy = oy * 2 - 1 + kh
        vy = (iy >= 0) & (iy < H)
        for kw in range(3):
            ix = ox * 2 - 1 + kw
            vx = (ix >= 0) & (ix < W)
            v = a[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            ok = (vy[:, None] & vx[None, :])[None, :, :, None]
            better = ok & (v > y)
            y = torch.where(better, v, y)
            am = torch.where(better, torch.tensor(kh * 3 + kw, dtype=torch.uint8), am)
    return y, am


def maxpool_bwd_ref(dy, am, H, W):
    """float64 scatter of dy [N][OH][OW][C] to the recorded positions -> (da, abs_da): the gradient and the sum of the
    magnitudes that met in each element (at most four: the windows that overlap a pixel)"""
    N, OH, OW, C = dy.shape
    da = torch.zeros((N, H, W, C), dtype=torch.float64)
    ab = torch.zeros_like(da)
    d64 = dy.double()
    for oy in range(OH):
        for ox in range(OW):
            a = am[:, oy, ox].long()
            iy, ix = oy * 2 - 1 + a // 3, ox * 2 - 1 + a % 3           # [N][C]
            n = torch.arange(N)[:, None].expand(N, C)
            ch = torch.arange(C)[None, :].expand(N, C)
            da.index_put_((n, iy, ix, ch), d64[:, oy, ox], accumulate=True)
            ab.index_put_((n, iy, ix, ch), d64[:, oy, ox].abs(), accumulate=True)
    return da, ab


def maxpool_bwd_gather_ref(dy, am, H, W):
    """the same as maxpool_bwd_ref, vectorised over the image (for the large shapes): per input pixel, the (up to four) windows
    that cover it, in the kernels' order"""
    N, OH, OW, C = dy.shape
    d64 = dy.double()
    da = torch.zeros((N, H, W, C), dtype=torch.float64)
    ab = torch.zeros_like(da)
    iy, ix = torch.arange(H), torch.arange(W)
    for wy in range(2):
        oy = (iy + wy) // 2
        vy = (oy < OH) & ((wy == 0) | (oy != iy // 2))
        for wx in range(2):
            ox = (ix + wx) // 2
            vx = (ox < OW) & ((wx == 0) | (ox != ix // 2))
            oyc, oxc = oy.clamp(max=OH - 1), ox.clamp(max=OW - 1)
            want = ((iy - (oyc * 2 - 1))[:, None] * 3 + (ix - (oxc * 2 - 1))[None, :])[None, :, :, None]
            hit = (am[:, oyc][:, :, oxc].long() == want) & (vy[:, None] & vx[None, :])[None, :, :, None]
            g = d64[:, oyc][:, :, oxc]
            da += torch.where(hit, g, torch.zeros((), dtype=torch.float64))
            ab += torch.where(hit, g.abs(), torch.zeros((), dtype=torch.float64))
    return da, ab


# ------------------------------------------------------------------------------------------------
# input pipeline
# ------------------------------------------------------------------------------------------------
def augment_ref(x, prm, mean, std, dtype=torch.float64):
    """x [B][R][C][S] raw fp32; prm [B][4] = (cos, sin, exponent or 0, rotated flag) fp32, the layout PTBatchAugment builds
    (preproc/_pt.py) -> unit range, in-plane rotation (F.affine_grid + F.grid_sample bilinear / zeros / align_corners=False),
    gamma, normalise -- in `dtype` (float64: the reference; float32: torch's own fp32, the yardstick)"""
    B, R, C, S = x.shape
    out = []
    for b in range(B):
        xb = x[b].to(dtype)
        mn, mx = xb.min(), xb.max()
        v = ((xb - mn) / (mx - mn)).permute(2, 0, 1)[None]                 # [1][S][R][C]
        cs, sn, ex, rot = (prm[b, i].to(dtype) for i in range(4))
        if float(rot) != 0.0:
            theta = torch.stack([torch.stack([cs, -sn, torch.zeros((), dtype=dtype)]),
                                 torch.stack([sn, cs, torch.zeros((), dtype=dtype)])])[None]
            grid = F.affine_grid(theta, (1, S, R, C), align_corners=False)
            v = F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        if float(ex) != 0.0:
            v = v.clamp_min(0) ** ex
        out.append(((v - mean) / std)[0].permute(1, 2, 0))
    return torch.stack(out)


def exact_attention_qk(gen, n, h, d):
    """q with entries in {0, +-1, +-2, +-4} and k multiples of 0.5 with |k| <= 8: every product is a multiple of 0.5 up to 32,
    every partial sum of d <= 16 of them (up to 512) is exact in fp32, and so is the score under a power-of-two scale; the first
    bf16 piece of such operands already holds them exactly.  Rows 0 .. 3 of q are +-4 throughout, key 0 is +-8 with the same
    signs and key 1 its negative: those rows' scores reach +-(4 * 8 * d) * scale"""
    qv = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0])
    q = qv[torch.randint(0, 7, (n, h, d), generator=gen)]
    k = torch.randint(-16, 17, (n, h, d), generator=gen).float() * 0.5
    v = torch.randn(n, h, d, generator=gen)
    sgn = torch.where(torch.rand(h, d, generator=gen) < 0.5, -1.0, 1.0)
    q[:4] = 4.0 * sgn
    k[0] = 8.0 * sgn
    k[1] = -8.0 * sgn
    return q, k, v


# ------------------------------------------------------------------------------------------------
# bf16 activation storage: the bound of a stored output, the rounding table, the mistakes it must catch
# ------------------------------------------------------------------------------------------------
U16 = 2.0 ** -8             # unit roundoff of bf16 round-to-nearest (8 significand bits)
BF16_MIN_NORMAL = 2.0 ** -126
BF16_HALF_SUBNORMAL = 2.0 ** -134   # half the spacing 2^-133 of the bf16 subnormals


def stored16_bound(ref, B):
    """bound of |stored - ref| for a result whose fp32 value v lies within B of the float64 reference and is then stored as bf16,
    rounded to nearest.  |stored - ref| <= |stored - v| + |v - ref|.  For a normal v, 2^e <= |v| < 2^(e+1), the bf16 neighbours are
    2^(e-7) apart, so |stored - v| <= 2^(e-8) <= u16 |v| <= u16 (|ref| + B); below the normal range (|v| < 2^-126) the neighbours
    are 2^-133 apart whatever v is, so |stored - v| <= 2^-134.  Hence B + max(u16 (|ref| + B), 2^-134) -- the maximum, because
    v may be normal where ref is not, and the other way round.  (No allowance for overflow: the callers' values are far from
    the largest finite bf16, 3.39e38.)"""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    B = torch.as_tensor(B, dtype=torch.float64)
    return B + (U16 * (ref.abs() + B)).clamp_min(BF16_HALF_SUBNORMAL)


def _bf16_from_bits(bits):
    """int64 tensor of bf16 bit patterns -> bfloat16 tensor"""
    return bits.to(torch.int16).view(torch.bfloat16) if bits.numel() else torch.empty(0, dtype=torch.bfloat16)


def bf16_round_cases():
    """-> (c, idt): bf16 tensors, a multiple of four long, whose fp32 sum c.float() + idt.float() is EXACT and, rounded to bf16,
    meets every rounding decision of a bf16 store.  For every non-negative bit pattern 0x0000 .. 0x7F80 of c (zero, the subnormals,
    every normal value, +Inf) and ulp = the spacing of bf16 at c (2^-133 up to the smallest normal's binade):
      * idt in {0, +-1/4, +-1/2, +-3/4 ulp} wherever idt is itself a bf16 value (not below the binade of 2^-131) -- a quarter and
        three quarters round down / up, a half is a tie that goes to the even neighbour; c = 0x7F7F, the largest finite bf16, goes to
        +Inf at + 1/2 ulp (a tie, 0x7F7F is odd) and at + 3/4;
      * idt = -2 c: the sum is -c, which the ReLU turns into +0 (and +0 + -0, which is +0 already);
      * a NaN in c, and a NaN in idt.
    The expectation is (c.float() + idt.float()).relu().bfloat16() on the CPU: round to nearest even, subnormals kept, anything
    from the largest finite bf16 + 1/2 ulp on to Inf, NaN stays NaN (test_elem_edges_cpu.py checks all four on this table)."""
    p = torch.arange(0, 0x7F81, dtype=torch.int64)
    e = (p >> 7).clamp_min(1)
    c64 = _bf16_from_bits(p).double()
    ulp = torch.ldexp(torch.ones_like(c64), (e - 134).to(torch.int32))
    cs, ds = [], []
    for q in (0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75):
        d64 = q * ulp
        s64 = c64 + d64
        ok = (d64.bfloat16().double() == d64) & (s64.float().double() == s64) & (p < 0x7F80 if q else p >= 0)
        cs.append(p[ok])
        ds.append(d64[ok].bfloat16())
    neg = p[(p >= 1) & (p < 0x7F00)]                       # -2 c is a bf16 value below the last binade
    cs.append(neg)
    ds.append((-2.0 * _bf16_from_bits(neg).double()).bfloat16())
    nan = torch.tensor(float("nan")).bfloat16().view(torch.int16).long() & 0xffff
    one = torch.tensor(1.0).bfloat16()
    cs.append(torch.stack([torch.zeros((), dtype=torch.int64), nan, torch.tensor(0x3F80)]))
    ds.append(torch.stack([torch.tensor(-0.0).bfloat16(), one, torch.tensor(float("nan")).bfloat16()]))
    c, idt = _bf16_from_bits(torch.cat(cs)), torch.cat(ds)
    pad = -c.numel() % 4
    c, idt = torch.cat([c, torch.zeros(pad, dtype=torch.bfloat16)]), torch.cat([idt, torch.zeros(pad, dtype=torch.bfloat16)])
    s = c.double() + idt.double()
    fin = torch.isfinite(s)
    assert torch.equal((c.float() + idt.float()).double()[fin], s[fin]), "bf16_round_cases: a sum is not exact in fp32"
    return c, idt


def bf16_round_expect(c, idt):
    """what a bf16 store of relu(c + idt) holds, by torch's CPU conversion"""
    return (c.float() + idt.float()).relu().bfloat16()


def bf16_bits(t):
    """the bit patterns of a bf16 tensor as int64 in 0 .. 0xFFFF, every NaN as 0x7FC0 (NaN is compared as NaN)"""
    b = t.contiguous().view(torch.int16).long() & 0xffff
    return torch.where(torch.isnan(t.float()), torch.full_like(b, 0x7FC0), b)


def emulate_bf16_store(v32, how="rne"):
    """integer-arithmetic twin of the kernels' store conversion on the fp32 bit patterns of v32 -> bf16 tensor.  how: "rne" (add
    0x7FFF + the bit that becomes the last one, drop 16 bits: to nearest, ties to even; subnormals and the carry into Inf come out
    of the same addition), "trunc" (drop 16 bits), "away" (add 0x8000, drop 16 bits: ties away from zero) -- the two mistakes"""
    u = v32.contiguous().view(torch.int32).long() & 0xffffffff
    r = {"rne": (u + 0x7FFF + ((u >> 16) & 1)) >> 16, "trunc": u >> 16, "away": (u + 0x8000) >> 16}[how]
    r = torch.where(torch.isnan(v32), (u >> 16) | 0x40, r)
    r = torch.where(r >= 0x8000, r - 0x10000, r)
    return r.to(torch.int16).view(torch.bfloat16)


def misread_bf16_as_fp32(x16):
    """the addressing mistake of a kernel that reads a bf16 tensor x16 [rows][C] at fp32 stride: element i comes from bytes
    4 i .. 4 i + 3, the storage viewed as float32 pairs -- which exist for the first half of the elements only (the rest lies past
    the tensor's end: the reason the wrappers refuse mixed storage) -> fp32 [rows // 2][C]"""
    rows, C = x16.shape
    return x16.contiguous().view(torch.int16).reshape(-1).view(torch.float32)[:(rows // 2) * C].reshape(rows // 2, C)


# ------------------------------------------------------------------------------------------------
# activation plane images (koaf_act_planes): hi = fp16(x'), lo = fp16(x' - hi) of the transformed, scaled, clamped activation x'
# ------------------------------------------------------------------------------------------------
H16_MAX = 65504.0


def act_scale(amax=None, fscale=0.0):
    """the operand scale: 2^(15 - e) from amax = m 2^e, m in [0.5, 1) (e held to +-100; 1 when amax is not positive), else fscale,
    else 1 -- re-derived from math.frexp, not from the kernel"""
    if amax is not None:
        if not amax > 0.0:
            return 1.0
        e = min(max(math.frexp(amax)[1], -100), 100)
        return 2.0 ** (15 - e)
    return fscale if fscale != 0.0 else 1.0


def act_planes_ref(tf, x, fsc, sc=None, sh=None, x2=None, sc2=None):
    """float64 x' of fp32 / widened inputs x [npix][C] (x2 likewise), per-channel sc, sh, sc2 [C] -> (ref, e, raw, k):
    raw the unclamped value, ref = raw clamped to the fp16 range ([0, 65504] behind the ReLU of tf 1), k the fp32 roundings on
    the way to x' and e = k u sum|terms| fsc their bound.  fsc is a power of two: the products sc * fsc are exact, so
      tf 0: x * fsc -- exact, k = 0;
      tf 1: fmaf(x, sc fsc, sh fsc) -- k = 1 over |sc x| + |sh|;
      tf 2: fmaf(sc fsc, x, fmaf(-sc2 fsc, x2, sh fsc)) -- k = 2 over |sc x| + |sh| + |sc2 x2|.
    Clamping is 1-Lipschitz: e holds for the clamped value"""
    x64 = x.double()
    if tf == 0:
        raw, terms, k, lo = x64 * fsc, torch.zeros_like(x64), 0, -H16_MAX
    elif tf == 1:
        p = x64 * sc.double()
        raw, terms, k, lo = (p + sh.double()) * fsc, p.abs() + sh.double().abs(), 1, 0.0
    else:
        p, q = x64 * sc.double(), x2.double() * sc2.double()
        raw, terms, k, lo = (p + sh.double() - q) * fsc, p.abs() + sh.double().abs() + q.abs(), 2, -H16_MAX
    e = k * U * terms * fsc
    return raw.clamp(lo, H16_MAX), e, raw, k


def act_planes_bound(ref, e):
    """|hi + lo - ref|: x' is within e of ref, and split2h's contract (koaf_pieces.h) is hi = fp16(x'), lo = fp16(x' - hi) from
    the exact residual: |x' - hi| <= 2^-11 |x'|, and lo keeps that to 2^-11 relative again, or to half the fp16 subnormal spacing,
    2^-25: |hi + lo - x'| <= 2^-22 |x'| + 2^-25"""
    return e + 2.0 ** -22 * (ref.abs() + e) + 2.0 ** -25


def act_hi_decided(raw, e, tf):
    """-> bool mask: elements whose fp16 rounding the k roundings cannot change.  x' lies in [clamp(raw - e), clamp(raw + e)];
    fp16 rounding is monotone, so where both ends round (float64 -> fp16 directly, to nearest even: numpy's conversion) to the same
    fp16 value every x' in between does, and so does fl32(ref), which lies in between as well (k = 0: it is x' itself; k >= 1:
    e >= u |raw|).  The others straddle a rounding boundary and are left out of the bit comparison, counted"""
    lo = 0.0 if tf == 1 else -H16_MAX
    a = np.clip((raw - e).numpy(), lo, H16_MAX).astype(np.float16)
    b = np.clip((raw + e).numpy(), lo, H16_MAX).astype(np.float16)
    return torch.from_numpy(a == b)


def act_planes_unpack(planes, npix, C):
    """int16 [2 npix C + 8] -> (hi, lo) fp16 [npix][C] and the 8-element chunk behind them"""
    ps = npix * C
    assert planes.numel() == 2 * ps + 8
    p = planes.cpu()
    return p[:ps].view(torch.float16).reshape(npix, C), p[ps:2 * ps].view(torch.float16).reshape(npix, C), p[2 * ps:]


# (C, n8) of the per-element cases, n8 = npix C / 8 the kernel's work items (256 to a block): 1, 255, 256, 257 at C = 8; at C = 64
# n8 is a multiple of 8 (256, and 264 = 33 pixels: a second, ragged block); at C = 520 a multiple of 65 (65, and 260 = 4 pixels)
ACT_SHAPES = [(8, 1), (8, 255), (8, 256), (8, 257), (64, 256), (64, 264), (520, 65), (520, 260)]
ACT_CAP_N8 = 16384 * 256 + 1        # one work item past the kernel's own grid cap (16384 blocks), C = 8


def act_case(C, n8, tf, store, seed=0):
    """the inputs of one koaf_act_planes case -> dict(npix, x, x2, sc, sh, sc2, amax, fscale): CPU tensors, the activation among
    the sources (x for tf 0 / 1, x2 for tf 2) rounded to `store` and widened; sc in [0.75, 1.25], sh and sc2 of order 0.02, so the
    terms do not cancel to much less than their magnitudes (the share of undecided fp16 roundings stays near 2 k u / 2^-11).
    tf 1 runs at the fixed activation scale 16, tf 0 likewise, tf 2 at amax = 1.5 max|value|, a loose bound as koaf_bn_bwd_finalize's is"""
    npix = n8 * 8 // C
    assert npix * C == n8 * 8
    g = torch.Generator().manual_seed(3000 + seed + 7 * C + n8 % 100003 + 1000 * tf + (500 if store == torch.bfloat16 else 0))
    x = torch.randn(npix, C, generator=g)
    sc, sh, sc2 = torch.rand(C, generator=g) * 0.5 + 0.75, torch.randn(C, generator=g) * 0.02, torch.randn(C, generator=g) * 0.02
    x2 = amax = None
    fscale = 16.0
    if tf == 2:
        x2 = stored(torch.randn(npix, C, generator=g), store)
        amax = torch.tensor([1.5 * float((x.double() * sc.double() + sh.double() - x2.double() * sc2.double()).abs().max())])
        fscale = 0.0
    else:
        x = stored(x, store)
    return dict(npix=npix, x=x, x2=x2, sc=sc if tf else None, sh=sh if tf else None, sc2=sc2 if tf == 2 else None, amax=amax,
                fscale=fscale)


def emulate_act_planes(tf, x, fsc, sc=None, sh=None, x2=None, sc2=None):
    """numpy twin of the kernel's arithmetic -> (hi, lo) fp16: the fused multiply-adds are formed in float64 (the product of two
    fp32 values is exact there) and rounded to fp32, the clamp, hi = fp16(x'), lo = fp16(x' - hi) from the exact fp32 residual"""
    f32, f64 = np.float32, np.float64
    v = x.numpy().astype(f64)
    fsc = f32(fsc)
    if tf == 0:
        u, lo = (v * f64(fsc)).astype(f32), -H16_MAX
    elif tf == 1:
        a, b = (sc.numpy() * fsc).astype(f64), (sh.numpy() * fsc).astype(f64)
        u, lo = (v * a + b).astype(f32), 0.0
    else:
        a, b, k = (sc.numpy() * fsc).astype(f64), (sh.numpy() * fsc).astype(f64), (sc2.numpy() * fsc).astype(f64)
        inner = (-k * x2.numpy().astype(f64) + b).astype(f32)
        u, lo = (a * v + inner.astype(f64)).astype(f32), -H16_MAX
    xp = np.clip(u, f32(lo), f32(H16_MAX))
    hi = xp.astype(np.float16)
    return torch.from_numpy(hi), torch.from_numpy((xp - hi.astype(f32)).astype(np.float16))


def act_planes_check(hi, lo, tf, case, what):
    """the per-element asserts on (hi, lo) fp16 [npix][C] of one case (the kernel's on the GPU, the emulation's on the CPU)
    -> share of the elements left out of the bit comparison of hi"""
    fsc = act_scale(None if case["amax"] is None else float(case["amax"]), case["fscale"])
    ref, e, raw, k = act_planes_ref(tf, case["x"], fsc, case["sc"], case["sh"], case["x2"], case["sc2"])
    assert k == tf                          # tf 0: no rounding, tf 1: one fused multiply-add, tf 2: two
    got = hi.double() + lo.double()
    assert torch.isfinite(got).all(), what + ": non-finite pieces"
    err, bound = (got - ref).abs(), act_planes_bound(ref, e)
    assert (err <= bound).all(), (f"{what}: {int((err > bound).sum())}/{err.numel()} elements beyond k u sum|terms| fsc + 2^-22 |ref| + 2^-25 "
                                  f"(k = {k}); worst {float((err - bound).max()):.3e} over")
    ok = act_hi_decided(raw, e, tf)
    want = ref.float().half()
    same = hi.view(torch.int16) == want.view(torch.int16)
    assert same[ok].all(), f"{what}: hi is not fp16(x') bit for bit at {int((~same & ok).sum())} decided elements"
    return 1.0 - float(ok.double().mean())
