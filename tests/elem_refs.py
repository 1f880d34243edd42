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


def draw_preact(gen, shape, sc, sh, scale=1.0):
    """fp32 randn tensor [..., C] with no borderline element (rejected and redrawn, not excluded from the comparison)"""
    c = torch.randn(*shape, generator=gen) * scale
    for _ in range(64):
        bad = borderline(c, sc, sh)
        n = int(bad.sum())
        if n == 0:
            return c
        c[bad] = torch.randn(n, generator=gen) * scale
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
