"""float64 references, derived error bounds and fp32 numpy restatements of the softmax losses (koaf_loss.hip) and the optimizer
steps (koaf_optim.hip), for test_loss_edges_gpu.py and test_optim_edges_gpu.py; checked on the CPU by
test_loss_optim_refs_cpu.py (the references against torch in float64, every bound from both sides).

Bounds.  u = 2^-24 (elem_refs.U).  One rounding costs u relative; sqrtf, the division, expf, logf, log1pf, expm1f are counted
as 1 ulp = 2 u, powf as 2 ulp = 4 u.  A chain of k roundings over terms t_i errs by at most gamma(k) * sum|t_i|, an fp32 sum
whose longest addition chain is m by gamma(m) * sum|t_i| (elem_refs.gamma).  A fused multiply-add rounds once where the count
below has two: every bound here holds with and without contraction.

Softmax losses.  The kernel forms, per element, with m the row maximum, jm its first index, s1 = sum_{j != jm} exp(x_j - m):
    ls = log1p(s1), log p_j = (x_j - m) - ls, logpt = w * log p_t, pt = exp(logpt), om = -expm1(logpt)
    focal: l = -om^g * logpt, dl = -om^g + g * om^(g - 1) * pt * logpt;  cross-entropy: l = -logpt, dl = -1
    d_j = (dl * w * wgt) * (j == t ? -expm1(log p_t) : -exp(log p_j))
Counts (units of u; C classes, g = gamma, a_j = m - x_j):
    ls:       s1 carries C - 2 additions, 2 per expf and the arguments' roundings (|a| e^-|a| <= 0.37 each): its error reaches
              log1p(s1) divided by 1 + s1, plus log1pf's 2 ls <= 2 log C: absolute <= 2 C + 4
    log p_j:  |x_j - m| + (2 C + 4) + |log p_j| absolute, so the RELATIVE error of p_j = exp(..) is <= 2 a_j + 2 C + 6 = kp_j.
              The target's factor 1 - p_t = -expm1(log p_t): where x_t = m, log p_t = -ls exactly and its relative error C + 3 passes
              through (p |log p| / (1 - p) <= 1): kp_t = C + 5; elsewhere p_t <= 1/2 and the absolute error is scaled by
              p_t / (1 - p_t) <= 1: kp_t = (2 a_t + 2 C + 4) p_t / (1 - p_t) + 2.  A group owes K_P = max_j (kp_j |d_j|) / max_j |d_j|:
              an element far below the maximum is charged its own spread only in proportion to its own size
    log p_t:  relative: C + 3 where x_t = m (s1's relative error and log1pf), 2 + (2 C + 4) / log 2 elsewhere (|log p_t| >= log 2),
              and the product with w                                                                          <= 3 C + 9 = K_LP
    om:       K_LP * p |logpt| / (1 - p) + 2 <= K_LP + 2;  om^g: g (K_LP + 2) + 4
    dl:       both terms have one sign.  g (K_LP + 2) + 4 for the first; the second adds |g - 1| (K_LP + 2) + 5 for the power,
              0.65 g K_LP + 2 for pt (pt logpt^2 / om <= 0.65), K_LP for logpt, two products and the sum
    d_j:      dl, then w, wgt (one reciprocal, and the denominator's own sum for a weighted mean) and the last product: 4
"""
import numpy as np
import torch
import torch.nn.functional as F

from elem_refs import U, gamma

LOSS_ONE_BLOCK = 8192       # koaf_loss.hip: elements one block covers; beyond it the grid form runs
LOSS_CHUNK = 4096           # elements per block of the grid form
MARGINS = (0, 1, 4, 8, 12, 16)


def cdiv(a, b):
    return -(-a // b)


def worst_fraction(got, ref, bound):
    """max over the elements of |got - ref| / bound (inf where got is not finite); <= 1 means inside the bound"""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    bound = np.broadcast_to(bound, err.shape)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bound)
    return float(f.max())


# =================================================================================================
# softmax losses
# =================================================================================================
def loss_inputs(B, C, S, seed, margins=MARGINS, sides=(1, -1)):
    """-> (x [B][C][S] fp32, target [B][S] int64, group [B][S] int64).  Logits are multiples of 2^-10, |x| < 16.  Element i has the
    confidence grade (margin, side) = grades[i % len]: its target logit is the best other logit + margin (side 1, winning) or
    - margin (side -1, losing); group = index into loss_groups(margins, sides).  C = 1 has no other class: group 0."""
    g = torch.Generator().manual_seed(seed)
    n = B * S
    grades = loss_groups(margins, sides)
    gi = torch.arange(n) % len(grades)
    mg = torch.tensor([a for a, _ in grades], dtype=torch.float64)[gi]
    sd = torch.tensor([s for _, s in grades], dtype=torch.float64)[gi]
    tg = torch.randint(0, C, (n,), generator=g)
    x = torch.randint(-1023, 1024, (n, C), generator=g).double() / 1024.0          # others in (-1, 1)
    if C > 1:
        x = x - (sd * mg / 2)[:, None]
        oh = F.one_hot(tg, C).bool()
        top = x.masked_fill(oh, -1e9).max(1).values
        x[oh] = top + sd * mg
    else:
        gi = torch.zeros(n, dtype=torch.int64)
    assert float(x.abs().max()) < 16 and torch.equal(x * 1024, (x * 1024).round())
    x = x.float().view(B, S, C).permute(0, 2, 1).contiguous()
    return x, tg.view(B, S), gi.view(B, S)


def loss_groups(margins=MARGINS, sides=(1, -1)):
    out = []
    for a in margins:
        for s in sides:
            if (a, s) not in out and not (a == 0 and s == -1 and (0, 1) in out):
                out.append((a, s))
    return out


def softmax_loss_ref(x, tg, cw=None, gamma_=2.0, focal=True, mean=True):
    """float64 formulas on the fp32 inputs.  x [B][C][...], tg [B][...], cw [C] or None
    -> dict(l = per-element loss (unreduced, 0 where the target is out of range), loss = reduced scalar, d = dlogits [B][C][...],
            wgt = the reduction's factor, valid = mask, nbad = out-of-range labels other than -100,
            kp [B][C][...] = the counted relative error of every element's softmax factor, in u (module docstring: kp_j))"""
    x64 = x.double()
    C = x.shape[1]
    valid = (tg >= 0) & (tg < C)
    t = tg.clamp(0, C - 1)
    m = x64.max(1, keepdim=True).values
    lsm = (x64 - m) - (x64 - m).exp().sum(1, keepdim=True).log()
    lp = lsm.gather(1, t.unsqueeze(1)).squeeze(1)
    w = torch.ones_like(lp) if cw is None else cw.double()[t]
    w = torch.where(valid, w, torch.zeros_like(w))
    logpt = w * lp
    if focal:
        pt, om = logpt.exp(), -torch.expm1(logpt)
        pw = om ** gamma_
        l = -pw * logpt
        dl = -pw + (0.0 if gamma_ == 0 else gamma_ * om ** (gamma_ - 1.0) * pt * logpt)
        wgt = 1.0 / valid.numel() if mean else 1.0
    else:
        l = -logpt
        dl = -torch.ones_like(logpt)
        wgt = 1.0 / float(w.sum()) if float(w.sum()) != 0 else float("inf")
    l = torch.where(valid, l, torch.zeros_like(l))
    oh = F.one_hot(t, C).movedim(-1, 1).double()
    d = (dl * w * wgt).unsqueeze(1) * (oh - lsm.exp())
    d = torch.where(valid.unsqueeze(1), d, torch.zeros_like(d))
    loss = l.sum() * wgt
    a = m - x64
    kp = 2 * a + 2 * C + 6
    at, pt_s = a.gather(1, t.unsqueeze(1)), lsm.gather(1, t.unsqueeze(1)).exp()
    kt = torch.where(at == 0, torch.full_like(at, C + 5.0), (2 * at + 2 * C + 4) * pt_s / (1 - pt_s).clamp_min(0.5) + 2)
    kp = kp.scatter(1, t.unsqueeze(1), kt)
    return dict(l=l, loss=loss, d=d, wgt=wgt, valid=valid, nbad=int(((~valid) & (tg != -100)).sum()), kp=kp)


def torch_loss_fp32(x, tg, cw=None, gamma_=2.0, focal=True, mean=True):
    """torch's own fp32 CPU result of the same operation (the yardstick): (loss, dlogits), as the reference's losses form them.
    A label outside [0, C) goes in as -100: torch refuses any other, the kernel treats them alike"""
    xx = x.clone().requires_grad_(True)
    tg = torch.where((tg < 0) | (tg >= x.shape[1]), torch.full_like(tg, -100), tg)
    if focal:
        logpt = -F.cross_entropy(xx, tg, weight=cw, reduction="none")
        l = -((1 - logpt.exp()) ** gamma_) * logpt
        loss = l.mean() if mean else l.sum()
    else:
        loss = F.cross_entropy(xx, tg, weight=cw)
    loss.backward()
    return loss.detach(), xx.grad


def loss_form(n):
    return "grid" if n > LOSS_ONE_BLOCK else "one-block"


def sum_chain(n):
    """longest chain of fp32 additions behind one sum over n elements in the form that runs.  One block: a lane adds
    ceil(n / 256) elements, the LDS tree 8 more.  Grid: 4096 / 256 = 16 per lane and the tree's 8 in every chunk, then the second
    stage over the ceil(n / 4096) partials: ceil(that / 256) per lane and 8."""
    if n <= LOSS_ONE_BLOCK:
        return cdiv(n, 256) + 8
    return min(n, LOSS_CHUNK) // 256 + 8 + cdiv(cdiv(n, LOSS_CHUNK), 256) + 8


def k_lp(C):
    return 3 * C + 9


def k_grad(n, C, gamma_, focal, weighted_mean, kp):
    """roundings of one gradient element of a group whose softmax factors owe K_P = kp, relative to the group's largest |d| (module
    docstring): K_P, the focal factor dl, the products with w and wgt, the reciprocal behind wgt and the last product (4), and for
    a weighted mean the chain of the denominator's sum"""
    if focal:
        kl = k_lp(C)
        kdl = (2.65 * gamma_ + abs(gamma_ - 1) + 1) * (kl + 2) + 15
    else:
        kdl = 0
    return int(np.ceil(kp + kdl + 4 + (sum_chain(n) if weighted_mean else 0)))


def loss_group_report(d, ref, dyard, group, ngroups, n, C, gamma_, focal, weighted_mean):
    """per confidence group: the 4 x yardstick rule with its counted floor.  d, dyard [B][C][...] (kernel, torch fp32), ref from
    softmax_loss_ref, group [B][...].  Elements whose target is out of range or whose class weight is 0 are left out (they are
    held to exactly 0 by the caller).  -> list of dict(group, err, yard, floor, bar, k, dmax, ok)"""
    d, dyard, d64 = (np.asarray(torch.as_tensor(a).double().movedim(1, -1).reshape(-1, C)) for a in (d, dyard, ref["d"]))
    grp = np.asarray(group.reshape(-1))
    keep = np.asarray((ref["valid"] & (ref["d"].abs().sum(1) > 0)).reshape(-1)) if C > 1 else np.asarray(ref["valid"].reshape(-1))
    ekp = np.asarray(ref["kp"].movedim(1, -1).reshape(-1, C)) * np.abs(d64)
    out = []
    for gi in range(ngroups):
        sel = keep & (grp == gi)
        if not sel.any():
            continue
        dmax = float(np.abs(d64[sel]).max())
        k = k_grad(n, C, gamma_, focal, weighted_mean, float(ekp[sel].max()) / dmax if dmax > 0 else 0.0)
        fin = bool(np.isfinite(d[sel]).all())
        err = float(np.abs(d[sel] - d64[sel]).max()) if fin else float("inf")
        yard = float(np.abs(dyard[sel] - d64[sel]).max())
        floor = gamma(k) * dmax
        bar = max(4 * yard, floor)
        out.append(dict(group=gi, err=err, yard=yard, floor=floor, bar=bar, k=k, dmax=dmax, ok=err <= bar))
    return out


def loss_scalar_report(loss, ref, lyard, n, C, gamma_, focal, weighted_mean):
    """the same rule for the reduced loss: floor gamma(m) * sum|l_i| * wgt, m = sum_chain(n): the longest addition chain of the
    form that ran and nothing else"""
    m = sum_chain(n)
    floor = gamma(m) * float(ref["l"].abs().sum()) * ref["wgt"]
    err, yard = abs(float(loss) - float(ref["loss"])), abs(float(lyard) - float(ref["loss"]))
    bar = max(4 * yard, floor)
    return dict(err=err, yard=yard, floor=floor, bar=bar, m=m, ok=bool(np.isfinite(float(loss))) and err <= bar)


# ---- fp32 numpy restatement of the kernel (its arithmetic and its summation order), with faults to plant --------------------
def _lane_tree(v):
    """v [..., k, 256] fp32: each of 256 lanes adds its k values in order, then the LDS tree -> [...]"""
    acc = np.zeros(v.shape[:-2] + (256,), dtype=np.float32)
    for i in range(v.shape[-2]):
        acc = acc + v[..., i, :]
    o = 128
    while o > 0:
        acc = acc[..., :o] + acc[..., o:2 * o]
        o >>= 1
    return acc[..., 0]


def emulate_sum(v, drop_chunk=None):
    """the kernels' sum of v [n] fp32 in the form that runs for n elements; drop_chunk: leave that chunk's partial out"""
    v = np.asarray(v, dtype=np.float32)
    n = v.size
    if n <= LOSS_ONE_BLOCK:
        k = cdiv(n, 256)
        return _lane_tree(np.pad(v, (0, k * 256 - n)).reshape(k, 256))
    nblk = cdiv(n, LOSS_CHUNK)
    part = _lane_tree(np.pad(v, (0, nblk * LOSS_CHUNK - n)).reshape(nblk, LOSS_CHUNK // 256, 256))
    if drop_chunk is not None:
        part[drop_chunk] = 0
    k = cdiv(nblk, 256)
    return _lane_tree(np.pad(part, (0, k * 256 - nblk)).reshape(k, 256))


def loss_kernel_f32(x, tg, cw=None, gamma_=2.0, focal=True, mean=True, lse_form=False, count_ignored=False, drop_chunk=None):
    """-> (loss fp32, dlogits [B][C][...] fp32).  Faults: lse_form -- lse = m + log s and x - lse, as the kernel had it;
    count_ignored -- the weighted mean's denominator counts out-of-range targets with weight 1; drop_chunk -- that chunk's loss
    partial is left out of the second stage"""
    f = np.float32
    xs = np.asarray(x.movedim(1, -1).reshape(-1, x.shape[1]), dtype=f)          # [n][C]
    t = np.asarray(tg.reshape(-1))
    n, C = xs.shape
    valid = (t >= 0) & (t < C)
    tc = np.clip(t, 0, C - 1)
    w = np.ones(n, dtype=f) if cw is None else np.asarray(cw, dtype=f)[tc]
    if focal:
        wsum = f(n)
    else:
        wsum = emulate_sum(np.where(valid, w, f(1) if count_ignored else f(0)).astype(f))
    with np.errstate(all="ignore"):
        wgt = f(1) / wsum if mean or not focal else f(1)
        m = xs.max(1)
        jm = xs.argmax(1)                   # (first index of the maximum, as the kernel's strict comparison keeps it)
        xt = xs[np.arange(n), tc]
        if lse_form:
            s = np.zeros(n, dtype=f)
            for j in range(C):
                s = s + np.exp(xs[:, j] - m)
            lse = m + np.log(s)
            lp = xt - lse
            logp = xs - lse[:, None]
            omp = f(1) - np.exp(lp)
        else:
            s1 = np.zeros(n, dtype=f)
            for j in range(C):
                s1 = s1 + np.where(jm == j, f(0), np.exp(xs[:, j] - m))
            ls = np.log1p(s1)
            lp = (xt - m) - ls
            logp = (xs - m[:, None]) - ls[:, None]
            omp = -np.expm1(lp)
        logpt = w * lp
        if focal:
            pt = np.exp(logpt)
            om = f(1) - pt if lse_form else -np.expm1(logpt)
            g = f(gamma_)
            pw = np.power(om, g)
            li = -pw * logpt
            pw1 = np.zeros(n, dtype=f) if gamma_ == 0 else g * np.power(om, g - f(1))
            dl = -pw + pw1 * pt * logpt
        else:
            li = -logpt
            dl = np.full(n, -1, dtype=f)
        c = dl * w * wgt
        term = -np.exp(logp)
        term[np.arange(n), tc] = omp
        d = np.where(valid[:, None], c[:, None] * term, f(0)).astype(f)
        li = np.where(valid, li, f(0)).astype(f)
        loss = f(emulate_sum(li, drop_chunk) * wgt)
    return loss, torch.from_numpy(d.reshape(tuple(tg.shape) + (C,))).movedim(-1, 1).contiguous()


# =================================================================================================
# optimizer steps: one step of each rule in float64, as a pure function of (p, g, state, scalars)
# =================================================================================================
def _f32(v):
    return float(np.float32(v))


def sgd_scalars(lr, momentum=0.0, dampening=0.0, wd=0.0, maximize=False):
    """the scalars as sgd_kernel receives them (koaf_sgd_step): lr, weight decay as floats, mu = float(momentum),
    omd = float(1 - dampening) from the double difference, sign = -1 | 1"""
    return dict(lr=_f32(lr), mu=_f32(momentum), omd=_f32(1.0 - dampening), wd=_f32(wd), sign=-1.0 if maximize else 1.0)


def rms_scalars(lr, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0, maximize=False):
    """koaf_rmsprop_step: al = float(alpha), oma = float(1 - alpha) from the double difference"""
    return dict(lr=_f32(lr), alpha=_f32(alpha), oma=_f32(1.0 - alpha), eps=_f32(eps), wd=_f32(wd), mu=_f32(momentum),
                sign=-1.0 if maximize else 1.0)


def adam_scalars(lr, b1, b2, eps, wd, step):
    """koaf_adam_step: omb1 = float(1 - beta1), b2 = float(beta2), omb2 = float(1 - beta2), step_size = float(double(float lr) /
    (1 - beta1^step)), bc2_sqrt = float(sqrt(1 - beta2^step)); adam_hyper_kernel derives the last two by the same formulas"""
    lr = _f32(lr)
    return dict(lr=lr, omb1=_f32(1.0 - b1), b2=_f32(b2), omb2=_f32(1.0 - b2), eps=_f32(eps), wd=_f32(wd),
                step_size=_f32(lr / (1.0 - b1 ** step)), bc2_sqrt=_f32(np.sqrt(1.0 - b2 ** step)))


def adam_hyper_ref(lr32, b1, b2, step):
    """hyper[3] after koaf_adam_hyper has advanced the device step to `step`: float32 of the float64 formulas"""
    lr = float(np.float32(lr32))
    return np.array([lr, lr / (1.0 - b1 ** step), np.sqrt(1.0 - b2 ** step)], dtype=np.float64)


SLACK = 1.0 + 1e-4      # the second order: every count below stays under 200, (200 u)^2 / (200 u) = 1.2e-5


def _d(t):
    return torch.as_tensor(t).double()


def sgd_step64(p, g, buf, sc, mom=False, nest=False, first=False):
    """-> dict(p, buf) and bounds dict(p, buf) per element.  Counts (k beside each line, units of u * the terms named):
    g' = sign g + wd p: 2 over |g| + |wd p| (0 without weight decay: the sign is exact);  buf = mu buf + omd g': g' again, the two
    products and the sum: 4 over |mu buf| + |omd| (|g| + |wd p|);  first: buf = g';  Nesterov st = g' + mu buf: 6;
    p -= lr st: st's count + 2 over |p| + |lr| * st's terms   -> K_SGD = 8 (Nesterov), 6 (momentum), 4 (plain)"""
    p, g = _d(p), _d(g)
    lr, mu, omd, wd, sign = sc["lr"], sc["mu"], sc["omd"], sc["wd"], sc["sign"]
    g1 = sign * g + wd * p
    Tg = g.abs() + (wd * p).abs()
    kg = 2 if wd != 0 else 0
    out, bnd = {}, {}
    if mom:
        if first:
            b1, Tb, kb = g1, Tg, kg
        else:
            b = _d(buf)
            b1 = mu * b + omd * g1
            Tb, kb = (mu * b).abs() + abs(omd) * Tg, kg + 2
        st, Ts, ks = (g1 + mu * b1, Tg + abs(mu) * Tb, kb + 2) if nest else (b1, Tb, kb)
        out["buf"], bnd["buf"] = b1, gamma(max(kb, 1)) * Tb * SLACK
    else:
        st, Ts, ks = g1, Tg, kg
    out["p"] = p - lr * st
    bnd["p"] = gamma(ks + 2) * (p.abs() + abs(lr) * Ts) * SLACK
    return out, bnd


def rms_step64(p, g, sq, gavg, buf, sc):
    """-> dict(p, sq[, gavg][, buf]) and per-element bounds.  E(.) are absolute errors in units of u (module docstring for the unit
    costs):  E(g') = 2 (|g| + |wd p|);  sq' = alpha sq + (oma g') g': E = 2 |alpha sq| + (3 |B| + 2 E(g') |oma g'|), B the second term;
    centered: d = g' - ga: E(d) = E(g') + |d|;  oma < 0.5: ga' = ga + oma d: oma E(d) + |oma d| + |ga'|, else ga' = g' - d (1 - oma):
    E(g') + (1 - oma) E(d) + 2 |d (1 - oma)| + |ga'|;  var = sq' - ga'^2: E(sq') + 2 E(ga') |ga'| + ga'^2 + |var| -- divided by var this
    is where (sq + ga^2) / (sq - ga^2) enters;  avg = sqrt(.) + eps: half the relative error under the root, 2 for sqrtf, 1 for the
    sum;  q = g' / avg: + 2;  buf' = mu buf + q;  p' = p - lr (q | buf'): the product and the difference"""
    p, g, sq = _d(p), _d(g), _d(sq)
    lr, al, oma, eps, wd, mu, sign = (sc[k] for k in ("lr", "alpha", "oma", "eps", "wd", "mu", "sign"))
    g1 = sign * g + wd * p
    Eg = 2 * (g.abs() + (wd * p).abs()) if wd != 0 else torch.zeros_like(g)
    A, Bt = al * sq, oma * g1 * g1
    sq1 = A + Bt
    Esq = 2 * A.abs() + 3 * Bt.abs() + 2 * Eg * (oma * g1).abs()
    out, bnd = {"sq": sq1}, {"sq": U * Esq * SLACK}
    if gavg is not None:
        ga = _d(gavg)
        d = g1 - ga
        Ed = Eg + d.abs()
        ga1 = ga + oma * d
        if oma < 0.5:
            Ega = oma * Ed + (oma * d).abs() + ga1.abs()
        else:
            Ega = Eg + (1 - oma) * Ed + 2 * (d * (1 - oma)).abs() + ga1.abs()
        var = sq1 - ga1 * ga1
        Evar = Esq + 2 * Ega * ga1.abs() + ga1 * ga1 + var.abs()
        out["gavg"], bnd["gavg"] = ga1, U * Ega * SLACK
    else:
        var, Evar = sq1, Esq
    root = var.sqrt()
    avg = root + eps
    Eavg = (Evar / var / 2 + 2) * root + avg
    q = g1 / avg
    Eq = Eg / avg + (Eavg / avg + 2) * q.abs()
    if buf is not None:
        b = _d(buf)
        b1 = mu * b + q
        Eb = 2 * (mu * b).abs() + Eq + q.abs()
        out["buf"], bnd["buf"] = b1, U * Eb * SLACK
        out["p"] = p - lr * b1
        bnd["p"] = U * (abs(lr) * Eb + 2 * abs(lr) * ((mu * b).abs() + q.abs()) + p.abs()) * SLACK
    else:
        out["p"] = p - lr * q
        bnd["p"] = U * (abs(lr) * Eq + 2 * (lr * q).abs() + p.abs()) * SLACK
    return out, bnd


def adam_step64(p, g, m, v, vmax, sc, adamw=False):
    """-> dict(p, m, v[, vmax]) and per-element bounds.  adamw: p1 = p (1 - lr wd): the product lr wd, the difference, the product:
    3 |p1|;  else g' = g + wd p: 2 (|g| + |wd p|).  m' = m + (g' - m) omb1: E(d) = E(g') + |d|, then omb1 E(d) + |omb1 d| + |m'|.
    v' = v b2 + (omb2 g') g': 2 |v b2| + 3 |B| + 2 E(g') |omb2 g'|.  vd = max(vmax, v') inherits at most E(v').  denom = sqrt(vd) /
    bc2_sqrt + eps: half of vd's relative error, 2 + 2 for sqrtf and the division, 1 for the sum.  q = m' / denom: + 2.
    p' = p1 - step_size q: the product and the difference."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    lr, omb1, b2, omb2, eps, wd, ss, bc = (sc[k] for k in ("lr", "omb1", "b2", "omb2", "eps", "wd", "step_size", "bc2_sqrt"))
    if adamw:
        p1, Ep1 = p * (1.0 - lr * wd), 3 * (p * (1.0 - lr * wd)).abs()
        g1, Eg = g, torch.zeros_like(g)
    else:
        p1, Ep1 = p, torch.zeros_like(p)
        g1 = g + wd * p
        Eg = 2 * (g.abs() + (wd * p).abs()) if wd != 0 else torch.zeros_like(g)
    d = g1 - m
    m1 = m + d * omb1
    Em = omb1 * (Eg + d.abs()) + (omb1 * d).abs() + m1.abs()
    A, Bt = v * b2, omb2 * g1 * g1
    v1 = A + Bt
    Ev = 2 * A.abs() + 3 * Bt.abs() + 2 * Eg * (omb2 * g1).abs()
    out, bnd = {"m": m1, "v": v1}, {"m": U * Em * SLACK, "v": U * Ev * SLACK}
    vd = v1
    if vmax is not None:
        vd = torch.maximum(_d(vmax), v1)
        out["vmax"] = vd
    S = vd.sqrt() / bc
    den = S + eps
    Eden = (Ev / vd / 2 + 4) * S + den
    q = m1 / den
    Eq = Em / den + (Eden / den + 2) * q.abs()
    out["p"] = p1 - ss * q
    bnd["p"] = U * (Ep1 + abs(ss) * Eq + (ss * q).abs() + p1.abs() + (ss * q).abs()) * SLACK
    return out, bnd


# ---- fp32 numpy restatements of the three kernels, with and without fused multiply-adds, with faults to plant ----------------
class F32:
    """fp32 arithmetic on numpy arrays; fused: a * b + c rounds once (the exact float64 product, one rounding of the sum)"""

    def __init__(self, fused):
        self.fused = fused

    def mad(self, a, b, c):
        a, b, c = (np.asarray(t, dtype=np.float32) for t in (a, b, c))
        if self.fused:
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        return a * b + c


def _tail_mask(n, skip_tail):
    keep = np.ones(n, dtype=bool)
    if skip_tail:
        keep[(n // 4) * 4:] = False
    return keep


def sgd_kernel_f32(p, g, buf, sc, mom=False, nest=False, first=False, fused=False, skip_tail=False, ignore_first=False,
                   wd_after_moment=False):
    """faults: skip_tail -- the n % 4 tail is not updated; ignore_first -- the buffer is read on the first step;
    wd_after_moment -- the buffer takes the gradient before the weight decay is added"""
    f, A = np.float32, F32(fused)
    p0, g, b0 = np.asarray(p, dtype=f), np.asarray(g, dtype=f), None if buf is None else np.asarray(buf, dtype=f)
    lr, mu, omd, wd, sign = (f(sc[k]) for k in ("lr", "mu", "omd", "wd", "sign"))
    with np.errstate(all="ignore"):
        g1 = A.mad(wd, p0, sign * g)
        st, b1 = g1, None
        if mom:
            gm = sign * g if wd_after_moment else g1
            b1 = gm if (first and not ignore_first) else A.mad(mu, b0, omd * gm)
            st = A.mad(mu, b1, g1) if nest else b1
        p1 = A.mad(-lr, st, p0)
    keep = _tail_mask(p0.size, skip_tail)
    out = {"p": np.where(keep, p1, p0)}
    if mom:
        out["buf"] = np.where(keep, b1, b0)
    return out


def rms_kernel_f32(p, g, sq, gavg, buf, sc, fused=False, skip_tail=False, wd_after_moment=False):
    f, A = np.float32, F32(fused)
    p0, g, s0 = (np.asarray(t, dtype=f) for t in (p, g, sq))
    lr, al, oma, eps, wd, mu, sign = (f(sc[k]) for k in ("lr", "alpha", "oma", "eps", "wd", "mu", "sign"))
    with np.errstate(all="ignore"):
        g1 = A.mad(wd, p0, sign * g)
        gs = sign * g if wd_after_moment else g1
        s1 = A.mad(oma * gs, gs, al * s0)
        out = {}
        if gavg is not None:
            a0 = np.asarray(gavg, dtype=f)
            a1 = A.mad(oma, g1 - a0, a0) if oma < f(0.5) else A.mad(-(g1 - a0), f(1) - oma, g1)
            avg = np.sqrt(A.mad(-a1, a1, s1)) + eps
            out["gavg"] = a1
        else:
            avg = np.sqrt(s1) + eps
        if buf is not None:
            b1 = A.mad(mu, np.asarray(buf, dtype=f), g1 / avg)
            p1 = A.mad(-lr, b1, p0)
            out["buf"] = b1
        else:
            p1 = A.mad(-lr, g1 / avg, p0)
    out["p"], out["sq"] = p1, s1
    keep = _tail_mask(p0.size, skip_tail)
    old = {"p": p0, "sq": s0, "gavg": gavg, "buf": buf}
    return {k: np.where(keep, val, np.asarray(old[k], dtype=f)) for k, val in out.items()}


def adam_kernel_f32(p, g, m, v, vmax, sc, adamw=False, fused=False, skip_tail=False, wd_after_moment=False, no_writeback=False):
    """faults: wd_after_moment -- the first moment takes the gradient before the (coupled) weight decay is added;
    no_writeback -- amsgrad's maximum is used but not stored"""
    f, A = np.float32, F32(fused)
    p0, g0, m0, v0 = (np.asarray(t, dtype=f) for t in (p, g, m, v))
    lr, omb1, b2, omb2, eps, wd, ss, bc = (f(sc[k]) for k in ("lr", "omb1", "b2", "omb2", "eps", "wd", "step_size", "bc2_sqrt"))
    with np.errstate(all="ignore"):
        if adamw:
            pj, gj = p0 * A.mad(-lr, wd, f(1)), g0
        else:
            pj, gj = p0, A.mad(wd, p0, g0)
        gm = g0 if wd_after_moment else gj
        m1 = A.mad(gm - m0, omb1, m0)
        v1 = A.mad(omb2 * gj, gj, v0 * b2)
        out = {"m": m1, "v": v1}
        vd = v1
        if vmax is not None:
            x0 = np.asarray(vmax, dtype=f)
            vd = np.maximum(x0, v1)
            out["vmax"] = x0 if no_writeback else vd
        den = np.sqrt(vd) / bc + eps
        out["p"] = A.mad(-ss, m1 / den, pj)
    keep = _tail_mask(p0.size, skip_tail)
    old = {"p": p0, "m": m0, "v": v0, "vmax": vmax}
    return {k: np.where(keep, val, np.asarray(old[k], dtype=f)) for k, val in out.items()}


def optim_inputs(n, seed, pad=0, sentinel=0.0):
    """random, non-trivial operands and state of n elements (+ pad sentinel elements): p, g, buf, gavg signed; sq, v, vmax >= 0.
    |gavg| <= 0.5 sqrt(sq) (the centered RMSprop's variance keeps half of sq at least); vmax lies below the new second moment in the even
    elements and above it in the odd ones for the usual beta2 (0.5 v | 2 (v + g^2))"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n, generator=gen)         # noqa: E731
    p, g, buf, m = r(), r(), r() * 0.5, r() * 0.3
    sq = torch.rand(n, generator=gen) + 0.05
    gavg = (torch.rand(n, generator=gen) - 0.5) * sq.sqrt()
    v = torch.rand(n, generator=gen) * 0.5 + 0.01
    odd = (torch.arange(n) % 2).bool()
    vmax = torch.where(odd, 2 * (v + g * g), 0.5 * v)
    out = dict(p=p, g=g, buf=buf, m=m, sq=sq, gavg=gavg, v=v, vmax=vmax)
    if pad:
        out = {k: torch.cat([t, torch.full((pad,), sentinel)]) for k, t in out.items()}
    return out
