"""Cases and references for the BatchNorm (csrc/batchnorm.hip) and 2-D pooling (csrc/elementwise.hip) edge tests.

Pure torch, no GPU needed to import. Two kinds of reference:

* exact: small-integer bf16 data (|x|, |dz| <= 4, means in multiples of 0.5), so every partial sum is a multiple of 0.5
  below 2^23 and fp32 addition is exact in any order, atomics included. The oracles are fp64 / integer sums and the
  kernels are held to equality;
* element-wise: Gaussian bf16 data against fp64, with a per-element bound made of the output's bf16 rounding and the
  fp32 roundings of the terms (``apply_bound``), or a distance in fp32 ulps (``ulps``).

The oracles take tensors on any device (the two block-cap pooling cases are too large for a CPU oracle to stay quick;
they are evaluated with the same torch code on the device). tests/test_bn_pool_edges_cpu.py checks this file on its own.
"""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
CL = torch.channels_last
STAT_SLOTS = 128                 # BIGDL_STAT_SLOTS (csrc/kernels.h); the GPU test asserts it against the extension
EXACT_LIMIT = 2 ** 23            # sums of multiples of 0.5: below 2^23 every partial sum is an fp32 number
XMAX, DMAX, MEANMAX = 4, 4, 2.0

# channel counts: G = C / 8 groups; 256 / G rows per iteration, 256 % G idle threads, 256-group chunks
BN_CHANNELS = (8, 24, 40, 88, 64, 1032, 2048, 2056, 4096)
UNROLL = 4                       # default row unroll of the streaming passes (BIGDL_BN_UNROLL)


# ------------------------------------------------------------------ launch geometry (mirrors of the host code)
def rpi_of(C):
    """Rows per iteration of a 256-thread block in the first 256-group chunk."""
    return 256 // min(C // 8, 256)


def reduce_geometry(P, C, det=False):
    """(blocks, rows per block, capped) of launch_reduce."""
    rpi = rpi_of(C)
    want = -(-P // (rpi * 16))
    blocks = min(want, 2048)
    if det:
        blocks = min(blocks, 2 * STAT_SLOTS)
    capped = blocks < want
    blocks = max(blocks, 1)
    rpb = -(-P // blocks)
    return -(-P // rpb), rpb, capped


def stationary_geometry(P, C):
    """(bx, gy, rows per block, capped) of stationary_grid."""
    G = C // 8
    rpi, gy = rpi_of(C), -(-G // 256)
    rpb = rpi * 8
    bx = -(-P // rpb)
    cap = 8192 // gy
    capped = bx > cap
    if capped:
        bx = cap
        rpb = -(-P // bx)
    return max(bx, 1), gy, rpb, capped


def row_counts(C):
    """P = 1; rpi - 1, rpi, rpi + 1; a count that is no multiple of U * rpi (the unrolled tail re-reads row rbeg and must
    add nothing); one past a whole number of rows-per-block of the apply passes (8 rpi); one past two nominal blocks of the reduction
    (16 rpi each; launch_reduce re-balances them into three blocks with a shorter last one)."""
    rpi = rpi_of(C)
    ps = {1, rpi - 1, rpi, rpi + 1, 2 * UNROLL * rpi + rpi + 2, 3 * 8 * rpi + 1, 2 * 16 * rpi + 1}
    return sorted(p for p in ps if p >= 1)


# block-cap cases (C, P): the workload's branch of each launch
REDUCE_CAP = (1032, 2048 * 16 + 1)          # launch_reduce: blocks > 2048
APPLY_CAP = (2056, 4096 * 8 + 1)            # stationary_grid: bx > 8192 / gy with gy = 2
DET_CAP = (2048, 256 * 16 + 1)              # deterministic mode: blocks > 2 * STAT_SLOTS


# ------------------------------------------------------------------ integer data
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def int_rows(P, C, seed, lim=XMAX):
    return torch.randint(-lim, lim + 1, (P, C), generator=_gen(P, C, seed, lim)).to(BF)


def half_means(C, seed):
    """Multiples of 0.5 in [-MEANMAX, MEANMAX]."""
    n = int(2 * MEANMAX)
    return torch.randint(-n, n + 1, (C,), generator=_gen(C, seed, 5)).float() / 2


def stats_inputs(P, C):
    """Integer x whose last row, and the last row of every reduction block, is 3 or 4 everywhere: a dropped or doubled
    tail row changes both sums in every channel."""
    x = int_rows(P, C, 1)
    _, rpb, _ = reduce_geometry(P, C)
    mark = (3 + (torch.arange(C) % 2)).to(BF)
    x[rpb - 1::rpb] = mark
    x[P - 1] = mark
    return x


def stats_oracle(x):
    xd = x.double()
    return xd.sum(0), (xd * xd).sum(0)


MASKS = ("none", "z", "zm", "aff", "zm+aff")


def pack_mask(m):
    """bool [P, C] -> uint8 [P * C / 8]: bit e of byte (p, g) is element 8 g + e."""
    P, C = m.shape
    w = (2 ** torch.arange(8, device=m.device)).to(torch.int32)
    return (m.view(P, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)


def unpack_mask(zm, P, C):
    b = zm.view(P, C // 8, 1).to(torch.int32)
    return ((b >> torch.arange(8, device=zm.device).view(1, 1, 8)) & 1).bool().view(P, C)


def aff_exact(C, seed):
    """[scale | shift] with bf16-representable entries (x * scale + shift of an integer |x| <= 4 is then an fp32 number,
    so the fused multiply-add, its fp64 evaluation and any unfused form agree), except the first two channels:
      0: scale 1, shift -3: x = 3 gives exactly 0 (masked), x = 4 gives 1;
      1: scale 1 + 3 * 2^-23, shift -(3 + 2^-20): x = 3 gives 3 + 4.5 ulp - (3 + 4 ulp) = 2^-23 > 0 (ulp = 2^-22) under
         the fused multiply-add of the kernels; a separately rounded product (3 + 4 ulp, ties to even) would give 0."""
    g = _gen(C, seed, 7)
    scale = ((torch.randn(C, generator=g) * 0.7).to(BF).float())
    scale[scale == 0] = 0.5
    shift = (torch.randn(C, generator=g) * 1.5).to(BF).float()
    scale[0], shift[0] = 1.0, -3.0
    scale[1], shift[1] = 1.0 + 3 * 2.0 ** -23, -(3.0 + 2.0 ** -20)
    return torch.cat([scale, shift])


def aff_pre(x, aff):
    """fp64 value of fma(x, scale, shift): the product is exact in fp64 (8 x 24 bits), the sum has the sign of the exact
    sum, which is the sign of the fp32 fused multiply-add (no underflow in these ranges)."""
    C = x.shape[-1]
    a = aff.to(x.device).double()
    return x.double() * a[:C] + a[C:]


def mask_inputs(kind, P, C, x):
    """(z, zm, aff, expected bool mask) of one mask source; everything the kernel reads is written here."""
    z = zm = aff = None
    m = torch.ones(P, C, dtype=torch.bool)
    if kind == "z":
        z = torch.randint(-2, 3, (P, C), generator=_gen(P, C, 11)).to(BF)
        z.view(-1)[::7] = -0.0                  # -0.0 and +0.0 are both "not positive"
        z.view(-1)[3::11] = 2.0 ** -126         # the smallest normal is positive
        m = z.float() > 0
    if kind in ("zm", "zm+aff"):
        n = P * C // 8
        zm = ((torch.arange(n) * 37 + 11) % 256).to(torch.uint8)   # every byte value once n >= 256
        m = unpack_mask(zm, P, C)
    if kind in ("aff", "zm+aff"):
        aff = aff_exact(C, 3)
        if kind == "aff":
            m = aff_pre(x, aff) > 0
    return z, zm, aff, m


def bwd_reduce_oracle(dz, x, mean, mask):
    """(sum dz m, sum dz m (x - mean)) per channel in fp64."""
    d = dz.double() * mask.to(dz.device).double()
    return d.sum(0), (d * (x.double() - mean.to(x.device).double())).sum(0)


def abs_budget(dz, x, mean):
    """Largest sum of |terms| any channel can reach: the exactness budget of a case, from the data alone."""
    d = dz.double().abs()
    return max(d.sum(0).max().item(), (d * (x.double() - mean.double()).abs()).sum(0).max().item(),
               (x.double() ** 2).sum(0).max().item())


def exact_coef_inputs(C, P, seed):
    """invstd, gamma, mean and a one-slot `red` for which A, B, D of bn_bwd_coeff_kernel are exact in fp32 whatever the
    contraction: invstd and gamma are powers of two, red = P * (j / 64) so the means are j / 64, mean in quarters."""
    g = _gen(C, P, seed, 13)
    invstd = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    gamma = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (C,), generator=g)).float()
    mean = torch.randint(-8, 9, (C,), generator=g).float() / 4
    j = torch.randint(-128, 129, (2, C), generator=g).float()
    red = (j * P / 64).reshape(-1)
    assert P * 128 < 2 ** 24
    return invstd, gamma, mean, red


def coeff_ref(red, nslots, mean, invstd, gamma, P, training):
    """fp64 A, B, D, dgamma increment, dbeta increment of bn_bwd_coeff_kernel. red: [nslots][2][C] or None."""
    C = mean.numel()
    is_, mu = invstd.double(), mean.double()
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    A = g * is_
    if not training:
        z = torch.zeros(C, dtype=torch.float64)
        return {"A": A, "B": z, "D": z.clone(), "dgamma": z.clone(), "dbeta": z.clone()}
    s = red.double().view(nslots, 2, C).sum(0)
    mdy, mdyx = s[0] / P, s[1] / P * is_
    return {"A": A, "B": -g * is_ * is_ * mdyx, "D": g * is_ * (mu * is_ * mdyx - mdy), "dgamma": s[1] * is_,
            "dbeta": s[0], "D_terms": (g * is_ * mu * is_ * mdyx).abs().maximum((g * is_ * mdy).abs())}


def finalize_ref(stats, nslots, gamma, beta, rmean, rvar, P, eps, momentum, training):
    """fp64 outputs of bn_finalize_kernel. The variance is clamped at 0 as the kernel's is."""
    C = stats.numel() // (2 * max(nslots, 1)) if training else rmean.numel()
    out = {}
    if training:
        s = stats.double().view(nslots, 2, C).sum(0)
        mean = s[0] / P
        var = (s[1] / P - mean * mean).clamp_min(0)
        out["var_raw"] = s[1] / P - mean * mean
        if rmean is not None:
            unb = var * P / (P - 1) if P > 1 else var
            out["running_mean"] = momentum * mean + (1 - momentum) * rmean.double()
            out["running_var"] = momentum * unb + (1 - momentum) * rvar.double()
            out["running_var_terms"] = (momentum * unb).abs().maximum(((1 - momentum) * rvar.double()).abs())
            out["running_mean_terms"] = (momentum * mean).abs().maximum(((1 - momentum) * rmean.double()).abs())
    else:
        mean, var = rmean.double(), rvar.double()
    invstd = (var + eps).rsqrt()
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    out.update(save_mean=mean, save_invstd=invstd, scale=g * invstd, shift=b - mean * g * invstd,
               shift_terms=b.abs().maximum((mean * g * invstd).abs()))
    return out


def slot_buffer(C, nslots, fill, seed, mean=0.3, std=1.0, P=1000):
    """Synthetic [nslots][2][C] statistics whose slot sums are those of P rows of N(mean_c, std_c): `fill` = "all",
    "high" (slots >= 32 only) or "one" (nslots = 1)."""
    g = _gen(C, nslots, seed, 17)
    mu = torch.randn(C, generator=g) * mean
    sd = torch.rand(C, generator=g) * std + 0.5
    s1, s2 = mu * P, (sd * sd + mu * mu) * P
    w = torch.rand(nslots, 1, generator=g) + 0.1
    if fill == "high":
        w[:32] = 0
    w = w / w.sum()
    return torch.stack([w * s1, w * s2], 1).float().contiguous()     # [nslots][2][C]


# ------------------------------------------------------------------ fp32 ulps and the bf16 output bound
def spacing(v, mant):
    """Spacing of a binary format with `mant` explicit mantissa bits at |v| (fp64 tensor); normal range."""
    e = torch.frexp(v.abs().clamp_min(2.0 ** -120))[1].double() - 1      # floor(log2 |v|)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), e - mant)


def ulps(got, ref, at=None):
    """Largest |got - ref| in fp32 ulps, the ulp taken at `at` (default: the reference itself; for a difference of two
    terms the larger term, since the fp32 roundings of the terms are what the result inherits)."""
    ref = ref.double()
    at = ref if at is None else at.double()
    return ((got.double().cpu() - ref).abs() / spacing(at, 23)).max().item()


def apply_bound(exact, terms, extra=None):
    """(1 + 2^-6) h(exact) + 4 * 2^-24 * sum |terms| [+ extra]: h is half the bf16 spacing at the exact value (the
    output rounding; 2^-6 lets the fp32 error move the value across a binade edge), each fp32 operation adds at most
    2^-24 of a term's magnitude and there are at most 4 of them (product or fma, adds, the ReLU is exact)."""
    b = (1 + 2.0 ** -6) * 0.5 * spacing(exact, 7) + 4 * 2.0 ** -24 * terms
    return b if extra is None else b + extra


def fp32_term(terms):
    return 4 * 2.0 ** -24 * terms


def bn_apply_ref(x, scale, shift, res=None, res_scale=None, res_shift=None, relu=False):
    """fp64 (y, pre-ReLU value, sum |terms|, extra bound of the rounded shortcut term, pre-ReLU value for the sign)."""
    xd = x.double()
    pre = xd * scale.double() + shift.double()
    terms = (xd * scale.double()).abs() + shift.double().abs()
    extra = None
    if res is not None:
        q = res.double()
        if res_scale is not None:
            q = q * res_scale.double() + res_shift.double()
            terms = terms + (res.double() * res_scale.double()).abs() + res_shift.double().abs()
            extra = spacing(q, 7)                  # the shortcut term is rounded to bf16 before the add
            # what the kernel adds, bit for bit: the fp64 value is exact (8 x 24-bit product, fp32 addend of similar
            # size), its fp32 rounding is the fused multiply-add's result, then bf16. Used for the sign mask only
            pre_m = pre + q.float().to(BF).double()
        else:
            terms = terms + q.abs()
        pre = pre + q
    y = pre.clamp_min(0) if relu else pre
    return y, pre, terms, extra, (pre if extra is None else pre_m)


# ------------------------------------------------------------------ end to end against autograd
def bn_autograd(x, gamma, beta, res, relu, dz, eps, momentum, dtype):
    """F.batch_norm (training) [+ res] [ReLU] and its autograd gradients on the CPU in `dtype`. x, res, dz: [P, C]."""
    C = x.shape[1]
    xs = x.to(dtype).requires_grad_(True)
    g = gamma.to(dtype).requires_grad_(True) if gamma is not None else None
    b = beta.to(dtype).requires_grad_(True) if beta is not None else None
    r = res.to(dtype).requires_grad_(True) if res is not None else None
    rm, rv = torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype)
    y = F.batch_norm(xs, rm, rv, g, b, True, momentum, eps)
    if r is not None:
        y = y + r
    if relu:
        y = torch.relu(y)
    y.backward(dz.to(dtype))
    return {"y": y.detach(), "dx": xs.grad, "dgamma": g.grad if g is not None else None,
            "dbeta": b.grad if b is not None else None, "dres": r.grad if r is not None else None,
            "running_mean": rm, "running_var": rv}


def yardstick(hi, lo, name):
    """max(error of the fp32 CPU result, bf16 rounding error of the fp64 result), per tensor."""
    return max((lo[name].double() - hi[name]).abs().max().item(),
               (hi[name].to(BF).double() - hi[name]).abs().max().item())


def fp32_sum_bounds(x, dy, gamma, P, C, eps, momentum):
    """Per-channel error bounds of the fp32-kept outputs of a training BN (running statistics from 0 / 1, dgamma and
    dbeta added onto 0), from the kernels' accumulation scheme: a sum whose longest fp32 addition chain is n terms
    long is off by at most n u sum |terms| (u = 2^-24); n as in var_bound, + 2 for the product inside a term and the
    final cast. dy: the masked output gradient in fp64.
      dbeta = sum dy                       : n u sum |dy|
      running_mean = m mean                : m n u sum |x| / P + 2 u |.|
      running_var = m var P / (P - 1) + 1 - m : m P / (P - 1) dvar + 3 u |.|, dvar of var_bound
      dgamma = invstd sum dy (x - mean)    : invstd (n u sum |dy| |x - mean| + dmean sum |dy|) + |dgamma| dinv / invstd,
                                             dmean = n u sum |x| / P + u |mean|, dinv / invstd = dvar / (2 (var + eps)) + 3 u
    """
    u = 2.0 ** -24
    dvar, n = var_bound(x, P, C)
    n += 2
    xd = x.double()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    invstd = (var + eps).rsqrt()
    sx, sdy = xd.abs().sum(0), dy.abs().sum(0)
    dmean = n * u * sx / P + u * mean.abs()
    rmean, rvar = momentum * mean, momentum * var * P / max(P - 1, 1) + (1 - momentum)
    dgamma = invstd * (dy * (xd - mean)).sum(0)
    dinv = dvar / (2 * (var + eps)) + 3 * u
    tiny = 1e-30
    return {"dbeta": n * u * sdy + tiny,
            "running_mean": momentum * dmean + 2 * u * rmean.abs() + tiny,
            "running_var": momentum * P / max(P - 1, 1) * dvar + 3 * u * rvar.abs(),
            "dgamma": invstd * (n * u * (dy.abs() * (xd - mean).abs()).sum(0) + dmean * sdy) + dgamma.abs() * dinv + tiny}


def gauss_rows(P, C, seed, mu=0.0, std=1.0):
    return (torch.randn(P, C, generator=_gen(P, C, seed, 19)) * std + mu).to(BF)


def offset_rows(P, C, mu):
    """x = mu + randn with channel 0 constant at 100 and channel 1 all zero."""
    x = gauss_rows(P, C, 23, mu)
    x[:, 0] = 100.0
    x[:, 1] = 0.0
    return x


def var_bound(x, P, C):
    """|var_kernel - var| <= n 2^-23 (E[x^2] + 2 mean^2) per channel, n the longest fp32 addition chain: rows per
    thread + rows per iteration (the LDS combine) + blocks per slot (the atomics) of the case."""
    blocks, rpb, _ = reduce_geometry(P, C)
    rpi = rpi_of(C)
    n = -(-rpb // rpi) + rpi + -(-blocks // STAT_SLOTS)
    xd = x.double()
    ex2, mean = (xd * xd).mean(0), xd.mean(0)
    return n * 2.0 ** -23 * (ex2 + 2 * mean * mean), n


# ------------------------------------------------------------------ pooling
def pool_out(H, k, s, p, ceil):
    """torch's output size rule."""
    o = (-(-(H + 2 * p - k) // s) if ceil else (H + 2 * p - k) // s) + 1
    if ceil and (o - 1) * s >= H + p:
        o -= 1
    return o


def _windows(t, k, s, p, OH, OW, value):
    """t [N, C, H, W] -> list over taps (row-major) of the strided views [N, C, OH, OW] of the padded tensor."""
    H, W = t.shape[2], t.shape[3]
    eh, ew = max(0, (OH - 1) * s + k - H - p), max(0, (OW - 1) * s + k - W - p)
    tp = F.pad(t, (p, ew, p, eh), value=value)
    return [tp[:, :, r:r + (OH - 1) * s + 1:s, c:c + (OW - 1) * s + 1:s] for r in range(k) for c in range(k)]


def maxpool_oracle(x, k, s, p, ceil=False):
    """(y, idx) over windows in row-major tap order: the first in-bounds tap starts as the winner, a later tap replaces
    it when it is greater or NaN (so the first maximum wins, and a NaN wins with the last NaN's tap stored). The winner
    is always an in-bounds tap. x: float tensor [N, C, H, W] (any float dtype, values compared as given)."""
    N, C, H, W = x.shape
    OH, OW = pool_out(H, k, s, p, ceil), pool_out(W, k, s, p, ceil)
    vals = _windows(x, k, s, p, OH, OW, 0.0)
    oks = _windows(torch.ones(1, 1, H, W, dtype=torch.bool, device=x.device), k, s, p, OH, OW, False)
    best = torch.zeros(N, C, OH, OW, dtype=x.dtype, device=x.device)
    idx = torch.full((N, C, OH, OW), 255, dtype=torch.uint8, device=x.device)
    has = torch.zeros(1, 1, OH, OW, dtype=torch.bool, device=x.device)
    for t, (v, ok) in enumerate(zip(vals, oks)):
        take = ok & (~has | (v > best) | v.isnan())
        best = torch.where(take, v, best)
        idx = torch.where(take, torch.tensor(t, dtype=torch.uint8, device=x.device), idx)
        has = has | ok
    assert bool(has.all())
    return best, idx


def maxpool_bwd_oracle(dy, idx, H, W, k, s, p):
    """dx [N, C, H, W] in fp64: every output's gradient goes to the pixel of its stored tap."""
    N, C, OH, OW = dy.shape
    buf = torch.zeros(N, C, max((OH - 1) * s + k, p + H), max((OW - 1) * s + k, p + W), dtype=torch.float64,
                      device=dy.device)
    d = dy.double()
    for t in range(k * k):
        r, c = divmod(t, k)
        buf[:, :, r:r + (OH - 1) * s + 1:s, c:c + (OW - 1) * s + 1:s] += d * (idx == t)
    dx = buf[:, :, p:p + H, p:p + W]
    # taps outside the image are never winners: nothing may be lost
    assert torch.equal(dx.sum((0, 2, 3)), d.sum((0, 2, 3)))
    return dx


def pre_elements(x, pre):
    """bf16(relu(fma(x, scale, shift))) per channel for an integer x and bf16-representable scale / shift (exact in
    fp32, so the only rounding is the one to bf16). x [N, C, H, W]."""
    C = x.shape[1]
    a = pre.to(x.device).double()
    v = x.double() * a[:C].view(1, C, 1, 1) + a[C:].view(1, C, 1, 1)
    assert torch.equal(v.float().double(), v)
    return v.clamp_min(0).float().to(BF)


def int_image(N, C, H, W, seed, lo=-2, hi=2):
    """Small integers: ties in nearly every window."""
    return torch.randint(lo, hi + 1, (N, C, H, W), generator=_gen(N, C, H, W, seed)).to(BF).contiguous(memory_format=CL)


# (name, (N, C, H, W), k, s, p, ceil): the kernel each reaches is asserted nowhere (the launcher chooses), the shapes are
# chosen so that generic fwd / fixed fwd / generic bwd / fixed bwd / k3s2 bwd are all reached
MAXPOOL_CASES = [
    ("k3s2p1-even", (2, 8, 8, 10), 3, 2, 1, False),          # fixed fwd, k3s2 bwd
    ("k3s2p1-c24", (2, 24, 6, 4), 3, 2, 1, False),            # k3s2 bwd, bnred declines (256 % 3 != 0)
    ("k3s2p1-ow1", (1, 8, 6, 2), 3, 2, 1, False),             # OW = 1: no right neighbour
    ("k3s2p1-oh1", (2, 16, 2, 6), 3, 2, 1, False),            # OH = 1: no lower neighbour
    ("k3s2p1-1x1out", (3, 8, 2, 2), 3, 2, 1, False),          # OH = OW = 1
    ("k3s2p1-odd", (2, 8, 7, 9), 3, 2, 1, False),             # fixed fwd, fixed bwd (H != 2 OH)
    ("k3s2p0", (2, 8, 9, 8), 3, 2, 0, False),                 # fixed bwd, pad 0
    ("k3s2p0-ceil", (2, 24, 8, 6), 3, 2, 0, True),            # last window reaches past the image
    ("k3s2p1-ceil", (1, 8, 6, 7), 3, 2, 1, True),
    ("k3s2p1-h1", (2, 8, 1, 5), 3, 2, 1, False),              # H = 1
    ("k3s2p1-w2", (2, 8, 5, 2), 3, 2, 1, False),              # W = 2 (k3s2: OW = 1)
    ("k3s2p1-3x3", (2, 8, 3, 3), 3, 2, 1, False),
    ("k2s2-odd", (2, 8, 5, 7), 2, 2, 0, False),               # generic fwd / bwd
    ("k2s2-ceil", (2, 24, 5, 7), 2, 2, 0, True),
    ("k3s1p1", (2, 8, 5, 4), 3, 1, 1, False),                 # generic, overlapping windows
    ("k3s3p1", (1, 16, 7, 8), 3, 3, 1, False),
    ("k5s2p2", (1, 8, 9, 6), 5, 2, 2, False),
]
MAXPOOL_BIG = ("k3s2p1-past-8192-blocks", (3, 8, 1680, 1680), 3, 2, 1, False)      # 3 * 840^2 granules > 8192 * 256
BNRED_BIG = (3, 8, 840, 840)                                                        # 3 * 420^2 granules > 2048 * 256
BNRED_CASES = [(2, 8, 8, 10), (2, 16, 6, 10), (1, 64, 10, 6), (3, 8, 2, 2), (1, 8, 6, 2), (2, 16, 2, 6)]

# (name, (N, C, H, W), k, s, p, ceil)
AVGPOOL_CASES = [
    ("k7s1p0-head", (2, 8, 7, 7), 7, 1, 0, False),
    ("k7s1p0-9x8", (2, 24, 9, 8), 7, 1, 0, False),
    ("k3s2p1", (2, 8, 9, 7), 3, 2, 1, False),
    ("k3s2p1-c24", (1, 24, 8, 8), 3, 2, 1, False),
    ("k2s2-odd", (2, 8, 5, 7), 2, 2, 0, False),
    ("k2s2-odd-ceil", (2, 24, 5, 7), 2, 2, 0, True),
    ("k3s2p1-ceil", (2, 8, 8, 6), 3, 2, 1, True),             # the last window reaches past the padding
]


def avgpool_ref(x, dy, k, s, p, ceil, count_pad):
    """fp64 (y, dx, sum |terms| of y, sum |terms| of dx) from F.avg_pool2d and its autograd."""
    xs = x.double().requires_grad_(True)
    y = F.avg_pool2d(xs, k, s, p, ceil_mode=ceil, count_include_pad=count_pad)
    y.backward(dy.double())
    ya = F.avg_pool2d(x.double().abs(), k, s, p, ceil_mode=ceil, count_include_pad=count_pad)
    xa = torch.zeros_like(xs).requires_grad_(True)
    F.avg_pool2d(xa, k, s, p, ceil_mode=ceil, count_include_pad=count_pad).backward(dy.double().abs())
    return y.detach(), xs.grad, ya, xa.grad


def nhwc_rows(t):
    """[N, C, H, W] -> [N H W, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ------------------------------------------------------------------ Gaussian cases of the two apply passes
APPLY_SHAPES = [(259, 24), (67, 64), (131, 88), (9, 2056), (2049, 8)]
APPLY_MODES = ("plain", "res", "ra", "relu", "res+relu+zm", "ra+relu+zm")


def apply_inputs(P, C, mode):
    """Gaussian bf16 x / res and arbitrary fp32 scale / shift (chosen here, not produced by bn_finalize)."""
    g = _gen(P, C, len(mode), 29)
    d = {"x": gauss_rows(P, C, 31, 0.2, 1.5), "scale": torch.randn(C, generator=g) * 0.8,
         "shift": torch.randn(C, generator=g), "res": None, "res_scale": None, "res_shift": None,
         "relu": "relu" in mode, "zm": "zm" in mode}
    if "res" in mode or "ra" in mode:
        d["res"] = gauss_rows(P, C, 37, -0.1, 1.0)
    if "ra" in mode:
        d["res_scale"], d["res_shift"] = torch.randn(C, generator=g) * 0.6, torch.randn(C, generator=g) * 0.5
    return d


def bwd_apply_ref(dz, x, mask, co):
    """fp64 (dx, sum |terms|, masked dz) of dx = A dy + B x + D."""
    dy = torch.where(mask.to(dz.device), dz.double(), torch.zeros((), dtype=torch.float64, device=dz.device))
    xd = x.double()
    dx = co["A"] * dy + co["B"] * xd + co["D"]
    return dx, (co["A"] * dy).abs() + (co["B"] * xd).abs() + co["D"].abs(), dy
