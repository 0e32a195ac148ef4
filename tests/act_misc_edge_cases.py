"""Cases, data, fp64 oracles, bounds and comparison functions for the point-wise activation kernels
(csrc/activation.hip: act_fwd / act_bwd, 19 kinds) and the misc NN kernels (csrc/nn_misc.hip: across-channel LRN, Philox
dropout, embedding gather / scatter, bilinear resize, row log-softmax). Pure torch / numpy: it imports no GPU code.
tests/test_act_misc_edges_cpu.py checks this file on its own, tests/test_act_misc_edges_gpu.py holds the kernels to it.

Two kinds of reference, as in tests/step_tail_edge_cases.py:
* exact legs: data for which the documented formula is one rounded operation (or none), so the kernel equals the fp64
  oracle rounded once to the dtype, bit for bit, NaN positions and the sign of zero included;
* element-wise legs: ``|got - want| <= allowed x bound`` per element against fp64, the bound derived below per kind.
  U24 = 2^-24 is the relative error of one fp32 rounding; ``ulp32`` is the fp32 spacing (two roundings).
"""

import torch

from tests import step_tail_edge_cases as st
from tests.recurrent_cases import _keep_mask, _philox_np  # noqa: F401  (the Philox layout of lstm_drop_rep is the same)

BF, F32, F64 = st.BF, st.F32, st.F64
U24 = st.U24
TINY = 2.0 ** -126        # smallest normal fp32: below it the hardware exponential may flush to zero
gen, f32v, bits, same_bits, same_bits_nan = st.gen, st.f32v, st.bits, st.same_bits, st.same_bits_nan
ulp32, bf16_half_spacing, guarded, canaries_ok = st.ulp32, st.bf16_half_spacing, st.guarded, st.canaries_ok

ACT_GRID_CAP = 8192       # blocks_for() of csrc/activation.hip: 8 elements per lane
MISC_GRID_CAP = 16384     # blocks_for() of csrc/nn_misc.hip
ACT_PAST_CAP = st.past_cap(8, ACT_GRID_CAP, extra=3)               # 8192 x 256 x 8 + 11
DROPOUT_PAST_CAP = st.past_cap(4, MISC_GRID_CAP, extra=1)          # 16384 x 256 x 4 + 5
LRN_PAST_CAP_COLS = MISC_GRID_CAP * 256 + 1
ROWS_PAST_CAP = MISC_GRID_CAP * 4 + 1                              # one wave per row, 4 per block: 65537 rows
assert (ACT_PAST_CAP, DROPOUT_PAST_CAP, ROWS_PAST_CAP) == (8192 * 256 * 8 + 11, 16384 * 256 * 4 + 5, 65537)


def rnd(t64, dtype):
    """The fp64 value rounded to the kernel's number format (through fp32 for bf16, as the kernel stores it)."""
    t = t64.to(F32)
    return t.to(BF) if dtype == BF else t


# ================================================================================================== activations
# name: (kind code of csrc/activation.hip, a, b) with the parameters the tests use (dyadic, exact in bf16)
ACT = {
    "Tanh": (0, 0.0, 0.0), "Sigmoid": (1, 0.0, 0.0), "ELU": (2, 0.5, 0.0), "LeakyReLU": (3, 0.25, 0.0),
    "ReLU6": (4, 0.0, 0.0), "SoftPlus": (5, 2.0, 0.0), "SoftSign": (6, 0.0, 0.0), "HardTanh": (7, -0.5, 2.0),
    "HardSigmoid": (8, 0.0, 0.0), "LogSigmoid": (9, 0.0, 0.0), "TanhShrink": (10, 0.0, 0.0),
    "SoftShrink": (11, 0.5, 0.0), "HardShrink": (12, 0.5, 0.0), "Threshold": (13, 0.25, -3.0), "Exp": (14, 0.0, 0.0),
    "Log": (15, 0.0, 0.0), "Sqrt": (16, 0.0, 0.0), "Square": (17, 0.0, 0.0), "Abs": (18, 0.0, 0.0),
}
ACT_EXACT = ("LeakyReLU", "ReLU6", "HardTanh", "SoftShrink", "HardShrink", "Threshold", "Abs")
ACT_EXP = ("Sigmoid", "ELU", "SoftPlus", "LogSigmoid", "Exp")      # behind __expf: sigma 30 data, cap 8
ACT_POSITIVE = ("Log", "Sqrt")
ACT_N = (1, 7, 8, 9, 15, 16, 17, 1001, 2057)
# cap of the element-wise legs: 8 where a fast intrinsic feeds further arithmetic, 4 for one rounded operation chain
ACT_CAP = {k: (8.0 if k in ACT_EXP + ("Log",) else 4.0) for k in ACT}

# What a NaN input gives. forward: True = the NaN stays. backward: the derivative factor at a NaN x (and the y of it),
# "nan" or a number; dx = dy * factor. Source: the reference's formula, with the Scala line it follows.
NAN_RULE = {
    "Tanh": (True, "nan", "Tanh.scala: tanh(x)"), "Sigmoid": (True, "nan", "Sigmoid.scala: 1 / (1 + exp(-x))"),
    "ELU": (True, "nan", "ELU.scala: x > 0 fails, alpha * (exp(x) - 1)"),
    "LeakyReLU": (True, "a", "LeakyReLU.scala: x > 0 fails, negval * x; gradient negval * g"),
    "ReLU6": (True, 0.0, "ReLU6.scala = HardTanh(0, 6); HardTanh.scala:93-97 (both compares fail, x stays)"),
    "SoftPlus": (True, "nan", "SoftPlus.scala: log1p(exp(beta x)) / beta"),
    "SoftSign": (True, "nan", "SoftSign.scala: x / (1 + |x|)"),
    "HardTanh": (True, 0.0, "HardTanh.scala:93-97 (both compares fail, x stays)"),
    "HardSigmoid": (True, 0.0, "HardSigmoid.scala:41-46 (both compares fail, 0.2 x + 0.5)"),
    "LogSigmoid": (True, "nan", "LogSigmoid.scala: -log(1 + exp(-x))"),
    "TanhShrink": (True, "nan", "TanhShrink.scala: x - tanh(x)"),
    "SoftShrink": (False, 0.0, "SoftShrink.scala:45-50 (both compares fail, 0)"),
    "HardShrink": (False, 0.0, "HardShrink.scala:43-46 (both compares fail, 0)"),
    "Threshold": (True, 0.0, "Threshold.scala:83 (x <= th fails, x stays); :205 (x > th fails, 0)"),
    "Exp": (True, "nan", "Exp.scala"), "Log": (True, "nan", "Log.scala"), "Sqrt": (True, "nan", "Sqrt.scala"),
    "Square": (True, "nan", "Square.scala"), "Abs": (True, 0.0, "Abs.scala: |x|; gradient sign(x) g, sign(NaN) = 0"),
}



def act_f64(kind, x, a=0.0, b=0.0):
    """The documented formula in fp64 on the operand the kernel was given. a / b are the fp32-narrowed parameters. The
    compares are written as in the reference, so NaN and -0 come out as its formula gives them."""
    x = x.to(F64)
    a, b = f32v(a), f32v(b)
    z = torch.zeros_like(x)
    if kind == "Tanh":
        return torch.tanh(x)
    if kind == "Sigmoid":
        return torch.sigmoid(x)
    if kind == "ELU":
        return torch.where(x > 0, x, a * torch.expm1(x))
    if kind == "LeakyReLU":
        return torch.where(x > 0, x, a * x)
    if kind in ("ReLU6", "HardTanh"):
        lo, hi = (0.0, 6.0) if kind == "ReLU6" else (a, b)
        return torch.where(x < lo, z + lo, torch.where(x > hi, z + hi, x))
    if kind == "SoftPlus":
        return torch.where(x * a > 20, x, torch.nn.functional.softplus(a * x, 1.0, 1e9) / a)
    if kind == "SoftSign":
        return x / (1 + x.abs())
    if kind == "HardSigmoid":
        t = 0.2 * x + 0.5
        return torch.where(t < 0, z, torch.where(t > 1, z + 1, t))
    if kind == "LogSigmoid":
        return torch.where(torch.isnan(x), x, torch.clamp(x, max=0.0) - torch.log1p(torch.exp(-x.abs())))
    if kind == "TanhShrink":
        return x - torch.tanh(x)
    if kind == "SoftShrink":
        return torch.where(x > a, x - a, torch.where(x < -a, x + a, z))
    if kind == "HardShrink":
        return torch.where((x > a) | (x < -a), x, z)
    if kind == "Threshold":
        return torch.where(x <= a, z + b, x)
    if kind == "Exp":
        return torch.exp(x)
    if kind == "Log":
        return torch.log(x)
    if kind == "Sqrt":
        return torch.sqrt(x)
    if kind == "Square":
        return x * x
    if kind == "Abs":
        return x.abs()
    raise ValueError(kind)


def act_df64(kind, x, y, a=0.0, b=0.0):
    """dy/dx in fp64 from the x and the y handed to the backward (kinds whose derivative is a function of y use y).
    Clamp-style kinds pass the gradient on the closed interval (both engines; the reference's HardTanh.scala:135-173
    zeroes it at x == min and x == max: a known deviation, profiles/act_misc_edge_errors.txt)."""
    x, y = x.to(F64), y.to(F64)
    a, b = f32v(a), f32v(b)
    one, z = torch.ones_like(x), torch.zeros_like(x)
    if kind == "Tanh":
        return 1 - y * y
    if kind == "Sigmoid":
        return y * (1 - y)
    if kind == "ELU":
        return torch.where(x > 0, one, y + a)
    if kind == "LeakyReLU":
        return torch.where(x > 0, one, z + a)
    if kind in ("ReLU6", "HardTanh"):
        lo, hi = (0.0, 6.0) if kind == "ReLU6" else (a, b)
        return torch.where((x >= lo) & (x <= hi), one, z)
    if kind == "SoftPlus":
        return torch.where(x * a > 20, one, torch.sigmoid(a * x))
    if kind == "SoftSign":
        return 1 / (1 + x.abs()) ** 2
    if kind == "HardSigmoid":
        return torch.where((x >= -2.5) & (x <= 2.5), z + f32v(0.2), z)
    if kind == "LogSigmoid":
        return torch.sigmoid(-x)
    if kind == "TanhShrink":
        return torch.tanh(x) ** 2
    if kind in ("SoftShrink", "HardShrink"):
        return torch.where((x > a) | (x < -a), one, z)
    if kind == "Threshold":
        return torch.where(x > a, one, z)
    if kind == "Exp":
        return y
    if kind == "Log":
        return 1 / x
    if kind == "Sqrt":
        return 0.5 / y
    if kind == "Square":
        return 2 * x
    if kind == "Abs":
        return torch.where(x > 0, one, torch.where(x < 0, -one, z))
    raise ValueError(kind)


def act_bound(kind, x, a=0.0, b=0.0):
    """Per-element unit of the forward error, fp32 result: the fp32 spacing at the formula's largest term, + for the
    kinds behind __expf a term U24 |t| |d result / d log e^t| (the argument t x log2(e) is rounded before the hardware
    exp2, an error that grows with |t|), + TINY where a result can fall among the denormals."""
    x = x.to(F64)
    a = f32v(a)
    y = act_f64(kind, x, a, b)
    fin = torch.where(torch.isfinite(y), y, torch.zeros_like(y))
    s = torch.sigmoid(x)
    if kind == "Sigmoid":
        return ulp32(fin) + U24 * x.abs() * s * (1 - s) + TINY
    if kind == "ELU":
        e = torch.exp(torch.clamp(x, max=0.0))
        return torch.where(x > 0, ulp32(x), ulp32(a * torch.clamp(e, min=1.0)) + U24 * x.abs() * a * e)
    if kind == "SoftPlus":
        return ulp32(fin) + U24 * (a * x).abs() * torch.sigmoid(a * x) / a + TINY
    if kind == "HardSigmoid":
        return ulp32(torch.maximum((0.2 * x).abs(), torch.full_like(x, 0.5)))
    if kind == "LogSigmoid":
        lp = torch.log1p(torch.exp(-x.abs()))
        return ulp32(torch.maximum(torch.clamp(x, max=0.0).abs(), lp)) + U24 * x.abs() * torch.sigmoid(-x.abs()) + TINY
    if kind == "TanhShrink":
        return ulp32(x)
    if kind == "SoftShrink":
        return ulp32(torch.maximum(x.abs(), torch.full_like(x, a)))
    if kind == "Exp":
        return ulp32(fin) + U24 * x.abs() * fin + TINY
    if kind == "Log":
        # the hardware log2 is a difference of order 2^-24 |x| near x == 1: the unit does not fall below an ulp of 1
        return ulp32(torch.clamp(fin.abs(), min=1.0))
    return ulp32(fin)


def act_dbound(kind, x, y, dy, a=0.0, b=0.0):
    """Unit of the backward error: |dy| x the unit of the derivative factor (the product's own rounding is within it)."""
    x, y, dy = x.to(F64), y.to(F64), dy.to(F64)
    a = f32v(a)
    df = act_df64(kind, x, y, a, b)
    fin = torch.where(torch.isfinite(df), df, torch.zeros_like(df))
    u = ulp32(fin)
    if kind == "Tanh":
        u = ulp32(torch.ones_like(x))                          # 1 - y^2: the terms are 1 and y^2
    elif kind == "Sigmoid":
        u = ulp32(y)                                           # y (1 - y): 1 - y is rounded at 1
    elif kind == "ELU":
        u = ulp32(torch.where(x > 0, torch.ones_like(x), torch.full_like(x, a)))
    elif kind in ("SoftPlus", "LogSigmoid"):
        t = a * x if kind == "SoftPlus" else x
        u = u + U24 * t.abs() * fin * (1 - fin) + TINY
    elif kind == "TanhShrink":
        u = 2 * u                                              # the square doubles tanhf's relative error
    return dy.abs() * u + TINY


def elem_ratio(got, want64, bound):
    """Largest |got - want| / bound over the elements. NaN exactly where the oracle is NaN and the oracle's inf by sign
    and position are required (inf returned otherwise); an oracle value beyond the format's range may come out as inf.
    0 / 0 counts as 0. A bf16 result adds half a bf16 spacing at the value x (1 + 2^-6) to the bound."""
    want64 = want64.to(F64).to(got.device)
    bound = bound.to(F64).to(got.device)
    g = got.to(F64)
    if got.shape != want64.shape or not torch.equal(torch.isnan(g), torch.isnan(want64)):
        return float("inf")
    big = want64.abs() > torch.finfo(got.dtype).max
    inf_w = torch.isinf(want64)
    if not torch.equal(g[inf_w], want64[inf_w]):
        return float("inf")
    ok = ~(torch.isnan(want64) | inf_w | (big & torch.isinf(g) & (torch.sign(g) == torch.sign(want64))))
    if got.dtype == BF:
        bound = bound + bf16_half_spacing(torch.where(ok, want64, torch.zeros_like(want64))) * (1 + 2.0 ** -6)
    err = (g - want64).abs()[ok]
    r = torch.where(err == 0, torch.zeros_like(err), err / bound[ok])
    return float(r.max()) if r.numel() else 0.0


def exact_equal(got, want64):
    """Exact legs: got == the fp64 oracle rounded once to got's format, by bits (the sign of zero included); NaN
    exactly where the oracle is NaN."""
    return same_bits_nan(got, rnd(want64.cpu(), got.dtype))


def _next(t, up):
    """The neighbouring number of the tensor's own format (fp32 or bf16), towards +inf (up) or -inf."""
    it = torch.int32 if t.dtype == F32 else torch.int16
    i = t.contiguous().view(it).clone()
    pos = t >= 0
    i = torch.where(pos == up, i + 1, i - 1)
    zero = t == 0
    mn = torch.tensor(1, dtype=it)
    i = torch.where(zero, mn if up else (mn | torch.iinfo(it).min), i)
    return i.view(t.dtype)


def act_thresholds(kind, a=0.0, b=0.0):
    return {"LeakyReLU": [0.0], "ReLU6": [0.0, 6.0], "HardTanh": [a, b], "SoftShrink": [a, -a], "HardShrink": [a, -a],
            "Threshold": [a], "Abs": [0.0], "HardSigmoid": [2.5, -2.5], "Square": [0.0]}[kind]


def act_edge_table(kind, dtype, a=0.0, b=0.0):
    """Each threshold and one ulp (of the dtype) either side, +-0, +-inf, the largest finite value, denormals, plain
    numbers, four NaN. An odd number of entries, so a cyclic fill puts every entry at every position of a granule."""
    th = torch.tensor(act_thresholds(kind, a, b), dtype=dtype)
    mx = torch.finfo(dtype).max
    den = [2.0 ** -149, -2.0 ** -149, 2.0 ** -127] if dtype == F32 else [2.0 ** -133, -2.0 ** -133, 2.0 ** -127]
    plain = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), mx, -mx, 1.0, -1.0, 3.0, -7.0, 0.375] + den,
                         dtype=dtype)
    if dtype == F32:
        nan = torch.tensor([0x7FC00000, 0x7F800001, -0x400000, -0x7FFFFF], dtype=torch.int32).view(F32)
    else:
        nan = torch.tensor([0x7FC0, 0x7F81, -0x40, -0x7F], dtype=torch.int16).view(BF)
    tab = torch.cat([th, _next(th, True), _next(th, False), plain, nan])
    if tab.numel() % 2 == 0:
        tab = torch.cat([tab, torch.tensor([2.0], dtype=dtype)])
    return tab


def cyclic(tab, n, shift=0):
    return tab[(torch.arange(n) + shift) % tab.numel()]


def int_dy(n, seed, dtype):
    """Non-zero small integers: dy x {0, 1, -1, a dyadic slope} is exact and the sign of a zero product is dy's."""
    g = torch.randint(1, 5, (n,), generator=gen(seed)) * (torch.randint(0, 2, (n,), generator=gen(seed + 1)) * 2 - 1)
    return g.to(dtype)


def act_gauss(kind, n, seed, dtype):
    """Gaussian data (sigma 2; sigma 30 for the exp kinds; positive for Log / Sqrt) with a sweep of magnitudes
    2^-20 .. 2^6 in both signs in front."""
    x = torch.randn(n, generator=gen(seed)) * (30.0 if kind in ACT_EXP else 2.0)
    sw = 2.0 ** torch.arange(-20, 7).float()
    sw = torch.cat([sw, -sw, sw * 1.171875, -sw * 1.171875])
    m = min(n, sw.numel())
    x[:m] = sw[:m]
    if kind in ACT_POSITIVE:
        x = x.abs().clamp_min(2.0 ** -20)
    return x.to(dtype)


# ================================================================================================== LRN
def lrn_window(c, C, size):
    pre = (size - 1) // 2
    return max(0, c - pre), min(C - 1, c - pre + size - 1)


def lrn_oracle(x, size, alpha, beta, k):
    """(y, scale) in fp64: scale = k + alpha / size * sum x^2 over [c - (size-1)//2, c - (size-1)//2 + size - 1] clipped
    to the channels; y = x scale^-beta. alpha / size is the fp32 quotient the host function forms."""
    x = x.to(F64)
    C = x.shape[1]
    an = float(torch.tensor(alpha, dtype=F32) / size)
    sq = x * x
    sc = torch.empty_like(x)
    for c in range(C):
        lo, hi = lrn_window(c, C, size)
        sc[:, c] = f32v(k) + an * sq[:, lo:hi + 1].sum(1)
    return x * sc.pow(-f32v(beta)), sc


def lrn_bwd_oracle(x, y, scale, gy, size, alpha, beta):
    """gx = gy s^-beta - 2 (alpha / size) beta x sum_{j: c in window(j)} gy_j y_j / s_j, fp64, from the x, y, scale and
    gy handed to the backward. Returns (gx, sum of the magnitudes of its terms)."""
    x, y, s, gy = (t.to(F64) for t in (x, y, scale, gy))
    C = x.shape[1]
    an = float(torch.tensor(alpha, dtype=F32) / size)
    beta = f32v(beta)
    r = gy * y / s
    acc, mag = torch.zeros_like(x), torch.zeros_like(x)
    for c in range(C):
        for j in range(C):
            lo, hi = lrn_window(j, C, size)
            if lo <= c <= hi:
                acc[:, c] += r[:, j]
                mag[:, c] += r[:, j].abs()
    first = gy * s.pow(-beta)
    coef = 2 * an * beta
    return first - coef * x * acc, first.abs() + coef * x.abs() * mag


def lrn_y_bound(y64, s64, beta):
    """U24 |y| (4 + |beta log2 s|): __powf is exp2(-beta log2 s), whose argument is rounded at |beta log2 s|; 4 covers the
    running window's error in s (x beta), log2, exp2 and the product."""
    return U24 * y64.abs() * (4 + (f32v(beta) * torch.log2(s64)).abs()) + TINY


def lrn_gx_bound(mag, s64, size, beta):
    """2^-24 x chain x sum |terms|: chain = the window's adds and subtractions (size + 1), quotient, products, the final
    difference (4) and __powf's |beta log2 s|."""
    return U24 * (size + 5 + (f32v(beta) * torch.log2(s64)).abs()) * mag + TINY


def lrn_scale_chain_bound(x, size, alpha, k):
    """Dynamic-range leg: the kernel keeps one running window sum per column, adds the entering channel and subtracts the
    leaving one. Bound of scale[c]: 2^-24 x (adds + subtractions so far, + 2 for the product and k) x alpha_n x the
    largest running sum so far (+ one rounding of the result)."""
    x = x.to(F64)
    C = x.shape[1]
    pre = (size - 1) // 2
    an = float(torch.tensor(alpha, dtype=F32) / size)
    sq = x * x
    out = torch.empty_like(x)
    ops = min(max(size - pre - 1, 0), C)
    peak = sq[:, :ops].sum(1) if ops else torch.zeros_like(sq[:, 0])
    for c in range(C):
        lo, hi = lrn_window(c, C, size)
        ops += (c + size - pre - 1 < C) + (c - pre - 1 >= 0)
        peak = torch.maximum(peak, sq[:, lo:hi + 1].sum(1) + (sq[:, lo - 1] if lo > 0 else 0))
        out[:, c] = U24 * (ops + 2) * (an * peak + abs(k))
    return out


def lrn_int(N, C, H, W, seed):
    return torch.randint(-4, 5, (N, C, H, W), generator=gen(seed)).float()


def lrn_exact_geometry():
    """(size, C) of the exact scale leg: size = 1 .. 7 x C in {1, 2, size - 1, size, size + 1, 13}."""
    out = []
    for size in range(1, 8):
        for C in sorted({1, 2, size - 1, size, size + 1, 13} - {0}):
            out.append((size, C))
    return out


# ================================================================================================== dropout
DROPOUT_SEEDS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1)
DROPOUT_N = (1, 2, 3, 4, 5, 6, 7, 8, 9, 1003)
M32 = 0xFFFFFFFF
# (seed, element index) whose 24-bit uniform is exactly 0 (one draw in 2^24 is): u >= p keeps it at p == 0, u > p would not
DROPOUT_ZERO_DRAW = (9, 2792111)


def _mul32(A, c):
    """(high, low) 32-bit halves of A x c for a 32-bit constant A and an int64 tensor of 32-bit values, without leaving
    int64: c is split in 16-bit halves."""
    t, u = A * (c & 0xFFFF), A * (c >> 16)
    low = ((u & 0xFFFF) << 16) + t
    return (u >> 16) + (low >> 32), low & M32


def philox4x32(ctr, key, rounds=10):
    """Philox-4x32-10 (Salmon et al., SC'11) on int64 tensors holding 32-bit words: ctr = (c0, c1, c2, c3), key =
    (k0, k1). Device-agnostic, so the largest case is compared on the device."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(rounds):
        h0, l0 = _mul32(0xD2511F53, c0)
        h1, l1 = _mul32(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def dropout_keep(seed, n, p, device="cpu", swap=None):
    """Keep mask of bigdl_dropout: counter = element index / 4 (c2 = c3 = 0), lane = index % 4, key = (seed low, seed
    high), keep = (v >> 8) 2^-24 >= p with p narrowed to fp32. ``swap`` plants an error for the sensitivity checks."""
    i = torch.arange(n, dtype=torch.int64, device=device)
    q, lane = i >> 2, i & 3
    if swap == "counter":
        q = (i + 4) >> 2
    z = torch.zeros_like(q)
    k0, k1 = seed & M32, (seed >> 32) & M32
    if swap == "key":
        k0, k1 = k1, k0
    key = (z + k0, z + k1)
    r = torch.stack(philox4x32((q & M32, q >> 32, z, z), key))
    if swap == "lane":
        lane = 3 - lane
    v = r.gather(0, lane[None])[0]
    u = (v >> 8).to(F64) * 2.0 ** -24
    return u > f32v(p) if swap == "gt" else u >= f32v(p)


def dropout_oracle(x, keep, mul):
    """keep ? round(float(x) * mul) : +0, in x's format (one fp32 product, then nearest-even for bf16)."""
    prod = rnd(x.to(F64) * f32v(mul), x.dtype)
    return torch.where(keep.to(x.device), prod, torch.zeros_like(prod))


def dropout_input(n, seed, dtype):
    x = torch.randn(n, generator=gen(seed)) * 2
    sp = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 3.0e38, 2.0 ** -140])
    idx = torch.randperm(n, generator=gen(seed + 1))[:min(n // 2, 4 * sp.numel())]
    x[idx] = sp.repeat(4)[:idx.numel()]
    return x.to(dtype)


# ================================================================================================== embedding
EMB_D = (1, 3, 4, 5, 63, 64, 65, 256, 260)
EMB_ROWS = (1, 3, 4, 5)


def emb_fwd_oracle(W, ids, mask_zero):
    """LookupTable on raw 1-based ids: k = (long)id - 1; k < 0 -> zero row with mask_zero, row 0 without; k >= nIndex ->
    zero row."""
    k = ids.to(torch.int64) - 1
    if not mask_zero:
        k = k.clamp_min(0)
    ok = (k >= 0) & (k < W.shape[0])
    out = W[k.clamp(0, W.shape[0] - 1)]
    return torch.where(ok[:, None], out, torch.zeros_like(out))


def emb_fwd_idx_oracle(W, idx):
    ok = (idx >= 0) & (idx < W.shape[0])
    out = W[idx.clamp(0, W.shape[0] - 1)]
    return torch.where(ok[:, None], out, torch.zeros_like(out))


def emb_bwd_oracle(gW0, keys, gout, scale, twice=None):
    """gW0 + scale x sum of the gradient rows per key in fp64 (keys outside [0, nIndex) skipped). Returns (gW, sum of
    |terms| per element, longest run per row). ``twice``: a row added twice, for the sensitivity check."""
    g = gout.to(F64) * f32v(scale)
    ok = (keys >= 0) & (keys < gW0.shape[0])
    out, mag = gW0.to(F64).clone(), gW0.to(F64).abs()
    out.index_add_(0, keys[ok], g[ok])
    mag.index_add_(0, keys[ok], g[ok].abs())
    if twice is not None:
        out[keys[twice]] += g[twice]
    run = torch.bincount(keys[ok], minlength=gW0.shape[0])
    return out, mag, run


def emb_keys(ids, pad):
    """Keys of embedding_bwd_ids: (long)id - 1, the padding row skipped."""
    k = ids.to(torch.int64) - 1
    return torch.where(k == pad, torch.full_like(k, -1), k) if pad >= 0 else k


def emb_ids(rows, nIndex, seed, dtype):
    """Random 1-based ids with the first and last row, 0, a negative id and nIndex + 1 in front."""
    ids = torch.randint(1, nIndex + 1, (rows,), generator=gen(seed))
    sp = torch.tensor([1, nIndex, 0, -2, nIndex + 1])
    m = min(rows, sp.numel())
    ids[:m] = sp[torch.randperm(sp.numel(), generator=gen(seed + 1))[:m]] if rows < sp.numel() else sp
    return ids.to(dtype)


# ================================================================================================== bilinear resize
def resize_scales(H, W, OH, OW, align):
    """As ops/nnk.py _scales: doubles, narrowed to fp32 by the binding."""
    sh = (H - 1) / (OH - 1) if align and OH > 1 else H / OH
    sw = (W - 1) / (OW - 1) if align and OW > 1 else W / OW
    return sh, sw


def resize_axis(o, n, scale, floor_shift=None):
    """The kernel's fp32 index arithmetic: s = o * scale in fp32, floor, clamp, f = s - i0. ``floor_shift`` plants a floor
    moved by one at the integer landings, for the sensitivity check."""
    s = torch.arange(o, dtype=F32) * torch.tensor(scale, dtype=F32)
    i0 = s.floor().long()
    if floor_shift is not None:
        i0 = torch.where(s == s.floor(), i0 + floor_shift, i0).clamp_min(0)
    i0 = i0.clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, (s - i0.float()).to(F64)


def resize_oracle(x, OH, OW, align, floor_shift=None):
    """Interpolation in fp64 on the fp32 indices and fractions. Returns (y, largest corner magnitude)."""
    x = x.to(F64)
    H, W = x.shape[-2:]
    sh, sw = resize_scales(H, W, OH, OW, align)
    h0, h1, fh = resize_axis(OH, H, sh, floor_shift)
    w0, w1, fw = resize_axis(OW, W, sw, floor_shift)
    fh = fh.view(OH, 1)
    a, b = x[..., h0, :][..., w0], x[..., h0, :][..., w1]
    c, d = x[..., h1, :][..., w0], x[..., h1, :][..., w1]
    top, bot = a + (b - a) * fw, c + (d - c) * fw
    mag = torch.stack([a.abs(), b.abs(), c.abs(), d.abs()]).max(0).values
    return top + (bot - top) * fh, mag


def resize_bwd_oracle(gy, H, W, align):
    """(gx, sum |terms|, contributions per element) in fp64; a corner that is clamped onto its neighbour adds twice."""
    gy = gy.to(F64)
    NC = gy.shape[0] * gy.shape[1]
    OH, OW = gy.shape[-2:]
    sh, sw = resize_scales(H, W, OH, OW, align)
    h0, h1, fh = resize_axis(OH, H, sh)
    w0, w1, fw = resize_axis(OW, W, sw)
    g = gy.reshape(NC, OH * OW)
    gx, mag, cnt = (torch.zeros(NC, H * W, dtype=F64) for _ in range(3))
    for hi, wh in ((h0, 1 - fh), (h1, fh)):
        for wi, ww in ((w0, 1 - fw), (w1, fw)):
            idx = (hi.view(OH, 1) * W + wi.view(1, OW)).reshape(-1)
            t = g * (wh.view(OH, 1) * ww.view(1, OW)).reshape(-1)
            gx.index_add_(1, idx, t)
            mag.index_add_(1, idx, t.abs())
            cnt.index_add_(1, idx, torch.ones_like(t))
    shp = gy.shape[:2] + (H, W)
    return gx.view(shp), mag.view(shp), cnt.view(shp)


# (H, W, OH, OW): each extent 1 in turn, 7 -> 3, 3 -> 9 and 5 -> 7 (products that land on integers after rounding),
# identity, exact 2x
RESIZE_GEO = ((1, 5, 4, 6), (5, 1, 4, 6), (5, 6, 1, 4), (5, 6, 4, 1), (7, 7, 3, 3), (3, 3, 9, 9), (5, 5, 7, 7),
              (3, 5, 9, 7), (6, 5, 6, 5), (4, 5, 8, 10))


# ================================================================================================== log-softmax
LSM_COLS = (1, 2, 63, 64, 65, 1000, 10001)
LSM_ROWS = (1, 3, 4, 5)


def lsm_oracle(x, skip_last=False):
    x = x.to(F64)
    if skip_last:                                          # the planted error of the sensitivity check
        return x - torch.logsumexp(x[:, :-1], 1, keepdim=True)
    return torch.log_softmax(x, 1)


def lsm_bound(x):
    """U24 (4 + |max| + |lse| + |x| + sum_j p_j |x_j - max|): the roundings of max + log(sum) - x (the xent_loss_row
    form) and the exponentials' argument error, which enters log(sum) weighted by p_j."""
    x = x.to(F64)
    m = x.max(1, keepdim=True).values
    lse = torch.logsumexp(x, 1, keepdim=True)
    d = (x - m).abs()
    d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
    spread = (torch.softmax(x, 1) * d).sum(1, keepdim=True)
    xa = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))
    return U24 * (4 + m.abs() + lse.abs() + xa + spread)


def lsm_bwd_oracle(y, gy):
    """gx = gy - exp(y) sum gy in fp64 from the y handed in. Returns (gx, bound): 2^-24 (|gy| + p x chain x sum |gy|),
    chain = the lane's terms + 6 shuffles + exp, product, difference (4) + |y| (the exponential's argument)."""
    y, gy = y.to(F64), gy.to(F64)
    p = y.exp()
    cols = y.shape[1]
    chain = (cols + 63) // 64 + 10 + y.abs()
    return gy - p * gy.sum(1, keepdim=True), U24 * (gy.abs() + p * chain * gy.abs().sum(1, keepdim=True)) + TINY


def lsm_gauss(rows, cols, sigma, offset, seed):
    return torch.randn(rows, cols, generator=gen(seed)) * sigma + offset
