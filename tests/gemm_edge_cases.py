"""Cases, oracles, bounds and host-rule mirrors for the matrix-product kernels: gemm_bf16_kernel<0|1|2>
(csrc/gemm_bf16.hip), bmm_nt_kernel (csrc/bmm.hip), gemm_f32_kernel / gemv_f32_kernel (csrc/tensor_math.hip).
CPU only: nothing native is imported here. tests/test_gemm_edges_cpu.py checks this file, tests/test_gemm_edges_gpu.py
holds the kernels to it.

Exact leg. Operands are nonzero integers: {-4..-1, 1..4} for the bf16 kernels (K <= 8200: every partial sum is at most
16 * 8200 = 131200 < 2^24), [-64, 64] \\ {0} for the fp32 kernels (K <= 33: at most 33 * 4096 = 135168 < 2^24), so an
fp32 accumulation is exact in any order, split or not. alpha, beta and colscale are powers of two (or 0) of at least
1/4, bias and the old C / colsum / M are integers: every final value is a multiple of 1/4 far below 2^22, an fp32
number. The expected value is computed in int64 in units of 1/4 (``quarters``) and compared with torch.equal; a bf16
result is the round-to-nearest-even bf16 of that fp32 number (f2bf of csrc/common.h), compared bit for bit up to the
sign of zero. No operand is zero, so a dropped, duplicated or misplaced term changes the value. ``kind == "pos"`` is
position coded: A[m, k] = 1 iff k == m % K and B holds distinct integers, so C[m, :] = B[m % K, :] and an index
permutation can be read from the failure.

Rounded leg (K <= 264). Operands are randn rounded to the kernel's input type; the operation is repeated in fp64 on
those values and compared per element against
    B_ij = |alpha| (K + S + 2) 2^-24 sum_k |a_ik b_kj|  +  R 2^-24 (|alpha| sum_k |a_ik b_kj| + |bias_j| + |beta C_old|)
S = slices of the reduction (1 when unsplit), R = one fp32 rounding each for the alpha scale, the bias add and the
beta * C_old add where present (beta is a power of two: its product is exact). First term: an fp32 sum of K terms in
any order or tree rounds at most K - 1 times on any path to the result, each time on a partial sum that is at most
sum |a b| (1 + small); S more roundings combine the slices; bf16 x bf16 products are exact in fp32, and for the fp32
kernels the fused multiply-add rounds the product and the add once, which is the rounding already counted; 2 to spare
for the second-order terms. How the MFMA rounds inside one instruction is not documented, so the test asserts
max_ij |kernel - exact| / B_ij <= allowed, with ``ALLOWED`` = twice the largest ratio measured on an MI355X against
the fp64 reference, two digits, never above 1 (profiles/gemm_edge_errors.txt). A bf16 result adds half a bf16 ulp of
the number that is rounded (``bf16_half_ulp``), not a fixed 2^-9 (profiles/recurrent_edge_errors.txt records why).

Guards. ``guard`` makes every tensor a kernel sees a view inside a larger allocation: operands surrounded by NaN
(the gap between a row's extent and its leading dimension included), written tensors by a sentinel; ``Guard.ok``
compares every byte outside the view with a snapshot.
"""
import functools
from dataclasses import dataclass

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
FORMS = ("nt", "nn", "tn")
NAN = float("nan")
SENTINEL = -1234.5
PAD_R, PAD_C, HEAD = 3, 8, 64        # surround of an "inside" view (rows, columns) and of a dense one (elements)

# Allowed largest |kernel - fp64| / B per leg: 2 x the largest ratio measured on an MI355X, rounded up to two
# significant digits, never above the cap of 1 (the derivation). The table stands in profiles/gemm_edge_errors.txt.
CAP = 1.0
ALLOWED = {"gemm_bf16_f32": 0.083, "gemm_bf16_bf16": 1.0, "gemm_bf16_colsum": 0.029, "bmm_nt": 0.22,
           "gemm_f32": 0.061, "gemv_f32": 0.044}


# ------------------------------------------------------------------------------------------------- host-rule mirrors
GB_SLOT = 256 * 256 + 256            # floats per (tile, slice) slot of the split workspace
GB_CUS = 256


def gb_split(M, N, K):
    """Mirror of gb_split (csrc/gemm_bf16.hip): (slices, K-tiles per slice)."""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    nk = (K + 63) // 64
    s = max(1, min(GB_CUS // tiles, nk // 8, 16))
    per = max(1, (nk + s - 1) // s)
    return ((nk + per - 1) // per if nk > 0 else 1), per


def gb_slices(M, N, K):
    """[k_begin, k_end) of every slice, in elements."""
    ns, per = gb_split(M, N, K)
    return [(s * per * 64, min(K, (s + 1) * per * 64)) for s in range(ns)]


def gb_ws_bytes(M, N, K):
    ns, _ = gb_split(M, N, K)
    if ns <= 1:
        return 0
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    return tiles * ns * GB_SLOT * 4 + tiles * 4


# hand-written: (M, N, K) -> (nk, slices, K-tiles per slice, K-tiles of the last slice)
GB_SPLIT_TABLE = {
    (8, 8, 960): (15, 1, 15, 15),
    (8, 8, 1024): (16, 2, 8, 8),
    (8, 8, 1032): (17, 2, 9, 8),
    (8, 8, 8192): (128, 16, 8, 8),
    (8, 8, 8200): (129, 15, 9, 3),
    (264, 264, 1024): (16, 2, 8, 8),
    (264, 264, 1032): (17, 2, 9, 8),
}


# ------------------------------------------------------------------------------------------------------------ guards
def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guard:
    """``view`` = cut(buf) inside ``buf``; ``seal`` after the view is filled, ``ok`` after the launch."""

    def __init__(self, buf_shape, dtype, fill, device, cut):
        self.buf = torch.full(tuple(buf_shape), fill, dtype=dtype, device=device)
        self.view = cut(self.buf)
        mask = torch.zeros(tuple(buf_shape), dtype=torch.bool, device=device)
        cut(mask).fill_(True)
        self.outside = ~mask
        self.before = None

    def seal(self):
        self.before = _bits(self.buf)[self.outside].clone()
        return self

    def ok(self):
        return torch.equal(_bits(self.buf)[self.outside], self.before)


def guard(shape, dtype, fill, device, layout="inside", src=None, step=1):
    """A guarded tensor of ``shape``. 1-D: every ``step``-th element of a buffer with PAD_C elements on both sides.
    [..., R, C] ``inside``: rows PAD_R .. and columns PAD_C .. of [..., R + 2 PAD_R, C8 + 2 PAD_C] with C8 = C rounded
    up to 8 (leading dimension a multiple of 8, larger than the extent); ``dense``: contiguous, HEAD elements on both
    sides. Bases stay 16-byte aligned for 2- and 4-byte types."""
    shape = tuple(shape)
    if len(shape) == 1:
        (n,) = shape
        g = Guard((2 * PAD_C + max(n, 1) * step,), dtype, fill, device, lambda t: t[PAD_C:PAD_C + n * step:step])
    elif layout == "dense":
        n = 1
        for s in shape:
            n *= s
        g = Guard((2 * HEAD + n,), dtype, fill, device, lambda t: t[HEAD:HEAD + n].view(shape))
    else:
        R, C = shape[-2:]
        C8 = -(-C // 8) * 8
        g = Guard(shape[:-2] + (R + 2 * PAD_R, C8 + 2 * PAD_C), dtype, fill, device,
                  lambda t: t[..., PAD_R:PAD_R + R, PAD_C:PAD_C + C])
    if src is not None:
        g.view.copy_(src)
    return g


# ------------------------------------------------------------------------------------------------------------ values
def _gen(*key):
    seed = 1469598103
    for k in key:
        for ch in str(k):
            seed = (seed * 1099511 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(seed)


def ints(shape, hi, g, lo=1):
    """int64 values of magnitude lo..hi and random sign: never zero."""
    mag = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    return mag * (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1)


def quarters(q):
    """int64 multiples of 1/4 -> the fp32 number (exact: checked by the CPU tests)."""
    return (q.double() / 4).float()


def _q4(x):
    q = round(4 * x)
    assert q == 4 * x, x
    return q


def bf16_half_ulp(x):
    """Half a bf16 ulp (8 significand bits) of |x|, element-wise in fp64; 0 at 0."""
    x = x.abs().double()
    _, e = torch.frexp(x)                      # |x| = m 2^e, m in [0.5, 1): ulp = 2^(e - 8)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - 9), torch.zeros_like(x))


def bf16_equal(got, want):
    """Bit equality of two bf16 tensors, the sign of zero aside."""
    g, w = _bits(got.contiguous()).int() & 0xffff, _bits(want.contiguous()).int() & 0xffff
    return bool(((g == w) | (((g | w) & 0x7fff) == 0)).all())


def bound(alpha, K, S, absprod, bias=None, beta_old=None, bf16_exact=None):
    """B_ij of the module docstring (fp64)."""
    mag = abs(alpha) * absprod
    total, R = mag.clone(), 1
    if bias is not None:
        total, R = total + bias.abs(), R + 1
    if beta_old is not None:
        total, R = total + beta_old.abs(), R + 1
    b = (K + S + 2) * U * mag + R * U * total
    if bf16_exact is not None:
        b = b + bf16_half_ulp(bf16_exact.abs() + b)
    return b


def ratio(got, exact, b):
    """max_ij |got - exact| / B_ij, with the place of the maximum."""
    r = (got.double() - exact).abs() / b
    r = torch.where(b > 0, r, ((got.double() - exact) != 0).double() * float("inf")).nan_to_num(nan=float("inf"))
    i = int(r.argmax())
    return float(r.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


# -------------------------------------------------------------------------------------------------- gemm_bf16 cases
@dataclass(frozen=True)
class GB:
    form: str
    M: int
    N: int
    K: int
    out: str = "f32"          # "f32" | "bf16"
    alpha: float = 1.0
    beta: float = 0.0
    bias: str = ""            # "" | "f32" | "bf16"
    colscale: float = 0.0     # 0: no colsum (TN only)
    layout: str = "inside"    # "inside": every ld > extent; "dense": ld == extent
    kind: str = "int"         # "int" | "pos" | "randn"

    @property
    def id(self):
        s = f"{self.form}-{self.M}x{self.N}x{self.K}-{self.out}"
        if self.alpha != 1.0:
            s += f"-a{self.alpha:g}"
        if self.beta != 0.0:
            s += f"-b{self.beta:g}"
        if self.bias:
            s += f"-bias{self.bias}"
        if self.colscale:
            s += f"-cs{self.colscale:g}"
        return s + ("-dense" if self.layout == "dense" else "") + ("" if self.kind == "int" else "-" + self.kind)

    @property
    def slices(self):
        return gb_split(self.M, self.N, self.K)[0]


GB_EXTENTS = (8, 16, 24, 40, 64, 72, 120, 128, 136, 248, 256, 264)
GB_K_PIPE = {8: 1, 56: 1, 64: 1, 72: 2, 128: 2, 136: 3, 192: 3, 200: 4, 256: 4}      # K -> nk
GB_SPLIT_SHAPES = tuple(GB_SPLIT_TABLE)[:6]
GB_SPLIT_COLSUM = GB("tn", 264, 264, 1032, colscale=0.25)


def _gb_exact_cases():
    out = []
    for f in FORMS:
        # M / N boundaries, K = 72: two K-tiles, the second a tail of one granule
        for e in GB_EXTENTS:
            out += [GB(f, e, 24, 72), GB(f, 8, e, 72)]
        out.append(GB(f, 264, 264, 72))
        # the pipeline's branches on nk, dense at one partial tile and row-strided at four
        for K in GB_K_PIPE:
            out += [GB(f, 40, 24, K, layout="dense"), GB(f, 264, 264, K)]
        out.pop()                                       # (264, 264, 256) comes below with an epilogue
        # epilogue variants
        for M, N, K in ((72, 40, 136), (264, 264, 256)):
            out += [GB(f, M, N, K, out="bf16"), GB(f, M, N, K, alpha=0.5), GB(f, M, N, K, alpha=-2.0, out="bf16"),
                    GB(f, M, N, K, beta=1.0), GB(f, M, N, K, alpha=-2.0, beta=0.5, layout="dense")]
            if f == "tn":
                out += [GB(f, M, N, K, colscale=1.0), GB(f, M, N, K, alpha=0.5, beta=1.0, colscale=0.25)]
            else:
                out += [GB(f, M, N, K, alpha=0.5, bias="f32"), GB(f, M, N, K, out="bf16", bias="bf16"),
                        GB(f, M, N, K, alpha=-2.0, beta=0.5, bias="bf16", layout="dense"),
                        GB(f, M, N, K, out="bf16", alpha=0.5, bias="f32")]
        # position coded: C[m, :] = B[m % K, :]
        out += [GB(f, 40, 24, 8, kind="pos"), GB(f, 264, 8, 24, kind="pos")]
    return tuple(dict.fromkeys(out))                    # (8, 24) arises twice from the extents


def _gb_split_cases():
    out = []
    for f in FORMS:
        out += [GB(f, *s) for s in GB_SPLIT_SHAPES]
        out += [GB(f, 8, 8, 8200, out="bf16", alpha=0.5), GB(f, 264, 264, 1024, alpha=-2.0, beta=0.5)]
    out += [GB_SPLIT_COLSUM, GB("tn", 8, 8, 8200, colscale=1.0), GB("nt", 264, 264, 1032, out="bf16", bias="f32")]
    return tuple(out)


def _gb_rounded_cases():
    out = []
    for f in FORMS:
        for M, N, K in ((264, 520, 200), (40, 24, 72)):
            out += [GB(f, M, N, K, kind="randn"), GB(f, M, N, K, out="bf16", kind="randn"),
                    GB(f, M, N, K, alpha=0.5, beta=1.0, kind="randn"), GB(f, M, N, K, alpha=-2.0, beta=0.5, kind="randn")]
            if f == "tn":
                out += [GB(f, M, N, K, colscale=0.25, kind="randn"), GB(f, M, N, K, colscale=1.0, out="bf16", kind="randn")]
            else:
                out += [GB(f, M, N, K, bias="f32", kind="randn"), GB(f, M, N, K, bias="bf16", alpha=0.5, kind="randn"),
                        GB(f, M, N, K, out="bf16", bias="bf16", kind="randn"),
                        GB(f, M, N, K, out="bf16", bias="f32", alpha=0.5, kind="randn")]
    return tuple(out)


GB_EXACT, GB_SPLIT, GB_ROUNDED = _gb_exact_cases(), _gb_split_cases(), _gb_rounded_cases()


def gb_shapes(c):
    """Stored shapes of a and b."""
    return ((c.K, c.M) if c.form == "tn" else (c.M, c.K)), ((c.N, c.K) if c.form == "nt" else (c.K, c.N))


def gb_ops(c, a, b):
    """Stored operands -> A [M, K], B [K, N]."""
    return (a.t() if c.form == "tn" else a), (b.t() if c.form == "nt" else b)


@functools.lru_cache(maxsize=None)
def gb_problem(c):
    """Stored operands, old values and the expected results of one case, computed once.
    Keys: a, b (bf16); old (fp32 [M, N] or None); bias (its dtype, or None); cs_old (fp32 [M] or None);
    exact legs: want (fp32), want_cs (fp32), ia, ib (int64 A [M, K], B [K, N]), q (int64 quarters);
    rounded leg: exact, b (fp64), exact_cs, b_cs (fp64)."""
    g = _gen("gb", c.id)
    sa, sb = gb_shapes(c)
    p = {"old": None, "bias": None, "cs_old": None, "want_cs": None}
    if c.kind == "randn":
        a, b = torch.randn(*sa, generator=g).to(BF16), torch.randn(*sb, generator=g).to(BF16)
        A, B = (t.double() for t in gb_ops(c, a, b))
        exact, absprod = c.alpha * (A @ B), A.abs() @ B.abs()
        bias = beta_old = None
        if c.bias:
            p["bias"] = (torch.randn(c.N, generator=g) * 4).to(BF16 if c.bias == "bf16" else F32)
            bias = p["bias"].double().expand(c.M, c.N)
            exact = exact + bias
        if c.beta != 0.0:
            p["old"] = torch.randn(c.M, c.N, generator=g) * 30
            beta_old = c.beta * p["old"].double()
            exact = exact + beta_old
        p.update(a=a, b=b, exact=exact,
                 bound=bound(c.alpha, c.K, c.slices, absprod, bias, beta_old, exact if c.out == "bf16" else None))
        if c.colscale:
            p["cs_old"] = torch.randn(c.M, generator=g) * 10
            p["exact_cs"] = p["cs_old"].double() + c.colscale * A.sum(1)
            p["bound_cs"] = bound(c.colscale, c.K, c.slices, A.abs().sum(1), None, p["cs_old"].double())
        return p
    if c.kind == "pos":
        assert c.K * c.N <= 256                          # distinct integers that bf16 holds
        ia = (torch.arange(c.K)[None, :] == (torch.arange(c.M) % c.K)[:, None]).long()
        ib = 1 + torch.arange(c.K * c.N).view(c.K, c.N)
    else:
        ia, ib = ints((c.M, c.K), 4, g), ints((c.K, c.N), 4, g)
    q = _q4(c.alpha) * (ia @ ib)
    if c.bias:
        ibias = ints((c.N,), 40, g)
        p["bias"] = ibias.to(BF16 if c.bias == "bf16" else F32)
        q = q + 4 * ibias
    if c.beta != 0.0:
        iold = ints((c.M, c.N), 1000, g)
        p["old"] = iold.float()
        q = q + _q4(c.beta) * iold
    if c.colscale:
        ics = ints((c.M,), 1000, g)
        p["cs_old"] = ics.float()
        p["q_cs"] = 4 * ics + _q4(c.colscale) * ia.sum(1)
        p["want_cs"] = quarters(p["q_cs"])
    p.update(a=(ia.t() if c.form == "tn" else ia).contiguous().to(BF16),
             b=(ib.t() if c.form == "nt" else ib).contiguous().to(BF16), ia=ia, ib=ib, q=q, want=quarters(q))
    return p


# ----------------------------------------------------------------------------------------------------- bmm_nt cases
@dataclass(frozen=True)
class BM:
    M: int
    N: int
    K: int
    batch: int = 1
    alpha: float = 1.0
    accum: bool = False
    bcast: str = ""           # "" | "a" | "b": that operand has batch stride 0
    layout: str = "inside"
    kind: str = "int"

    @property
    def id(self):
        return (f"{self.batch}x{self.M}x{self.N}x{self.K}-a{self.alpha:g}" + ("-accum" if self.accum else "")
                + (f"-bcast_{self.bcast}" if self.bcast else "") + ("-dense" if self.layout == "dense" else "")
                + ("" if self.kind == "int" else "-" + self.kind))


BM_EXTENTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)
BM_KS = (32, 64, 96, 128, 160)


def _bm_cases():
    out = []
    for i, M in enumerate(BM_EXTENTS):                  # every extent as M and (reversed) as N
        out.append(BM(M, BM_EXTENTS[-1 - i], BM_KS[i % 5], batch=(1, 3)[i % 2], alpha=(1.0, 0.5)[(i // 2) % 2],
                      accum=i % 3 == 1, layout=("inside", "dense")[i % 4 == 3]))
    for K in BM_KS:                                     # every K at four tiles, three of them partial
        out.append(BM(65, 130, K, batch=3, alpha=0.5, accum=K % 64 == 32))
    out += [BM(130, 130, 96, accum=True), BM(33, 17, 96, batch=3, bcast="b", accum=True),
            BM(17, 65, 160, batch=3, bcast="a", alpha=0.5), BM(130, 8, 32, batch=3, kind="pos")]
    return tuple(out)


BM_EXACT = _bm_cases()
BM_ROUNDED = (BM(130, 65, 160, batch=3, kind="randn"), BM(33, 130, 96, alpha=0.5, accum=True, kind="randn"),
              BM(17, 15, 32, batch=3, accum=True, bcast="b", kind="randn"))


@functools.lru_cache(maxsize=None)
def bm_problem(c):
    """a [Ba, M, K], b [Bb, N, K] (bf16; the broadcast operand has one batch), old [batch, M, N] (fp32 or None) and
    want (fp32) or exact / bound (fp64)."""
    g = _gen("bm", c.id)
    Ba, Bb = (1 if c.bcast == "a" else c.batch), (1 if c.bcast == "b" else c.batch)
    p = {"old": None}
    if c.kind == "randn":
        a, b = torch.randn(Ba, c.M, c.K, generator=g).to(BF16), torch.randn(Bb, c.N, c.K, generator=g).to(BF16)
        A, B = a.double().expand(c.batch, -1, -1), b.double().expand(c.batch, -1, -1).transpose(1, 2)
        exact, beta_old = c.alpha * (A @ B), None
        if c.accum:
            p["old"] = torch.randn(c.batch, c.M, c.N, generator=g) * 30
            beta_old = p["old"].double()
            exact = exact + beta_old
        p.update(a=a, b=b, exact=exact, bound=bound(c.alpha, c.K, 1, A.abs() @ B.abs(), None, beta_old))
        return p
    if c.kind == "pos":
        assert c.K * c.N <= 256
        ia = (torch.arange(c.K)[None, :] == (torch.arange(c.M) % c.K)[:, None]).long().expand(Ba, -1, -1)
        ib = (1 + torch.arange(c.K * c.N).view(c.K, c.N)).t().expand(Bb, -1, -1)
    else:
        ia, ib = ints((Ba, c.M, c.K), 4, g), ints((Bb, c.N, c.K), 4, g)
    q = _q4(c.alpha) * (ia.expand(c.batch, -1, -1) @ ib.expand(c.batch, -1, -1).transpose(1, 2))
    if c.accum:
        iold = ints((c.batch, c.M, c.N), 1000, g)
        p["old"] = iold.float()
        q = q + 4 * iold
    p.update(a=ia.contiguous().to(BF16), b=ib.contiguous().to(BF16), ia=ia, ib=ib, q=q, want=quarters(q))
    return p


# layer-level leg through ops.bmm.matmul: (a shape, b shape); K in {1, 31, 33}, a vector b, broadcast leading dims
MATMUL_CASES = (((3, 17, 1), (3, 1, 33)), ((2, 1, 15, 31), (3, 31, 9)), ((3, 33, 33), (33,)), ((16, 33), (33, 65)))


@functools.lru_cache(maxsize=None)
def matmul_problem(i):
    """Integer a, b and upstream gradient g (fp32) with the exact forward and both gradients (fp32, from int64)."""
    sa, sb = MATMUL_CASES[i]
    gen = _gen("matmul", i)
    ia, ib = ints(sa, 4, gen), ints(sb, 4, gen)
    a = ia.double().requires_grad_(True)                # integers below 2^53: fp64 autograd is exact here
    b = ib.double().requires_grad_(True)
    out = torch.matmul(a, b)
    ig = ints(tuple(out.shape), 4, gen)
    out.backward(ig.double())
    return dict(a=ia.float(), b=ib.float(), g=ig.float(), out=out.detach().float(), ga=a.grad.float(), gb=b.grad.float(),
                out64=out.detach(), ga64=a.grad, gb64=b.grad)


# ------------------------------------------------------------------------------------------- gemm_f32 / gemv_f32
@dataclass(frozen=True)
class GF:
    M: int
    N: int
    K: int
    batch: int = 1
    ta: bool = False          # A, B, C stored transposed and addressed through strides
    tb: bool = False
    tc: bool = False
    min: str = ""             # "" | "full" | "row" (broadcast row vector, row stride 0) | "inplace" (M is C)
    bsb0: bool = False        # B has batch stride 0
    alpha: float = 1.0
    beta: float = 0.0
    kind: str = "int"

    @property
    def id(self):
        return (f"{self.batch}x{self.M}x{self.N}x{self.K}" + "".join(n for n, f in (("-tA", self.ta), ("-tB", self.tb),
                ("-tC", self.tc), ("-bsb0", self.bsb0)) if f) + (f"-M{self.min}" if self.min else "")
                + f"-a{self.alpha:g}-b{self.beta:g}" + ("" if self.kind == "int" else "-" + self.kind))


GF_EXTENTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)
GF_KS = (0, 1, 3, 4, 5, 15, 16, 17, 33)


def _gf_cases():
    out = []
    mins = ("", "full", "row", "inplace")
    ab = ((1.0, 1.0), (0.5, 0.5), (1.0, 0.0), (0.5, 1.0), (0.0, 0.5), (1.0, 0.5))
    for i, M in enumerate(GF_EXTENTS):
        al, be = ab[i % 6] if mins[i % 4] else (0.5 + 0.5 * (i % 8 == 0), 0.0)      # no M: no beta, alpha not 0
        out.append(GF(M, GF_EXTENTS[-1 - i], GF_KS[(i + 1) % 9], batch=(1, 3)[i % 2], ta=i % 2 == 1, tb=i % 3 == 1,
                      tc=i % 4 == 1, min=mins[i % 4], alpha=al, beta=be))
    for i, K in enumerate(GF_KS):                       # every K at four tiles, three of them partial
        al, be = ab[(i + 2) % 6] if mins[(i + 1) % 4] else (0.5, 0.0)
        out.append(GF(65, 130, K, batch=(3, 1)[i % 2], ta=i % 3 == 0, tb=i % 2 == 0, tc=i % 3 == 1,
                      min=mins[(i + 1) % 4], bsb0=i % 4 == 0, alpha=al, beta=be))
    out += [GF(17, 33, 0), GF(17, 33, 0, batch=3, min="row", beta=0.5), GF(33, 17, 0, min="inplace", tc=True, beta=1.0),
            GF(130, 65, 33, batch=3, bsb0=True, kind="pos"), GF(64, 64, 16, min="full", beta=0.0),
            GF(65, 17, 5, batch=3, min="inplace", beta=0.0, alpha=0.5)]
    assert len(set(out)) == len(out)
    return tuple(out)


GF_EXACT = _gf_cases()
GF_ROUNDED = (GF(130, 70, 200, batch=3, kind="randn"), GF(70, 130, 264, ta=True, tb=True, tc=True, min="full", alpha=0.5,
                                                         beta=0.5, kind="randn"),
              GF(33, 17, 72, min="row", beta=1.0, kind="randn"))


@functools.lru_cache(maxsize=None)
def gf_problem(c):
    """A [batch, M, K], B [batch or 1, K, N], mold ([batch, M, N], [N] for a row, or None) in fp32, and want (fp32) or
    exact / bound (fp64)."""
    g = _gen("gf", c.id)
    Bb = 1 if c.bsb0 else c.batch
    p = {"mold": None}
    mshape = (c.N,) if c.min == "row" else (c.batch, c.M, c.N)
    if c.kind == "randn":
        a, b = torch.randn(c.batch, c.M, c.K, generator=g), torch.randn(Bb, c.K, c.N, generator=g)
        A, B = a.double(), b.double().expand(c.batch, -1, -1)
        exact, beta_old = c.alpha * (A @ B), None
        if c.min:
            p["mold"] = torch.randn(*mshape, generator=g) * 30
            if c.beta != 0.0:
                beta_old = (c.beta * p["mold"].double()).expand(c.batch, c.M, c.N)
                exact = exact + beta_old
        p.update(a=a, b=b, exact=exact, bound=bound(c.alpha, c.K, 1, A.abs() @ B.abs(), None, beta_old))
        return p
    if c.kind == "pos":
        ia = (torch.arange(c.K)[None, :] == (torch.arange(c.M) % c.K)[:, None]).long().expand(c.batch, -1, -1)
        ib = (1 + torch.arange(c.K * c.N).view(c.K, c.N)).expand(Bb, -1, -1)
    else:
        ia, ib = ints((c.batch, c.M, c.K), 64, g), ints((Bb, c.K, c.N), 64, g)
    q = _q4(c.alpha) * (ia @ ib.expand(c.batch, -1, -1))
    if c.min:
        im = ints(mshape, 1000, g)
        p["mold"] = im.float()
        q = q + _q4(c.beta) * im
    p.update(a=ia.contiguous().float(), b=ib.contiguous().float(), ia=ia, ib=ib, q=q, want=quarters(q))
    return p


@dataclass(frozen=True)
class GV:
    M: int
    K: int
    ta: bool = False
    sx: int = 1               # element steps of x, M and y
    sm: int = 0               # 0: no M
    sy: int = 1
    alpha: float = 1.0
    beta: float = 0.0
    kind: str = "int"

    @property
    def id(self):
        return (f"{self.M}x{self.K}" + ("-tA" if self.ta else "") + f"-sx{self.sx}-sm{self.sm}-sy{self.sy}"
                + f"-a{self.alpha:g}-b{self.beta:g}" + ("" if self.kind == "int" else "-" + self.kind))


GV_MS, GV_KS = (1, 3, 4, 5, 9), (0, 1, 63, 64, 65, 129)


def _gv_cases():
    out = []
    ab = ((1.0, 1.0), (0.5, 0.5), (1.0, 0.0), (0.0, 0.5))
    for i, K in enumerate(GV_KS):
        for j, M in enumerate(GV_MS):
            if (i + j) % 2:
                continue
            n = i + j
            sm = (0, 1, 2)[(i + 2 * j) % 3]
            al, be = ab[n % 4] if sm else (0.5 + 0.5 * (n % 4 == 0), 0.0)                # no M: no beta, alpha not 0
            out.append(GV(M, K, ta=n % 4 >= 2, sx=(1, 3)[n % 3 == 0], sm=sm, sy=(1, 2)[j % 2 == 0 and i > 0], alpha=al,
                          beta=be))
    out += [GV(9, 0), GV(9, 0, sm=1, beta=0.5), GV(5, 65, sm=2, beta=0.0), GV(9, 33, ta=True, sx=2, sy=3, kind="pos")]
    assert len(set(out)) == len(out)
    return tuple(out)


GV_EXACT = _gv_cases()
GV_ROUNDED = (GV(9, 264, kind="randn"), GV(5, 200, ta=True, sx=2, sm=2, sy=3, alpha=0.5, beta=0.5, kind="randn"),
              GV(130, 72, sm=1, beta=1.0, kind="randn"))


@functools.lru_cache(maxsize=None)
def gv_problem(c):
    """A [M, K], x [K], mold ([M] or None) in fp32 and want (fp32) or exact / bound (fp64)."""
    g = _gen("gv", c.id)
    p = {"mold": None}
    if c.kind == "randn":
        a, x = torch.randn(c.M, c.K, generator=g), torch.randn(c.K, generator=g)
        exact, beta_old = c.alpha * (a.double() @ x.double()), None
        if c.sm:
            p["mold"] = torch.randn(c.M, generator=g) * 30
            if c.beta != 0.0:
                beta_old = c.beta * p["mold"].double()
                exact = exact + beta_old
        p.update(a=a, x=x, exact=exact, bound=bound(c.alpha, c.K, 1, a.double().abs() @ x.double().abs(), None, beta_old))
        return p
    if c.kind == "pos":
        ia = (torch.arange(c.K)[None, :] == (torch.arange(c.M) % c.K)[:, None]).long()
        ix = 1 + torch.arange(c.K)
    else:
        ia, ix = ints((c.M, c.K), 64, g), ints((c.K,), 64, g)
    q = _q4(c.alpha) * (ia @ ix)
    if c.sm:
        im = ints((c.M,), 1000, g)
        p["mold"] = im.float()
        q = q + _q4(c.beta) * im
    p.update(a=ia.float(), x=ix.float(), ia=ia, ix=ix, q=q, want=quarters(q))
    return p
