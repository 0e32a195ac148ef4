"""Cases, data, fp64 one-step oracles, per-element bounds and tile-rule mirrors for the recurrent kernels: the fused
LSTM steps (csrc/lstm.hip), the GRU steps (csrc/gru.hip), the persistent whole-sequence kernels (csrc/lstm_seq.hip),
the flat LSTM cell (lstm_cell_fwd / lstm_cell_bwd of csrc/elementwise.hip) and the dropout replication kernels
(csrc/lstm_drop.hip). Pure torch / numpy: tests/test_recurrent_edges_cpu.py checks this file on its own,
tests/test_recurrent_edges_gpu.py holds the kernels to it.

Method: one step at a time, on exactly the operands the kernel used
---------------------------------------------------------------------
Every step kernel takes its GEMM operands as bf16 tensors and the rest of its state in fp32, so one step has an fp64
oracle on bit-identical inputs: the products of two bf16 numbers are exact in fp32 and in fp64, and an fp64 sum of
a few thousand of them is exact to 2^-53 relative. What is left to the kernel is fp32 accumulation, the fp32 gate
functions and a handful of fp32 products. A persistent launch saves every hand-off (h16, cs, acts, dg16; the GRU's
gates, h16, rh16, dn16, drz16), so it is verified by induction: step t's oracle is fed the kernel's own saved step
t - 1 tensors, and the first wrong element at any step fails under a bound that does not grow with T.

Bounds (u = 2^-24, the unit round-off of fp32; all to first order in u)
----------------------------------------------------------------------
* an fp32 sum or product rounds to nearest: |fl(x op y) - (x op y)| <= u |x op y|. ``V`` carries a value and an
  absolute error bound through +, -, * by this rule (products: |a| e_b + |b| e_a + u |ab|); ``V.out()`` adds the one
  extra u of the "(ops + 1) u" chain rule at every stored result. A contracted multiply-add rounds once where the rule
  counts twice, so the bound holds with or without FMA contraction.
* pre-activation (``dot``): n exact bf16 products accumulated in fp32 in any order, KS chunk sums, the addends x
  (the input projection, dout, a carry ...):

      |da| <= (n + KS + 2 + (addends - 1)) u (sum |x| + sum_k |w_k h_k|)

  the standard chain bound, of the form of the (n + 4) 2^-23 sum|terms| used for the sparse kernels. With no GEMM
  operand (first / last step) only the roundings of the additions remain (none for a single addend).
* gate functions, ``sigm`` and ``tanh_f`` of csrc/rnn_step.h built on __expf (exp2 of the argument times log2 e):
  ASSUMING a hardware exp2 within 1 ulp (2u relative) and a correctly rounded divide, the argument product costs a
  relative |a| u on e = exp(-a), so e is off by (|a| + 2) u relative. sigma = 1 / (1 + e) has
  |d sigma / d ln e| = sigma (1 - sigma) <= 1/4, the sum 1 + e and the divide add about u more:

      |d sigma| <= 1/4 |da| + c_s u,   c_s = 1/4 (|a| + 2) + 1

  tanh = (1 - e) / (1 + e) with e = exp(-2|a|): e is off by (2|a| + 2) u relative, |dt / d ln e| = 2e / (1 + e)^2
  <= 1/2, the difference, the sum and the divide add about 2u:

      |d tanh| <= |da| + c_t u,   c_t = 1/2 (2|a| + 2) + 2

  (1/4 and 1 are the Lipschitz constants of sigma and tanh, so the |da| terms are rigorous.) The 1-ulp exp2 has NOT
  been measured on this hardware; the measured ratios of profiles/recurrent_edge_errors.txt are the evidence that the
  constants suffice. The flat cell kernels call the library tanhf instead and are held to the same constants.
* everything downstream (c, h, dg, dc, dx, dhp) is propagated through the cell formulas by ``V``. 1 - y^2 is taken
  as the product and the difference it is, so its absolute error u y^2 is kept where 1 - y^2 is small.
* a result the kernel stores only as bf16 (the bf16-I/O output and input gradient of the persistent LSTM) adds one
  round-to-nearest: half a bf16 ulp of the rounded number, 2^(floor(log2 |x|) - 8). That is 2^-9 |x| only at the top
  of a binade and 2^-8 |x| at its bottom (bf16 has 8 significand bits), so the bound takes the half ulp itself
  (``bf16_half_ulp``) and not a fixed relative 2^-9, which a correctly rounded store misses by up to 2x.
* quantities a persistent backward keeps in registers (the LSTM's dc, the GRU's dhp) are carried by the oracle in
  fp64 from the top, with their error bound: the bound of step t is the running sum of the per-step bounds.

A check is the ratio |kernel - oracle| / bound per element, capped at 1.

Sensitivity: the cases carry "spikes" (a state operand of 8 in every batch row, weights of +-1 in the spike
columns of the edge rows, the projection input chosen to cancel them) so that one dropped product or one bf16 ulp of
one operand exceeds the chain bound several times over even at K = 4096, where a typical product is smaller than
the bound. The sequence cases add spikes that last through the steps (see ``lstm_seq_inputs``, ``gru_seq_inputs``).
tests/test_recurrent_edges_cpu.py plants each error on these very inputs.

The tile-rule mirrors below follow the rules' own arithmetic; their independence comes from the hand-written tables
(LSTM_STEP_SHAPES and the others), which state for every case what the issue names it for and are asserted against
the mirrors in the CPU test and before every launch.
"""
import math

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U24 = 2.0 ** -24
SENTINEL = 0xA5
PLAIN = (0, 2, 1, 3)       # positions of the i, f, g, o blocks in nn.LSTM's (i, g, f, o) gate axis
IFGO = (0, 1, 2, 3)        # LSTMPeephole's (i, f, g, o)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================ tile-rule mirrors
def ksplit(K, cap):
    """K chunks of at least 256, at most ``cap``, stepping down until the chunk is a whole number of 32-wide k-steps."""
    ks = max(1, min(cap, K // 256))
    while ks > 1 and K % (ks * 32) != 0:
        ks -= 1
    return ks


def lstm_nb(H, B):
    """Two batch tiles per workgroup once the one-tile grid has more than 256 workgroups."""
    return 2 if (H // 16) * ((B + 15) // 16) > 256 else 1


def lstm_fwd_tile(H, B):
    NB = lstm_nb(H, B)
    KS = 1
    for k in range(8 if NB == 2 else 16, 1, -1):
        if H % (k * 32) == 0:
            KS = k
            break
    if 64 * KS < 256 * NB:
        NB = 1
    waves = max(KS, 4 * NB)
    steps = H // KS // 32
    return {"NB": NB, "KS": KS, "waves": waves, "pad_waves": waves - KS, "ksteps": steps, "groups": steps // 4,
            "tail": steps % 4, "grid": (H // 16, (B + 16 * NB - 1) // (16 * NB))}


def lstm_bwd_tile(H, B):
    ks0 = ksplit(4 * H, 16)
    KS = max(ks0, 4)
    NB = 1 if KS * 64 < 512 else lstm_nb(H, B)
    NU = 2 if (NB == 2 and KS == 16 and (H // 16) * ((B + 31) // 32) > 256) else 1
    steps = 4 * H // KS // 32
    ch = 4 if NU * NB > 2 else 8
    return {"NB": NB, "NU": NU, "KS": KS, "ksteps": steps, "groups": steps // ch, "tail": steps % ch,
            "grid": (H // (16 * NU), (B + 16 * NB - 1) // (16 * NB))}


def gru_tile(K):
    KS = ksplit(K, 16)
    steps = K // KS // 32
    return {"KS": KS, "waves": max(KS, 4), "idle_waves": max(KS, 4) - KS, "ksteps": steps, "groups": steps // 8,
            "tail": steps % 8}


NGRP = 8


def seq_shape(B, H, gru=False):
    """Batch rows per group, 16-row tiles per group and the fill of the 8 groups of a persistent launch."""
    Bg = (B + NGRP - 1) // NGRP
    live = (B + Bg - 1) // Bg
    return {"ok": H in (256, 512, 1024) and Bg <= (16 if gru else 32), "Bg": Bg, "NT": 2 if Bg > 16 else 1,
            "live_groups": live, "full_groups": B // Bg, "last_rows": B - (live - 1) * Bg, "empty_groups": NGRP - live,
            "grid": NGRP * (H // 32)}


# what each (B, H) of the step legs is there for; tests assert these against the mirrors before every launch
LSTM_STEP_SHAPES = {
    (1, 32): {"fwd": {"KS": 1, "pad_waves": 3, "NB": 1}, "bwd": {"KS": 4, "NB": 1, "NU": 1}},
    (5, 96): {"fwd": {"KS": 3, "pad_waves": 1, "NB": 1}, "bwd": {"KS": 4, "NB": 1, "NU": 1}},
    (17, 160): {"fwd": {"KS": 5, "NB": 1, "grid": (10, 2)}, "bwd": {"KS": 4, "NB": 1, "grid": (10, 2)}},
    (16, 544): {"fwd": {"KS": 1, "ksteps": 17, "groups": 4, "tail": 1}, "bwd": {"KS": 4, "ksteps": 17, "groups": 2, "tail": 1}},
    (5, 1088): {"fwd": {"KS": 2, "ksteps": 17, "groups": 4, "tail": 1}, "bwd": {"KS": 8, "ksteps": 17}},
    (37, 512): {"fwd": {"KS": 16, "ksteps": 1, "groups": 0, "tail": 1}, "bwd": {"KS": 8, "NB": 1}},
    (257, 256): {"fwd": {"NB": 2, "KS": 8, "grid": (16, 9)}, "bwd": {"KS": 4, "NB": 1}},
    (129, 512): {"fwd": {"NB": 2, "KS": 8}, "bwd": {"NB": 2, "NU": 1, "KS": 8}},
    (65, 1024): {"fwd": {"NB": 2, "KS": 8}, "bwd": {"NB": 2, "NU": 1, "KS": 16}},
    (130, 1024): {"fwd": {"NB": 2, "KS": 8}, "bwd": {"NB": 2, "NU": 2, "KS": 16, "groups": 2, "tail": 0}},
}
LSTM_FWD_VARIANTS = ("plain", "first", "peep", "mask", "peep_mask", "mask_first")
LSTM_BWD_VARIANTS = ("plain", "last", "peep", "mask", "peep_mask", "carry")

# (B, H) of the GRU step legs: B % 16 in {1, 15, 0}; K = H (modes 0, 1, 3) and 2H (modes 2, 4)
GRU_STEP_SHAPES = {
    (1, 32): {"K": {"KS": 1, "idle_waves": 3, "tail": 1}, "K2": {"KS": 1, "tail": 2}},
    (15, 96): {"K": {"KS": 1, "idle_waves": 3, "groups": 0, "tail": 3}, "K2": {"KS": 1, "tail": 6}},
    (16, 544): {"K": {"KS": 1, "ksteps": 17, "groups": 2, "tail": 1}, "K2": {"KS": 2, "ksteps": 17}},
    (32, 96): {"K": {"KS": 1}, "K2": {"KS": 1}},
    (17, 1024): {"K": {"KS": 4, "idle_waves": 0, "groups": 1, "tail": 0}, "K2": {"KS": 8, "groups": 1, "tail": 0}},
}
GRU_VARIANTS = ("full", "first", "last")       # first: A = None and hprev = None; last: no recurrent operand, no dout

# persistent launches: (B, H, T)
LSTM_SEQ_SHAPES = {
    (1, 256, 4): {"Bg": 1, "NT": 1, "empty_groups": 7},
    (8, 256, 2): {"Bg": 1, "NT": 1, "empty_groups": 0},
    (9, 256, 4): {"Bg": 2, "NT": 1, "full_groups": 4, "last_rows": 1, "empty_groups": 3},
    (128, 256, 2): {"Bg": 16, "NT": 1, "empty_groups": 0},
    (129, 256, 1): {"Bg": 17, "NT": 2, "last_rows": 10, "empty_groups": 0},
    (256, 256, 2): {"Bg": 32, "NT": 2, "empty_groups": 0},
    (9, 512, 2): {"Bg": 2, "NT": 1},
    (129, 1024, 2): {"Bg": 17, "NT": 2, "last_rows": 10},
}
GRU_SEQ_SHAPES = {
    (1, 256, 4): {"Bg": 1, "empty_groups": 7},
    (8, 256, 2): {"Bg": 1, "empty_groups": 0},
    (9, 256, 4): {"Bg": 2, "full_groups": 4, "last_rows": 1, "empty_groups": 3},
    (128, 256, 1): {"Bg": 16, "empty_groups": 0},
    (9, 1024, 2): {"Bg": 2},
}
# partial sums of one pre-activation in the persistent kernels (the KS of the chain bound): the LSTM forward keeps 4
# accumulator chains per wave (2 with two batch tiles); its backward 2 chains in each of the 4 gate-block waves
SEQ_FWD_KS, SEQ_BWD_KS = 4, 8
# persistent GRU: every GEMM runs 2 accumulator chains per wave; the r/z GEMM splits K over 2 waves (4 partial sums),
# the n GEMM and both backward GEMMs over 4 waves (8); the bound takes the larger count for all of them
GRU_SEQ_KS = 8
# the optional argument each sequence case leaves out (the others pass everything)
LSTM_SEQ_OPT = {(1, 256, 4): "no_c0", (8, 256, 2): "no_hT", (9, 256, 4): "no_dout", (128, 256, 2): "no_dhT_dcT"}
GRU_SEQ_OPT = {(1, 256, 4): "no_h0", (8, 256, 2): "no_dout", (9, 256, 4): "no_dhT"}

CELL_SHAPES = ((3, 32), (5, 96), (2049, 1024))     # 8192 blocks x 256 threads = 2097152 < 2049 x 1024: second trip
DROP_SHAPES = ((5, 3, 12, 32, 0.3), (3, 2, 36, 64, 0.5))
WGRAD_SHAPES = ((3, 9, 256), (2, 37, 96))


def reaches(mirror, want):
    """The entries of ``want`` that the mirror does not give (empty: the case reaches what it is named for)."""
    return {k: (v, mirror.get(k)) for k, v in want.items() if mirror.get(k) != v}


# ================================================================================================ values with bounds
class V:
    """fp64 value with a first-order absolute error bound of its fp32 evaluation."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v.to(F64)
        self.e = torch.zeros_like(self.v) if e is None else e.to(F64)

    @staticmethod
    def lift(x):
        if isinstance(x, V):
            return x
        return V(x if torch.is_tensor(x) else torch.tensor(float(x), dtype=F64))

    def __add__(self, o):
        o = V.lift(o)
        v = self.v + o.v
        return V(v, self.e + o.e + U24 * v.abs())

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.e)

    def __sub__(self, o):
        return self + (-V.lift(o))

    def __rsub__(self, o):
        return V.lift(o) + (-self)

    def __mul__(self, o):
        o = V.lift(o)
        v = self.v * o.v
        return V(v, self.v.abs() * o.e + o.v.abs() * self.e + U24 * v.abs())

    __rmul__ = __mul__

    def out(self):
        """A stored result: the "+ 1" of the (ops + 1) u chain rule."""
        return V(self.v, self.e + U24 * self.v.abs())

    def rows(self, idx):
        return V(self.v[idx], self.e[idx])

    def where(self, cond, other):
        other = V.lift(other)
        return V(torch.where(cond, self.v, other.v), torch.where(cond, self.e, other.e))


def c_sigma(a):
    return 0.25 * (a.abs() + 2.0) + 1.0


def c_tanh(a):
    return 0.5 * (2.0 * a.abs() + 2.0) + 2.0


def sig(a):
    return V(torch.sigmoid(a.v), 0.25 * a.e + c_sigma(a.v) * U24)


def tanh(a):
    return V(torch.tanh(a.v), a.e + c_tanh(a.v) * U24)


def dot(A, W, KS, addends=()):
    """sum_k A[b][k] W[n][k] + addends, accumulated in fp32 in KS chunks: the value and the chain bound. ``A`` None:
    no GEMM (the additions alone round)."""
    adds = [V.lift(x) for x in addends if x is not None]
    v = e = mag = 0.0
    for x in adds:
        v = v + x.v
        e = e + x.e
        mag = mag + x.v.abs()
    n = 0
    if A is not None:
        a64, w64 = A.to(F64), W.to(F64)
        v = v + a64 @ w64.t()
        mag = mag + a64.abs() @ w64.abs().t()
        n = A.shape[1] + KS + 2
    count = n + max(0, len(adds) - 1)
    if not torch.is_tensor(v):
        raise ValueError("dot: neither a GEMM operand nor an addend")
    return V(v, e + count * U24 * mag)


def ratio(got, want):
    """Largest |got - want.v| / want.e over the elements; inf for a difference where the bound is 0 or a non-number."""
    g = got.detach().to("cpu", F64)
    if g.shape != want.v.shape:
        raise ValueError(f"shape {tuple(g.shape)} vs {tuple(want.v.shape)}")
    if g.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(g).all()):
        return math.inf
    d = (g - want.v).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / want.e)
    return float(r.max())


def worst(got, want):
    """Index and figures of the element with the largest ratio (for failure messages)."""
    g = got.detach().to("cpu", F64)
    d = (g - want.v).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / want.e).reshape(-1)
    i = int(r.argmax())
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), g.shape))
    return {"index": idx, "got": float(g.reshape(-1)[i]), "want": float(want.v.reshape(-1)[i]),
            "bound": float(want.e.reshape(-1)[i]), "ratio": float(r[i])}


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def rne_bf16(x32):
    """Round-to-nearest-even bf16 of an fp32 tensor (torch's cast)."""
    assert x32.dtype == F32
    return x32.to(BF)


def bf16_half_ulp(y):
    """Half a bf16 ulp at the non-negative fp64 magnitudes ``y``: 2^(floor(log2 y) - 8), between 2^-9 y and 2^-8 y
    (8 significand bits: the unit round-off of bf16 is 2^-8, reached at the bottom of a binade); 0 at 0."""
    _, ex = torch.frexp(y)
    return torch.where(y > 0, torch.ldexp(torch.ones_like(y), ex - 9), torch.zeros_like(y))


def bf16_next(t, idx):
    """``t`` with element ``idx`` moved one bf16 ulp away from zero."""
    out = t.clone()
    raw = out.view(torch.int16)
    raw[idx] = raw[idx] + 1
    return out


# ================================================================================================ guarded views
def guarded(n, dtype, device, off=0, guard=256):
    """A view of ``n`` elements inside a larger allocation of sentinel bytes, ``off`` elements past a 256-byte
    boundary; returns (view, whole allocation as bytes, leading guard bytes)."""
    esz = torch.empty((), dtype=dtype).element_size()
    lead = guard + off * esz
    full = torch.full((lead + n * esz + guard,), SENTINEL, dtype=torch.uint8, device=device)
    return full[lead:lead + n * esz].view(dtype), full, lead


def canaries_ok(full, lead, nbytes):
    return bool((full[:lead] == SENTINEL).all()) and bool((full[lead + nbytes:] == SENTINEL).all())


# ================================================================================================ LSTM oracles
def _blocks(t, H):
    return t.reshape(t.shape[0], 4, H)


def lstm_fwd(inp, peep_o_from_prev=False):
    """One forward step of csrc/lstm.hip on the operands of ``inp`` (see ``lstm_fwd_inputs``): V's of acts [B, 4H],
    c, h [B, H]. A masked row keeps c, emits h = 0 and zero activations, all exactly."""
    xg, order, KS = inp["xg"], inp["order"], inp["KS"]
    B, H = xg.shape[0], xg.shape[1] // 4
    W, hp = inp.get("W16"), inp.get("h16_prev")
    cp = V(inp["c_prev"]) if inp.get("c_prev") is not None else V(torch.zeros(B, H))
    peep = inp.get("peep")
    x = _blocks(xg.to(F64), H)
    pi, pf, pg, po = order

    def pre(q, extra=None):
        return dot(hp, W[q * H:(q + 1) * H] if hp is not None else None, KS, [x[:, q], extra])

    wi = wf = wo = None
    if peep is not None:
        wi, wf, wo = (V(p.to(F64).unsqueeze(0)) for p in peep)
    ig = sig(pre(pi, wi * cp if peep is not None else None))
    fg = sig(pre(pf, wf * cp if peep is not None else None))
    gg = tanh(pre(pg))
    c = fg * cp + ig * gg
    og = sig(pre(po, (wo * (cp if peep_o_from_prev else c)) if peep is not None else None))
    h = og * tanh(c)
    acts = [None] * 4
    acts[pi], acts[pf], acts[pg], acts[po] = ig, fg, gg, og
    av = V(torch.stack([a.v for a in acts], 1).reshape(B, 4 * H), torch.stack([a.e for a in acts], 1).reshape(B, 4 * H))
    c, h = c.out(), h.out()
    if inp.get("mask") is not None:
        valid = inp["mask"].bool().unsqueeze(1)
        av = av.where(valid, torch.zeros(B, 4 * H, dtype=F64))
        c = c.where(valid, cp)
        h = h.where(valid, torch.zeros(B, H, dtype=F64))
    return {"acts": av, "c": c, "h": h}


def lstm_bwd(inp):
    """One backward step of csrc/lstm.hip: V's of dg [B, 4H], dc (the updated in-place buffer) and, with a carry
    buffer, carry. ``dc`` may come in as a V (a persistent launch carries it in registers). A masked row emits
    dg = 0, keeps dc and hands cin + dg_{t+1} . U on through the carry."""
    acts, order, KS = inp["acts"], inp["order"], inp["KS"]
    B, H = acts.shape[0], acts.shape[1] // 4
    a = _blocks(acts.to(F64), H)
    pi, pf, pg, po = order
    ig, fg, gg, og = (V(a[:, q]) for q in (pi, pf, pg, po))
    c = V(inp["c_t"])
    cp = V(inp["c_prev"]) if inp.get("c_prev") is not None else V(torch.zeros(B, H))
    dcn = V.lift(inp["dc"])
    cin = inp.get("carry")
    peep = inp.get("peep")
    A, W = inp.get("dg16_next"), inp.get("WT16")
    dh = dot(A, W if A is not None else None, KS, [inp.get("dout"), inp.get("dh_ext"), cin]) \
        if (A is not None or any(inp.get(k) is not None for k in ("dout", "dh_ext", "carry"))) \
        else V(torch.zeros(B, H))
    tc = tanh(c)
    dog = dh * tc * og * (1.0 - og)
    dcv = dh * og * (1.0 - tc * tc) + dcn
    if peep is not None:
        wi, wf, wo = (V(p.to(F64).unsqueeze(0)) for p in peep)
        dcv = dcv + dog * wo
    di = dcv * gg * ig * (1.0 - ig)
    df = dcv * cp * fg * (1.0 - fg)
    dgg = dcv * ig * (1.0 - gg * gg)
    dcp = dcv * fg
    if peep is not None:
        dcp = dcp + di * wi + df * wf
    dg = [None] * 4
    dg[pi], dg[pf], dg[pg], dg[po] = di.out(), df.out(), dgg.out(), dog.out()
    dgv = V(torch.stack([g.v for g in dg], 1).reshape(B, 4 * H), torch.stack([g.e for g in dg], 1).reshape(B, 4 * H))
    dcp = dcp.out()
    res = {}
    carry = V(torch.zeros(B, H)) if cin is not None else None
    if inp.get("mask") is not None:
        valid = inp["mask"].bool().unsqueeze(1)
        dgv = dgv.where(valid, torch.zeros(B, 4 * H, dtype=F64))
        dcp = dcp.where(valid, dcn)
        moved = dot(A, W if A is not None else None, KS, [cin]) if A is not None else V(cin)
        carry = carry.where(valid, moved)
    res["dg"], res["dc"] = dgv, dcp
    if carry is not None:
        res["carry"] = carry
    return res


# ================================================================================================ GRU oracles
def gru_fwd_rz(W, A, xg, KS):
    """FWD_RZ: s = sigma(h16_{t-1} . U_rz^T + xg[:, :2H]); r = s[:, :H], z = s[:, H:]."""
    H = W.shape[0] // 2
    s = sig(dot(A, W if A is not None else None, KS, [xg[:, :2 * H].to(F64)]))
    return {"r": V(s.v[:, :H], s.e[:, :H]), "z": V(s.v[:, H:], s.e[:, H:])}


def gru_fwd_n(W, A, xg, z, hprev, KS):
    """FWD_N on the kernel's own z and (r h)16: n = tanh((r h)16 . U_n^T + xg[:, 2H:]), h = (1 - z) n + z h_{t-1}."""
    H = W.shape[0]
    n = tanh(dot(A, W, KS, [xg[:, 2 * H:3 * H].to(F64)]))
    zv = V(z)
    hp = V(hprev) if hprev is not None else V(torch.zeros_like(z))
    return {"n": n, "h": ((1.0 - zv) * n + zv * hp).out()}


def gru_bwd_h(W, A, dhp, dout, z, n, hprev, KS):
    """BWD_H: dh = drz16_{t+1} . U_rz + dhp + dout; dn, dz and the z-path dhp' = dh z. W is [H, 2H]."""
    zv, nv = V(z), V(n)
    hp = V(hprev) if hprev is not None else V(torch.zeros_like(z))
    dh = dot(A, W if A is not None else None, KS, [V.lift(dhp), dout])
    dn = dh * (1.0 - zv) * (1.0 - nv * nv)
    dz = dh * (hp - nv) * zv * (1.0 - zv)
    return {"dn": dn.out(), "dz": dz.out(), "dhp": (dh * zv).out()}


def gru_bwd_r(W, A, dhp, r, hprev, KS):
    """BWD_R: d(r h) = dn16 . U_n; dr = d(rh) h r (1 - r); dhp' = dhp + d(rh) r. W is [H, H] (U_n transposed)."""
    rv = V(r)
    hp = V(hprev) if hprev is not None else V(torch.zeros_like(r))
    v = dot(A, W, KS, [])
    return {"dr": (v * hp * rv * (1.0 - rv)).out(), "dhp": (V.lift(dhp) + v * rv).out()}


def gru_bwd_h0(W, A, dhp, KS):
    return {"dh0": dot(A, W, KS, [V.lift(dhp)])}


# ================================================================================================ inputs
def spike_cols(b, K):
    k1 = (37 * b + 5) % K
    return k1, (k1 + K // 2) % K


def edge_rows(B):
    """Rows at tile and group edges (first, last of the first tile, first of the second, last) and row 1."""
    return sorted({0, 1, 15, 16, B - 1} & set(range(B)))


def masked_rows(B):
    """The first and the last row of a tile and row 2; the other rows (the first of the second tile too) stay valid."""
    return sorted({0, 2, 15} & set(range(B)))


def spiked_operands(B, K, N, g, scale):
    """bf16 state [B, K] (Gaussian x 0.25, an 8 at both spike columns of every row) and weights [N, K] (Gaussian x
    ``scale``; in the spike columns of the edge rows, +1 / -1 in alternating output rows)."""
    A = torch.randn(B, K, generator=g) * 0.25
    W = torch.randn(N, K, generator=g) * scale
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    for b in edge_rows(B):
        k1, k2 = spike_cols(b, K)
        W[:, k1] = sign
        W[:, k2] = -sign
    for b in range(B):
        k1, k2 = spike_cols(b, K)
        A[b, k1] = 8.0
        A[b, k2] = 8.0
    return A.to(BF), W.to(BF)


def _target_preact(B, N, g):
    """Pre-activations to aim for: Gaussian, every 7th column x 3 so that |a| reaches about 8 (the saturated end)."""
    a = torch.randn(B, N, generator=g)
    a[:, ::7] *= 3.0
    return a


def lstm_fwd_inputs(B, H, variant, seed=0):
    g = gen(1000 + seed + 7 * B + H)
    order = IFGO if variant in ("peep", "mask") else PLAIN
    h16, W16 = spiked_operands(B, H, 4 * H, g, 1.0 / math.sqrt(H))
    first = variant in ("first", "mask_first")
    pre = torch.zeros(B, 4 * H, dtype=F64) if first else h16.to(F64) @ W16.to(F64).t()
    xg = (_target_preact(B, 4 * H, g).to(F64) - pre).to(F32)
    inp = {"W16": W16, "h16_prev": None if first else h16, "xg": xg, "order": order,
           "c_prev": None if variant == "first" else torch.randn(B, H, generator=g),
           "KS": lstm_fwd_tile(H, B)["KS"], "variant": variant, "B": B, "H": H}
    if variant in ("peep", "peep_mask"):
        inp["peep"] = tuple(torch.randn(H, generator=g) * 0.5 for _ in range(3))
    if variant in ("mask", "peep_mask", "mask_first"):
        m = torch.ones(B, dtype=torch.uint8)
        m[masked_rows(B)] = 0
        inp["mask"] = m
        inp["h_state"] = torch.randn(B, H, generator=g)
    return inp


def lstm_general(inp):
    """Whether the launch takes the general instantiation (anything optional, or a layout other than nn.LSTM's)."""
    return inp.get("peep") is not None or inp.get("mask") is not None or inp.get("h_state") is not None \
        or inp.get("carry") is not None or tuple(inp["order"]) != PLAIN


def lstm_bwd_inputs(B, H, variant, seed=0):
    g = gen(2000 + seed + 7 * B + H)
    order = IFGO if variant in ("peep", "mask") else PLAIN
    dg16, WT16 = spiked_operands(B, 4 * H, H, g, 1.0 / math.sqrt(4 * H))
    last = variant == "last"
    rec = torch.zeros(B, H, dtype=F64) if last else dg16.to(F64) @ WT16.to(F64).t()
    acts = torch.rand(B, 4 * H, generator=g) * 0.96 + 0.02
    gpos = order[2]
    acts[:, gpos * H:(gpos + 1) * H] = acts[:, gpos * H:(gpos + 1) * H] * 2.0 - 1.0
    c_t = torch.randn(B, H, generator=g)
    c_t[:, ::7] *= 3.0
    # dout cancels the spikes of the recurrent term, so dh is a Gaussian of unit size
    dout = (torch.randn(B, H, generator=g).to(F64) - rec).to(F32)
    inp = {"WT16": WT16, "dg16_next": None if last else dg16, "dout": dout,
           "dh_ext": None if last else torch.randn(B, H, generator=g), "acts": acts,
           "c_prev": torch.randn(B, H, generator=g), "c_t": c_t, "dc": torch.randn(B, H, generator=g),
           "order": order, "KS": lstm_bwd_tile(H, B)["KS"], "variant": variant, "B": B, "H": H}
    if variant in ("peep", "peep_mask"):
        inp["peep"] = tuple(torch.randn(H, generator=g) * 0.5 for _ in range(3))
    if variant in ("mask", "peep_mask", "carry"):
        inp["carry"] = torch.randn(B, H, generator=g)          # non-zero on valid and on masked rows
    if variant in ("mask", "peep_mask"):
        m = torch.ones(B, dtype=torch.uint8)
        m[masked_rows(B)] = 0
        inp["mask"] = m
    return inp


ROW_KEYS = ("h16_prev", "xg", "c_prev", "mask", "h_state", "dg16_next", "dout", "dh_ext", "acts", "c_t", "dc", "carry",
            "h16", "rh16", "drz16", "dn16", "hprev", "z", "n", "r", "dhp")


def take_rows(inp, rows):
    """The case restricted to batch rows ``rows`` (a row's outputs depend on its own row of every operand only)."""
    out = dict(inp)
    for k in ROW_KEYS:
        if torch.is_tensor(inp.get(k)):
            out[k] = inp[k][rows]
        elif isinstance(inp.get(k), V):
            out[k] = inp[k].rows(rows)
    return out


def gru_inputs(B, H, variant, seed=0):
    """Operands of the five gru_step modes at one (B, H): U_rz [2H, H], U_n [H, H], their transposes for the backward
    GEMMs, spiked bf16 state operands and fp32 cell state; xg / dout cancel the spikes."""
    g = gen(3000 + seed + 7 * B + H)
    first, last = variant == "first", variant == "last"
    h16, Wrz = spiked_operands(B, H, 2 * H, g, 1.0 / math.sqrt(H))
    rh16, Wn = spiked_operands(B, H, H, g, 1.0 / math.sqrt(H))
    drz16, WrzT = spiked_operands(B, 2 * H, H, g, 1.0 / math.sqrt(2 * H))
    dn16, WnT = spiked_operands(B, H, H, g, 1.0 / math.sqrt(H))
    xg = _target_preact(B, 3 * H, g).to(F64)
    if not first:
        xg[:, :2 * H] -= h16.to(F64) @ Wrz.to(F64).t()
    xg[:, 2 * H:] -= rh16.to(F64) @ Wn.to(F64).t()
    hprev = None if first else torch.randn(B, H, generator=g)
    dout = torch.randn(B, H, generator=g).to(F64)
    if not last:
        dout -= drz16.to(F64) @ WrzT.to(F64).t()
    return {"B": B, "H": H, "variant": variant, "Wrz": Wrz, "Wn": Wn, "WrzT": WrzT, "WnT": WnT,
            "h16": None if first else h16, "rh16": rh16, "drz16": None if last else drz16, "dn16": dn16,
            "xg": xg.to(F32), "hprev": hprev, "dout": None if last else dout.to(F32),
            "z": torch.rand(B, H, generator=g) * 0.96 + 0.02, "r": torch.rand(B, H, generator=g) * 0.96 + 0.02,
            "n": torch.rand(B, H, generator=g) * 1.92 - 0.96, "dhp": torch.randn(B, H, generator=g),
            "KS": gru_tile(H)["KS"], "KS2": gru_tile(2 * H)["KS"]}


def seq_spike_units(b, H):
    """(j, u0, u1): the unit whose top-step output gradient is made large in edge row b, and the units that receive
    its gate gradients through a weight of 1 (backward spikes of the sequence cases)."""
    j = (spike_cols(b, H)[0] + 11) % H
    return j, (j + 7) % H, (j + 13) % H


def lstm_seq_inputs(B, H, T, seed=0):
    """A whole sequence for the persistent LSTM: spiked h0 / W16 (step 0 is held to the same sensitivity as the step
    legs), xg of step 0 cancelling the spikes, Gaussian c0, dout, dhT, dcT; the optional arguments that
    LSTM_SEQ_OPT drops for this case are None."""
    g = gen(4000 + seed + 7 * B + H + T)
    h16, W16 = spiked_operands(B, H, 4 * H, g, 1.0 / math.sqrt(H))
    xg = torch.randn(B, T, 4 * H, generator=g)
    xg[:, :, ::7] *= 3.0
    dout = torch.randn(B, T, H, generator=g)
    dhT = torch.randn(B, H, generator=g)
    W16 = W16.clone()
    for b in edge_rows(B):
        # backward spike: a large gradient of the top step's output (through dout and through dhT, so it is there
        # when either is absent) makes a large dg16[T - 1] in unit j; a weight of 1 from its o-gate row to one unit
        # makes one large product in that unit's recurrent gradient
        j = spike_cols(b, H)[0]
        dout[b, T - 1, j] = 256.0
        dhT[b, j] = 256.0
        W16[3 * H + j, (j + 7) % H] = 1.0
    xg[:, 0] = (xg[:, 0].to(F64) - h16.to(F64) @ W16.to(F64).t()).to(F32)
    opt = LSTM_SEQ_OPT.get((B, H, T), "")
    return {"B": B, "H": H, "T": T, "opt": opt, "W16": W16, "h0_16": h16, "xg": xg,
            "c0": None if opt == "no_c0" else torch.randn(B, H, generator=g),
            "dout": None if opt == "no_dout" else dout, "dhT": None if opt == "no_dhT_dcT" else dhT,
            "dcT": None if opt == "no_dhT_dcT" else torch.randn(B, H, generator=g)}


def gru_seq_inputs(B, H, T, seed=0):
    """A whole sequence for the persistent GRU, spiked so that every GEMM of every step holds a product that is large
    against its chain bound:
    * forward: h0 has an 8 at the two spike columns of every row, U_rz and U_n have +-1 in the spike columns of the
      edge rows; xg gives r and z a pre-activation of 6 at those units at every step, so z ~ 1 keeps the 8 in h_t and
      r ~ 1 carries it into (r h)16; xg of step 0 cancels the spikes' sum in the other units (later steps see the
      difference of the two nearly equal spikes, which is small);
    * backward: the top step's output gradient (dout and dhT) is 256 in unit j of the edge rows, which makes large
      dz, dn there at every step below (dh z is carried down); U_rz[H + j][u0] = 1 and U_n[j][u1] = 1 turn them
      into one large product of BWD_H / BWD_H0 and of BWD_R.
    h0 = None (GRU_SEQ_OPT) leaves the forward without state spikes; the +-1 weights remain."""
    g = gen(5000 + seed + 7 * B + H + T)
    opt = GRU_SEQ_OPT.get((B, H, T), "")
    h16, Wrz = spiked_operands(B, H, 2 * H, g, 1.0 / math.sqrt(H))
    _, Wn = spiked_operands(B, H, H, g, 1.0 / math.sqrt(H))
    if opt == "no_h0":
        h16 = torch.zeros(B, H, dtype=BF)
    xg = torch.randn(B, T, 3 * H, generator=g)
    xg[:, :, ::7] *= 3.0
    dout, dhT = torch.randn(B, T, H, generator=g), torch.randn(B, H, generator=g)
    for b in range(B):
        for k in spike_cols(b, H):
            xg[b, :, k] = 6.0
            xg[b, :, H + k] = 6.0
    for b in edge_rows(B):
        j, u0, u1 = seq_spike_units(b, H)
        dout[b, T - 1, j] = 256.0
        dhT[b, j] = 256.0
        Wrz[H + j, u0] = 1.0
        Wn[j, u1] = 1.0
    pre = h16.to(F64) @ Wrz.to(F64).t()
    xg[:, 0, :2 * H] = (xg[:, 0, :2 * H].to(F64) - pre).to(F32)
    # h0 in fp32 is the bf16 operand itself: the kernel's fp32 h_{-1} and its GEMM operand then agree exactly
    h0 = h16.to(F32)
    r = torch.sigmoid(xg[:, 0, :H].to(F64) + pre[:, :H]).to(F32)
    xg[:, 0, 2 * H:] = (xg[:, 0, 2 * H:].to(F64) - (r * h0).to(BF).to(F64) @ Wn.to(F64).t()).to(F32)
    return {"B": B, "H": H, "T": T, "opt": opt, "Wrz": Wrz, "Wn": Wn, "h0_16": h16,
            "h0": None if opt == "no_h0" else h0, "xg": xg, "dout": None if opt == "no_dout" else dout,
            "dhT": None if opt == "no_dhT" else dhT}


def cell_inputs(B, H, seed=0):
    """The flat cell: gate pre-activations [B, 4H] in nn.LSTM's (i, g, f, o) order and the backward's operands."""
    g = gen(6000 + seed + 7 * B + H)
    gates = torch.randn(B, 4 * H, generator=g)
    gates[:, ::7] *= 3.0
    acts = torch.rand(B, 4 * H, generator=g) * 0.96 + 0.02
    acts[:, H:2 * H] = acts[:, H:2 * H] * 2.0 - 1.0
    c_t = torch.randn(B, H, generator=g)
    c_t[:, ::7] *= 3.0
    return {"B": B, "H": H, "gates": gates, "c_prev": torch.randn(B, H, generator=g), "acts": acts, "c_t": c_t,
            "dh": torch.randn(B, H, generator=g), "dc": torch.randn(B, H, generator=g)}


def cell_fwd(ci, with_c_prev=True):
    return lstm_fwd({"xg": ci["gates"], "order": PLAIN, "KS": 0, "c_prev": ci["c_prev"] if with_c_prev else None})


def cell_bwd(ci, with_c_prev=True, with_dh=True, with_dc=True):
    B, H = ci["B"], ci["H"]
    return lstm_bwd({"acts": ci["acts"], "order": PLAIN, "KS": 0, "c_t": ci["c_t"],
                     "c_prev": ci["c_prev"] if with_c_prev else None,
                     "dc": ci["dc"] if with_dc else torch.zeros(B, H), "dout": ci["dh"] if with_dh else None})


# ================================================================================================ dropout replication
def _philox_np(seed, ctr):
    """Philox-4x32-10 (csrc/lstm_drop.hip philox4) over a numpy array of 64-bit counters -> 4 uint32 arrays."""
    import numpy as np

    M = np.uint64(0xFFFFFFFF)
    ctr = ctr.astype(np.uint64)
    c0, c1 = ctr & M, ctr >> np.uint64(32)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M, p0 & M, n0 & M, n2 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def _keep_mask(seed, ids, p):
    import numpy as np

    r = _philox_np(seed, ids >> 2)
    sel = np.choose((ids & 3).astype(np.int64), r)
    return ((sel >> np.uint64(8)).astype(np.float64) / 16777216.0) >= p


def drop_keep(seed, off, B, T, K, p):
    """Keep mask [4, T, B, K] of lstm_drop_rep: element id ((g T + t) B + b) K + k + off, one Philox draw per 4 ids.
    The kernel compares in fp32: p is rounded to fp32 first (the 24-bit uniform is exact in both)."""
    import numpy as np

    g_, t_, b_, k_ = np.meshgrid(np.arange(4), np.arange(T), np.arange(B), np.arange(K), indexing="ij")
    ids = (((g_ * T + t_) * B + b_) * K + k_ + off).astype(np.int64)
    p32 = float(np.float32(p))
    return torch.as_tensor(_keep_mask(seed, ids, p32))


def drop_rep_oracle(x, keep, mul, Kp, ones):
    """y [4, T*B, Kp] bf16: RNE_bf16(fp32(x mul)) where kept, +0 where dropped, 1 in the ones column, +0 padding.
    x is [B, T, K] fp32 or bf16."""
    B, T, K = x.shape
    prod = (x.to(F32) * torch.tensor(mul, dtype=F32)).permute(1, 0, 2).unsqueeze(0).expand(4, T, B, K)
    y = torch.zeros(4, T, B, Kp, dtype=F32)
    y[..., :K] = torch.where(keep, prod, torch.zeros((), dtype=F32))
    if ones:
        y[..., K] = 1.0
    return y.reshape(4, T * B, Kp).to(BF)


def drop_rep_bwd_oracle(dy, keep, mul, add):
    """dx [B, T, K] = add + sum_g dy[g] keep mul as a V: 4 products, 4 additions -> (4 + 2) u sum|terms|."""
    G, TB, K = dy.shape
    T, B = keep.shape[1], keep.shape[2]
    terms = dy.to(F64).reshape(4, T, B, K) * keep.to(F64) * float(torch.tensor(mul, dtype=F32))
    v, mag = terms.sum(0), terms.abs().sum(0)
    if add is not None:
        a = add.to(F64).permute(1, 0, 2)
        v, mag = v + a, mag + a.abs()
    return V(v.permute(1, 0, 2), (4 + 2) * U24 * mag.permute(1, 0, 2))


# ================================================================================================ weight gradient
def wgrad_oracle(dg16, h16):
    """dU [G, H] = sum over the T*B rows of dg16[row]^T h16[row] as a V under (T B + 4) u sum|terms|."""
    T, B, G = dg16.shape
    a, b = dg16.reshape(T * B, G).to(F64), h16.reshape(T * B, -1).to(F64)
    return V(a.t() @ b, (T * B + 4) * U24 * (a.abs().t() @ b.abs()))


# ================================================================================================ modes and sequences
def gru_mode(gi, mode):
    """The oracle of gru_step mode 0..4 on the operands of ``gru_inputs``."""
    if mode == 0:
        return gru_fwd_rz(gi["Wrz"], gi["h16"], gi["xg"], gi["KS"])
    if mode == 1:
        return gru_fwd_n(gi["Wn"], gi["rh16"], gi["xg"], gi["z"], gi["hprev"], gi["KS"])
    if mode == 2:
        return gru_bwd_h(gi["WrzT"], gi["drz16"], gi["dhp"], gi["dout"], gi["z"], gi["n"], gi["hprev"], gi["KS2"])
    if mode == 3:
        return gru_bwd_r(gi["WnT"], gi["dn16"], gi["dhp"], gi["r"], gi["hprev"], gi["KS"])
    return gru_bwd_h0(gi["WrzT"], gi["drz16"], gi["dhp"], gi["KS2"])


GRU_MODE_OPERAND = {0: ("h16", "Wrz"), 1: ("rh16", "Wn"), 2: ("drz16", "WrzT"), 3: ("dn16", "WnT"), 4: ("drz16", "WrzT")}


def lstm_seq_fwd_step(si, saved, t, xg=None):
    """Oracle inputs of step t of a persistent LSTM forward from the tensors the launch saved (``saved``: h16
    [T + 1, B, H], cs [T, B, H]); ``xg`` overrides the projection input (bf16 I/O: its fp32 value)."""
    xg = si["xg"] if xg is None else xg
    return {"W16": si["W16"], "h16_prev": saved["h16"][t], "xg": xg[:, t].to(F32), "order": PLAIN, "KS": SEQ_FWD_KS,
            "c_prev": (si.get("c0") if t == 0 else saved["cs"][t - 1])}


def lstm_seq_bwd_step(si, saved, t, dc, dout=None, dhT=None):
    """Oracle inputs of step t of the backward sweep: dg16[t + 1] as the kernel handed it on, dc carried as a V."""
    T = si["T"]
    return {"WT16": si["W16"].t(), "dg16_next": saved["dg16"][t + 1] if t < T - 1 else None,
            "dout": dout[:, t].to(F32) if dout is not None else None, "dh_ext": dhT if t == T - 1 else None,
            "acts": saved["acts"][t], "c_prev": (si.get("c0") if t == 0 else saved["cs"][t - 1]), "c_t": saved["cs"][t],
            "dc": dc, "order": PLAIN, "KS": SEQ_BWD_KS}


def emulate_lstm_seq(si):
    """The persistent LSTM on the host: every step is the fp64 oracle, its results rounded to the kernel's storage
    formats (what a correct kernel could have saved). For the sensitivity checks of the sequence cases."""
    B, H, T = si["B"], si["H"], si["T"]
    saved = {"h16": torch.zeros(T + 1, B, H, dtype=BF), "cs": torch.zeros(T, B, H), "acts": torch.zeros(T, B, 4 * H),
             "dg16": torch.zeros(T, B, 4 * H, dtype=BF)}
    saved["h16"][0] = si["h0_16"]
    for t in range(T):
        o = lstm_fwd(lstm_seq_fwd_step(si, saved, t))
        saved["h16"][t + 1] = o["h"].v.to(F32).to(BF)
        saved["cs"][t] = o["c"].v.to(F32)
        saved["acts"][t] = o["acts"].v.to(F32)
    dc = V(si["dcT"] if si["dcT"] is not None else torch.zeros(B, H))
    saved["bwd_inputs"] = [None] * T
    for t in range(T - 1, -1, -1):
        saved["bwd_inputs"][t] = lstm_seq_bwd_step(si, saved, t, dc, si["dout"], si["dhT"])
        o = lstm_bwd(saved["bwd_inputs"][t])
        saved["dg16"][t] = o["dg"].v.to(F32).to(BF)
        dc = o["dc"]
    return saved


def gru_seq_fwd_step(si, saved, t):
    """(operands of FWD_RZ, operands of FWD_N) of step t of a persistent GRU forward from what the launch saved:
    h16 [T + 1, B, H], rh16 [T, B, H], gates [3, T, B, H], out [B, T, H]."""
    hprev = si.get("h0") if t == 0 else saved["out"][:, t - 1]
    return {"Wrz": si["Wrz"], "Wn": si["Wn"], "h16": saved["h16"][t], "rh16": saved["rh16"][t], "xg": si["xg"][:, t],
            "z": saved["gates"][1, t], "hprev": hprev, "KS": GRU_SEQ_KS}


def gru_seq_bwd_step(si, saved, t, dhp, dout=None):
    T = si["T"]
    hprev = si.get("h0") if t == 0 else saved["out"][:, t - 1]
    return {"WrzT": si["Wrz"].t(), "WnT": si["Wn"].t(), "drz16": saved["drz16"][t + 1] if t < T - 1 else None,
            "dn16": saved["dn16"][t], "dhp": dhp, "dout": dout[:, t] if dout is not None else None,
            "r": saved["gates"][0, t], "z": saved["gates"][1, t], "n": saved["gates"][2, t], "hprev": hprev,
            "KS": GRU_SEQ_KS, "KS2": GRU_SEQ_KS}


def emulate_gru_seq(si):
    B, H, T = si["B"], si["H"], si["T"]
    saved = {"h16": torch.zeros(T + 1, B, H, dtype=BF), "rh16": torch.zeros(T, B, H, dtype=BF),
             "gates": torch.zeros(3, T, B, H), "out": torch.zeros(B, T, H), "dn16": torch.zeros(T, B, H, dtype=BF),
             "drz16": torch.zeros(T, B, 2 * H, dtype=BF)}
    saved["h16"][0] = si["h0_16"]
    for t in range(T):
        gi = gru_seq_fwd_step(si, saved, t)
        rz = gru_mode(gi, 0)
        saved["gates"][0, t], saved["gates"][1, t] = rz["r"].v.to(F32), rz["z"].v.to(F32)
        hp = gi["hprev"] if gi["hprev"] is not None else torch.zeros(B, H)
        saved["rh16"][t] = (saved["gates"][0, t] * hp).to(BF)
        gi = gru_seq_fwd_step(si, saved, t)
        o = gru_mode(gi, 1)
        saved["gates"][2, t] = o["n"].v.to(F32)
        saved["out"][:, t] = o["h"].v.to(F32)
        saved["h16"][t + 1] = saved["out"][:, t].to(BF)
    dhp = V(si["dhT"] if si["dhT"] is not None else torch.zeros(B, H))
    # the operands of every backward GEMM as (mode, step, oracle inputs), for the sensitivity checks
    saved["bwd_inputs"] = []
    for t in range(T - 1, -1, -1):
        gi = gru_seq_bwd_step(si, saved, t, dhp, si["dout"])
        saved["bwd_inputs"].append((2, t, gi))
        o = gru_mode(gi, 2)
        saved["dn16"][t] = o["dn"].v.to(F32).to(BF)
        saved["drz16"][t, :, H:] = o["dz"].v.to(F32).to(BF)
        gi = gru_seq_bwd_step(si, saved, t, o["dhp"], si["dout"])
        saved["bwd_inputs"].append((3, t, gi))
        o = gru_mode(gi, 3)
        saved["drz16"][t, :, :H] = o["dr"].v.to(F32).to(BF)
        dhp = o["dhp"]
    saved["bwd_inputs"].append((4, -1, {"WrzT": si["Wrz"].t(), "drz16": saved["drz16"][0], "dhp": dhp,
                                        "KS2": GRU_SEQ_KS}))
    return saved
