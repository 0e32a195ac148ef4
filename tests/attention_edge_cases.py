"""Cases and fp64 references for the fused attention kernels (csrc/attention.hip), shared by
tests/test_attention_edges_gpu.py (kernel vs reference) and tests/test_attention_edges_cpu.py (the reference's own
sanity and the sensitivity the GPU tests rely on). Everything here runs on the CPU.

Reference: softmax(q k^T + bias [+ causal]) o dropmask @ v in fp64 on the bf16-rounded q, k, v, gradients by autograd.

* The bias is added the way the kernel and the fp32 math path add it, (s.float() + bias.float()).double(): a -1e9
  entry absorbs the score (fp32 spacing at 1e9 is 64), which matters only for rows whose every key carries -1e9.
* The causal mask is TOP-LEFT aligned for every (Lq, Lk): key kj is visible to query qi iff kj <= qi, i.e.
  triu(-1e9, diagonal=1) over [Lq, Lk]. That is the kernel's rule (attn_fwd_kernel: ``a.causal && kj > qi``);
  a bottom-right alignment for Lq != Lk would be a deliberate change of both.

Yardstick: the same computation with the kernel's documented bf16 roundings (P o mask before P V and dV, dO, dS
before dK and dQ); E_t = max |rounded - exact| per output tensor, measured from the reference alone.
"""
import functools
from dataclasses import dataclass

import torch

NEG = -1e9
SEED = 0x1234_5678_9ABC_DEF0          # nonzero high 32 bits: both halves of the kernel's seed are exercised
TENSORS = ("o", "dq", "dk", "dv")


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H: int
    Lq: int
    Lk: int
    D: int
    bias: str = "none"
    causal: bool = False
    p: float = 0.0

    def __str__(self):
        return self.name


def _c(tag, B, H, Lq, Lk, D, **kw):
    p = f"-p{kw['p']}" if kw.get("p") else ""
    return Case(f"{tag}-{B}x{H}x{Lq}x{Lk}x{D}{p}", B, H, Lq, Lk, D, **kw)


# 64-row / 64-key tiles, 16-row waves, 32-wide MFMA k-step: one below, at and one above each boundary
TILE_PAIRS = [(1, 1), (15, 16), (17, 65), (65, 17), (64, 64), (130, 129), (63, 129), (1, 63), (64, 15), (130, 64),
              (65, 1), (63, 63)]
CONTIGUOUS_BIASES = ["b11k", "1h11", "11qk", "bhq1", "1hqk", "bhqk", "qk2d", "hqk3d"]
STRIDED_BIASES = ["expand", "transposed", "slice"]

CASES = (
    [_c("tile", 1, 2, lq, lk, 64) for lq, lk in TILE_PAIRS]
    + [_c("dim", 1, 2, lq, lk, d) for d in (32, 64, 96, 128) for lq, lk in ((65, 65), (17, 129))]
    + [_c("causal", 1, 2, lq, lk, d, causal=True)
       for lq, lk, d in ((1, 1, 64), (64, 64, 64), (65, 65, 128), (130, 130, 64), (17, 129, 64), (130, 65, 32))]
    + [_c(b, 2, 3, 65, 129, 32, bias=b) for b in CONTIGUOUS_BIASES + STRIDED_BIASES]
    + [_c(b, 3, 2, 65, 129, 64, bias=b) for b in ("pad_tile0", "inf_tail", "inf_batch", "neg_batch")]
    # dropout: p exact in fp32. The binding rounds p through float, so for a p like 0.1 the host helper
    # (dropout_mask, double p) and the device (float p) disagree on about 7 / 2^32 of the elements; such values
    # are deliberately not tested.
    + [_c("drop_causal", 1, 2, 130, 130, 64, causal=True, p=0.5),
       _c("drop_pad", 3, 2, 65, 129, 64, bias="pad_tile0", p=0.125),
       _c("drop", 2, 3, 130, 129, 64, p=0.125),
       _c("drop", 2, 3, 130, 129, 64, p=0.5)]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _gen(case, salt):
    g = torch.Generator()
    g.manual_seed(CASES.index(case) * 16 + salt)
    return g


@functools.lru_cache(maxsize=None)
def inputs(case):
    """q (pre-scaled by D^-1/2), k, v: fp32 tensors holding bf16-representable values; dO: fp32. [B, H, L, D]."""
    g = _gen(case, 0)
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.D
    q = (torch.randn(B, H, Lq, D, generator=g) * D ** -0.5).bfloat16().float()
    k = torch.randn(B, H, Lk, D, generator=g).bfloat16().float()
    v = torch.randn(B, H, Lk, D, generator=g).bfloat16().float()
    do = torch.randn(B, H, Lq, D, generator=g)
    return q, k, v, do


def make_bias(case, device="cpu"):
    """The case's bias on ``device``. Strided layouts are views of a buffer that is moved first, so the view (and
    not a compacted copy of it) is what reaches the kernel."""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    g = _gen(case, 1)
    kind = case.bias

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(device)

    if kind == "none":
        return None
    if kind == "b11k":
        return rn(B, 1, 1, Lk)
    if kind == "1h11":
        return rn(1, H, 1, 1)
    if kind == "11qk":
        return rn(1, 1, Lq, Lk)
    if kind == "bhq1":
        return rn(B, H, Lq, 1)
    if kind == "1hqk":
        return rn(1, H, Lq, Lk)
    if kind == "bhqk":
        return rn(B, H, Lq, Lk)
    if kind == "qk2d":
        return rn(Lq, Lk)
    if kind == "hqk3d":
        return rn(H, Lq, Lk)
    if kind == "expand":                       # strides (Lk, 0, 0, 1)
        return rn(B, 1, 1, Lk).expand(B, H, Lq, Lk)
    if kind == "transposed":                   # last stride Lq, not 1
        return rn(B, H, Lk, Lq).transpose(2, 3)
    if kind == "slice":                        # storage offset != 0, row stride Lk + 7
        return rn(B, H, Lq + 3, Lk + 7)[:, :, 2:2 + Lq, 5:5 + Lk]
    m = torch.zeros(B, 1, 1, Lk)
    if kind == "pad_tile0":                    # the whole first 64-key tile masked, for batches 0 and 2 only
        m[0, ..., :64] = NEG
        m[2, ..., :64] = NEG
    elif kind == "inf_tail":                   # -inf over the last third of the keys
        m[..., Lk - Lk // 3:] = float("-inf")
    elif kind == "inf_batch":                  # batch 1: every key -inf (fully masked rows)
        m[1] = float("-inf")
    elif kind == "neg_batch":                  # batch 1: every key -1e9 (near-uniform average)
        m[1] = NEG
    else:
        raise ValueError(kind)
    return m.to(device)


def dead_batch(case):
    """Index of the batch whose every key is -inf (the reference is undefined there), or None."""
    return 1 if case.bias == "inf_batch" else None


def live_batches(case):
    return [b for b in range(case.B) if b != dead_batch(case)]


def drop_mask(case):
    if case.p == 0:
        return None
    from bigdl_amd.ops.flash_attention import dropout_mask

    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    return dropout_mask(SEED, B * H, Lq, Lk, case.p).view(B, H, Lq, Lk)


def _r16(t):
    return t.float().bfloat16().double()


def compute(case, perturb=None):
    """Exact fp64 result and its bf16-rounded twin. ``perturb`` (CPU sensitivity checks only): "drop_last_key"
    hides key Lk - 1 from every query, "hide_diagonal" turns the causal rule into kj < qi.
    Returns (exact, rounded): dicts over o, dq, dk, dv (+ lse in exact), restricted to the live batches."""
    q32, k32, v32, do32 = inputs(case)
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    q, k, v = (t.double().requires_grad_(True) for t in (q32, k32, v32))
    do = do32.double()
    bias = make_bias(case)
    s = q @ k.transpose(-1, -2)
    if bias is not None:
        b4 = bias.float()
        while b4.dim() < 4:
            b4 = b4.unsqueeze(0)
        if dead_batch(case) is not None:
            b4 = b4.clone()
            b4[dead_batch(case)] = 0.0
        x = (s.detach().float() + b4).double()           # fp32 add: what the kernel and the math path compute
        s = x + (s - s.detach())                         # value x, gradient of s
    if case.causal:
        s = s + torch.triu(torch.full((Lq, Lk), NEG, dtype=torch.float64), diagonal=1)   # top-left aligned
    if perturb == "drop_last_key":
        s = s + torch.cat([torch.zeros(Lq, Lk - 1, dtype=torch.float64),
                           torch.full((Lq, 1), NEG, dtype=torch.float64)], 1)
    elif perturb == "hide_diagonal":
        d = torch.zeros(Lq, Lk, dtype=torch.float64)
        i = torch.arange(min(Lq, Lk))
        d[i, i] = NEG
        s = s + d
    elif perturb is not None:
        raise ValueError(perturb)
    M = drop_mask(case)
    M = M.double() if M is not None else None
    P = torch.softmax(s, -1)
    Pd = P * M if M is not None else P
    o = Pd @ v
    o.backward(do)
    live = live_batches(case)
    exact = {"o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad,
             "lse": torch.logsumexp(s.detach(), -1)}
    with torch.no_grad():
        q, k, v, P, Pd = q.detach(), k.detach(), v.detach(), P.detach(), Pd.detach()
        Pd16 = _r16(Pd)
        o_r = Pd16 @ v
        do16 = _r16(do)
        dv_r = Pd16.transpose(-1, -2) @ do16
        dP = do16 @ v.transpose(-1, -2)
        if M is not None:
            dP = dP * M
        delta = (do * o_r).sum(-1, keepdim=True)
        dS16 = _r16(P * (dP - delta))
        rounded = {"o": o_r, "dq": dS16 @ k, "dk": dS16.transpose(-1, -2) @ q, "dv": dv_r}
    exact = {n: t[live] for n, t in exact.items()}
    rounded = {n: t[live] for n, t in rounded.items()}
    return exact, rounded


@functools.lru_cache(maxsize=None)
def reference(case):
    """(exact, E): exact fp64 tensors over the live batches and the yardstick E_t = max |rounded - exact|."""
    exact, rounded = compute(case)
    E = {t: (rounded[t] - exact[t]).abs().max().item() for t in TENSORS}
    return exact, E
