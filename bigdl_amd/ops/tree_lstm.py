"""Fused BinaryTreeLSTM on the GPU engine: one launch per tree level and direction (csrc/treelstm.hip).

The schedule is built once per forward on the host in C++ (``_C.treelstm_schedule``: an explicit-stack walk from every
root, validation that each reachable node has exactly one parent, nodes grouped by height, one int32 table uploaded in
one copy). State is slot-major and written by the children: a node stores its bf16 h and fp32 c into its parent's slot
``[slot][side * Hp + unit]``, so a composer row's GEMM operand is one contiguous ``2 * Hp`` row and the same buffer is
the dense operand of the weight-gradient GEMM after the backward sweep. ``Hp`` / ``Ip`` are the hidden / input widths
rounded up to 32; weights are packed per forward (bf16, zero-padded, gate rows of a unit adjacent). After the sweep the
weight gradients and the leaves' input gradient are dense GEMMs on the in-tree kernel (ops/gemm.py), the bias
gradients fixed-order column sums of the fp32 gate gradients. Nothing uses atomics: results are bitwise reproducible.

Switch: ``BIGDL_TREELSTM_FUSED`` / Engine property ``bigdl.treelstm.fused`` / ``set_fused``; unset means
``DEFAULT_FUSED``. ``last_route()`` says whether the last BinaryTreeLSTM forward ran "fused" or through the per-level
torch "loop" (CPU tensors, the switch off, or a batch whose trees do not validate).
"""
import os

import torch

from . import gemm, native

BF16 = torch.bfloat16
DEFAULT_FUSED = True    # the GPU engine's default (README "Fused BinaryTreeLSTM"; profiles/treelstm_fused_ab.txt)

_FUSED = [None]
_ROUTE = [None]


def set_fused(v):
    """True / False, "1" / "0", or None for the engine's default."""
    _FUSED[0] = None if v is None or v == "" else str(v).lower() in ("1", "true", "yes")


def fused(is_cuda=True):
    """Whether a caller with GPU tensors (``is_cuda``) takes the fused route."""
    v = _FUSED[0]
    if v is None:
        env = os.environ.get("BIGDL_TREELSTM_FUSED", "")
        v = DEFAULT_FUSED if env == "" else env.lower() in ("1", "true", "yes")
    return bool(v) and bool(is_cuda)


def last_route():
    """"fused" or "loop": the route of the last BinaryTreeLSTM forward (None before the first)."""
    return _ROUTE[0]


def _set_route(route):
    _ROUTE[0] = route


def _up(n, m):
    return (n + m - 1) // m * m


def schedule(trees, L):
    """(table int32 CPU, meta) for a batch of trees [B, N, 3] over inputs of L words, or None when a tree does not
    validate (no root or several, a child index out of range, a node with two parents, a cycle)."""
    if trees.dim() != 3 or trees.shape[2] != 3 or trees.shape[0] < 1 or L < 1:
        return None
    tab, meta = native.get().treelstm_schedule(trees.detach().to("cpu", torch.int64).contiguous(), int(L))
    return (tab, meta) if meta else None


def _pack(w, lead, H, Hp, wide, widep):
    """[lead * H, wide] -> zero-padded [lead, Hp, widep] fp32."""
    p = torch.zeros(lead, Hp, widep, device=w.device)
    p[:, :H, :wide] = w.detach().float().view(lead, H, wide)
    return p


def _unit_major(p):
    """[lead, Hp, ...] -> bf16 [Hp * lead, ...]: the gate rows of a hidden unit adjacent (row = unit * lead + gate)."""
    from . import to_bf16

    return to_bf16(p.transpose(0, 1).reshape(p.shape[0] * p.shape[1], -1))


class _TreeLSTMFused(torch.autograd.Function):
    """BinaryTreeLSTM forward / backward on the level kernels; ``sched`` is ``schedule``'s result."""

    @staticmethod
    def forward(ctx, inputs, leafW, leafB, leftW, leftB, rightW, rightB, sched, N, gateOutput):
        C = native.get()
        tab_cpu, meta = sched
        S, Lc, nlev = meta[0], meta[1], meta[2]
        levels = [tuple(meta[6 + 3 * k:9 + 3 * k]) for k in range(nlev)]
        B, L, I = inputs.shape
        H = leftW.shape[1]
        Hp, Ip = _up(H, 32), _up(I, 32)
        ng, nl = (5, 2) if gateOutput else (4, 1)
        dev = inputs.device
        tab = tab_cpu.pin_memory().to(dev, non_blocking=True)
        Z, Sp, Lp = S, _up(S + 1, 16), _up(Lc, 16)
        # operands: [leftWeight | rightWeight] as one [ng * Hp, 2 * Hp] matrix, the leaf weight [nl * Hp, Ip]
        Wp = torch.cat([_pack(leftW, ng, H, Hp, H, Hp), _pack(rightW, ng, H, Hp, H, Hp)], 2)
        Wlp = _pack(leafW, nl, H, Hp, I, Ip)
        bias = _pack((leftB.detach() + rightB.detach()).view(-1, 1), ng, H, Hp, 1, 1).view(ng, Hp).t().reshape(-1)
        lbias = _pack(leafB.view(-1, 1), nl, H, Hp, 1, 1).view(nl, Hp).t().reshape(-1)
        x = inputs.detach().float().contiguous().view(B * L, I)
        xl16 = torch.zeros(Lp, Ip, dtype=BF16, device=dev)
        lacts = torch.zeros(Lp, nl * Hp, device=dev)
        hch16 = torch.zeros(Sp, 2 * Hp, dtype=BF16, device=dev)
        cch = torch.zeros(Sp, 2 * Hp, device=dev)
        acts = torch.zeros(Sp, (ng + 1) * Hp, device=dev)
        out = torch.zeros(B * N, H, device=dev)
        s, _, e = levels[0]
        C.treelstm_gather_x(x, tab, s, e - s, xl16, Lc)
        C.treelstm_fwd_level(_unit_major(Wlp), xl16, lbias, tab, s, e - s, cch, hch16, out, lacts, Lc, Z, True)
        W16 = _unit_major(Wp)
        for s, _, e in levels[1:]:
            C.treelstm_fwd_level(W16, hch16, bias, tab, s, e - s, cch, hch16, out, acts, Z + 1, Z, False)
        ctx.save_for_backward(tab, Wp, Wlp, xl16, lacts, hch16, cch, acts)
        ctx.geo = (levels, meta[4], meta[5], Lc, Z, B, L, I, H, N, bool(gateOutput), inputs.dtype)
        return out.view(B, N, H)

    @staticmethod
    def backward(ctx, gout):
        from . import to_bf16

        C = native.get()
        tab, Wp, Wlp, xl16, lacts, hch16, cch, acts = ctx.saved_tensors
        levels, off0, items0, Lc, Z, B, L, I, H, N, go, in_dtype = ctx.geo
        ng, Hp = Wp.shape[0], Wp.shape[1]
        nl, Ip = Wlp.shape[0], Wlp.shape[2]
        Sp, Lp, K = hch16.shape[0], xl16.shape[0], ng * Hp
        dev = gout.device
        gout = gout.float().contiguous().view(B * N, H)
        # W_left^T, W_right^T: [side][unit of the child][gate * Hp + unit of the parent]
        WT16 = to_bf16(Wp.view(ng, Hp, 2, Hp).permute(2, 3, 0, 1).reshape(2, Hp, K))
        dg = torch.zeros(Sp, K, device=dev)
        dg16 = torch.zeros(Sp, K, dtype=BF16, device=dev)
        dcp = torch.zeros(Sp, 2 * Hp, device=dev)
        dgl = torch.zeros(Lp, nl * Hp, device=dev)
        dgl16 = torch.zeros(Lp, nl * Hp, dtype=BF16, device=dev)
        for s, sp, e in reversed(levels[1:]):
            C.treelstm_bwd_level(WT16, dg16, gout, tab, s, sp - s, e - s, acts, cch, dcp, dg, dg16, Z + 1, Z, go, False)
        s, sp, e = levels[0]
        C.treelstm_bwd_level(WT16, dg16, gout, tab, s, sp - s, e - s, lacts, cch, dcp, dgl, dgl16, Lc, Z, go, True)
        # dense GEMMs over the slot buffers (their tile padding is zero rows)
        dW = gemm.gemm(dg16, hch16, trans_a=True).view(ng, Hp, 2, Hp)
        db = C.treelstm_colsum(dg).view(ng, Hp)[:, :H].reshape(ng * H)
        dWl = gemm.gemm(dgl16, xl16, trans_a=True).view(nl, Hp, Ip)[:, :H, :I].reshape(nl * H, I)
        dbl = C.treelstm_colsum(dgl).view(nl, Hp)[:, :H].reshape(nl * H)
        dxl = gemm.gemm(dgl16, to_bf16(Wlp.view(nl * Hp, Ip)))
        gin = torch.empty(B * L, I, device=dev)
        C.treelstm_leaf_dx(dxl, tab, off0, items0, gin, Lc)
        return (gin.view(B, L, I).to(in_dtype), dWl, dbl, dW[:, :H, 0, :H].reshape(ng * H, H), db,
                dW[:, :H, 1, :H].reshape(ng * H, H), db.clone(), None, None, None)


def forward(m, inputs, trees):
    """The fused forward of BinaryTreeLSTM ``m``, or None when this call stays on the loop."""
    if not (inputs.is_cuda and inputs.dim() == 3 and fused(True)):
        _set_route("loop")
        return None
    sched = schedule(trees, inputs.shape[1])
    if sched is None:
        _set_route("loop")
        return None
    _set_route("fused")
    return _TreeLSTMFused.apply(inputs, m.leafWeight, m.leafBias, m.leftWeight, m.leftBias, m.rightWeight,
                                m.rightBias, sched, trees.shape[1], m.gateOutput)
