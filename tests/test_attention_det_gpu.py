"""The ordered dQ kernel of csrc/attention.hip (attn_dq_kernel: deterministic mode, or BIGDL_ATTN_DQ=ordered /
ops.flash_attention.set_dq_mode("ordered")) against the fp64 reference of tests/attention_edge_cases.py.

dQ is held to the yardstick of tests/test_attention_edges_gpu.py, |got - exact| <= 3 E_dq + 1e-6 max|exact| with
E_dq = max |bf16-rounded reference - exact| measured from the reference alone. The ordered kernel keeps the atomic
route's rounding points (P fp32, dS rounded to bf16 before the dQ MFMA) and only changes the order of the fp32 sum
over key blocks, so the same factor 3 applies; it is not to be raised. o, dK and dV come from the same code in both
modes and are compared bit for bit. Every test restores the modes it found.
"""
import functools

import pytest
import torch

from tests.attention_edge_cases import (CASES, NEG, SEED, TENSORS, dead_batch, inputs, live_batches, make_bias,
                                        reference)

pytestmark = pytest.mark.gpu

IDS = [c.name for c in CASES]


class _modes:
    """Deterministic mode and the explicit dQ mode for the body, both restored on exit."""

    def __init__(self, det, dq=None):
        self.det, self.dq = det, dq

    def __enter__(self):
        from bigdl_amd.ops import flash_attention as fa
        from bigdl_amd.ops import native

        self.saved = native.deterministic()
        native.get()
        native.set_deterministic(self.det)
        fa.set_dq_mode(self.dq)
        return self

    def __exit__(self, *exc):
        from bigdl_amd.ops import flash_attention as fa
        from bigdl_amd.ops import native

        fa.set_dq_mode(None)
        native.set_deterministic(self.saved)


@functools.lru_cache(maxsize=None)
def run_case(case, det):
    """Forward + backward of the case through ops.flash_attention with deterministic mode ``det``; CPU tensors."""
    from bigdl_amd.ops.flash_attention import dq_route, flash_attention

    q, k, v, do = inputs(case)
    bias = make_bias(case, "cuda")
    with _modes(det):
        assert dq_route() == ("ordered" if det else "atomic")
        dev = [t.cuda().requires_grad_(True) for t in (q, k, v)]
        o = flash_attention(dev[0], dev[1], dev[2], bias, case.causal, case.p, SEED)
        o.backward(do.cuda())
        torch.cuda.synchronize()
    out = {"o": o.detach(), "dq": dev[0].grad, "dk": dev[1].grad, "dv": dev[2].grad}
    return {n: t.cpu() for n, t in out.items()}


def _r16(t):
    return t.float().bfloat16().double()


def _dq_reference(q32, k32, v32, do32, bias, causal):
    """Exact fp64 dQ and the yardstick E_dq, computed the way attention_edge_cases.compute does (no dropout)."""
    Lq, Lk = q32.shape[-2], k32.shape[-2]
    q, k, v = (t.double().requires_grad_(True) for t in (q32, k32, v32))
    do = do32.double()
    s = q @ k.transpose(-1, -2)
    if bias is not None:
        x = (s.detach().float() + bias.float()).double()
        s = x + (s - s.detach())
    if causal:
        s = s + torch.triu(torch.full((Lq, Lk), NEG, dtype=torch.float64), diagonal=1)
    P = torch.softmax(s, -1)
    (P @ v).backward(do)
    with torch.no_grad():
        P, kd, vd = P.detach(), k.detach(), v.detach()
        P16 = _r16(P)
        o_r = P16 @ vd
        do16 = _r16(do)
        dP = do16 @ vd.transpose(-1, -2)
        delta = (do * o_r).sum(-1, keepdim=True)
        rounded = _r16(P * (dP - delta)) @ kd
    exact = q.grad
    return exact, (rounded - exact).abs().max().item()


@pytest.mark.parametrize("kind", ["causal", "padding"])
def test_dq_is_written_not_accumulated(kind):
    """The bare binding with dq pre-filled with NaN: the ordered kernel stores every element (the atomic route adds
    into the buffer and leaves NaN). B*H = 2, D = 64, Lq = Lk = 130: three key blocks, the last with 2 live keys."""
    from bigdl_amd.ops import native

    B, H, L, D = 1, 2, 130, 64
    g = torch.Generator().manual_seed(130)
    q = (torch.randn(B, H, L, D, generator=g) * D ** -0.5).bfloat16().float()
    k = torch.randn(B, H, L, D, generator=g).bfloat16().float()
    v = torch.randn(B, H, L, D, generator=g).bfloat16().float()
    do = torch.randn(B, H, L, D, generator=g)
    causal = kind == "causal"
    bias = None
    if not causal:
        bias = torch.zeros(B, 1, 1, L)
        bias[..., 100:] = NEG                            # the whole last key block and a part of the second
    exact, E = _dq_reference(q, k, v, do, bias, causal)
    C = native.get()
    q16, k16, v16 = (t.cuda().reshape(B * H, L, D).bfloat16().contiguous() for t in (q, k, v))
    b = bias.cuda() if bias is not None else None
    o = torch.empty(B * H, L, D, device="cuda")
    lse = torch.empty(B * H, L, device="cuda")
    mlog = torch.empty(2, B * H, L, device="cuda")
    dq = torch.full((B * H, L, D), float("nan"), device="cuda")
    dk, dv = torch.empty_like(o), torch.empty_like(o)
    delta = torch.empty(B * H, L, device="cuda")
    with _modes(True):
        C.attn_fwd(q16, k16, v16, b, H, causal, o, lse, mlog, 0.0, 0)
        C.attn_bwd(q16, k16, v16, b, H, causal, o, mlog, do.cuda().reshape(B * H, L, D).contiguous(), dq, dk, dv,
                   delta, 0.0, 0)
        torch.cuda.synchronize()
    got = dq.cpu().view(B, H, L, D)
    assert torch.isfinite(got).all()
    err = (got.double() - exact).abs()
    bound = 3 * E + 1e-6 * exact.abs().max().item()
    print(f"DET_RATIO attention nan-{kind} dq err={err.max().item():.3e} E={E:.3e} ratio={err.max().item() / E:.3f}")
    assert (err <= bound).all(), (err.max().item(), bound)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_edge_case_ordered(case):
    exact, E = reference(case)
    got = run_case(case, True)
    live = live_batches(case)
    for t in TENSORS:
        assert not torch.isnan(got[t]).any(), t
    err = (got["dq"][live].double() - exact["dq"]).abs()
    bound = 3 * E["dq"] + 1e-6 * exact["dq"].abs().max().item()
    worst = err.max().item()
    print(f"DET_RATIO attention {case.name} dq err={worst:.3e} E={E['dq']:.3e} "
          f"ratio={worst / E['dq'] if E['dq'] > 0 else float(worst > 0):.3f}")
    assert (err <= bound).all(), (worst, bound)          # 3 E_dq: see the module docstring; not to be raised
    dead = dead_batch(case)
    if dead is not None:
        for t in TENSORS:
            assert (got[t][dead] == 0).all(), t
    if case.causal and case.Lq < case.Lk:
        assert (got["dk"][:, :, case.Lq:] == 0).all() and (got["dv"][:, :, case.Lq:] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_only_the_dq_route_changes(case):
    det, default = run_case(case, True), run_case(case, False)
    for t in ("o", "dk", "dv"):
        assert torch.equal(det[t], default[t]), t


def _backward_twice(BH, Lq, Lk, D, p, det, dq_mode=None):
    """Two backward calls of the bare binding from the same inputs; returns the two dQ (device tensors)."""
    from bigdl_amd.ops import native

    C = native.get()
    g = torch.Generator().manual_seed(D * 1000 + int(p * 100))
    q16 = (torch.randn(BH, Lq, D, generator=g) * D ** -0.5).bfloat16().cuda()
    k16 = torch.randn(BH, Lk, D, generator=g).bfloat16().cuda()
    v16 = torch.randn(BH, Lk, D, generator=g).bfloat16().cuda()
    do = torch.randn(BH, Lq, D, generator=g).cuda()
    bias = torch.randn(1, 1, Lq, Lk, generator=g).cuda()
    o = torch.empty(BH, Lq, D, device="cuda")
    lse = torch.empty(BH, Lq, device="cuda")
    mlog = torch.empty(2, BH, Lq, device="cuda")
    out = []
    with _modes(det, dq_mode):
        C.attn_fwd(q16, k16, v16, bias, 1, False, o, lse, mlog, p, SEED)
        for _ in range(2):
            ordered = bool(C.attn_dq_ordered())
            dq = (torch.empty if ordered else torch.zeros)(BH, Lq, D, device="cuda")
            dk, dv = torch.empty_like(k16, dtype=torch.float32), torch.empty_like(v16, dtype=torch.float32)
            delta = torch.empty(BH, Lq, device="cuda")
            C.attn_bwd(q16, k16, v16, bias, 1, False, o, mlog, do, dq, dk, dv, delta, p, SEED)
            out.append(dq)
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D,p", [(32, 0.0), (64, 0.0), (96, 0.0), (128, 0.0), (64, 0.3)])
def test_bitwise_repeat(D, p):
    a, b = _backward_twice(3, 100, 200, D, p, det=True)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_switch():
    """set_dq_mode("ordered") / BIGDL_ATTN_DQ=ordered with deterministic mode off give the bits of deterministic
    mode on; "atomic" or nothing set stays on the atomic route (asked of the route query, not guessed from bits)."""
    from bigdl_amd.ops import flash_attention as fa

    det = _backward_twice(3, 100, 200, 64, 0.0, det=True)[0]
    explicit = _backward_twice(3, 100, 200, 64, 0.0, det=False, dq_mode="ordered")[0]
    assert torch.equal(det, explicit)
    with _modes(False, "atomic"):
        assert fa.dq_route() == "atomic"
    with _modes(False, None):
        assert fa.dq_route() == "atomic"
    with _modes(True, "atomic"):
        assert fa.dq_route() == "ordered"               # deterministic mode always takes the ordered kernel
    with _modes(False, "ordered"):
        assert fa.dq_route() == "ordered"


def test_switch_reads_the_environment(monkeypatch):
    from bigdl_amd.ops import flash_attention as fa
    from bigdl_amd.ops import native

    saved = native.deterministic()
    try:
        native.get()
        native.set_deterministic(False)
        monkeypatch.setenv("BIGDL_ATTN_DQ", "ordered")
        fa.set_dq_mode(None)
        assert fa.dq_route() == "ordered"
        monkeypatch.setenv("BIGDL_ATTN_DQ", "atomic")
        fa.set_dq_mode(None)
        assert fa.dq_route() == "atomic"
        monkeypatch.delenv("BIGDL_ATTN_DQ")
        fa.set_dq_mode(None)
        assert fa.dq_route() == "atomic"
    finally:
        monkeypatch.undo()
        fa.set_dq_mode(None)
        native.set_deterministic(saved)
