"""LSTMPeephole and maskZero LSTM sequences on the GPU: the general instantiation of the fused step kernels of
csrc/lstm.hip behind _LSTMPeepSeq against an fp64 loop of the same formulas, the modules that route to them against
the CPU engine, and the general instantiation against the plain one."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

ORDER_LSTM, ORDER_PEEP = (0, 2, 1, 3), (0, 1, 2, 3)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _det_mask(B, T):
    """Row b is valid on t in [lo_b, hi_b): row 0 full, row 1 fully masked, row 2 a trailing pad, row 3 a leading pad,
    row 4 both; the rows after them cycle through the pads with other lengths."""
    m = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        k, n = b % 5, 1 + (b // 5) % (T - 1)           # n in 1 .. T-1
        lo, hi = [(0, T), (0, 0), (0, n), (n, T), (1, T - 1)][k]
        m[b, lo:hi] = True
    assert m[0].all() and not m[1].any() and m[2, 0] and not m[2, -1] and not m[3, 0] and m[3, -1]
    return m


def _loop_ref(xg, h0, c0, U, pI, pF, pO, mask, order):
    pi, pf, pg, po = order
    H = h0.shape[1]
    blk = lambda g, k: g[:, k * H:(k + 1) * H]  # noqa: E731
    h, c, outs = h0, c0, []
    for t in range(xg.shape[1]):
        g = xg[:, t] + h @ U.t()
        a_i, a_f, a_g, a_o = blk(g, pi), blk(g, pf), blk(g, pg), blk(g, po)
        if pI is not None:
            a_i, a_f = a_i + pI * c, a_f + pF * c
        c2 = torch.sigmoid(a_f) * c + torch.sigmoid(a_i) * torch.tanh(a_g)
        if pO is not None:
            a_o = a_o + pO * c2
        h2 = torch.sigmoid(a_o) * torch.tanh(c2)
        o = h2
        if mask is not None:
            m = mask[:, t].unsqueeze(1)
            h2, c2 = torch.where(m, h2, h), torch.where(m, c2, c)
            o = o * m.to(o.dtype)
        outs.append(o)
        h, c = h2, c2
    return torch.stack(outs, 1), h, c


def _inputs(B, T, H, peep):
    torch.manual_seed(0)
    xg = torch.randn(B, T, 4 * H) * 0.5
    h0, c0 = torch.randn(B, H) * 0.5, torch.randn(B, H) * 0.5
    U = (torch.randn(4 * H, H) / H ** 0.5).to(torch.bfloat16).float()
    ps = [torch.randn(H) * 0.5 for _ in range(3)] if peep else [None, None, None]
    go, gh, gc = torch.randn(B, T, H), torch.randn(B, H), torch.randn(B, H)
    return (xg, h0, c0, U), ps, (go, gh, gc)


def _run_gpu(ts, ps, gs, mask, order):
    from bigdl_amd.nn.recurrent import _LSTMPeepSeq

    dev = [t.cuda().requires_grad_(True) for t in ts]
    pd = [p.cuda().requires_grad_(True) if p is not None else None for p in ps]
    out, hT, cT = _LSTMPeepSeq.apply(*dev, *pd, mask.cuda() if mask is not None else None, order)
    torch.autograd.backward([out, hT, cT], [g.cuda() for g in gs])
    torch.cuda.synchronize()
    return [out.detach(), hT.detach(), cT.detach()], [t.grad for t in dev] + [p.grad for p in pd if p is not None]


_REF = {}


def _reference(B, T, H, peep, masked, order):
    """fp64 loop + autograd, computed once per case and shared."""
    key = (B, T, H, peep, masked, order)
    if key not in _REF:
        ts, ps, gs = _inputs(B, T, H, peep)
        mask = _det_mask(B, T) if masked else None
        leaves = [t.double().requires_grad_(True) for t in ts]
        pl = [p.double().requires_grad_(True) if p is not None else None for p in ps]
        outs = _loop_ref(*leaves, *pl, mask, order)
        torch.autograd.backward(list(outs), [g.double() for g in gs])
        _REF[key] = ([o.detach() for o in outs], [t.grad for t in leaves] + [p.grad for p in pl if p is not None])
    return _REF[key]


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("peep", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("B,T,H", [(5, 3, 32), (37, 6, 64), (5, 3, 192), (72, 4, 1024), (150, 3, 512)])
def test_peephole_steps_match_fp64_reference(B, T, H, peep, masked):
    """(a) forward / backward step kernels and the peephole-gradient reduction vs the fp64 loop; gate order (i, f, g, o)
    with peepholes, nn.LSTM's (i, g, f, o) without."""
    order = ORDER_PEEP if peep else ORDER_LSTM
    ts, ps, gs = _inputs(B, T, H, peep)
    mask = _det_mask(B, T) if masked else None
    (ro, rh, rc), rgrads = _reference(B, T, H, peep, masked, order)
    (out, hT, cT), grads = _run_gpu(ts, ps, gs, mask, order)
    errs = {"out": _rel(out, ro), "hT": _rel(hT, rh), "cT": _rel(cT, rc)}
    names = ["dxg", "dh0", "dc0", "dU", "dpI", "dpF", "dpO"]
    gerrs = {n: _rel(g, r) for n, g, r in zip(names, grads, rgrads)}
    print(f"B={B} T={T} H={H} peep={peep} mask={masked}: {errs} {gerrs}")
    assert len(grads) == (7 if peep else 4) and all(g is not None for g in grads)
    for n, e in errs.items():
        assert e < 1e-2, (n, e)
    for n, e in gerrs.items():
        assert e < 2e-2, (n, e)
    if masked:
        mk = mask.cuda()
        assert (out[~mk] == 0).all()
        dead = ~mk.any(1)
        assert dead.any()
        assert torch.equal(hT[dead], ts[1].cuda()[dead]) and torch.equal(cT[dead], ts[2].cuda()[dead])
        assert (grads[0][dead] == 0).all()
        assert (grads[0][~mk] == 0).all()


def test_peephole_backward_is_deterministic():
    """(b) no float atomics anywhere: two runs give identical bits."""
    B, T, H = 37, 6, 64
    ts, ps, gs = _inputs(B, T, H, True)
    mask = _det_mask(B, T)
    o1, g1 = _run_gpu(ts, ps, gs, mask, ORDER_PEEP)
    o2, g2 = _run_gpu(ts, ps, gs, mask, ORDER_PEEP)
    for a, b in zip(o1 + g1, o2 + g2):
        assert torch.equal(a, b)


def _varied_lengths(x, full_at=0):
    """Zero x[b, len_b:] with len_b spread over [1, T], len_b = T at row `full_at`."""
    B, T = x.shape[:2]
    for b in range(B):
        n = T if b == full_at else 1 + (b * 7) % (T - 1)
        x[b, n:] = 0
    return x


def _configs():
    from bigdl_amd import nn

    return {
        "peephole": (lambda: nn.Recurrent().add(nn.LSTMPeephole(64, 128)), 64, False),
        "peephole_mask": (lambda: nn.Recurrent(maskZero=True).add(nn.LSTMPeephole(64, 128)), 64, True),
        "lstm_mask": (lambda: nn.Recurrent(maskZero=True).add(nn.LSTM(64, 128)), 64, True),
        # BiRecurrent has no maskZero argument: unmasked
        "bi_peephole": (lambda: nn.BiRecurrent().add(nn.LSTMPeephole(32, 64)), 32, False),
    }


def _module_case(build, I, masked, seed=0):
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(seed)
    torch.manual_seed(seed)
    cpu = build()
    gpu = copy.deepcopy(cpu).to("cuda")
    x = torch.randn(8, 20, I).to(torch.bfloat16).float()
    if masked:
        x = _varied_lengths(x)
    return cpu, gpu, x


def _compare_with_cpu(cpu, gpu, x):
    yc = cpu.forward(x)
    yg = gpu.forward(x.cuda())
    assert _rel(yg, yc) < 2e-2, _rel(yg, yc)
    gy = torch.randn_like(yc)
    gc = cpu.backward(x, gy)
    gg = gpu.backward(x.cuda(), gy.cuda())
    assert _rel(gg, gc) < 3e-2, _rel(gg, gc)
    wc = torch.cat([g.reshape(-1) for g in cpu.parameters()[1]])
    wg = torch.cat([g.float().cpu().reshape(-1) for g in gpu.parameters()[1]])
    assert _rel(wg, wc) < 3e-2, _rel(wg, wc)
    return yc, yg


def _cmuls(m):
    from bigdl_amd import nn

    out, todo = [], [m]
    while todo:
        k = todo.pop(0)
        if type(k) is nn.CMul:
            out.append(k)
        todo.extend(k.modules_list())
    return out


@pytest.mark.parametrize("name", ["peephole", "peephole_mask", "lstm_mask", "bi_peephole"])
def test_peephole_and_masked_modules_match_cpu_engine(name, monkeypatch):
    """(c) the routed modules against the fp32 CPU engine (Cell.sequence), bf16-rounded input; the GPU side goes
    through _LSTMPeepSeq (once per direction), the CPU side never."""
    from bigdl_amd.nn import recurrent as rc

    calls, orig = [], rc._LSTMPeepSeq.forward

    def spy(ctx, xg, *a):
        calls.append(xg.is_cuda)
        return orig(ctx, xg, *a)

    monkeypatch.setattr(rc._LSTMPeepSeq, "forward", staticmethod(spy))
    build, I, masked = _configs()[name]
    cpu, gpu, x = _module_case(build, I, masked)
    yc, yg = _compare_with_cpu(cpu, gpu, x)
    assert calls == [True] * (2 if name == "bi_peephole" else 1)
    if masked:
        dead = (x.abs().amax(-1) == 0)
        assert dead.any() and (yg.cpu()[dead] == 0).all()
    pc, pg = _cmuls(cpu), _cmuls(gpu)
    assert len(pc) == len(pg) == (0 if name == "lstm_mask" else 6 if name == "bi_peephole" else 3)
    for a, b in zip(pg, pc):
        assert float(b.gradWeight.abs().max()) > 0
        assert _rel(a.gradWeight, b.gradWeight) < 3e-2, _rel(a.gradWeight, b.gradWeight)


@pytest.mark.parametrize("name", ["peephole", "peephole_mask", "lstm_mask"])
def test_native_path_runs_without_the_python_loop(name, monkeypatch):
    """(d) with Cell.sequence disabled the three Recurrent configurations still run forward and backward on the GPU;
    with BIGDL_LSTM_PEEP_FUSED switched off they need the Python loop again."""
    from bigdl_amd.nn import recurrent as rc

    def no_loop(self, x2, hid, mask=None):
        raise RuntimeError("Cell.sequence called")

    monkeypatch.setattr(rc.Cell, "sequence", no_loop)
    build, I, masked = _configs()[name]
    _, gpu, x = _module_case(build, I, masked)
    y = gpu.forward(x.cuda())
    g = gpu.backward(x.cuda(), torch.ones_like(y))
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and torch.isfinite(g).all()
    rc._PEEP_FUSED[0] = False
    try:
        with pytest.raises(RuntimeError, match="Cell.sequence called"):
            gpu.forward(x.cuda())
    finally:
        rc._PEEP_FUSED[0] = True


@pytest.mark.parametrize("name", ["peephole_h48", "lstm_relu_mask", "gru_mask"])
def test_fallbacks_stay_on_the_python_loop(name, monkeypatch):
    """(e) shapes and cells outside the fused path keep Cell.sequence on the GPU and match the CPU engine."""
    from bigdl_amd import nn
    from bigdl_amd.nn import recurrent as rc

    build, masked = {
        "peephole_h48": (lambda: nn.Recurrent().add(nn.LSTMPeephole(64, 48)), False),
        "lstm_relu_mask": (lambda: nn.Recurrent(maskZero=True).add(nn.LSTM(64, 128, activation=nn.ReLU())), True),
        "gru_mask": (lambda: nn.Recurrent(maskZero=True).add(nn.GRU(64, 128)), True),
    }[name]

    def boom(*a, **k):
        raise AssertionError("_LSTMPeepSeq used outside its shapes")

    monkeypatch.setattr(rc._LSTMPeepSeq, "forward", staticmethod(boom))
    cpu, gpu, x = _module_case(build, 64, masked)
    _compare_with_cpu(cpu, gpu, x)


def test_peephole_sequence_replays_from_a_hip_graph():
    """(f) forward + backward captured in a HIP graph (no host synchronisation inside): two replays equal the eager
    run bit for bit."""
    from bigdl_amd.nn.recurrent import _LSTMPeepSeq

    B, T, H = 37, 6, 64
    ts, ps, gs = _inputs(B, T, H, True)
    mask = _det_mask(B, T).cuda()
    eager_o, eager_g = _run_gpu(ts, ps, gs, mask, ORDER_PEEP)
    leaves = [t.cuda().requires_grad_(True) for t in list(ts) + list(ps)]
    gd = [g.cuda() for g in gs]

    def step():
        outs = _LSTMPeepSeq.apply(*leaves, mask, ORDER_PEEP)
        grads = torch.autograd.grad(list(outs), leaves, gd)
        return [o.detach() for o in outs] + list(grads)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = step()
    for _ in range(2):
        for r in res:
            r.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(res, eager_o + eager_g):
            assert torch.equal(a, b)


def plain_and_general_step(C, B, H, seed=0):
    """One forward and one backward step on the same finite random operands, once as the plain call (no optional
    argument: the specialised instantiation) and once with zero peepholes, nn.LSTM's gate order, h_state and carry
    given and no mask (the general instantiation doing the plain math). Returns the two lists of results
    (c_out, h_out, h16_out, acts, dg_out, dg16_out, dc)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    W16 = (rnd(4 * H, H) / H ** 0.5).to(torch.bfloat16)
    WT16 = W16.t().contiguous()
    h16_prev, dg16_next = (rnd(B, H) * 0.5).to(torch.bfloat16), (rnd(B, 4 * H) * 0.1).to(torch.bfloat16)
    xg, c_prev, dout, dh_ext, dc_in = rnd(B, 4 * H) * 0.5, rnd(B, H) * 0.5, rnd(B, H), rnd(B, H), rnd(B, H)
    zero = torch.zeros(H, device="cuda")
    f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    runs = []
    for general in (False, True):
        opt = dict(pI=zero, pF=zero, pO=zero, order=ORDER_LSTM) if general else {}
        fk = dict(h_state=torch.zeros(B, H, device="cuda"), **opt) if general else {}
        bk = dict(carry=torch.zeros(B, H, device="cuda"), **opt) if general else {}
        c_out, h_out, acts = f32(B, H), f32(B, H), f32(B, 4 * H)
        h16_out = torch.empty(B, H, device="cuda", dtype=torch.bfloat16)
        C.lstm_fwd_step(W16, h16_prev, xg, c_prev, c_out, h_out, h16_out, acts, **fk)
        dc, dg_out = dc_in.clone(), f32(B, 4 * H)
        dg16_out = torch.empty(B, 4 * H, device="cuda", dtype=torch.bfloat16)
        C.lstm_bwd_step(WT16, dg16_next, dout, dh_ext, acts, c_prev, c_out, dc, dg_out, dg16_out, **bk)
        runs.append([c_out, h_out, h16_out, acts, dg_out, dg16_out, dc])
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("B,T,H", [(5, 2, 32), (37, 2, 64), (72, 2, 1024), (150, 2, 512), (130, 2, 1024)])
def test_plain_and_general_instantiations_agree(B, T, H):
    """(g) the two instantiations of the step kernels are one body: with zero peepholes, nn.LSTM's gate order and no
    mask the general one gives the plain one's values exactly (torch.equal: a zero peephole term may turn -0 into +0
    and nothing else). One step out of the middle of a T = 2 sequence: h16_prev and dg16_next are both there, and so
    are dout and dh_ext. Shapes: KS < 4 with padded waves; a batch tail; NB = 2 in both directions (H = 1024, K split
    16 in the backward); NB = 2 with 8 K chunks in both directions; NB = 2 with NU = 2 in the backward, which needs
    4H / 16 >= 256 and more than 256 two-tile workgroups, so H = 1024 and B > 128."""
    from bigdl_amd.ops import native

    plain, general = plain_and_general_step(native.get(), B, H)
    names = ["c_out", "h_out", "h16_out", "acts", "dg_out", "dg16_out", "dc"]
    for n, a, b in zip(names, plain, general):
        assert torch.isfinite(a.float()).all(), n
        assert torch.equal(a, b), (n, (a.float() - b.float()).abs().max().item())
