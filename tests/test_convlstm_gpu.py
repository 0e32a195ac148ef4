"""Fused ConvLSTMPeephole on the GPU (csrc/convlstm.hip, nn/recurrent.py _ConvLSTMSeq).

1. forward / backward step through the raw bindings, element by element against the fp64 LSTM step oracles of
   tests/recurrent_cases.py: a ConvLSTM step is an LSTM step whose operand rows are the im2col of h (n = k^2 C, one
   partial sum, order IFGO); dg is stored as bf16 only, so its bound takes the documented half bf16 ulp.
   Spikes: 8 at two opposite corner pixels of every image, +-1 weights on the two corner taps, xg / dout cancelling.
2. the peephole-gradient reduction, exact on small integers and bitwise repeatable.
3. _ConvLSTMSeq against its own torch form on the CPU in fp64; 4. the modules against the CPU engine.
Worst ratios of a run are printed (``convlstm-ratio``); profiles/convlstm_errors.txt records them."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from tests import recurrent_cases as rc

pytestmark = pytest.mark.gpu
BF, F32, F64 = rc.BF, rc.F32, rc.F64

# (B, C, H, W, kC)
CASES = [(1, 16, 1, 1, 3), (2, 16, 3, 5, 3), (3, 48, 7, 9, 3), (1, 32, 17, 33, 5), (2, 64, 6, 6, 1), (1, 144, 4, 4, 3),
         # the kernel's tile constant TM = 128: W + p <= TM + 2p stages one contiguous halo tile (W = 129 is the last
         # such width for 3x3), anything wider one row band per tap row (W = 130 the first)
         (1, 16, 1, 129, 3), (1, 16, 2, 130, 3),
         # the largest kernel: a 3-pixel halo on a wide image, 7 row bands (the largest LDS footprint of a launch)
         (1, 16, 4, 132, 7)]


def _n():
    from bigdl_amd.ops import native

    return native.get()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _check(leg, case, got, want):
    r = rc.ratio(got.reshape(want.v.shape), want)
    print(f"convlstm-ratio {leg} {case} {r:.4f}")
    assert r <= 1, (leg, case, rc.worst(got.reshape(want.v.shape), want))


def _spiked(B, H, W, K, N, k, g):
    """bf16 operand [B, H, W, K] and weight [N, k, k, K] (as the convolution applies it) with the spikes."""
    a = torch.randn(B, H, W, K, generator=g) * 0.25
    w = torch.randn(N, k, k, K, generator=g) / math.sqrt(k * k * K)
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    a[:, 0, 0, 0], a[:, H - 1, W - 1, K - 1] = 8.0, 8.0
    w[:, 0, 0, 0], w[:, k - 1, k - 1, K - 1] = sign, -sign
    return a.to(BF), w.to(BF)


def _im2col(a, w):
    """Rows [B H W, k^2 K] of the operand in fp64 and the weight [N, k^2 K] in F.unfold's (channel, tap) column order."""
    B, H, W, K = a.shape
    k = w.shape[1]
    cols = F.unfold(a.to(F64).permute(0, 3, 1, 2), k, padding=(k - 1) // 2)
    return cols.transpose(1, 2).reshape(B * H * W, K * k * k), w.permute(0, 3, 1, 2).reshape(w.shape[0], -1)


def _guarded(arena, shape, dtype, src=None):
    v, full, lead = rc.guarded(math.prod(shape), dtype, "cuda")
    arena.append((full, lead, v.numel() * v.element_size()))
    v = v.view(shape)
    return v if src is None else v.copy_(src.reshape(shape))


def _peep(C, g, on):
    return tuple(torch.randn(C, generator=g) * 0.5 for _ in range(3)) if on else None


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("peep", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_fwd_step(case, peep, first):
    B, C, H, W, k = case
    g = rc.gen(100 + C + H + W)
    h16, U = _spiked(B, H, W, C, 4 * C, k, g)
    P = B * H * W
    cp = torch.randn(P, C, generator=g)
    if first:
        h16, cp = torch.zeros_like(h16), torch.zeros_like(cp)
    A, Wm = _im2col(h16, U)
    target = torch.randn(P, 4 * C, generator=g)
    target[:, ::7] *= 3.0
    xg = (target.to(F64) - A @ Wm.to(F64).t()).to(F32)
    ps = _peep(C, g, peep)
    inp = {"W16": Wm, "h16_prev": A, "xg": xg, "order": rc.IFGO, "KS": 1, "c_prev": cp}
    if peep:
        inp["peep"] = ps
    arena = []
    c_out, h_out, acts = (_guarded(arena, (B, H, W, n), F32) for n in (C, C, 4 * C))
    h16_out = _guarded(arena, (B, H, W, C), BF)
    dps = [p.cuda() for p in ps] if peep else [None] * 3
    _n().convlstm_fwd_step(U.cuda(), h16.cuda(), xg.view(B, H, W, 4 * C).cuda(), cp.view(B, H, W, C).cuda(), c_out, h_out,
                           h16_out, acts, pI=dps[0], pF=dps[1], pO=dps[2], hard=False)
    torch.cuda.synchronize()
    assert all(rc.canaries_ok(*it) for it in arena)
    o = rc.lstm_fwd(inp)
    name = f"{case}-{'peep' if peep else 'nopeep'}-{'first' if first else 'later'}"
    _check("fwd_acts", name, acts, o["acts"])
    _check("fwd_c", name, c_out, o["c"])
    _check("fwd_h", name, h_out, o["h"])
    assert rc.same_bits(h16_out.cpu(), rc.rne_bf16(h_out.cpu()))


@pytest.mark.parametrize("variant", ["last", "mid", "nodout"])
@pytest.mark.parametrize("peep", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_bwd_step(case, peep, variant):
    B, C, H, W, k = case
    g = rc.gen(200 + C + H + W)
    P = B * H * W
    dgn, wf = _spiked(B, H, W, 4 * C, C, k, g)       # wf: the weight as applied; the kernel takes it tap-flipped
    A, Wm = _im2col(dgn, wf)
    last = variant == "last"
    rec = torch.zeros(P, C, dtype=F64) if last else A @ Wm.to(F64).t()
    acts = torch.rand(P, 4 * C, generator=g) * 0.96 + 0.02
    acts[:, 2 * C:3 * C] = acts[:, 2 * C:3 * C] * 2.0 - 1.0
    c_t = torch.randn(P, C, generator=g)
    c_t[:, ::7] *= 3.0
    dout = None if variant == "nodout" else (torch.randn(P, C, generator=g).to(F64) - rec).to(F32)
    ps = _peep(C, g, peep)
    inp = {"WT16": Wm, "dg16_next": None if last else A, "dout": dout,
           "dh_ext": torch.randn(P, C, generator=g) if last else None, "acts": acts,
           "c_prev": torch.randn(P, C, generator=g), "c_t": c_t, "dc": torch.randn(P, C, generator=g),
           "order": rc.IFGO, "KS": 1}
    if peep:
        inp["peep"] = ps
    arena = []
    dc = _guarded(arena, (B, H, W, C), F32, inp["dc"])
    dg16 = _guarded(arena, (B, H, W, 4 * C), BF)
    dev = {n: (inp[n].view(B, H, W, -1).cuda() if inp[n] is not None else None)
           for n in ("dout", "dh_ext", "acts", "c_prev", "c_t")}
    dps = [p.cuda() for p in ps] if peep else [None] * 3
    _n().convlstm_bwd_step(wf.flip(1, 2).contiguous().cuda(), None if last else dgn.cuda(), dev["dout"], dev["dh_ext"],
                           dev["acts"], dev["c_prev"], dev["c_t"], dc, dg16, pI=dps[0], pF=dps[1], pO=dps[2], hard=False)
    torch.cuda.synchronize()
    assert all(rc.canaries_ok(*it) for it in arena)
    o = rc.lstm_bwd(inp)
    name = f"{case}-{'peep' if peep else 'nopeep'}-{variant}"
    dgb = o["dg"]
    _check("bwd_dg", name, dg16.float(), rc.V(dgb.v, dgb.e + rc.bf16_half_ulp(dgb.v.abs() + dgb.e)))
    _check("bwd_dc", name, dc, o["dc"])


@pytest.mark.parametrize("T,P,C,slices", [(3, 35, 16, 1), (2, 1500, 48, 2)])
def test_peep_wgrad_exact_and_repeatable(T, P, C, slices):
    N = _n()
    assert N.convlstm_peep_wgrad_slices(T * P) == slices
    g = rc.gen(7)
    dg = torch.randint(-3, 4, (T, P, 4 * C), generator=g).double()
    cs = torch.randint(-4, 5, (T, P, C), generator=g).double()
    c0 = torch.randint(-4, 5, (P, C), generator=g).double()
    cprev = torch.cat([c0.unsqueeze(0), cs[:-1]])
    want = torch.stack([(dg[..., :C] * cprev).sum((0, 1)), (dg[..., C:2 * C] * cprev).sum((0, 1)),
                        (dg[..., 3 * C:] * cs).sum((0, 1))])
    outs = []
    for _ in range(2):
        part, out = torch.empty(slices, 3, C, device="cuda"), torch.empty(3, C, device="cuda")
        N.convlstm_peep_wgrad(dg.to(BF).cuda(), cs.float().cuda(), c0.float().cuda(), part, out)
        outs.append(out.cpu())
    assert torch.equal(outs[0].double(), want) and rc.same_bits(outs[0], outs[1])


@pytest.mark.parametrize("peep", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("hard", [False, True], ids=["sigmoid", "hard"])
def test_seq_matches_own_torch_form_fp64(hard, peep):
    from bigdl_amd.nn.recurrent import _ConvLSTMSeq

    B, T, Cin, C, H, W = 2, 3, 4, 16, 5, 7
    g = rc.gen(11)
    shapes = [(B, T, Cin, H, W), (B, C, H, W), (B, C, H, W), (4 * C, Cin, 3, 3), (4 * C,), (4 * C, C, 3, 3)]
    shapes += [(1, C, 1, 1)] * 3 if peep else []
    vals = [(torch.randn(s, generator=g) * (0.2 if len(s) == 4 and s[0] == 4 * C else 1.0)).to(BF) for s in shapes]
    gouts = [torch.randn(s, generator=g) for s in ((B, T, C, H, W), (B, C, H, W), (B, C, H, W))]
    res = []
    for dev, dt in (("cuda", F32), ("cpu", F64)):
        leaves = [v.to(dev, dt).requires_grad_(True) for v in vals]
        outs = _ConvLSTMSeq.apply(*leaves, *([] if peep else [None] * 3), hard)
        res.append(list(outs) + list(torch.autograd.grad(outs, leaves, [t.to(dev, dt) for t in gouts])))
    for k, (a, b) in enumerate(zip(*res)):
        assert a.shape == b.shape and _rel(a, b) < (1e-2 if k < 3 else 2e-2), (k, _rel(a, b))


def _module(name):
    from bigdl_amd import keras, nn

    if name == "keras":
        return keras.Sequential().add(keras.ConvLSTM2D(16, 3, returnSequences=True, inputShape=(3, 4, 6, 6)))
    if name == "3d":
        return nn.Recurrent().add(nn.ConvLSTMPeephole3D(4, 16, 3, 3))
    args = {"k3": (4, 16, 3, 3), "k5": (4, 16, 5, 5), "c8": (4, 8, 3, 3),
            "relu": (4, 16, 3, 3, 1, -1, nn.ReLU())}[name.split("-")[0]]
    return nn.Recurrent(maskZero=name.endswith("-mask")).add(nn.ConvLSTMPeephole(*args))


@pytest.mark.parametrize("name", ["k3", "k5", "keras", "c8", "relu", "k3-mask", "3d"])
def test_modules_match_cpu_engine_and_route(name, monkeypatch):
    """The usable configurations take the fused route (Cell.sequence never sees a GPU tensor), with a non-zero initial
    hidden state for ``k3``; outputSize 8, ReLU, maskZero and the 3-D cell still take the loop. Training and eval mode."""
    from bigdl_amd.nn.recurrent import Cell
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(5)
    cpu = _module(name)
    gpu = copy.deepcopy(cpu).to("cuda")
    loop, on_gpu = Cell.sequence, []

    def spy(self, x2, *a, **kw):
        on_gpu.append(x2.is_cuda)
        return loop(self, x2, *a, **kw)

    monkeypatch.setattr(Cell, "sequence", spy)
    x = torch.randn(*((2, 3, 4, 4, 6, 6) if name == "3d" else (2, 3, 4, 6, 6))).to(BF).float()
    if name == "k3":
        hid = [torch.randn(2, 16, 6, 6).to(BF).float() for _ in range(2)]
        cpu.setHiddenState(hid)
        gpu.setHiddenState([t.cuda() for t in hid])
    yc, yg = cpu.forward(x), gpu.forward(x.cuda())
    assert (True in on_gpu) == (name not in ("k3", "k5", "keras"))
    assert yg.shape == yc.shape and _rel(yg, yc) < 1e-2, _rel(yg, yc)
    gy = torch.randn_like(yc)
    assert _rel(gpu.backward(x.cuda(), gy.cuda()), cpu.backward(x, gy)) < 2e-2
    for a, b in zip(gpu.parameters()[1], cpu.parameters()[1]):
        assert _rel(a, b) < 2e-2, (a.shape, _rel(a, b))
    if name == "k3":
        for k in (1, 2):
            assert _rel(gpu.getHiddenState()[k], cpu.getHiddenState()[k]) < 1e-2
    assert _rel(gpu.evaluate().forward(x.cuda()), cpu.evaluate().forward(x)) < 1e-2


def test_stride2_is_not_usable():
    """Stride 2 cannot run end to end (the loop's strided h projection disagrees in size with the x projection), so
    only the predicate is checked."""
    from bigdl_amd import nn
    from bigdl_amd.nn.recurrent import _ConvLSTMSeq

    x = torch.zeros(1, 1, 4, 6, 6, device="cuda")
    assert _ConvLSTMSeq.usable(x, nn.ConvLSTMPeephole(4, 16, 3, 3))
    assert not _ConvLSTMSeq.usable(x, nn.ConvLSTMPeephole(4, 16, 3, 3, 2))
