"""Fused ConvLSTMPeephole3D on the GPU (csrc/convlstm3d.hip, nn/recurrent.py _ConvLSTM3dSeq).

1. forward / backward step through the raw bindings, element by element against the fp64 LSTM step oracles of
   tests/recurrent_cases.py: a ConvLSTM3D step is an LSTM step whose operand rows are the im2col of the operand over
   k^3 taps (n = k^3 C, one partial sum, order IFGO); dg is stored as bf16 only, so its bound takes the documented
   half bf16 ulp. Spikes: 8 at two opposite corner voxels of every volume, +-1 weights on the two corner taps, xg /
   dout cancelling.
2. _ConvLSTM3dSeq against its own torch form on the CPU in fp64; 3. the module against the CPU engine, switch on / unset.
Worst ratios of a run are printed (``convlstm3d-ratio``); profiles/convlstm3d_errors.txt records them."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from tests import recurrent_cases as rc

pytestmark = pytest.mark.gpu
BF, F32, F64 = rc.BF, rc.F32, rc.F64

# (B, C, D, H, W, kC). The kernel's tile is TM = 64 virtual voxels, a row band TM + 2p of them (p = (k - 1) / 2).
CASES = [(1, 16, 1, 1, 1, 3),       # every tap but the centre in padding
         (2, 16, 2, 3, 5, 3),       # tiles spanning rows, planes and volumes; row and plane bands all collapsed
         (1, 48, 3, 5, 7, 3),       # a 16-channel tail chunk and an inactive wave
         (1, 144, 2, 3, 3, 3),      # a third, partial channel tile
         (2, 64, 3, 4, 4, 1),       # k = 1
         # plane rule: plane stretches of L = 2p (W + p) + TM + 2p rows collapse while (H + p)(W + p) < L. W = 12, k = 3:
         # L = 92; H = 6 gives 91 (the last collapsed), H = 12 gives 169 (disjoint planes, overlapping rows)
         (1, 16, 3, 6, 12, 3), (1, 16, 3, 12, 12, 3),
         # row rule: row bands collapse while W + p <= TM + 2p: W = 65 is the last such width for k = 3, W = 66 the first
         # with disjoint row bands; W = 130 leaves a gap of a whole tile between them
         (1, 16, 1, 1, 65, 3), (1, 16, 1, 1, 66, 3), (1, 16, 2, 2, 130, 3),
         # LDS cap (160 KiB = 2409 staged rows): the largest kernel, k = 7, at its smallest shape, and at the widest image
         # with disjoint planes that still fits (7 x (6 x 45 + 70) = 2380 rows; REFUSED is the first that does not)
         (1, 16, 1, 1, 1, 7), (1, 16, 1, 5, 42, 7)]
REFUSED = (1, 16, 1, 5, 43, 7)     # 7 x (6 x 46 + 70) = 2422 rows


def _n():
    from bigdl_amd.ops import native

    return native.get()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _check(leg, case, got, want):
    r = rc.ratio(got.reshape(want.v.shape), want)
    print(f"convlstm3d-ratio {leg} {case} {r:.4f}")
    assert r <= 1, (leg, case, rc.worst(got.reshape(want.v.shape), want))


def _spiked(vol, K, N, k, g):
    """bf16 operand [B, D, H, W, K] and weight [N, k, k, k, K] (as the convolution applies it) with the spikes."""
    a = torch.randn(*vol, K, generator=g) * 0.25
    w = torch.randn(N, k, k, k, K, generator=g) / math.sqrt(k ** 3 * K)
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    a[:, 0, 0, 0, 0], a[:, -1, -1, -1, -1] = 8.0, 8.0
    w[:, 0, 0, 0, 0], w[:, -1, -1, -1, -1] = sign, -sign
    return a.to(BF), w.to(BF)


def _im2col(a, w):
    """Rows [B D H W, k^3 K] of the operand in fp64, the k^3 shifts of the zero-padded volume stacked in tap order, and
    the weight [N, k^3 K] in the same (tap, channel) column order."""
    B, D, H, W, K = a.shape
    k, p = w.shape[1], (w.shape[1] - 1) // 2
    ap = F.pad(a.to(F64), (0, 0, p, p, p, p, p, p))
    cols = [ap[:, dd:dd + D, dh:dh + H, dw:dw + W] for dd in range(k) for dh in range(k) for dw in range(k)]
    return torch.stack(cols, 4).reshape(B * D * H * W, k ** 3 * K), w.reshape(w.shape[0], -1)


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
    B, C, D, H, W, k = case
    vol = (B, D, H, W)
    g = rc.gen(100 + C + D + H + W)
    h16, U = _spiked(vol, C, 4 * C, k, g)
    P = math.prod(vol)
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
    c_out, h_out, acts = (_guarded(arena, (*vol, n), F32) for n in (C, C, 4 * C))
    h16_out = _guarded(arena, (*vol, C), BF)
    dps = [p.cuda() for p in ps] if peep else [None] * 3
    _n().convlstm3d_fwd_step(U.cuda(), h16.cuda(), xg.view(*vol, 4 * C).cuda(), cp.view(*vol, C).cuda(), c_out, h_out,
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
    B, C, D, H, W, k = case
    vol = (B, D, H, W)
    g = rc.gen(200 + C + D + H + W)
    P = math.prod(vol)
    dgn, wf = _spiked(vol, 4 * C, C, k, g)           # wf: the weight as applied; the kernel takes it tap-flipped
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
    dc = _guarded(arena, (*vol, C), F32, inp["dc"])
    dg16 = _guarded(arena, (*vol, 4 * C), BF)
    dev = {n: (inp[n].view(*vol, -1).cuda() if inp[n] is not None else None)
           for n in ("dout", "dh_ext", "acts", "c_prev", "c_t")}
    dps = [p.cuda() for p in ps] if peep else [None] * 3
    _n().convlstm3d_bwd_step(wf.flip(1, 2, 3).contiguous().cuda(), None if last else dgn.cuda(), dev["dout"],
                             dev["dh_ext"], dev["acts"], dev["c_prev"], dev["c_t"], dc, dg16, pI=dps[0], pF=dps[1],
                             pO=dps[2], hard=False)
    torch.cuda.synchronize()
    assert all(rc.canaries_ok(*it) for it in arena)
    o = rc.lstm_bwd(inp)
    name = f"{case}-{'peep' if peep else 'nopeep'}-{variant}"
    dgb = o["dg"]
    _check("bwd_dg", name, dg16.float(), rc.V(dgb.v, dgb.e + rc.bf16_half_ulp(dgb.v.abs() + dgb.e)))
    _check("bwd_dc", name, dc, o["dc"])


def test_tile_past_the_lds_cap_is_refused_before_a_launch():
    B, C, D, H, W, k = REFUSED
    N = _n()
    assert N.convlstm3d_supported(B, C, D, H, W - 1, k) and not N.convlstm3d_supported(B, C, D, H, W, k)
    z = {n: torch.zeros(B, D, H, W, n, device="cuda") for n in (C, 4 * C)}
    h16 = torch.zeros(B, D, H, W, C, device="cuda", dtype=BF)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        N.convlstm3d_fwd_step(torch.zeros(4 * C, k, k, k, C, device="cuda", dtype=BF), h16, z[4 * C], z[C],
                              torch.empty_like(z[C]), torch.empty_like(z[C]), torch.empty_like(h16))


@pytest.mark.parametrize("peep", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("hard", [False, True], ids=["sigmoid", "hard"])
def test_seq_matches_own_torch_form_fp64(hard, peep):
    from bigdl_amd.nn.recurrent import _ConvLSTM3dSeq

    B, T, Cin, C, vol = 2, 3, 4, 16, (3, 4, 5)
    g = rc.gen(11)
    shapes = [(B, T, Cin, *vol), (B, C, *vol), (B, C, *vol), (4 * C, Cin, 3, 3, 3), (4 * C,), (4 * C, C, 3, 3, 3)]
    shapes += [(1, C, 1, 1, 1)] * 3 if peep else []
    vals = [(torch.randn(s, generator=g) * (0.2 if len(s) == 5 and s[0] == 4 * C else 1.0)).to(BF) for s in shapes]
    gouts = [torch.randn(s, generator=g) for s in ((B, T, C, *vol), (B, C, *vol), (B, C, *vol))]
    res = []
    for dev, dt in (("cuda", F32), ("cpu", F64)):
        leaves = [v.to(dev, dt).requires_grad_(True) for v in vals]
        outs = _ConvLSTM3dSeq.apply(*leaves, *([] if peep else [None] * 3), hard)
        res.append(list(outs) + list(torch.autograd.grad(outs, leaves, [t.to(dev, dt) for t in gouts])))
    for k, (a, b) in enumerate(zip(*res)):
        assert a.shape == b.shape and _rel(a, b) < (1e-2 if k < 3 else 2e-2), (k, _rel(a, b))


@pytest.mark.parametrize("switch", [True, None], ids=["on", "unset"])
@pytest.mark.parametrize("name", ["k3", "c8", "mask"])
def test_module_matches_cpu_engine_and_route(name, switch, monkeypatch):
    """With the switch on the usable cell takes the fused route (Cell.sequence never sees a GPU tensor); unset, it takes
    the loop. outputSize 8 and maskZero take the loop in either setting. Training and eval mode."""
    from bigdl_amd import nn
    from bigdl_amd.nn import recurrent
    from bigdl_amd.utils.random_generator import RNG

    monkeypatch.delenv("BIGDL_CONVLSTM3D_FUSED", raising=False)
    monkeypatch.setattr(recurrent, "_CONVLSTM3D_FUSED", [None])      # restored after the test
    recurrent.set_convlstm3d_fused(switch)
    RNG.setSeed(5)
    cpu = nn.Recurrent(maskZero=name == "mask").add(nn.ConvLSTMPeephole3D(4, 8 if name == "c8" else 16, 3, 3))
    gpu = copy.deepcopy(cpu).to("cuda")
    loop, on_gpu = recurrent.Cell.sequence, []

    def spy(self, x2, *a, **kw):
        on_gpu.append(x2.is_cuda)
        return loop(self, x2, *a, **kw)

    monkeypatch.setattr(recurrent.Cell, "sequence", spy)
    x = torch.randn(2, 3, 4, 4, 6, 6).to(BF).float()
    yc, yg = cpu.forward(x), gpu.forward(x.cuda())
    assert (True in on_gpu) == (not (name == "k3" and switch))
    assert yg.shape == yc.shape and _rel(yg, yc) < 1e-2, _rel(yg, yc)
    gy = torch.randn_like(yc)
    assert _rel(gpu.backward(x.cuda(), gy.cuda()), cpu.backward(x, gy)) < 2e-2
    for a, b in zip(gpu.parameters()[1], cpu.parameters()[1]):
        assert _rel(a, b) < 2e-2, (a.shape, _rel(a, b))
    assert _rel(gpu.evaluate().forward(x.cuda()), cpu.evaluate().forward(x)) < 1e-2
