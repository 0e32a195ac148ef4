"""The plain-torch form of ``_ConvLSTMSeq`` (its forward and its hand-derived backward) in fp64 against autograd through
the per-step loop of ``_ConvLSTMBase.step``: every output and gradient to a relative 1e-9 (pure fp64 rounding over a few
thousand operations is about 1e-13)."""
import pytest
import torch

B, T, CIN, C, H, W = 2, 3, 3, 4, 5, 6

# kernelI, kernelC, padding, withPeephole, hard-sigmoid inner activation
CASES = [(3, 3, -1, True, False), (3, 3, 1, False, True), (5, 3, -1, True, True), (1, 5, -1, False, False)]


@pytest.mark.parametrize("kI,kC,pad,peep,hard", CASES)
def test_torch_form_matches_autograd_of_step_loop(kI, kC, pad, peep, hard):
    from bigdl_amd import nn
    from bigdl_amd.nn.recurrent import Cell, _ConvLSTMSeq

    torch.manual_seed(kI * 10 + kC)
    cell = nn.ConvLSTMPeephole(CIN, C, kI, kC, 1, pad, None, nn.HardSigmoid() if hard else None, withPeephole=peep)
    owners = [(cell.i2g, "weight"), (cell.i2g, "bias"), (cell.h2g, "weight")]
    if peep:
        owners += [(m, "weight") for m in (cell.peepI, cell.peepF, cell.peepO)]
    params = [torch.randn_like(getattr(m, w), dtype=torch.float64).mul_(0.3).requires_grad_(True) for m, w in owners]
    for (m, w), p in zip(owners, params):
        object.__setattr__(m, w, p)
    ins = [torch.randn(B, T, CIN, H, W, dtype=torch.float64), torch.randn(B, C, H, W, dtype=torch.float64),
           torch.randn(B, C, H, W, dtype=torch.float64)]
    ins = [t.requires_grad_(True) for t in ins]
    gouts = [torch.randn(B, T, C, H, W, dtype=torch.float64), torch.randn(B, C, H, W, dtype=torch.float64),
             torch.randn(B, C, H, W, dtype=torch.float64)]

    out, (h, c) = Cell.sequence(cell, ins[0], ins[1:])
    want = [out, h, c] + list(torch.autograd.grad([out, h, c], ins + params, gouts))
    pe = params[3:] if peep else [None, None, None]
    got = _ConvLSTMSeq.apply(*ins, *params[:3], *pe, hard)
    got = list(got) + list(torch.autograd.grad(got, ins + params, gouts))
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        a, b = a.detach(), b.detach()
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max()), k
