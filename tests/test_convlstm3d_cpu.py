"""The plain-torch form of ``_ConvLSTM3dSeq`` (its forward and its hand-derived backward) in fp64 against autograd
through the per-step loop of ``ConvLSTMPeephole3D.step``: every output and gradient to a relative 1e-9, as
tests/test_convlstm_cpu.py does for 2-D."""
import pytest
import torch

B, T, CIN, C, VOL = 2, 3, 3, 4, (3, 4, 5)
F64 = torch.float64

# kernelI, kernelC, padding, withPeephole, hard-sigmoid inner activation
CASES = [(3, 3, -1, True, False), (3, 3, 1, False, True), (1, 5, -1, True, True)]


@pytest.mark.parametrize("kI,kC,pad,peep,hard", CASES)
def test_torch_form_matches_autograd_of_step_loop(kI, kC, pad, peep, hard):
    from bigdl_amd import nn
    from bigdl_amd.nn.recurrent import Cell, _ConvLSTM3dSeq

    torch.manual_seed(kI * 10 + kC)
    cell = nn.ConvLSTMPeephole3D(CIN, C, kI, kC, 1, pad, None, nn.HardSigmoid() if hard else None, withPeephole=peep)
    owners = [(cell.i2g, "weight"), (cell.i2g, "bias"), (cell.h2g, "weight")]
    if peep:
        owners += [(m, "weight") for m in (cell.peepI, cell.peepF, cell.peepO)]
    params = [torch.randn_like(getattr(m, w), dtype=F64).mul_(0.3).requires_grad_(True) for m, w in owners]
    for (m, w), p in zip(owners, params):
        object.__setattr__(m, w, p)
    ins = [torch.randn(s, dtype=F64).requires_grad_(True) for s in ((B, T, CIN, *VOL), (B, C, *VOL), (B, C, *VOL))]
    gouts = [torch.randn(s, dtype=F64) for s in ((B, T, C, *VOL), (B, C, *VOL), (B, C, *VOL))]

    out, (h, c) = Cell.sequence(cell, ins[0], ins[1:])
    want = [out, h, c] + list(torch.autograd.grad([out, h, c], ins + params, gouts))
    got = _ConvLSTM3dSeq.apply(*ins, *params[:3], *(params[3:] if peep else [None] * 3), hard)
    got = list(got) + list(torch.autograd.grad(got, ins + params, gouts))
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-9 * float(b.detach().abs().max()), k
