"""_LSTMPeepSeq (the sequence function behind LSTMPeephole and the maskZero LSTM on the GPU): its plain-torch branch,
in fp64, against autograd through a straightforward loop of the same formulas (Cell.sequence's mask semantics)."""
import pytest
import torch

B, T, H = 3, 5, 4


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _mask():
    """Row 0: trailing zeros, row 1: leading zeros (BiRecurrent's reversed direction), row 2: fully masked; the batch
    of 3 leaves no room for a fourth row, so the full row is row 0 of the second mask."""
    m = torch.zeros(B, T, dtype=torch.bool)
    m[0, :3] = True
    m[1, 2:] = True
    return m


def _mask_full_row():
    m = _mask()
    m[0, :] = True
    return m


def loop_reference(xg, h0, c0, U, pI, pF, pO, mask, order):
    """The issue's formulas, one step after the other; autograd supplies the gradients."""
    pi, pf, pg, po = order
    Hh = h0.shape[1]
    blk = lambda g, k: g[:, k * Hh:(k + 1) * Hh]  # noqa: E731
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


@pytest.mark.parametrize("order", [(0, 2, 1, 3), (0, 1, 2, 3)], ids=["igfo", "ifgo"])
@pytest.mark.parametrize("mask", [None, _mask(), _mask_full_row()], ids=["nomask", "mask", "mask_full_row"])
@pytest.mark.parametrize("peep", [True, False], ids=["peep", "nopeep"])
def test_lstm_peep_seq_fp64_matches_autograd_loop(peep, mask, order):
    from bigdl_amd.nn.recurrent import _LSTMPeepSeq

    torch.manual_seed(0)
    xg = torch.randn(B, T, 4 * H, dtype=torch.float64)
    h0, c0 = torch.randn(B, H, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64)
    U = torch.randn(4 * H, H, dtype=torch.float64) * 0.5
    ps = [torch.randn(H, dtype=torch.float64) * 0.5 for _ in range(3)] if peep else [None, None, None]
    go = torch.randn(B, T, H, dtype=torch.float64)
    gh, gc = torch.randn(B, H, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64)

    def run(fn):
        leaves = [t.clone().requires_grad_(True) for t in (xg, h0, c0, U)]
        pl = [p.clone().requires_grad_(True) if p is not None else None for p in ps]
        out, hT, cT = fn(*leaves, *pl, mask, order)
        torch.autograd.backward([out, hT, cT], [go, gh, gc])
        return [out.detach(), hT.detach(), cT.detach()] + [t.grad for t in leaves] + [p.grad for p in pl if p is not None]

    got = run(_LSTMPeepSeq.apply)
    ref = run(loop_reference)
    names = ["out", "hT", "cT", "dxg", "dh0", "dc0", "dU", "dpI", "dpF", "dpO"]
    assert len(got) == (10 if peep else 7)
    for n, a, r in zip(names, got, ref):
        assert a is not None and a.dtype == torch.float64 and a.shape == r.shape, n
        assert _rel(a, r) <= 1e-9, (n, _rel(a, r))
    if mask is not None:
        assert (got[0][~mask] == 0).all()
        dead = ~mask.any(1)
        assert torch.equal(got[1][dead], h0[dead]) and torch.equal(got[2][dead], c0[dead])
        assert (got[3][dead] == 0).all()


def test_lstm_peep_seq_rejects_partial_peepholes_and_bad_order():
    from bigdl_amd.nn.recurrent import _LSTMPeepSeq

    xg, h0, c0, U = torch.randn(2, 3, 16), torch.zeros(2, 4), torch.zeros(2, 4), torch.randn(16, 4)
    p = torch.randn(4)
    with pytest.raises(AssertionError):
        _LSTMPeepSeq.apply(xg, h0, c0, U, p, None, p, None, (0, 1, 2, 3))
    with pytest.raises(AssertionError):
        _LSTMPeepSeq.apply(xg, h0, c0, U, None, None, None, None, (0, 1, 1, 3))


def test_cpu_engine_stays_on_the_python_loop(monkeypatch):
    """The modules route to _LSTMPeepSeq on the GPU only: on the CPU engine LSTMPeephole and the maskZero LSTM run
    Cell.sequence as before."""
    from bigdl_amd import nn
    from bigdl_amd.nn import recurrent as rc

    def boom(*a, **k):
        raise AssertionError("_LSTMPeepSeq used on the CPU engine")

    monkeypatch.setattr(rc._LSTMPeepSeq, "forward", staticmethod(boom))
    x = torch.randn(2, 4, 8)
    x[1, 2:] = 0
    for m in (nn.Recurrent().add(nn.LSTMPeephole(8, 32)), nn.Recurrent(maskZero=True).add(nn.LSTMPeephole(8, 32)),
              nn.Recurrent(maskZero=True).add(nn.LSTM(8, 32))):
        y = m.forward(x)
        m.backward(x, torch.ones_like(y))
        assert y.shape == (2, 4, 32)
