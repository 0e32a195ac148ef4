"""tests/conv_edge_cases.py checked on its own (no GPU): the exact leg really is exact, its outputs really are
rounded, and the comparisons of tests/test_conv_edges_gpu.py would notice a kernel that drops a row, drops a K
granule, wraps a border tap, shifts its output columns or truncates instead of rounding."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_edge_cases as ce

FWD = [c for c in ce.NT_CASES if c.fwd]


@pytest.mark.parametrize("case", ce.NT_CASES, ids=str)
def test_nt_partial_sums_are_exact_in_fp32(case):
    """Kdim max|x| max|w| + |bias| + |addend| quanta < 2^24, and the data stays inside the ranges the bound assumes."""
    assert ce.exactness_bound(case) < 2 ** 24
    d = ce.nt_inputs(case, "int")
    for name, lim in (("x", ce.XMAX), ("dy", ce.XMAX), ("w", ce.WMAX), ("bias", ce.BMAX), ("addend", ce.AMAX),
                      ("out0", ce.BMAX), ("bx", ce.XMAX)):
        t = d[name]
        assert t.abs().max() <= lim and torch.equal(t, t.round()) and t.abs().max() > 0, name
    if case.pre:
        xa = ce.pre_apply(case, "int")
        assert xa.abs().max() <= 2 * ce.XMAX + 2 and torch.equal(xa * 2, (xa * 2).round())
    for op in ce.fwd_ops(case) + ce.dgrad_ops(case):
        y, A = ce.nt_exact(case, "int", op)
        assert A.max() <= ce.exactness_bound(case) * ce.quantum(case, op)
        assert torch.equal(y / ce.quantum(case, op), (y / ce.quantum(case, op)).round())


@pytest.mark.parametrize("case", ce.WG_CASES, ids=str)
def test_wgrad_partial_sums_are_exact_in_fp32(case):
    assert ce.wg_exactness_bound(case) < 2 ** 24
    dw, db, Aw, Ab = ce.wg_reference(case, "int")
    assert max(Aw.max(), Ab.max()) <= ce.wg_exactness_bound(case)
    assert torch.equal(dw, dw.round()) and torch.equal(db, db.round())
    d = ce.wg_inputs(case, "int")
    assert d["dw0"].abs().max() > 0 and d["db0"].abs().max() > 0       # the kernels accumulate: a non-zero start


@pytest.mark.parametrize("case", ce.NT_CASES + ce.WG_CASES, ids=str)
def test_fp32_conv_equals_fp64_on_integer_data(case):
    """Whatever order an fp32 implementation sums in, it lands on the fp64 value."""
    N, C, H, K, R, st, pd, OH = case.dims
    kw = dict(stride=2) if case.pair else dict(stride=st, padding=pd)
    if isinstance(case, ce.WG):
        d = ce.wg_inputs(case, "int")
        w64 = torch.nn.grad.conv2d_weight(d["x"], d["dw0"].shape, d["dy"], **kw)
        w32 = torch.nn.grad.conv2d_weight(d["x"].float(), d["dw0"].shape, d["dy"].float(), **kw)
        assert torch.equal(w32.double(), w64)
        return
    d = ce.nt_inputs(case, "int")
    assert torch.equal(F.conv2d(d["x"].float(), d["w"].float(), **kw).double(), F.conv2d(d["x"], d["w"], **kw))
    if case.dgrad:
        g32 = torch.nn.grad.conv2d_input(d["x"].shape, d["w"].float(), d["dy"].float(), **kw)
        assert torch.equal(g32.double(), torch.nn.grad.conv2d_input(d["x"].shape, d["w"], d["dy"], **kw))


@pytest.mark.parametrize("case", ce.NT_CASES, ids=str)
def test_expected_outputs_are_really_rounded(case):
    """Some outputs exceed 256 (bf16 holds integers only up to there) and some round differently under truncation,
    so equality with the expectation checks the rounding mode, not just the sums."""
    for op in ce.fwd_ops(case) + ce.dgrad_ops(case):
        if op == "out32_acc":
            continue
        y, _ = ce.nt_exact(case, "int", op)
        assert (y.abs() / ce.quantum(case, op) > 256).float().mean() > 0, op
        assert (ce.round_bf16(y) != ce.trunc_bf16(y)).float().mean() > 0, op


def test_round_bf16_is_nearest_even():
    y = torch.tensor([257.0, 259.0, 258.0, 261.0, -257.0, -259.0, 1.0, 0.0], dtype=torch.float64)
    assert ce.round_bf16(y).double().tolist() == [256.0, 260.0, 258.0, 260.0, -256.0, -260.0, 1.0, 0.0]
    assert ce.trunc_bf16(y).double().tolist() == [256.0, 258.0, 258.0, 260.0, -256.0, -258.0, 1.0, 0.0]


@pytest.mark.parametrize("case,fault", [(c, f) for c in FWD for f in ce.FAULTS if ce.fault_applies(c, f)],
                         ids=lambda v: str(v))
def test_injected_fault_would_be_caught(case, fault):
    """Exact leg: the expectation changes in every output pixel the fault reaches. Gaussian leg: the faulty result
    leaves the per-element bound somewhere. (A border tap can only wrap where there is padding.)"""
    op = "bias_stats"
    rows = ce.fault_rows(case, fault)
    assert rows.any()
    good, _ = ce.nt_exact(case, "int", op)
    bad, _ = ce.nt_exact(case, "int", op, fault=fault)
    changed = (ce.round_bf16(good) != ce.round_bf16(bad)).any(dim=1)
    assert torch.equal(changed & rows, rows), f"{int((rows & ~changed).sum())} of {int(rows.sum())} pixels unchanged"
    ref, A = ce.nt_exact(case, "gauss", op)
    badg, _ = ce.nt_exact(case, "gauss", op, fault=fault)
    over = (ce.round_bf16(badg).double() - ref).abs() > ce.nt_bound(case, op, ref, A)
    assert over.any()


@pytest.mark.parametrize("case", FWD, ids=str)
def test_truncation_would_be_caught(case):
    op = "bias_stats"
    ref, A = ce.nt_exact(case, "gauss", op)
    assert ((ce.trunc_bf16(ref).double() - ref).abs() > ce.nt_bound(case, op, ref, A)).any()
    # and correct rounding of the exact value always passes, with room for the summation term
    assert ((ce.round_bf16(ref).double() - ref).abs() <= ce.BF16_ULP * ref.abs()).all()


@pytest.mark.parametrize("case", [c for c in ce.NT_CASES if c.fwd or c.dgrad], ids=str)
def test_reduction_reference_notices_a_wrong_output(case):
    """The statistics are referred to the expected output: zeroing its last pixel moves the reference sums, so a
    kernel whose sums merely agree with its own wrong output fails."""
    op = "bias_stats" if case.fwd else ce.dgrad_ops(case)[0]
    y, _ = ce.nt_exact(case, "int", op)
    want = ce.round_bf16(y)
    wrong = want.clone()
    wrong[-1, :, -1, -1] = 0
    a, b = ce.reduction_ref(case, "int", op, want), ce.reduction_ref(case, "int", op, wrong)
    assert not torch.equal(a[0][0], b[0][0]) or not torch.equal(a[1][0], b[1][0])
    for s, exact, bound in a:
        assert (bound[~exact] > 0).all()
