"""The sparse kernels (csrc/sparse.hip) element by element against the fp64 oracles of tests/sparse_cases.py, and the
three modules built on them against the CPU engine.

* exact leg: small integers, every sum below 2^24: torch.equal to the oracle on the atomic and the ordered route;
* gauss leg: per element |err| <= (n + 4) * 2^-23 * sum |terms| (sparse_cases.bound), derived, not measured;
* skipped indices, deterministic mode, the modules against the CPU engine computing in fp64, and the proof that the
  native path ran (torch.sparse.mm / to_dense / to_sparse raise meanwhile).

The op calls run under torch.cuda.set_sync_debug_mode("error"): nothing in them may wait on the host.
BIGDL_SPARSE_EDGE_PROFILE=<file> writes the largest measured err / bound per kernel (profiles/
sparse_native_errors.txt is such a file)."""
import contextlib
import functools
import os

import pytest
import torch

from bigdl_amd import nn
from bigdl_amd.ops import native
from bigdl_amd.ops import sparse as sp
from bigdl_amd.utils.table import T
from tests import sparse_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = [c.name for c in sc.CASES]
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    sp.set_native(True)
    yield
    sp.set_native(None)
    native.set_deterministic(False)
    path = os.environ.get("BIGDL_SPARSE_EDGE_PROFILE")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# tests/test_sparse_gpu.py with BIGDL_SPARSE_EDGE_PROFILE set, on one MI355X.\n"
                    "# kernel, largest measured |got - fp64 oracle| / bound over its Gaussian cases (<= 1 passes);\n"
                    "# bound = (n + 4) * 2^-23 * sum |terms| per element (tests/sparse_cases.py)\n")
            for k, r in sorted(RATIOS.items()):
                f.write(f"{k:40s} {r:.4f}\n")


@contextlib.contextmanager
def no_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


@contextlib.contextmanager
def deterministic():
    native.set_deterministic(True)
    try:
        yield
    finally:
        native.set_deterministic(False)


def within(kernel, got, ref, n, a):
    """Every element inside the derived bound; records the largest err / bound of ``kernel``."""
    got = got.detach().double().cpu()
    b = sc.bound(n, a).expand_as(ref)
    err = (got - ref).abs()
    pos = b > 0
    if bool(pos.any()):
        r = float((err[pos] / b[pos]).max())
        print(f"{kernel}: max err / bound = {r:.4f}")
        RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)
    bad = err > b
    assert not bool(bad.any()), f"{kernel}: {int(bad.sum())} elements outside the bound, worst err {float(err.max()):.3e}"


def test_sync_debug_mode_is_honoured():
    """The guard the other tests rely on: under mode "error" a host read of a device value raises."""
    t = torch.ones(1, device=DEV)
    with no_sync(), pytest.raises(RuntimeError):
        t.item()


# ------------------------------------------------------------------------------------------------- spmm family
@functools.lru_cache(maxsize=None)
def lin_data(name, N, exact):
    c = sc.CASE[name]
    rows, cols = sc.pattern(name)
    if exact:
        vals = sc.ints((c.nnz,), -3, 3, 1, nonzero=True)
        W, bias, gy = sc.ints((N, c.D), -4, 4, 2), sc.ints((N,), -8, 8, 3), sc.ints((c.B, N), -4, 4, 4)
    else:
        vals = sc.gauss((c.nnz,), 5)
        W, bias, gy = sc.gauss((N, c.D), 6), sc.gauss((N,), 7), sc.gauss((c.B, N), 8)
    return c, rows, cols, vals, W, bias, gy


def run_linear_ops(c, rows, cols, vals, W, bias, gy, scale, base):
    """spmm, spmm_wgrad on both routes (from gradWeight = base), sddmm: all under the no-sync guard."""
    x = sc.sparse(rows, cols, vals, c.B, c.D, DEV)
    Wd, bd, gyd = W.to(DEV), bias.to(DEV), gy.to(DEV)
    gWa = torch.full(W.shape, float(base), device=DEV)
    gWo = torch.full(W.shape, float(base), device=DEV)
    with no_sync():
        co = sp.Coo(x)
        y = sp.spmm(co, Wd, bd)
        assert sp.last_route("spmm") == "native"
        y0 = sp.spmm(co, Wd, None)
        assert sp.spmm_wgrad(co, gyd, gWa, scale) is gWa and sp.last_route("spmm_wgrad") == "native"
        with deterministic():
            sp.spmm_wgrad(co, gyd, gWo, scale)
            assert sp.last_route("spmm_wgrad") == "ordered"
        g = sp.sddmm(co, gyd, Wd)
        assert sp.last_route("sddmm") == "native"
    return y, y0, gWa, gWo, g


@pytest.mark.parametrize("N", sc.N_SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_spmm_family_exact(name, N):
    c, rows, cols, vals, W, bias, gy = lin_data(name, N, True)
    y, y0, gWa, gWo, g = run_linear_ops(c, rows, cols, vals, W, bias, gy, 0.5, 3)
    ry = sc.spmm_oracle(rows, cols, vals, W, bias, c.B)[0]
    assert torch.equal(y.cpu(), ry.float())
    assert torch.equal(y0.cpu(), sc.spmm_oracle(rows, cols, vals, W, None, c.B)[0].float())
    rg = (sc.wgrad_oracle(rows, cols, vals, gy, c.D, 0.5)[0] + 3).float()
    assert torch.equal(gWa.cpu(), rg), "atomic route"
    assert torch.equal(gWo.cpu(), rg), "ordered route"
    assert g.shape == (c.nnz,) and torch.equal(g.cpu(), sc.sddmm_oracle(rows, cols, gy, W)[0].float())


@pytest.mark.parametrize("N", sc.N_SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_spmm_family_gauss(name, N):
    c, rows, cols, vals, W, bias, gy = lin_data(name, N, False)
    y, y0, gWa, gWo, g = run_linear_ops(c, rows, cols, vals, W, bias, gy, 0.5, 0)
    mapping = "entries" if N <= 8 else "outputs"
    within(f"spmm_fwd ({mapping} mapping)", y, *sc.spmm_oracle(rows, cols, vals, W, bias, c.B))
    within(f"spmm_fwd ({mapping} mapping)", y0, *sc.spmm_oracle(rows, cols, vals, W, None, c.B))
    ref = sc.wgrad_oracle(rows, cols, vals, gy, c.D, 0.5)
    within("spmm_wgrad (atomic)", gWa, *ref)
    within("spmm_wgrad (ordered)", gWo, *ref)
    within(f"sddmm_rows ({'thread' if N <= 8 else 'group'} per entry)", g, *sc.sddmm_oracle(rows, cols, gy, W))


def test_spmm_forward_is_bitwise_reproducible():
    c, rows, cols, vals, W, bias, gy = lin_data("b67_mixed", 3, False)
    x = sc.sparse(rows, cols, vals, c.B, c.D, DEV)
    Wd, bd = W.to(DEV), bias.to(DEV)
    assert torch.equal(sp.spmm(x, Wd, bd), sp.spmm(x, Wd, bd))


# ------------------------------------------------------------------------------------------------- lookup
@functools.lru_cache(maxsize=None)
def lookup_data(name, nOut, exact, weighted):
    c = sc.CASE[name]
    rows, slots, ids = sc.lookup_pattern(name)
    if exact:
        wts = sc.ints((ids.numel(),), 1, 3, 11) if weighted else None
        Wt, gy = sc.ints((sc.N_INDEX, nOut), -4, 4, 12), sc.ints((c.B, nOut), -4, 4, 13)
    else:
        wts = sc.gauss((ids.numel(),), 14, positive=True) if weighted else None
        Wt, gy = sc.gauss((sc.N_INDEX, nOut), 15), sc.gauss((c.B, nOut), 16)
    return c, rows, slots, ids, wts, Wt, gy


def run_lookup_ops(c, rows, slots, ids, wts, Wt, gy, comb, scale, base):
    xi = sc.sparse(rows, slots, ids, c.B, sc.LOOKUP_L, DEV)
    xw = None if wts is None else sc.sparse(rows, slots, wts, c.B, sc.LOOKUP_L, DEV)
    Wd, gyd = Wt.to(DEV), gy.to(DEV)
    gWa = torch.full(Wt.shape, float(base), device=DEV)
    gWo = torch.full(Wt.shape, float(base), device=DEV)
    with no_sync():
        ci, cw = sp.Coo(xi), (None if xw is None else sp.Coo(xw))
        out, scales = sp.lookup_sparse(ci, cw, Wd, comb)
        assert sp.last_route("lookup_sparse") == "native"
        sp.lookup_sparse_backward(ci, cw, scales, gyd, gWa, scale)
        assert sp.last_route("lookup_sparse_backward") == "native"
        with deterministic():
            sp.lookup_sparse_backward(ci, cw, scales, gyd, gWo, scale)
            assert sp.last_route("lookup_sparse_backward") == "ordered"
    return out, scales, gWa, gWo


@pytest.mark.parametrize("nOut", sc.NOUT_SIZES)
@pytest.mark.parametrize("name", [n for n in NAMES if n != "b67_d1"])
def test_lookup_exact(name, nOut):
    """Combiner sum (s_b = 1): the other two scale by 1 / sum w or 1 / sqrt(sum w^2), which is no integer; they are
    held to the bound in test_lookup_gauss."""
    for weighted in (False, True):
        c, rows, slots, ids, wts, Wt, gy = lookup_data(name, nOut, True, weighted)
        out, scales, gWa, gWo = run_lookup_ops(c, rows, slots, ids, wts, Wt, gy, "sum", 0.5, 3)
        ref, rs, _, _ = sc.lookup_oracle(rows, ids, wts, Wt, "sum", c.B)
        assert torch.equal(out.cpu(), ref.float()) and torch.equal(scales.cpu(), rs.float())
        rg = (sc.lookup_bwd_oracle(rows, ids, wts, rs, gy, sc.N_INDEX, 0.5)[0] + 3).float()
        assert torch.equal(gWa.cpu(), rg), "atomic route"
        assert torch.equal(gWo.cpu(), rg), "ordered route"


@pytest.mark.parametrize("comb", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("nOut", sc.NOUT_SIZES)
@pytest.mark.parametrize("name", ["b1_130", "b5_edges", "b5_empty", "b67_mixed", "b67_contended"])
def test_lookup_gauss(name, nOut, comb):
    for weighted in (False, True):
        c, rows, slots, ids, wts, Wt, gy = lookup_data(name, nOut, False, weighted)
        out, scales, gWa, gWo = run_lookup_ops(c, rows, slots, ids, wts, Wt, gy, comb, 0.5, 0)
        ref, rs, a, n = sc.lookup_oracle(rows, ids, wts, Wt, comb, c.B)
        within("lookup_sparse_fwd", out, ref, n, a)
        within("lookup_sparse_fwd (row scale)", scales, rs, n[:, 0], rs.abs())
        # the backward takes s_b as an input: the oracle gets the kernel's own fp32 scales
        back = sc.lookup_bwd_oracle(rows, ids, wts, scales.cpu(), gy, sc.N_INDEX, 0.5)
        within("lookup_sparse_bwd (atomic)", gWa, *back)
        within("lookup_sparse_bwd (ordered)", gWo, *back)
        empty = torch.tensor([k == 0 for k in c.counts])
        assert int(out.cpu()[empty].count_nonzero()) == 0, "an empty row gives zeros"


# ------------------------------------------------------------------------------------------------- join
@pytest.mark.parametrize("name", [j[0] for j in sc.JOINS])
def test_concat_cols_equals_dense_cat(name):
    B, parts = sc.join_parts(name)
    xs = [sc.sparse(r, c, v, B, D, DEV) for r, c, v, D in parts]
    with no_sync():
        got = sp.concat_cols(xs)
    assert sp.last_route("concat_cols") == "native"
    ref = torch.cat([sc.sparse(r, c, v, B, D).to_dense() for r, c, v, D in parts], dim=1).to_sparse()
    assert got.is_coalesced() and ref.is_coalesced() and tuple(got.shape) == tuple(ref.shape)
    assert torch.equal(got._indices().cpu(), ref._indices()) and torch.equal(got._values().cpu(), ref._values())
    rows, cols, vals = sc.concat_oracle(parts, B)
    assert torch.equal(got._indices().cpu(), torch.stack([rows, cols]).reshape(2, -1))


def test_concat_of_nine_inputs_takes_the_torch_form():
    B, parts = sc.join_parts("two")
    xs = [sc.sparse(parts[1][0], parts[1][1], parts[1][2], B, 1, DEV)] * 9
    got = sp.concat_cols(xs)
    assert sp.last_route("concat_cols") == "torch" and tuple(got.shape) == (B, 9)


# ------------------------------------------------------------------------------------------------- skipped indices
def test_out_of_range_entries_are_skipped():
    """A column equal to D (last in its row) and a row equal to B (last of all) keep the list row-major sorted; the
    tensor is built without index validation. Integer data: the result equals the one with those entries removed."""
    c, rows, cols, vals, W, bias, gy = lin_data("b5_edges", 3, True)
    pos = int((rows == 2).nonzero()[-1]) + 1                    # behind row 2's last entry
    rows2 = torch.cat([rows[:pos], torch.tensor([2]), rows[pos:], torch.tensor([c.B])])
    cols2 = torch.cat([cols[:pos], torch.tensor([c.D]), cols[pos:], torch.tensor([5])])
    vals2 = torch.cat([vals[:pos], torch.tensor([2.0]), vals[pos:], torch.tensor([3.0])])
    keep = torch.ones(rows2.numel(), dtype=torch.bool)
    keep[pos] = keep[-1] = False
    assert torch.equal(rows2[keep], rows) and torch.equal(cols2[keep], cols)
    bad = run_linear_ops(c, rows2, cols2, vals2, W, bias, gy, 1.0, 0)
    good = run_linear_ops(c, rows, cols, vals, W, bias, gy, 1.0, 0)
    for b, g in zip(bad[:4], good[:4]):
        assert torch.equal(b, g)
    assert torch.equal(bad[4][keep.to(DEV)], good[4]) and int(bad[4][~keep.to(DEV)].count_nonzero()) == 0


def test_out_of_range_ids_are_skipped():
    c, rows, slots, ids, wts, Wt, gy = lookup_data("b5_edges", 63, True, True)
    ids2 = ids.clone()
    drop = torch.zeros(ids.numel(), dtype=torch.bool)
    first = [int((rows == b).nonzero()[0]) for b in (1, 2, 3)]
    ids2[first[0]], ids2[first[1] + 1], ids2[first[2] + 64] = 0.0, float(sc.N_INDEX + 1), float(sc.N_INDEX + 1)
    drop[[first[0], first[1] + 1, first[2] + 64]] = True
    for comb in ("sum", "mean", "sqrtn"):
        bad = run_lookup_ops(c, rows, slots, ids2, wts, Wt, gy, comb, 1.0, 0)
        good = run_lookup_ops(c, rows[~drop], slots[~drop], ids[~drop], wts[~drop], Wt, gy, comb, 1.0, 0)
        # the atomic route's order is free, so its bits are defined only where the terms are integers (sum)
        for k, (b, g) in enumerate(zip(bad, good)):
            assert k == 2 and comb != "sum" or torch.equal(b, g), comb


# ------------------------------------------------------------------------------------------------- deterministic mode
def test_deterministic_mode_is_bitwise_reproducible():
    c, rows, cols, vals, W, bias, gy = lin_data("b67_contended", 65, False)
    x = sp.Coo(sc.sparse(rows, cols, vals, c.B, c.D, DEV))
    gyd = gy.to(DEV)
    _, lrows, slots, ids, wts, Wt, lgy = lookup_data("b67_contended", 130, False, True)
    ci = sp.Coo(sc.sparse(lrows, slots, ids, c.B, sc.LOOKUP_L, DEV))
    cw = sp.Coo(sc.sparse(lrows, slots, wts, c.B, sc.LOOKUP_L, DEV))
    _, scales = sp.lookup_sparse(ci, cw, Wt.to(DEV), "sqrtn")
    runs = []
    with deterministic():
        for _ in range(2):
            gW = torch.zeros(W.shape, device=DEV)
            sp.spmm_wgrad(x, gyd, gW, 0.5)
            assert sp.last_route("spmm_wgrad") == "ordered"
            gT = torch.zeros(Wt.shape, device=DEV)
            sp.lookup_sparse_backward(ci, cw, scales, lgy.to(DEV), gT, 0.5)
            assert sp.last_route("lookup_sparse_backward") == "ordered"
            runs.append((gW, gT))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert int(runs[0][0][:, sc.HOT].count_nonzero()) == 65 and int(runs[0][1][sc.HOT - 1].count_nonzero()) == 130


# ------------------------------------------------------------------------------------------------- modules
def cpu64(m):
    """The CPU-engine copy of GPU module ``m`` with fp64 parameters and zeroed gradients: the reference."""
    ref = m.cloneModule().to("cpu")
    for w, g in ref._params:
        if getattr(ref, w, None) is not None:
            setattr(ref, w, getattr(m, w).detach().cpu().double())
            setattr(ref, g, torch.zeros_like(getattr(ref, w)))
    ref.scaleW, ref.scaleB = m.scaleW, m.scaleB
    return ref


def check_sparse_linear(m, ref, x, x64, gy, rows, cols, vals, kernel):
    """Forward, gradInput, gradWeight, gradBias of GPU SparseLinear ``m`` against its fp64 CPU copy ``ref``."""
    B = x.shape[0]
    W64, b64 = ref.weight, ref.bias
    y, y64 = m.forward(x), ref.forward(x64)
    _, a, n = sc.spmm_oracle(rows, cols, vals, W64, b64, B)
    within(f"{kernel} forward", y, y64, n, a)
    gi, gi64 = m.backward(x, gy.to(DEV)), ref.backward(x64, gy.double())
    if m.backwardStart >= 0 and m.backwardLength > 0:
        w = W64[:, m.backwardStart - 1:m.backwardStart - 1 + m.backwardLength]
        assert not gi.is_sparse and tuple(gi.shape) == (B, m.backwardLength)
        within(f"{kernel} gradInput window", gi, gi64, torch.full((1,), float(W64.shape[0])), gy.double().abs() @ w.abs())
    else:
        assert gi.is_sparse and torch.equal(gi._indices().cpu(), torch.stack([rows, cols]))
        _, a, n = sc.sddmm_oracle(rows, cols, gy, W64)
        within(f"{kernel} gradInput", gi._values(), gi64.coalesce()._values(), n, a)
    _, a, n = sc.wgrad_oracle(rows, cols, vals, gy, W64.shape[1], m.scaleW)
    within(f"{kernel} gradWeight", m.gradWeight, ref.gradWeight, n, a)
    within(f"{kernel} gradBias", m.gradBias, ref.gradBias, torch.full((1,), float(B)),
           m.scaleB * gy.double().abs().sum(0))


@pytest.mark.parametrize("window,scaleW", [(None, 1.0), ((3, 40), 1.0), (None, 0.5), ((sc.BIG_D - 6, 7), 0.5)])
def test_sparse_linear_module_against_cpu_engine(window, scaleW):
    c, rows, cols, vals, _, _, _ = lin_data("b67_mixed", 3, False)
    kw = {} if window is None else {"backwardStart": window[0], "backwardLength": window[1]}
    m = nn.SparseLinear(c.D, 3, **kw).to(DEV)
    m.scaleW = scaleW
    ref = cpu64(m)
    x = sc.sparse(rows, cols, vals, c.B, c.D, DEV)
    x64 = sc.sparse(rows, cols, vals.double(), c.B, c.D)
    check_sparse_linear(m, ref, x, x64, sc.gauss((c.B, 3), 21), rows, cols, vals, "SparseLinear")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("comb", ["sum", "mean", "sqrtn"])
def test_lookup_table_sparse_module_against_cpu_engine(comb, weighted):
    c, rows, slots, ids, wts, _, gy = lookup_data("b67_contended", 63, False, weighted)
    m = nn.LookupTableSparse(sc.N_INDEX, 63, comb).to(DEV)
    ref = cpu64(m)

    def inputs(dev, dt):
        xi = sc.sparse(rows, slots, ids.to(dt), c.B, sc.LOOKUP_L, dev)
        return xi if wts is None else T(xi, sc.sparse(rows, slots, wts.to(dt), c.B, sc.LOOKUP_L, dev))

    xg, xc = inputs(DEV, torch.float32), inputs("cpu", torch.float64)
    out, out64 = m.forward(xg), ref.forward(xc)
    _, rs, a, n = sc.lookup_oracle(rows, ids, wts, ref.weight, comb, c.B)
    within("LookupTableSparse forward", out, out64, n, a)
    gi = m.backward(xg, gy.to(DEV))
    ref.backward(xc, gy.double())
    for g in ([gi] if wts is None else [gi[1], gi[2]]):
        assert g.is_sparse and torch.equal(g._indices().cpu(), torch.stack([rows, slots]))
        assert int(g._values().count_nonzero()) == 0
    _, a, n = sc.lookup_bwd_oracle(rows, ids, wts, rs, gy, sc.N_INDEX, 1.0)
    within("LookupTableSparse gradWeight", m.gradWeight, ref.gradWeight, n, a)


def wide_and_deep(D1, D2):
    wide = nn.Sequential().add(nn.SparseJoinTable(2)).add(nn.SparseLinear(D1 + D2, 2))
    return nn.Sequential().add(nn.ParallelTable().add(wide).add(nn.Linear(8, 2))).add(nn.CAddTable())


def test_wide_and_deep_graph_against_cpu_engine():
    """SparseJoinTable -> SparseLinear beside a dense Linear under ParallelTable + CAddTable, on CUDA tensors. The
    wide branch is held to the bound against its fp64 CPU copy; the deep Linear computes in bf16, so the sum is
    checked as wide reference + the GPU's own deep output (one more fp32 addition, inside the + 4)."""
    B, parts = sc.join_parts("two", exact=False)
    (r1, c1, v1, D1), (r2, c2, v2, D2) = parts
    model = wide_and_deep(D1, D2).to(DEV)
    par = model.modules[0]
    wide, deep = par.modules[0], par.modules[1]
    join, lin = wide.modules
    ref_join, ref_lin = nn.SparseJoinTable(2), cpu64(lin)
    deep_x = sc.gauss((B, 8), 31)
    xs = T(T(sc.sparse(r1, c1, v1, B, D1, DEV), sc.sparse(r2, c2, v2, B, D2, DEV)), deep_x.to(DEV))
    out = model.forward(xs)
    rows, cols, vals = sc.concat_oracle(parts, B)
    joined = join.output
    assert joined.is_sparse and joined.is_coalesced() and torch.equal(joined._indices().cpu(), torch.stack([rows, cols]))
    assert torch.equal(joined._values().cpu(), vals)
    x64 = ref_join.forward(T(sc.sparse(r1, c1, v1.double(), B, D1), sc.sparse(r2, c2, v2.double(), B, D2)))
    y64 = ref_lin.forward(x64)
    _, a, n = sc.spmm_oracle(rows, cols, vals, ref_lin.weight, ref_lin.bias, B)
    within("wide & deep: SparseLinear forward", lin.output, y64, n, a)
    deep_out = deep.output.double().cpu()
    within("wide & deep: output", out, y64 + deep_out, n + 1, a + deep_out.abs())
    gy = sc.gauss((B, 2), 32)
    model.backward(xs, gy.to(DEV))
    ref_lin.backward(x64, gy.double())
    _, a, n = sc.wgrad_oracle(rows, cols, vals, gy, D1 + D2, 1.0)
    within("wide & deep: SparseLinear gradWeight", lin.gradWeight, ref_lin.gradWeight, n, a)
    within("wide & deep: SparseLinear gradBias", lin.gradBias, ref_lin.gradBias, torch.full((1,), float(B)),
           gy.double().abs().sum(0))
    _, a, n = sc.sddmm_oracle(rows, cols, gy, ref_lin.weight)
    within("wide & deep: SparseLinear gradInput", lin.gradInput._values(), ref_lin.gradInput.coalesce()._values(), n, a)


# ------------------------------------------------------------------------------------------------- the native path ran
def _forbid(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch sparse fallback called")

    monkeypatch.setattr(torch.sparse, "mm", refuse)
    monkeypatch.setattr(torch.Tensor, "to_dense", refuse)
    monkeypatch.setattr(torch.Tensor, "to_sparse", refuse)


def _runs_native_only(monkeypatch, run):
    with monkeypatch.context() as mp:
        _forbid(mp)
        run()
        torch.cuda.synchronize()
        try:
            sp.set_native(False)
            with pytest.raises(AssertionError, match="torch sparse fallback called"):
                run()
        finally:
            sp.set_native(True)


def test_sparse_linear_runs_native(monkeypatch):
    c, rows, cols, vals, _, _, gy = lin_data("b67_mixed", 3, False)
    m = nn.SparseLinear(c.D, 3).to(DEV)
    x = sc.sparse(rows, cols, vals, c.B, c.D, DEV)
    gyd = gy.to(DEV)

    def run():
        m.forward(x)
        m.backward(x, gyd)

    _runs_native_only(monkeypatch, run)


def test_lookup_table_sparse_runs_native(monkeypatch):
    c, rows, slots, ids, wts, _, gy = lookup_data("b67_mixed", 64, False, True)
    m = nn.LookupTableSparse(sc.N_INDEX, 64, "mean").to(DEV)
    x = T(sc.sparse(rows, slots, ids, c.B, sc.LOOKUP_L, DEV), sc.sparse(rows, slots, wts, c.B, sc.LOOKUP_L, DEV))
    gyd = gy.to(DEV)

    def run():
        m.forward(x)
        m.backward(x, gyd)

    _runs_native_only(monkeypatch, run)


def test_wide_and_deep_graph_runs_native(monkeypatch):
    B, parts = sc.join_parts("two", exact=False)
    (r1, c1, v1, D1), (r2, c2, v2, D2) = parts
    model = wide_and_deep(D1, D2).to(DEV)
    xs = T(T(sc.sparse(r1, c1, v1, B, D1, DEV), sc.sparse(r2, c2, v2, B, D2, DEV)), sc.gauss((B, 8), 41).to(DEV))
    gyd = sc.gauss((B, 2), 42).to(DEV)

    def run():
        model.forward(xs)
        model.backward(xs, gyd)

    _runs_native_only(monkeypatch, run)
