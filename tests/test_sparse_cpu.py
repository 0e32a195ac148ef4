"""CPU tier of the sparse ops (bigdl_amd/ops/sparse.py, tests/sparse_cases.py): the fp64 oracles against dense fp64
math, the ops' torch forms against the oracles, SparseLinear's backward window, and that every case generator
produces the edge it names."""
import pytest
import torch

from bigdl_amd import nn
from bigdl_amd.ops import sparse as sp
from bigdl_amd.utils.table import Table
from tests import sparse_cases as sc

SMALL_D = 257      # dense fp64 math is affordable here; the patterns are folded into it column-wise


def _folded(name, D=SMALL_D):
    """The case's pattern with its columns folded into [0, D) (duplicates dropped): small enough for dense math."""
    rows, cols = sc.pattern(name)
    B = sc.CASE[name].B
    key = torch.unique(rows * D + cols % D)
    return key // D, key % D, B


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_case_holds_its_edge(name):
    c = sc.CASE[name]
    rows, cols = sc.pattern(name)
    assert rows.numel() == c.nnz
    counts = torch.bincount(rows, minlength=c.B).tolist()
    assert tuple(counts) == c.counts
    key = rows * c.D + cols
    assert bool((key[1:] > key[:-1]).all()), "row-major sorted without duplicates"
    assert c.nnz == 0 or (int(cols.min()) >= 0 and int(cols.max()) < c.D)
    if c.hot >= 0:
        hit = torch.bincount(rows[cols == c.hot], minlength=c.B)
        assert all(int(hit[b]) == (1 if c.counts[b] else 0) for b in range(c.B))
    for b, k in enumerate(c.counts):
        if k >= 3 and c.D >= 2:
            mine = cols[rows == b]
            assert int(mine[0]) == 0 and int(mine[-1]) == c.D - 1


def test_cases_cover_the_listed_edges():
    by = {c.name: c for c in sc.CASES}
    assert {c.B for c in sc.CASES} == {1, 5, 67}
    assert {c.D for c in sc.CASES} == {1, sc.BIG_D}
    lengths = set(by["b67_mixed"].counts)
    assert {0, 1, 63, 64, 65, 130} <= lengths
    assert by["b67_mixed"].counts[0] == 0 and by["b67_mixed"].counts[-1] == 0
    assert by["b5_edges"].counts[0] == 0 and by["b5_edges"].counts[-1] == 0
    assert sorted(by["b5_one_row"].counts) == [0, 0, 0, 0, 130]
    assert by["b5_empty"].nnz == 0
    assert by["b67_contended"].hot == sc.HOT and min(by["b67_contended"].counts) >= 1
    assert sorted(len(m) for _, _, m in sc.JOINS) == [1, 2, 2, 3, 8]
    assert any(sc.CASE[n].nnz == 0 for _, _, m in sc.JOINS for n, _ in m)
    assert any(len({d for _, d in m}) > 1 for _, _, m in sc.JOINS)
    rows, slots, ids = sc.lookup_pattern("b67_contended")
    assert all(int(ids[(rows == b).nonzero()[0]]) == sc.HOT for b in range(67))
    assert int(ids.min()) >= 1 and int(ids.max()) <= sc.N_INDEX


@pytest.mark.parametrize("name", ["b5_edges", "b67_mixed", "b67_contended", "b5_empty"])
def test_linear_oracles_match_dense_math(name):
    rows, cols, B = _folded(name)
    N = 3
    vals = sc.gauss((rows.numel(),), 1).double()
    W, bias, gy = sc.gauss((N, SMALL_D), 2).double(), sc.gauss((N,), 3).double(), sc.gauss((B, N), 4).double()
    X = sc.dense(rows, cols, vals, B, SMALL_D)
    y, a, n = sc.spmm_oracle(rows, cols, vals, W, bias, B)
    assert torch.allclose(y, X @ W.t() + bias, rtol=0, atol=1e-12)
    assert torch.allclose(a, X.abs() @ W.abs().t() + bias.abs(), rtol=0, atol=1e-12)
    assert torch.equal(n[:, 0], torch.bincount(rows, minlength=B).double() + 1)
    g, a, n = sc.wgrad_oracle(rows, cols, vals, gy, SMALL_D, 0.5)
    assert torch.allclose(g, 0.5 * gy.t() @ X, rtol=0, atol=1e-12)
    assert torch.equal(n[0], torch.bincount(cols, minlength=SMALL_D).double())
    s, a, n = sc.sddmm_oracle(rows, cols, gy, W)
    assert torch.allclose(s, (gy @ W)[rows, cols], rtol=0, atol=1e-12)


def test_oracles_skip_out_of_range_entries():
    rows = torch.tensor([0, 0, 1, 2, 5])
    cols = torch.tensor([1, 9, 3, 2, 0])          # column 9 == D and row 5 == B are out of range
    vals = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    keep = torch.tensor([True, False, True, True, False])
    W, gy = sc.gauss((2, 9), 1), sc.gauss((5, 2), 2)
    for full, cut in zip(sc.spmm_oracle(rows, cols, vals, W, None, 5),
                         sc.spmm_oracle(rows[keep], cols[keep], vals[keep], W, None, 5)):
        assert torch.equal(full, cut)
    assert torch.equal(sc.wgrad_oracle(rows, cols, vals, gy, 9)[0], sc.wgrad_oracle(rows[keep], cols[keep], vals[keep], gy, 9)[0])
    assert torch.equal(sc.sddmm_oracle(rows, cols, gy, W)[0][keep], sc.sddmm_oracle(rows[keep], cols[keep], gy, W)[0])
    ids = torch.tensor([0.0, 3.0, 4.0, 1.0, 2.0])     # id 0 and id nIndex + 1 = 4 are skipped
    T = sc.gauss((3, 4), 3)
    keep = torch.tensor([False, True, False, True, False])
    for comb in ("sum", "mean", "sqrtn"):
        full = sc.lookup_oracle(rows, ids, None, T, comb, 5)
        cut = sc.lookup_oracle(rows[keep], ids[keep], None, T, comb, 5)
        assert torch.equal(full[0], cut[0]) and torch.equal(full[1], cut[1])


@pytest.mark.parametrize("comb", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("weighted", [False, True])
def test_lookup_oracles_match_dense_math(comb, weighted):
    rows, slots, ids = sc.lookup_pattern("b67_mixed")
    B, L, nOut = 67, sc.LOOKUP_L, 5
    wts = sc.gauss((ids.numel(),), 5, positive=True) if weighted else None
    T, gy = sc.gauss((sc.N_INDEX, nOut), 6).double(), sc.gauss((B, nOut), 7).double()
    idd = sc.dense(rows, slots, ids, B, L).long()
    wd = sc.dense(rows, slots, torch.ones_like(ids) if wts is None else wts, B, L)
    emb = T[(idd - 1).clamp_min(0)] * wd.unsqueeze(-1)
    den = {"sum": torch.ones(B, dtype=torch.float64), "mean": wd.sum(1), "sqrtn": (wd * wd).sum(1).sqrt()}[comb]
    s = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
    out, scales, a, n = sc.lookup_oracle(rows, ids, wts, T, comb, B)
    assert torch.allclose(out, emb.sum(1) * s[:, None], rtol=0, atol=1e-12)
    if comb != "sum":
        assert torch.allclose(scales, s, rtol=1e-14, atol=0)
    g, a, n = sc.lookup_bwd_oracle(rows, ids, wts, scales, gy, sc.N_INDEX, 0.5)
    ref = torch.zeros(sc.N_INDEX, nOut, dtype=torch.float64)
    coef = wd * s[:, None]
    ref.index_add_(0, (idd - 1).clamp_min(0).reshape(-1), 0.5 * (coef.unsqueeze(-1) * gy.unsqueeze(1)).reshape(-1, nOut))
    assert torch.allclose(g, ref, rtol=0, atol=1e-12)
    assert torch.equal(n[:, 0], torch.bincount(ids.long() - 1, minlength=sc.N_INDEX).double())


@pytest.mark.parametrize("name", ["one", "two", "three_with_empty", "all_empty"])
def test_concat_oracle_matches_dense_cat(name):
    B, parts = sc.join_parts(name)
    rows, cols, vals = sc.concat_oracle(parts, B)
    ref = torch.cat([sc.sparse(r, c, v, B, D).to_dense() for r, c, v, D in parts], dim=1).to_sparse().coalesce()
    assert torch.equal(torch.stack([rows, cols]), ref._indices()) and torch.equal(vals, ref._values())


# ------------------------------------------------------------------------------------------------- torch forms
@pytest.mark.parametrize("name", ["b5_edges", "b67_contended", "b5_empty", "b67_d1"])
def test_torch_forms_match_the_oracles(name):
    c = sc.CASE[name]
    rows, cols = sc.pattern(name)
    N = 3
    vals, W = sc.gauss((c.nnz,), 11), sc.gauss((N, c.D), 12)
    bias, gy = sc.gauss((N,), 13), sc.gauss((c.B, N), 14)
    x = sc.sparse(rows, cols, vals, c.B, c.D)
    y, a, n = sc.spmm_oracle(rows, cols, vals, W, bias, c.B)
    got = sp.spmm(x, W, bias)
    assert sp.last_route("spmm") == "torch" and sp.last_route() == "torch"
    assert bool(((got.double() - y).abs() <= sc.bound(n, a)).all())
    g, a, n = sc.wgrad_oracle(rows, cols, vals, gy, c.D, 0.5)
    gW = torch.zeros(N, c.D)
    assert sp.spmm_wgrad(x, gy, gW, 0.5) is gW and sp.last_route("spmm_wgrad") == "torch"
    assert bool(((gW.double() - g).abs() <= sc.bound(n, a)).all())
    s, a, n = sc.sddmm_oracle(rows, cols, gy, W)
    got = sp.sddmm(x, gy, W)
    assert got.shape == (c.nnz,) and bool(((got.double() - s).abs() <= sc.bound(n, a)).all())


@pytest.mark.parametrize("comb", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("weighted", [False, True])
def test_lookup_torch_form_matches_the_oracle(comb, weighted):
    rows, slots, ids = sc.lookup_pattern("b67_contended")
    B, nOut = 67, 7
    wts = sc.gauss((ids.numel(),), 21, positive=True) if weighted else None
    T, gy = sc.gauss((sc.N_INDEX, nOut), 22), sc.gauss((B, nOut), 23)
    xi = sc.sparse(rows, slots, ids, B, sc.LOOKUP_L)
    xw = None if wts is None else sc.sparse(rows, slots, wts, B, sc.LOOKUP_L)
    out, scales, a, n = sc.lookup_oracle(rows, ids, wts, T, comb, B)
    got, got_s = sp.lookup_sparse(xi, xw, T, comb)
    assert sp.last_route("lookup_sparse") == "torch"
    assert bool(((got.double() - out).abs() <= sc.bound(n, a)).all())
    g, a, n = sc.lookup_bwd_oracle(rows, ids, wts, scales, gy, sc.N_INDEX, 0.5)
    gW = torch.zeros(sc.N_INDEX, nOut)
    sp.lookup_sparse_backward(xi, xw, got_s, gy, gW, 0.5)
    assert bool(((gW.double() - g).abs() <= 2 * sc.bound(n, a)).all())     # the forward's s_b is itself rounded


@pytest.mark.parametrize("name", ["one", "two", "three_with_empty"])
def test_concat_torch_form_matches_the_oracle(name):
    B, parts = sc.join_parts(name)
    rows, cols, vals = sc.concat_oracle(parts, B)
    got = sp.concat_cols([sc.sparse(r, c, v, B, D) for r, c, v, D in parts]).coalesce()
    assert sp.last_route("concat_cols") == "torch"
    assert tuple(got.shape) == (B, sum(D for _, _, _, D in parts))
    assert torch.equal(got._indices(), torch.stack([rows, cols])) and torch.equal(got._values(), vals)


def test_uncoalesced_input_is_coalesced_first():
    idx = torch.tensor([[1, 0, 1], [2, 1, 2]])
    x = torch.sparse_coo_tensor(idx, torch.tensor([1.0, 2.0, 3.0]), (2, 4))
    W = sc.gauss((3, 4), 31)
    assert torch.allclose(sp.spmm(x, W), x.to_dense() @ W.t())
    assert sp.Coo(x).nnz == 2


def test_switch_follows_the_decode_switch_idiom(monkeypatch):
    sp.set_native(None)
    monkeypatch.delenv("BIGDL_SPARSE_NATIVE", raising=False)
    assert sp.native_on(True) == sp.NATIVE_GPU_DEFAULT and sp.native_on(False) is False
    monkeypatch.setenv("BIGDL_SPARSE_NATIVE", "0")
    assert sp.native_on(True) is False
    monkeypatch.setenv("BIGDL_SPARSE_NATIVE", "1")
    assert sp.native_on(True) is True and sp.native_on(False) is False
    try:
        sp.set_native(False)
        assert sp.native_on(True) is False
        from bigdl_amd.utils.engine import Engine
        Engine.setProperty("bigdl.sparse.native", "true")
        assert sp.native_on(True) is True
    finally:
        sp.set_native(None)


# ------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("start,length", [(1, 4), (3, 5), (257 - 6, 7)])
def test_sparse_linear_backward_window(start, length):
    """With backwardStart / backwardLength set, gradInput is gradOutput @ W[:, start - 1 : start - 1 + length]
    (1-based start, reference SparseLinear.scala:84-100); the parameter gradients do not change."""
    rows, cols, B = _folded("b5_edges")
    vals = sc.gauss((rows.numel(),), 41)
    x = sc.sparse(rows, cols, vals, B, SMALL_D)
    m = nn.SparseLinear(SMALL_D, 3, backwardStart=start, backwardLength=length)
    plain = nn.SparseLinear(SMALL_D, 3)
    plain.weight.copy_(m.weight), plain.bias.copy_(m.bias)
    gy = sc.gauss((B, 3), 42)
    y, yp = m.forward(x), plain.forward(x)
    assert torch.equal(y, yp)
    gi, gip = m.backward(x, gy), plain.backward(x, gy)
    assert not gi.is_sparse and tuple(gi.shape) == (B, length)
    assert torch.allclose(gi, gy @ m.weight[:, start - 1:start - 1 + length], rtol=1e-6, atol=1e-6)
    assert gip.is_sparse and torch.equal(gip.coalesce()._indices(), x._indices())
    assert torch.allclose(gip.to_dense(), (gy @ m.weight) * (x.to_dense() != 0), rtol=1e-6, atol=1e-6)
    assert torch.equal(m.gradWeight, plain.gradWeight) and torch.equal(m.gradBias, plain.gradBias)
    assert torch.allclose(m.gradWeight, gy.t() @ x.to_dense(), rtol=1e-5, atol=1e-6)
    assert torch.allclose(m.gradBias, gy.sum(0), rtol=1e-6, atol=1e-6)


def test_sparse_linear_scales_and_dense_input():
    rows, cols, B = _folded("b67_contended")
    x = sc.sparse(rows, cols, sc.gauss((rows.numel(),), 51), B, SMALL_D)
    m = nn.SparseLinear(SMALL_D, 2)
    m.scaleW, m.scaleB = 0.5, 0.25
    gy = sc.gauss((B, 2), 52)
    m.forward(x)
    m.backward(x, gy)
    assert torch.allclose(m.gradWeight, 0.5 * gy.t() @ x.to_dense(), rtol=1e-5, atol=1e-6)
    assert torch.allclose(m.gradBias, 0.25 * gy.sum(0), rtol=1e-6, atol=1e-6)
    d = nn.SparseLinear(SMALL_D, 2)
    d.weight.copy_(m.weight), d.bias.copy_(m.bias)
    xd = x.to_dense()
    assert torch.allclose(d.forward(xd), m.forward(x), rtol=1e-5, atol=1e-6)
    gi = d.backward(xd, gy)
    assert torch.allclose(gi, gy @ d.weight, rtol=1e-5, atol=1e-6)
    assert torch.allclose(d.gradWeight, gy.t() @ xd, rtol=1e-5, atol=1e-6)


def test_lookup_table_sparse_grad_input_is_zero_on_the_pattern():
    rows, slots, ids = sc.lookup_pattern("b5_edges")
    xi = sc.sparse(rows, slots, ids, 5, sc.LOOKUP_L)
    xw = sc.sparse(rows, slots, sc.gauss((ids.numel(),), 61, positive=True), 5, sc.LOOKUP_L)
    m = nn.LookupTableSparse(sc.N_INDEX, 4, "mean")
    t = Table()
    t[1], t[2] = xi, xw
    out = m.forward(t)
    ref = sc.lookup_oracle(rows, ids, xw._values(), m.weight, "mean", 5)[0]
    assert torch.allclose(out.double(), ref, rtol=1e-5, atol=1e-6)
    gi = m.backward(t, sc.gauss((5, 4), 62))
    for k, src in ((1, xi), (2, xw)):
        assert gi[k].is_sparse and torch.equal(gi[k]._indices(), src._indices())
        assert int(gi[k]._values().count_nonzero()) == 0
    one = nn.LookupTableSparse(sc.N_INDEX, 4)
    one.forward(xi)
    g1 = one.backward(xi, sc.gauss((5, 4), 63))
    assert g1.is_sparse and torch.equal(g1._indices(), xi._indices()) and int(g1._values().count_nonzero()) == 0


def test_sparse_join_table_module_keeps_other_paths():
    B, parts = sc.join_parts("two")
    ts = [sc.sparse(r, c, v, B, D) for r, c, v, D in parts]
    t = Table()
    t[1], t[2] = ts
    got = nn.SparseJoinTable(2).forward(t)
    assert got.is_sparse and tuple(got.shape) == (B, sc.BIG_D + 1)
    rows, cols, vals = sc.concat_oracle(parts, B)
    assert torch.equal(got.coalesce()._indices(), torch.stack([rows, cols]))
    small = Table()
    small[1], small[2] = ts[1], ts[1]
    down = nn.SparseJoinTable(1).forward(small)           # dimension 1: today's dense path
    assert tuple(down.shape) == (2 * B, 1)
