"""Checks of tests/gemm_edge_cases.py itself, without a GPU: the exact oracles against fp64 torch.matmul on the same
integers, the exactness conditions of every exact case, the gb_split mirror against a hand-written table, the CPU tier
of ops.gemm.gemm against the exact leg, the guards, and the sensitivity of both legs on the cases' own inputs (a
planted single-element fault changes an exact result, and exceeds a rounded bound at least four times)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gemm_edge_cases as gc  # noqa: E402

BF16, F32 = gc.BF16, gc.F32
GB_ALL_EXACT = gc.GB_EXACT + gc.GB_SPLIT


def _ab(kind, c, p):
    """[.., M, K] and [.., K, N] operands of any case, as stored values in fp64 (x of a gemv as a column)."""
    if kind == "gb":
        a, b = gc.gb_ops(c, p["a"], p["b"])
        return a.double(), b.double()
    if kind == "bm":
        return p["a"].double().expand(c.batch, -1, -1), p["b"].double().expand(c.batch, -1, -1).transpose(1, 2)
    if kind == "gf":
        return p["a"].double(), p["b"].double().expand(c.batch, -1, -1)
    return p["a"].double(), p["x"].double()[:, None]


def _old(kind, c, p):
    """beta * old as the oracle takes it (fp64), or 0."""
    if kind == "gb":
        return c.beta * p["old"].double() if p["old"] is not None else 0.0
    if kind == "bm":
        return p["old"].double() if p["old"] is not None else 0.0
    o = p["mold"]
    if o is None:
        return 0.0
    return c.beta * (o.double()[:, None] if kind == "gv" else o.double())


_EXACT = ([("gb", c, gc.gb_problem) for c in GB_ALL_EXACT] + [("bm", c, gc.bm_problem) for c in gc.BM_EXACT]
          + [("gf", c, gc.gf_problem) for c in gc.GF_EXACT] + [("gv", c, gc.gv_problem) for c in gc.GV_EXACT])
_ROUNDED = ([("gb", c, gc.gb_problem) for c in gc.GB_ROUNDED] + [("bm", c, gc.bm_problem) for c in gc.BM_ROUNDED]
            + [("gf", c, gc.gf_problem) for c in gc.GF_ROUNDED] + [("gv", c, gc.gv_problem) for c in gc.GV_ROUNDED])
_ids = lambda t: f"{t[0]}-{t[1].id}"      # noqa: E731


# ------------------------------------------------------------------------------------------------- the cases file
def test_case_tables_cover_the_issue():
    for f in gc.FORMS:
        mine = [c for c in gc.GB_EXACT if c.form == f]
        assert {c.M for c in mine} >= set(gc.GB_EXTENTS) and {c.N for c in mine} >= set(gc.GB_EXTENTS)
        for K, nk in gc.GB_K_PIPE.items():
            assert (K + 63) // 64 == nk
            assert any((c.M, c.N, c.K) == (40, 24, K) for c in mine) and any((c.M, c.N, c.K) == (264, 264, K) for c in mine)
        assert {(c.M, c.N, c.K) for c in gc.GB_SPLIT if c.form == f} >= set(gc.GB_SPLIT_SHAPES)
        assert {c.alpha for c in mine} >= {1.0, 0.5, -2.0} and {c.beta for c in mine} >= {0.0, 1.0, 0.5}
        assert {c.layout for c in mine} == {"inside", "dense"} and {c.out for c in mine} == {"f32", "bf16"}
    assert {c.bias for c in gc.GB_EXACT if c.form != "tn"} == {"", "f32", "bf16"}
    assert {c.colscale for c in gc.GB_EXACT if c.form == "tn"} == {0.0, 1.0, 0.25}
    assert all(c.beta == 0.0 for c in GB_ALL_EXACT + gc.GB_ROUNDED if c.out == "bf16")
    assert all(not (c.bias and c.form == "tn") and not (c.colscale and c.form != "tn") for c in GB_ALL_EXACT + gc.GB_ROUNDED)
    assert all(c.K <= 8200 and c.M % 8 == 0 and c.N % 8 == 0 and c.K % 8 == 0 for c in GB_ALL_EXACT + gc.GB_ROUNDED)
    bm = gc.BM_EXACT
    assert {c.M for c in bm} >= set(gc.BM_EXTENTS) and {c.N for c in bm} >= set(gc.BM_EXTENTS)
    assert {c.K for c in bm} == set(gc.BM_KS) and {c.batch for c in bm} == {1, 3} and {c.bcast for c in bm} == {"", "a", "b"}
    assert {(c.alpha, c.accum) for c in bm} == {(1.0, False), (1.0, True), (0.5, False), (0.5, True)}
    gf = gc.GF_EXACT
    assert {c.M for c in gf} >= set(gc.GF_EXTENTS) and {c.N for c in gf} >= set(gc.GF_EXTENTS)
    assert {c.K for c in gf} == set(gc.GF_KS) and {c.batch for c in gf} == {1, 3}
    assert {c.min for c in gf} == {"", "full", "row", "inplace"} and any(c.bsb0 for c in gf)
    assert all(any(getattr(c, t) for c in gf) for t in ("ta", "tb", "tc"))
    assert {c.alpha for c in gf} == {1.0, 0.5, 0.0} and {c.beta for c in gf} >= {1.0, 0.5, 0.0}
    gv = gc.GV_EXACT
    assert {c.M for c in gv} == set(gc.GV_MS) and {c.K for c in gv} >= set(gc.GV_KS)
    assert any(c.ta for c in gv) and {c.sx for c in gv} >= {1, 3} and {c.sm for c in gv} == {0, 1, 2} and {c.sy for c in gv} >= {1, 2}
    assert all(c.K <= 264 for _, c, _ in _ROUNDED) and all(c.K <= 33 for c in gf) and all(c.K <= 160 for c in bm)


@pytest.mark.parametrize("case", _EXACT, ids=_ids)
def test_exact_oracle(case):
    kind, c, prob = case
    p = prob(c)
    A, B = _ab(kind, c, p)
    # the stored operands are the integers, none of them zero (the position-coded A aside)
    assert torch.equal(A, A.round()) and torch.equal(B, B.round())
    assert c.kind == "pos" or (bool((A != 0).all()) and bool((B != 0).all()))
    # any partial sum in any order is bounded by sum |a b| < 2^24
    assert (float((A.abs() @ B.abs()).max()) if A.numel() and B.numel() else 0.0) < 2 ** 24
    ref = c.alpha * (A @ B) + _old(kind, c, p)
    if kind == "gb" and p["bias"] is not None:
        ref = ref + p["bias"].double()
    want = p["want"].double()
    assert torch.equal(want, ref.view(want.shape))                  # the int64 oracle is the fp64 product
    assert torch.equal(want * 4, p["q"].double())                   # and the fp32 number holds it
    assert float(want.abs().max() if want.numel() else 0.0) < 2 ** 21
    if kind == "gb" and c.colscale:
        cs = p["want_cs"].double()
        assert torch.equal(cs, p["cs_old"].double() + c.colscale * A.sum(1)) and torch.equal(cs * 4, p["q_cs"].double())
    if c.kind == "pos":                                             # C is a row gather of B
        rows = torch.arange(c.M) % c.K
        assert torch.equal(A @ B, B[..., rows, :] if kind != "gv" else B[rows])


@pytest.mark.parametrize("shape", list(gc.GB_SPLIT_TABLE), ids=lambda s: "x".join(map(str, s)))
def test_gb_split_mirror(shape):
    nk, ns, per, last = gc.GB_SPLIT_TABLE[shape]
    assert (shape[2] + 63) // 64 == nk
    assert gc.gb_split(*shape) == (ns, per)
    sl = gc.gb_slices(*shape)
    assert len(sl) == ns and sl[0][0] == 0 and sl[-1][1] == shape[2]
    assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
    assert -(-(sl[-1][1] - sl[-1][0]) // 64) == last
    tiles = ((shape[0] + 255) // 256) * ((shape[1] + 255) // 256)
    assert gc.gb_ws_bytes(*shape) == (0 if ns == 1 else tiles * ns * (65536 + 256) * 4 + tiles * 4)


def test_matmul_problem_is_exact():
    for i in range(len(gc.MATMUL_CASES)):
        p = gc.matmul_problem(i)
        for k in ("out", "ga", "gb"):
            assert torch.equal(p[k].double(), p[k + "64"])
        assert torch.equal(p["out"], torch.matmul(p["a"], p["b"]))


def test_bf16_half_ulp_and_equal():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3)).double() * 100
    err = (x.float().to(BF16).double() - x).abs()
    hu = gc.bf16_half_ulp(x)
    assert bool((err <= hu).all()) and float((err / hu).max()) > 0.99
    assert float(gc.bf16_half_ulp(torch.tensor(1.0))) == 2.0 ** -8 and float(gc.bf16_half_ulp(torch.tensor(1.99))) == 2.0 ** -8
    assert float(gc.bf16_half_ulp(torch.tensor(0.0))) == 0.0
    a = torch.tensor([0.0, 1.0, -3.0], dtype=BF16)
    assert gc.bf16_equal(a, torch.tensor([-0.0, 1.0, -3.0], dtype=BF16))
    assert not gc.bf16_equal(a, torch.tensor([0.0, 1.0078125, -3.0], dtype=BF16))


def test_guard_sees_a_stray_store():
    for layout, shape, step in (("inside", (5, 12), 1), ("dense", (5, 16), 1), ("inside", (2, 3, 7), 1), ("inside", (6,), 3)):
        g = gc.guard(shape, F32, gc.SENTINEL, "cpu", layout, step=step).seal()
        assert tuple(g.view.shape) == shape
        g.view.fill_(1.0)
        assert g.ok()
        flat = g.buf.view(-1)
        inside = (flat == 1.0).nonzero().flatten()
        flat[int(inside[-1]) + 1] = 0.0                 # the element after the last one of the view
        assert not g.ok()
    g = gc.guard((4, 8), BF16, gc.NAN, "cpu").seal()    # NaN surrounds compare by bits
    assert g.ok() and g.view.stride(0) % 8 == 0 and g.view.stride(0) > 8


# -------------------------------------------------------------------------------- the CPU tier on the exact leg
@pytest.mark.parametrize("c", GB_ALL_EXACT, ids=lambda c: c.id)
def test_cpu_gemm_reproduces_the_exact_leg(c):
    from bigdl_amd.ops.gemm import gemm

    p = gc.gb_problem(c)
    a = gc.guard(p["a"].shape, BF16, gc.NAN, "cpu", c.layout, src=p["a"]).seal()
    b = gc.guard(p["b"].shape, BF16, gc.NAN, "cpu", c.layout, src=p["b"]).seal()
    out = gc.guard((c.M, c.N), BF16 if c.out == "bf16" else F32, gc.SENTINEL, "cpu", c.layout,
                   src=p["old"] if c.beta != 0.0 else torch.full((c.M, c.N), gc.NAN)).seal()
    cs = None
    if c.colscale:
        cs = gc.guard((c.M,), F32, gc.SENTINEL, "cpu", src=p["cs_old"]).seal()
    gemm(a.view, b.view, trans_a=c.form == "tn", trans_b=c.form == "nt", out=out.view, alpha=c.alpha, beta=c.beta,
         bias=p["bias"], colsum=cs.view if cs else None, colscale=c.colscale or 1.0)
    if c.out == "bf16":
        assert gc.bf16_equal(out.view, p["want"].to(BF16))
    else:
        assert torch.equal(out.view, p["want"])
    if cs:
        assert torch.equal(cs.view, p["want_cs"]) and cs.ok()
    assert a.ok() and b.ok() and out.ok()


# ---------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("case", _EXACT, ids=_ids)
def test_exact_leg_sees_single_faults(case):
    kind, c, prob = case
    if c.K == 0:                              # an empty sum has no term to lose
        return
    p = prob(c)
    A, B = _ab(kind, c, p)
    A, B = A.reshape(-1, *A.shape[-2:])[-1], B.reshape(-1, *B.shape[-2:])[-1]      # the last batch
    want = p["want"].reshape(-1, A.shape[0], B.shape[1])[-1].double()
    rest = want - c.alpha * (A @ B)
    f32 = lambda t: t.float().double()        # noqa: E731
    if c.alpha != 0.0 and c.kind != "pos":
        # one dropped term, at the last row, column and k (the corner next to every tail)
        Ad = A.clone()
        Ad[-1, -1] = 0.0
        got = f32(c.alpha * (Ad @ B) + rest)
        assert not torch.equal(got, want) and torch.equal(got[:-1], want[:-1])
        # one K-tile (64, or the whole of a shorter reduction) counted twice
        kt = slice(max(0, ((c.K - 1) // 64) * 64), c.K)
        assert not torch.equal(f32(want + c.alpha * (A[:, kt] @ B[kt])), want)
    if A.shape[0] > 1 and c.alpha != 0.0:           # (alpha = 0 leaves beta * M, whose rows a broadcast M makes equal)
        sw = want.clone()
        sw[[0, -1]] = want[[-1, 0]]
        assert not torch.equal(sw, want)                # two rows swapped
    if kind == "gb" and c.slices > 1:
        for k0, k1 in gc.gb_slices(c.M, c.N, c.K):      # any one slice left out
            assert not torch.equal(f32(want - c.alpha * (A[:, k0:k1] @ B[k0:k1])), want)
    if kind == "gb" and c.colscale and c.N > 256:       # tile column 1 adding its column sum as well
        cs = p["want_cs"].double()
        assert not torch.equal(f32(cs + c.colscale * A.sum(1)), cs)


def test_split_colsum_case_has_a_second_tile_column():
    c = gc.GB_SPLIT_COLSUM
    assert c.N > 256 and c.M > 256 and c.slices == 2 and c.K % 64 != 0


@pytest.mark.parametrize("case", _ROUNDED, ids=_ids)
def test_rounded_bound_sees_single_faults(case):
    kind, c, prob = case
    p = prob(c)
    A, B = _ab(kind, c, p)
    exact, b = p["exact"], p["bound"]
    assert exact.shape == b.shape and bool((b > 0).all())
    b2 = b.reshape(-1, A.shape[-2], B.shape[-1])
    # the element whose bound is the median of all bounds: dropping its median-magnitude term
    flat = b2.flatten()
    i = int(flat.argsort()[flat.numel() // 2])
    bt, m, n = (int(v) for v in torch.unravel_index(torch.tensor(i), b2.shape))
    Ab, Bb = A.reshape(-1, *A.shape[-2:]), B.reshape(-1, *B.shape[-2:])
    terms = (c.alpha * Ab[bt % Ab.shape[0], m, :] * Bb[bt % Bb.shape[0], :, n]).abs()
    med = float(terms.sort().values[terms.numel() // 2])
    assert med / float(flat[i]) >= 4.0, (med, float(flat[i]))
    # an fp32 result rounded to bf16 once
    if not (kind == "gb" and c.out == "bf16"):
        r, _ = gc.ratio(exact.float().to(BF16), exact, b)
        assert r >= 4.0, r
    if kind == "gb" and c.colscale:
        cb = p["bound_cs"]
        j = int(cb.argsort()[cb.numel() // 2])
        col = (c.colscale * A[:, j]).abs()
        assert float(col.sort().values[col.numel() // 2]) / float(cb[j]) >= 4.0
        assert gc.ratio(p["exact_cs"].float().to(BF16), p["exact_cs"], cb)[0] >= 4.0
