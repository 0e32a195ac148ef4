"""The matrix-product kernels against the oracles of tests/gemm_edge_cases.py, element by element:
gemm_bf16_kernel<0|1|2> (csrc/gemm_bf16.hip) through ops.gemm.gemm and native gemm_bf16, bmm_nt_kernel (csrc/bmm.hip)
through native bmm_nt and ops.bmm.matmul, gemm_f32_kernel / gemv_f32_kernel (csrc/tensor_math.hip) through their
bindings with explicit strides.

* exact legs: integer operands, the result compared with torch.equal (bf16 results bit for bit) against int64;
* rounded legs: |kernel - fp64| / bound per element, at most ``ALLOWED`` (twice the measured maximum, capped at the
  derivation's 1; profiles/gemm_edge_errors.txt);
* every launch: operands inside NaN, written tensors inside sentinels, both checked byte for byte afterwards; a
  result that is not accumulated into starts as NaN, so equality also says that no old value was read;
* only operands the bindings admit are launched; what they refuse is asserted to raise.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gemm_edge_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, NAN, SENTINEL = gc.BF16, gc.F32, gc.NAN, gc.SENTINEL
DEV = "cuda"
_id = lambda c: c.id      # noqa: E731


def _n():
    from bigdl_amd.ops import native

    return native.get()


def _report(leg, case, value):
    """One line per measured figure (pytest -s shows them; profiles/gemm_edge_errors.txt holds their maxima)."""
    print(f"GEMM|{leg}|{case}|{value:.4g}")
    return value


def _put(src, layout="inside", step=1):
    return gc.guard(src.shape, src.dtype, NAN, DEV, layout, src=src, step=step)


def _diff(got, want):
    """Where an exact comparison failed: count and the first few (index, got, want)."""
    bad = (got.double() != want.double()).nonzero()
    return f"{bad.shape[0]} of {want.numel()} differ: " + "; ".join(
        f"{tuple(i.tolist())} got {float(got[tuple(i)])} want {float(want[tuple(i)])}" for i in bad[:6])


def _same(got, want, what=""):
    if want.dtype == BF16:
        assert gc.bf16_equal(got, want), what + " " + _diff(got.float(), want.float())
    else:
        assert torch.equal(got, want), what + " " + _diff(got, want)


def _bounded(leg, case, got, exact, b):
    r, at = gc.ratio(got, exact, b)
    _report(leg, case, r)
    assert r <= gc.ALLOWED[leg] <= gc.CAP, (leg, case, r, at, float(got[at]), float(exact[at]))


# ====================================================================================================== gemm_bf16
def _run_gb(c, p, through="ops", ws=None):
    """One launch on guarded tensors; returns (out, colsum or None) on the CPU after checking every guard."""
    a, b = _put(p["a"], c.layout), _put(p["b"], c.layout)
    out = gc.guard((c.M, c.N), BF16 if c.out == "bf16" else F32, SENTINEL, DEV, c.layout,
                   src=p["old"] if c.beta != 0.0 else torch.full((c.M, c.N), NAN))
    bias = _put(p["bias"]) if c.bias else None
    cs = gc.guard((c.M,), F32, SENTINEL, DEV, src=p["cs_old"]) if c.colscale else None
    guards = [g.seal() for g in (a, b, out, bias, cs) if g is not None]
    bv, cv = (bias.view if bias else None), (cs.view if cs else None)
    if through == "ops":
        from bigdl_amd.ops.gemm import gemm

        r = gemm(a.view, b.view, trans_a=c.form == "tn", trans_b=c.form == "nt", out=out.view, alpha=c.alpha,
                 beta=c.beta, bias=bv, colsum=cv, colscale=c.colscale or 1.0)
        assert r is out.view
    else:
        _n().gemm_bf16(a.view, b.view, out.view, gc.FORMS.index(c.form), c.alpha, c.beta, bv, cv, c.colscale or 1.0, ws)
    torch.cuda.synchronize()
    assert all(g.ok() for g in guards), c.id
    return out.view.cpu(), (cs.view.cpu() if cs else None)


def _gb_check_exact(c, p, out, cs):
    _same(out, p["want"].to(BF16) if c.out == "bf16" else p["want"], c.id)
    if c.colscale:
        _same(cs, p["want_cs"], c.id + " colsum")


@pytest.mark.parametrize("c", gc.GB_EXACT, ids=_id)
def test_gemm_bf16_exact(c):
    assert gc.gb_split(c.M, c.N, c.K)[0] == 1 and _n().gemm_bf16_ws_bytes(gc.FORMS.index(c.form), c.M, c.N, c.K) == 0
    p = gc.gb_problem(c)
    _gb_check_exact(c, p, *_run_gb(c, p))


@pytest.mark.parametrize("c", gc.GB_SPLIT, ids=_id)
def test_gemm_bf16_split_exact_and_reproducible(c):
    assert _n().gemm_bf16_ws_bytes(gc.FORMS.index(c.form), c.M, c.N, c.K) == gc.gb_ws_bytes(c.M, c.N, c.K)
    assert (c.slices > 1) == ((c.M, c.N, c.K) != (8, 8, 960))
    p = gc.gb_problem(c)
    out, cs = _run_gb(c, p)
    _gb_check_exact(c, p, out, cs)
    out2, cs2 = _run_gb(c, p)                            # fresh outputs, fresh workspace
    assert torch.equal(gc._bits(out), gc._bits(out2))
    assert cs is None or torch.equal(gc._bits(cs), gc._bits(cs2))


@pytest.mark.parametrize("form", gc.FORMS)
@pytest.mark.parametrize("shape", list(gc.GB_SPLIT_TABLE), ids=lambda s: "x".join(map(str, s)))
def test_gemm_bf16_ws_bytes_mirror(form, shape):
    assert _n().gemm_bf16_ws_bytes(gc.FORMS.index(form), *shape) == gc.gb_ws_bytes(*shape)


@pytest.mark.parametrize("form", gc.FORMS)
def test_gemm_bf16_reused_workspace(form):
    """The tickets are zeroed per launch: one workspace, left full of NaN bits, serves a split launch, an unsplit
    one and the split one again; a workspace one element short, or none, raises before any launch."""
    big, many = gc.GB(form, 264, 264, 1024, alpha=-2.0, beta=0.5), gc.GB(form, 8, 8, 8200)
    small = gc.GB(form, 40, 24, 72)
    need = max(gc.gb_ws_bytes(c.M, c.N, c.K) for c in (big, many))
    ws = torch.full((need // 4,), NAN, dtype=F32, device=DEV)
    for c in (big, small, big, many, many):
        p = gc.gb_problem(c)
        _gb_check_exact(c, p, *_run_gb(c, p, through="native", ws=ws))
    p = gc.gb_problem(big)
    short = torch.zeros(gc.gb_ws_bytes(big.M, big.N, big.K) // 4 - 1, dtype=F32, device=DEV)
    a, b = p["a"].to(DEV), p["b"].to(DEV)
    out = torch.zeros(big.M, big.N, device=DEV)
    for bad in (short, None):
        with pytest.raises(RuntimeError, match="workspace"):
            _n().gemm_bf16(a, b, out, gc.FORMS.index(form), 1.0, 0.0, None, None, 1.0, bad)
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("c", gc.GB_ROUNDED, ids=_id)
def test_gemm_bf16_rounded(c):
    p = gc.gb_problem(c)
    out, cs = _run_gb(c, p)
    _bounded("gemm_bf16_" + c.out, c.id, out, p["exact"], p["bound"])
    if c.colscale:
        _bounded("gemm_bf16_colsum", c.id, cs, p["exact_cs"], p["bound_cs"])


@pytest.mark.parametrize("form", gc.FORMS)
@pytest.mark.parametrize("shape,at", [((72, 40, 136), (71, 39, 135)), ((264, 264, 72), (256, 255, 64)),
                                      ((8, 8, 1032), (7, 0, 1024))], ids=["72x40x136", "264x264x72", "8x8x1032"])
def test_gemm_bf16_planted_nan_and_inf(form, shape, at):
    """A NaN in one element of A reaches row m of C (and colsum[m]) and nothing else; +inf in one element of B reaches
    column n and nothing else."""
    m, n, k = at
    c = gc.GB(form, *shape, colscale=0.25 if form == "tn" else 0.0)
    base = gc.gb_problem(c)
    for which, val in (("a", NAN), ("b", float("inf"))):
        p = dict(base)
        t = base[which].clone()
        if which == "a":
            t[(k, m) if form == "tn" else (m, k)] = val
        else:
            t[(n, k) if form == "nt" else (k, n)] = val
        p[which] = t
        out, cs = _run_gb(c, p)
        hit = torch.zeros(c.M, c.N, dtype=torch.bool)
        if which == "a":
            hit[m] = True
            assert bool(out[m].isnan().all())
        else:
            hit[:, n] = True
            assert not bool(out[:, n].isfinite().any())
        assert torch.equal(out[~hit], base["want"][~hit]), _diff(out.nan_to_num(1e30, 2e30, 3e30) * ~hit, base["want"] * ~hit)
        if cs is not None:
            rows = torch.arange(c.M) != m
            assert torch.equal(cs[rows], base["want_cs"][rows]) and bool(cs[m].isnan()) == (which == "a")
            assert which == "a" or torch.equal(cs, base["want_cs"])


# ========================================================================================================= bmm_nt
def _run_bm(c, p):
    a, b = _put(p["a"], c.layout), _put(p["b"], c.layout)
    out = gc.guard((c.batch, c.M, c.N), F32, SENTINEL, DEV, c.layout,
                   src=p["old"] if c.accum else torch.full((c.batch, c.M, c.N), NAN))
    guards = [g.seal() for g in (a, b, out)]
    av, bv = a.view.expand(c.batch, -1, -1), b.view.expand(c.batch, -1, -1)
    assert av.stride(1) % 8 == 0 and bv.stride(1) % 8 == 0 and av.data_ptr() % 16 == 0 and bv.data_ptr() % 16 == 0
    assert av.stride(0) % 8 == 0 and bv.stride(0) % 8 == 0
    assert not c.bcast or (av if c.bcast == "a" else bv).stride(0) == 0
    _n().bmm_nt(av, bv, out.view, c.alpha, c.accum)
    torch.cuda.synchronize()
    assert all(g.ok() for g in guards), c.id
    return out.view.cpu()


@pytest.mark.parametrize("c", gc.BM_EXACT, ids=_id)
def test_bmm_nt_exact(c):
    p = gc.bm_problem(c)
    _same(_run_bm(c, p), p["want"], c.id)


@pytest.mark.parametrize("c", gc.BM_ROUNDED, ids=_id)
def test_bmm_nt_rounded(c):
    p = gc.bm_problem(c)
    _bounded("bmm_nt", c.id, _run_bm(c, p), p["exact"], p["bound"])


def test_bmm_nt_planted_nan_and_inf():
    c = gc.BM(33, 65, 96, batch=3, alpha=0.5)
    base = gc.bm_problem(c)
    for which, val, idx in (("a", NAN, (2, 32, 95)), ("b", float("inf"), (1, 64, 64))):
        p = dict(base)
        t = base[which].clone()
        t[idx] = val
        p[which] = t
        out = _run_bm(c, p)
        hit = torch.zeros(c.batch, c.M, c.N, dtype=torch.bool)
        if which == "a":
            hit[idx[0], idx[1]] = True
        else:
            hit[idx[0], :, idx[1]] = True
        assert not bool(out[hit].isfinite().any()) and torch.equal(out[~hit], base["want"][~hit])


def test_bmm_nt_rule_errors():
    C = _n()
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)      # noqa: E731
    c = z(1, 4, 4, dt=F32)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        C.bmm_nt(z(1, 4, 48), z(1, 4, 48), c)
    with pytest.raises(RuntimeError):                                   # lda % 8 != 0
        C.bmm_nt(z(1, 4, 36)[:, :, :32], z(1, 4, 32), c)
    with pytest.raises(RuntimeError):                                   # ldb % 8 != 0
        C.bmm_nt(z(1, 4, 32), z(1, 4, 36)[:, :, :32], c)
    torch.cuda.synchronize()
    assert not c.any()


@pytest.mark.parametrize("i", range(len(gc.MATMUL_CASES)), ids=lambda i: "x".join(map(str, gc.MATMUL_CASES[i][0])))
def test_matmul_layer_exact(i):
    """ops.bmm.matmul, forward and both gradients, on small integers: the zero padding of K and the bf16 cast lose
    nothing, so all three are exact."""
    from bigdl_amd.ops.bmm import matmul

    p = gc.matmul_problem(i)
    a, b = p["a"].to(DEV).requires_grad_(True), p["b"].to(DEV).requires_grad_(True)
    out = matmul(a, b)
    out.backward(p["g"].to(DEV))
    torch.cuda.synchronize()
    _same(out.detach().cpu(), p["out"], "forward")
    _same(a.grad.cpu(), p["ga"], "grad a")
    _same(b.grad.cpu(), p["gb"], "grad b")


# ============================================================================================= gemm_f32 / gemv_f32
def _run_gf(c, p):
    def stored(src, t):              # a guarded tensor addressed as src's shape, stored transposed when t
        g = _put(src.transpose(1, 2).contiguous() if t else src)
        return g, (g.view.transpose(1, 2) if t else g.view)

    ga, A = stored(p["a"], c.ta)
    gb, B = stored(p["b"], c.tb)
    B = B.expand(c.batch, -1, -1)
    shape = (c.batch, c.M, c.N)
    start = p["mold"] if c.min == "inplace" else torch.full(shape, NAN)
    gC = gc.guard((c.batch, c.N, c.M) if c.tc else shape, F32, SENTINEL, DEV,
                  src=start.transpose(1, 2) if c.tc else start)
    C = gC.view.transpose(1, 2) if c.tc else gC.view
    guards, Min = [ga, gb, gC], None
    if c.min == "inplace":
        Min = C
    elif c.min:
        mold = p["mold"] if c.beta != 0.0 else torch.full_like(p["mold"], NAN)       # beta = 0 must not read M
        gm = _put(mold)
        guards.append(gm)
        Min = gm.view[None, None, :].expand(*shape) if c.min == "row" else gm.view
    for g in guards:
        g.seal()
    s = [A.stride(1), A.stride(2), B.stride(1), B.stride(2), C.stride(1), C.stride(2),
         Min.stride(1) if c.min else 0, Min.stride(2) if c.min else 0,
         A.stride(0), 0 if c.bsb0 else B.stride(0), C.stride(0), Min.stride(0) if c.min else 0]
    assert (c.min != "row") or s[6] == 0
    _n().gemm_f32(A, B, Min, C, c.batch, c.M, c.N, c.K, s, c.alpha, c.beta)
    torch.cuda.synchronize()
    assert all(g.ok() for g in guards), c.id
    return C.cpu()


@pytest.mark.parametrize("c", gc.GF_EXACT, ids=_id)
def test_gemm_f32_exact(c):
    p = gc.gf_problem(c)
    _same(_run_gf(c, p), p["want"], c.id)


@pytest.mark.parametrize("c", gc.GF_ROUNDED, ids=_id)
def test_gemm_f32_rounded(c):
    p = gc.gf_problem(c)
    _bounded("gemm_f32", c.id, _run_gf(c, p), p["exact"], p["bound"])


def test_gemm_f32_planted_nan_and_inf():
    c = gc.GF(65, 33, 17, batch=3, ta=True, alpha=0.5)
    base = gc.gf_problem(c)
    for which, val, idx in (("a", NAN, (2, 64, 16)), ("b", float("inf"), (1, 16, 32))):
        p = dict(base)
        t = base[which].clone()
        t[idx] = val
        p[which] = t
        out = _run_gf(c, p)
        hit = torch.zeros(c.batch, c.M, c.N, dtype=torch.bool)
        if which == "a":
            hit[idx[0], idx[1]] = True
        else:
            hit[idx[0], :, idx[2]] = True
        assert not bool(out[hit].isfinite().any()) and torch.equal(out[~hit], base["want"][~hit])


def _run_gv(c, p):
    ga = _put(p["a"].t().contiguous() if c.ta else p["a"])
    A = ga.view.t() if c.ta else ga.view
    gx = _put(p["x"], step=c.sx)
    gy = gc.guard((c.M,), F32, SENTINEL, DEV, src=torch.full((c.M,), NAN), step=c.sy)
    guards, Min = [ga, gx, gy], None
    if c.sm:
        gm = _put(p["mold"] if c.beta != 0.0 else torch.full_like(p["mold"], NAN), step=c.sm)
        guards.append(gm)
        Min = gm.view
    for g in guards:
        g.seal()
    s = [A.stride(0), A.stride(1), gx.view.stride(0) if c.K else c.sx, Min.stride(0) if c.sm else 0, gy.view.stride(0)]
    assert s[2:] == [c.sx, c.sm, c.sy] or c.M == 1
    _n().gemv_f32(A, gx.view, Min, gy.view, c.M, c.K, s, c.alpha, c.beta)
    torch.cuda.synchronize()
    assert all(g.ok() for g in guards), c.id
    return gy.view.cpu()


@pytest.mark.parametrize("c", gc.GV_EXACT, ids=_id)
def test_gemv_f32_exact(c):
    p = gc.gv_problem(c)
    _same(_run_gv(c, p), p["want"], c.id)


@pytest.mark.parametrize("c", gc.GV_ROUNDED, ids=_id)
def test_gemv_f32_rounded(c):
    p = gc.gv_problem(c)
    _bounded("gemv_f32", c.id, _run_gv(c, p), p["exact"], p["bound"])


def test_gemv_f32_planted_nan_and_inf():
    c = gc.GV(9, 65, ta=True, sx=2, sy=2)
    base = gc.gv_problem(c)
    p = dict(base)
    p["a"] = base["a"].clone()
    p["a"][8, 64] = NAN
    out = _run_gv(c, p)
    assert bool(out[8].isnan()) and torch.equal(out[:8], base["want"][:8])
    p = dict(base)
    p["x"] = base["x"].clone()
    p["x"][64] = float("inf")                           # x feeds every row
    assert not bool(_run_gv(c, p).isfinite().any())
