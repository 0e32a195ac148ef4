"""The dense bf16 GEMM kernel (csrc/gemm_bf16.hip) through ops.gemm, forms NT / NN / TN.

Inputs are random values rounded to bf16; the reference is a float64 product of those values on the CPU. Every
operand and result is an interior slice of a larger buffer: operands are surrounded by NaN (a load past an extent
poisons the result), results by a sentinel whose bits must not change (an out-of-range store shows up without a
fault).

Tolerances (relative Frobenius error): fp32 result < 1e-4 (fp32 accumulation of K <= 8200 terms of random sign is
about sqrt(K) * 2^-24 = 5e-6; one wrong row of a 264-row result is 6e-2); bf16 result < 4e-3 (one rounding to bf16
is at most 2^-9 = 2e-3 relative).

The TN form's first operand is [P, M] with M its contiguous inner extent, which the kernel's rules want a multiple
of 8: the degenerate table row (1, 8, 8) is run as written for NT / NN; for TN it must raise ValueError, and the
smallest TN problem the rules admit, (8, 8, 1) with a reduction of length one, is run instead.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FORMS = ["nt", "nn", "tn"]
SHAPES = [(40, 24, 8), (256, 256, 128), (256, 256, 320), (264, 520, 200), (256, 256, 8200), (512, 256, 4104),
          (1, 8, 8)]
SPLIT = [(256, 256, 8200), (512, 256, 4104)]
SENTINEL = -1234.5
PAD_R, PAD_C = 3, 8          # rows / columns of surround (columns: a multiple of 8 keeps the rule on leading dims)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _inside(rows, cols, fill, dtype, gen=None):
    """A [rows, cols] interior view of a larger GPU buffer pre-filled with ``fill``; returns (view, buffer)."""
    big = torch.full((rows + 2 * PAD_R, cols + 2 * PAD_C), fill, dtype=dtype, device="cuda")
    view = big[PAD_R:PAD_R + rows, PAD_C:PAD_C + cols]
    if gen is not None:
        view.copy_(gen)
    return view, big


def _surround_unchanged(big, rows, cols, fill):
    ref = torch.full_like(big, fill)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[PAD_R:PAD_R + rows, PAD_C:PAD_C + cols] = False
    return torch.equal(big[mask].view(torch.int16 if big.dtype == BF16 else torch.int32),
                       ref[mask].view(torch.int16 if big.dtype == BF16 else torch.int32))


_CACHE = {}


def _problem(form, M, N, K):
    """bf16 operands (CPU) and the float64 product, computed once per (form, shape)."""
    key = (form, M, N, K)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(FORMS.index(form) * 1000003 + M * 7919 + N * 104729 + K)
        sa = (K, M) if form == "tn" else (M, K)
        sb = (N, K) if form == "nt" else (K, N)
        a = torch.randn(*sa, generator=g).to(BF16)
        b = torch.randn(*sb, generator=g).to(BF16)
        ad = a.double().t() if form == "tn" else a.double()
        bd = b.double().t() if form == "nt" else b.double()
        _CACHE[key] = (a, b, ad @ bd)
    return _CACHE[key]


def _kw(form):
    return {"nt": dict(trans_b=True), "nn": {}, "tn": dict(trans_a=True)}[form]


def _operands(form, M, N, K):
    a, b, prod = _problem(form, M, N, K)
    av, _ = _inside(a.shape[0], a.shape[1], float("nan"), BF16, a.cuda())
    bv, _ = _inside(b.shape[0], b.shape[1], float("nan"), BF16, b.cuda())
    return av, bv, prod


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_fp32(form, shape):
    from bigdl_amd.ops.gemm import gemm

    M, N, K = shape
    if form == "tn" and M % 8:
        a = torch.zeros(K, 8, dtype=BF16, device="cuda")[:, :M]
        with pytest.raises(ValueError, match="multiple of 8"):
            gemm(a, torch.zeros(K, N, dtype=BF16, device="cuda"), trans_a=True)
        M, N, K = 8, 8, 1
    av, bv, prod = _operands(form, M, N, K)
    out, big = _inside(M, N, SENTINEL, torch.float32)
    r = gemm(av, bv, out=out, **_kw(form))
    torch.cuda.synchronize()
    assert r is out
    err = _rel(out, prod)
    print(f"gemm fp32 {form} {M}x{N}x{K}: rel err {err:.3e}")
    assert err < 1e-4
    assert _surround_unchanged(big, M, N, SENTINEL)
    if shape in SPLIT:      # the split reduction is combined in slice order: bitwise reproducible
        from bigdl_amd.ops import native

        assert native.get().gemm_bf16_ws_bytes(FORMS.index(form), M, N, K) > 0
        out2, _ = _inside(M, N, SENTINEL, torch.float32)
        gemm(av, bv, out=out2, **_kw(form))
        torch.cuda.synchronize()
        assert torch.equal(out, out2)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [(264, 520, 200), (512, 256, 4104)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_alpha_beta(form, shape):
    from bigdl_amd.ops.gemm import gemm

    M, N, K = shape
    av, bv, prod = _operands(form, M, N, K)
    old = torch.randn(M, N, generator=torch.Generator().manual_seed(11)) * 30
    big = torch.full((M + 2 * PAD_R, N + 2 * PAD_C), SENTINEL, dtype=torch.float32, device="cuda")
    out = big[PAD_R:PAD_R + M, PAD_C:PAD_C + N]
    out.copy_(old)
    gemm(av, bv, out=out, alpha=0.5, beta=1.0, **_kw(form))
    torch.cuda.synchronize()
    err = _rel(out, 0.5 * prod + old.double())
    print(f"gemm alpha/beta {form} {M}x{N}x{K}: rel err {err:.3e}")
    assert err < 1e-4
    assert _surround_unchanged(big, M, N, SENTINEL)


@pytest.mark.parametrize("form", ["nt", "nn"])
@pytest.mark.parametrize("bias_dtype", [torch.float32, BF16], ids=["bias32", "bias16"])
@pytest.mark.parametrize("shape", [(40, 24, 8), (264, 520, 200), (256, 256, 8200)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_bf16_out_with_bias(form, bias_dtype, shape):
    from bigdl_amd.ops.gemm import gemm

    M, N, K = shape
    av, bv, prod = _operands(form, M, N, K)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(12)) * 4).to(bias_dtype)
    out, big = _inside(M, N, SENTINEL, BF16)
    gemm(av, bv, out=out, bias=bias.cuda(), **_kw(form))
    torch.cuda.synchronize()
    err = _rel(out, prod + bias.double())
    print(f"gemm bf16 out + bias {form} {M}x{N}x{K}: rel err {err:.3e}")
    assert err < 4e-3
    assert _surround_unchanged(big, M, N, SENTINEL)
    # fp32 result with the same bias: the bias is added before any rounding
    o32 = gemm(av, bv, bias=bias.cuda(), **_kw(form))
    assert _rel(o32, prod + bias.double()) < 1e-4


@pytest.mark.parametrize("shape", [(40, 24, 8), (264, 520, 200), (256, 256, 8200), (512, 256, 4104)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_tn_colsum(shape):
    from bigdl_amd.ops.gemm import gemm

    M, N, K = shape
    av, bv, prod = _operands("tn", M, N, K)
    a = _problem("tn", M, N, K)[0]
    cs0 = torch.randn(M, generator=torch.Generator().manual_seed(13)) * 10
    csbig = torch.full((M + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    cs = csbig[8:8 + M]
    cs.copy_(cs0)
    out, big = _inside(M, N, SENTINEL, torch.float32)
    gemm(av, bv, trans_a=True, out=out, colsum=cs, colscale=0.25)
    torch.cuda.synchronize()
    e1, e2 = _rel(out, prod), _rel(cs, cs0.double() + 0.25 * a.double().sum(0))
    print(f"gemm tn colsum {M}x{N}x{K}: rel err {e1:.3e}, colsum {e2:.3e}")
    assert e1 < 1e-4 and e2 < 1e-4
    assert _surround_unchanged(big, M, N, SENTINEL)
    edge = torch.cat([csbig[:8], csbig[8 + M:]]).cpu()
    assert torch.equal(edge.view(torch.int32), torch.full((16,), SENTINEL).view(torch.int32))
    if shape in SPLIT:
        cs2 = cs0.cuda()
        out2 = torch.empty(M, N, device="cuda")
        gemm(av, bv, trans_a=True, out=out2, colsum=cs2, colscale=0.25)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(cs, cs2)


def test_gemm_gpu_rule_errors():
    from bigdl_amd.ops.gemm import gemm

    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device="cuda")      # noqa: E731
    with pytest.raises(ValueError):
        gemm(z(16, 32), z(32, 8), trans_a=True, trans_b=True)
    with pytest.raises(ValueError):
        gemm(z(16, 32), z(8, 32), trans_b=True, out=z(16, 8), beta=1.0)
    with pytest.raises(ValueError, match="multiple of 8"):
        gemm(z(16, 12), z(8, 12), trans_b=True)
    with pytest.raises(ValueError, match="16-byte"):
        gemm(z(16, 40)[:, 4:36], z(8, 32), trans_b=True)
