"""ops.gemm on CPU tensors: the semantics of the dense bf16 GEMM (three forms, alpha / beta / bias / colsum, strided
views, the alignment rules) against a float64 expression, and the backend switch."""
import pytest
import torch

BF16 = torch.bfloat16


def _bf(*shape, scale=1.0):
    return (torch.randn(*shape) * scale).to(BF16)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_gemm_cpu_matches_float64(form):
    from bigdl_amd.ops.gemm import gemm

    torch.manual_seed(1)
    M, N, K = 40, 24, 72
    # operands are row-strided views cut from larger tensors
    if form == "nt":
        a, b = _bf(M, K + 8)[:, :K], _bf(N, K + 16)[:, :K]
        prod = a.double() @ b.double().t()
        kw = dict(trans_b=True)
    elif form == "nn":
        a, b = _bf(M, K + 8)[:, :K], _bf(K, N + 8)[:, :N]
        prod = a.double() @ b.double()
        kw = {}
    else:
        a, b = _bf(K, M + 8)[:, :M], _bf(K, N + 8)[:, :N]
        prod = a.double().t() @ b.double()
        kw = dict(trans_a=True)
    # plain product, fp32 result
    assert _rel(gemm(a, b, **kw), prod) < 1e-5
    # alpha, beta into a pre-filled strided fp32 out
    big = torch.randn(M, N + 8)
    out = big[:, :N]
    old = out.clone()
    r = gemm(a, b, out=out, alpha=0.5, beta=1.0, **kw)
    assert r is out
    assert _rel(out, 0.5 * prod + old.double()) < 1e-5
    if form != "tn":
        bias = torch.randn(N)
        y = gemm(a, b, out_dtype=BF16, bias=bias, **kw)
        assert y.dtype == BF16
        assert _rel(y, prod + bias.double()) < 4e-3
        with pytest.raises(ValueError):
            gemm(a, b, colsum=torch.zeros(M), **kw)
    else:
        cs = torch.randn(M)
        cs0 = cs.clone()
        gemm(a, b, colsum=cs, colscale=0.25, **kw)
        assert _rel(cs, cs0.double() + 0.25 * a.double().sum(0)) < 1e-5
        with pytest.raises(ValueError):
            gemm(a, b, bias=torch.zeros(N), **kw)


def test_gemm_fp32_inputs_are_rounded_to_bf16():
    from bigdl_amd.ops.gemm import gemm

    torch.manual_seed(2)
    a, b = torch.randn(16, 32), torch.randn(8, 32)
    ref = a.to(BF16).double() @ b.to(BF16).double().t()
    assert _rel(gemm(a, b, trans_b=True), ref) < 1e-5


def test_gemm_rule_errors():
    from bigdl_amd.ops.gemm import gemm

    a, b = _bf(16, 32), _bf(8, 32)
    with pytest.raises(ValueError):                       # TT form
        gemm(a, b, trans_a=True, trans_b=True)
    with pytest.raises(ValueError):                       # beta with a bf16 result
        gemm(a, b, trans_b=True, out=torch.zeros(16, 8, dtype=BF16), beta=1.0)
    with pytest.raises(ValueError, match="multiple of 8"):   # inner extent of 12
        gemm(_bf(16, 12), _bf(8, 12), trans_b=True)
    with pytest.raises(ValueError, match="multiple of 8"):   # leading dimension of 36
        gemm(_bf(16, 36)[:, :32], b, trans_b=True)
    with pytest.raises(ValueError):                       # reduction lengths differ
        gemm(a, _bf(8, 40), trans_b=True)


def test_gemm_backend_switch():
    from bigdl_amd.ops import gemm as G
    from bigdl_amd.utils.engine import Engine

    saved = G.backend()
    try:
        G.set_backend("native")
        assert G.backend() == "native"
        G.set_backend("blas")
        assert G.backend() == "blas"
        with pytest.raises(ValueError):
            G.set_backend("rocblas")
        assert G.backend() == "blas"
        Engine.setProperty("bigdl.gemm.backend", "native")
        assert G.backend() == "native"
        Engine.setProperty("bigdl.gemm.backend", "blas")
        assert G.backend() == "blas"
        with pytest.raises(ValueError):
            Engine.setProperty("bigdl.gemm.backend", "vendor")
    finally:
        G.set_backend(saved)


def test_gemm_backend_default_is_blas():
    import os
    import subprocess
    import sys

    env = {k: v for k, v in os.environ.items() if k != "BIGDL_GEMM_BACKEND"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, %r); from bigdl_amd.ops import gemm; print(gemm.backend())" % root
    out = subprocess.check_output([sys.executable, "-c", code], env=env, text=True)
    assert out.strip().splitlines()[-1] == "blas"
