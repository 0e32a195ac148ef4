"""The ``native`` GEMM backend (ops/gemm.py) behind nn.Linear and the whole-sequence LSTM / GRU recurrent weight
gradients: the in-tree dense bf16 GEMM runs (torch's matmuls are patched to raise), computes what the fp32 reference
and the hipBLASLt route compute, accumulates on a second backward, honours scaleW / scaleB, and is bitwise
reproducible in deterministic mode. Tolerances are those of tests/test_linear_blas_gpu.py."""
import contextlib
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

M, K, N = 8192, 512, 2048          # the smallest shape the Linear route rule admits


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@contextlib.contextmanager
def _backend(name, deterministic=None):
    from bigdl_amd.ops import gemm as G
    from bigdl_amd.ops import native

    saved, saved_det = G.backend(), native.deterministic()
    try:
        G.set_backend(name)
        if deterministic is not None:
            native.set_deterministic(deterministic)
        yield
    finally:
        G.set_backend(saved)
        native.set_deterministic(saved_det)


@contextlib.contextmanager
def _linears_on_conv_kernels():
    """Keep every Linear (the cells' input projections) on the conv kernels under both backends, so that only the
    recurrent weight-gradient route differs between the two runs and the input gradient can be compared exactly."""
    from bigdl_amd.nn import linear as L

    saved = L._BLAS[0]
    L._BLAS[0] = False
    try:
        yield
    finally:
        L._BLAS[0] = saved


@contextlib.contextmanager
def _no_vendor_gemm():
    def boom(*a, **k):
        raise AssertionError("a vendor GEMM was called under the native backend")

    saved = torch.mm, torch.addmm, torch.matmul
    torch.mm = torch.addmm = torch.matmul = boom
    try:
        yield
    finally:
        torch.mm, torch.addmm, torch.matmul = saved


_DATA = {}


def _data():
    if not _DATA:
        from bigdl_amd import nn

        torch.manual_seed(3)
        _DATA["x"] = (torch.randn(M, K) * 0.5).to(torch.bfloat16).float()
        _DATA["gy"] = (torch.randn(M, N) * 0.1).to(torch.bfloat16).float()
        _DATA["ref"] = nn.Linear(K, N, withBias=True)
    return _DATA["x"], _DATA["gy"], _DATA["ref"]


def _module(ref, bias):
    from bigdl_amd import nn

    m = nn.Linear(K, N, withBias=bias)
    m.weight.data.copy_(ref.weight.data)
    if bias:
        m.bias.data.copy_(ref.bias.data)
    return m.to("cuda")


def _grads(m, bias):
    return m.gradWeight.float().cpu().clone(), (m.gradBias.float().cpu().clone() if bias else None)


@pytest.mark.parametrize("bias", [True, False])
def test_linear_native_route(bias):
    x, gy, ref = _data()
    xg, gg = x.cuda(), gy.cuda()
    with _backend("blas"):
        mb = _module(ref, bias)
        yb = mb.forward(xg)
        assert getattr(mb, "_xe", None) is not None, "blas route"
        gib = mb.backward(xg, gg)
        torch.cuda.synchronize()
        gwb, gbb = _grads(mb, bias)
    with _backend("native"):
        m = _module(ref, bias)
        with _no_vendor_gemm():
            y = m.forward(xg)
            assert getattr(m, "_xn", None) is not None and getattr(m, "_xe", None) is None, "native route"
            gi = m.backward(xg, gg)
            torch.cuda.synchronize()
        gw, gb = _grads(m, bias)
        with _no_vendor_gemm():         # a second backward into the same module doubles the gradients (beta = 1)
            m.forward(xg)
            m.backward(xg, gg)
            torch.cuda.synchronize()
        gw2, gb2 = _grads(m, bias)
    w = ref.weight.data.to(torch.bfloat16).float()
    y_ref = x @ w.t() + (ref.bias.data if bias else 0)
    errs = {"y": (_rel(y, y_ref), _rel(y, yb)), "gi": (_rel(gi, gy @ w), _rel(gi, gib)),
            "gw": (_rel(gw, gy.t() @ x), _rel(gw, gwb))}
    if bias:
        errs["gb"] = (_rel(gb, gy.sum(0)), _rel(gb, gbb))
    print("linear native route (vs fp32 reference, vs blas):", {k: tuple(f"{e:.2e}" for e in v) for k, v in errs.items()})
    assert y.dtype == yb.dtype and gi.dtype == gib.dtype
    assert max(errs["y"]) < 1e-2 and max(errs["gi"]) < 1e-2
    assert max(errs["gw"]) < 1e-3
    assert _rel(gw2, 2 * gw) < 1e-6
    if bias:
        assert max(errs["gb"]) < 1e-3
        assert _rel(gb2, 2 * gb) < 1e-6


def test_linear_native_route_scales():
    x, gy, ref = _data()
    xg, gg = x.cuda(), gy.cuda()
    with _backend("native"):
        m = _module(ref, True)
        m.scaleW, m.scaleB = 0.5, 2.0
        with _no_vendor_gemm():
            m.forward(xg)
            m.backward(xg, gg)
            torch.cuda.synchronize()
        gw, gb = _grads(m, True)
    assert _rel(gw, 0.5 * (gy.t() @ x)) < 1e-3
    assert _rel(gb, 2.0 * gy.sum(0)) < 1e-3


def test_linear_native_route_deterministic():
    x, gy, ref = _data()
    xg, gg = x.cuda(), gy.cuda()
    runs = []
    with _backend("native", deterministic=True):
        for _ in range(2):
            m = _module(ref, True)
            with _no_vendor_gemm():
                y = m.forward(xg)
                assert getattr(m, "_xn", None) is not None, "native route in deterministic mode"
                gi = m.backward(xg, gg)
                torch.cuda.synchronize()
            runs.append((y.cpu(), gi.cpu()) + _grads(m, True))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_lstm_recurrent_weight_gradient_native_route():
    from bigdl_amd import nn
    from bigdl_amd.nn import recurrent as R

    torch.manual_seed(5)
    B, T, H = 64, 128, 512
    base = nn.Recurrent().add(nn.LSTM(H, H))
    x = (torch.randn(B, T, H) * 0.5).cuda()
    gy = (torch.randn(B, T, H) * 0.1).cuda()
    res = {}
    for name in ("native", "blas"):
        with _backend(name), _linears_on_conv_kernels():
            assert R._recurrent_wgrad_native(B * T, H) == (name == "native")
            m = copy.deepcopy(base).cuda()
            m.training()
            m.forward(x)
            gi = m.backward(x, gy)
            torch.cuda.synchronize()
            res[name] = (gi.float().cpu(), m.cell.h2g.gradWeight.float().cpu().clone())
    assert torch.equal(res["native"][0], res["blas"][0])      # the input gradient does not depend on the route
    err = _rel(res["native"][1], res["blas"][1])
    print(f"lstm dU native vs blas: {err:.2e}")
    assert err < 1e-5                                           # fp32 accumulation both ways: summation order only


def test_gru_recurrent_weight_gradient_native_route():
    from bigdl_amd import nn, ops
    from bigdl_amd.nn import recurrent as R

    B, T, H = 64, 128, 1024
    if not ops.native.get().gru_seq_supported(B, H):
        pytest.skip("whole-sequence GRU not available for this shape")
    torch.manual_seed(6)
    base = nn.Recurrent().add(nn.GRU(H, H))
    x = (torch.randn(B, T, H) * 0.5).cuda()
    gy = (torch.randn(B, T, H) * 0.1).cuda()
    res = {}
    for name in ("native", "blas"):
        with _backend(name), _linears_on_conv_kernels():
            assert R._recurrent_wgrad_native(B * T, H, 2 * H) == (name == "native")
            assert not R._recurrent_wgrad_native(B * T, H, H)
            m = copy.deepcopy(base).cuda()
            m.training()
            m.forward(x)
            gi = m.backward(x, gy)
            torch.cuda.synchronize()
            res[name] = (gi.float().cpu(), m.cell.h2g.gradWeight.float().cpu().clone(),
                         m.cell.h2n.gradWeight.float().cpu().clone())
    errs = [_rel(res["native"][i], res["blas"][i]) for i in range(3)]
    print("gru native vs blas (gi, dUrz, dUn):", [f"{e:.2e}" for e in errs])
    assert errs[0] < 1e-6
    assert errs[1] < 1e-5
    assert errs[2] < 1e-5
