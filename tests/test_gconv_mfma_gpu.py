"""Grouped convolution on MFMA (csrc/gconv_mfma.hip): the three launches against fp64 (bit for bit on small integers,
per element on Gaussian data), the predicate, and nn.SpatialConvolution / conv_fn.group_conv2d on the route.

Measured max err / bound of the Gaussian cases: profiles/gconv_mfma_errors.txt."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF16, CL = torch.bfloat16, torch.channels_last

# N, G, cin_g, cout_g, H, W, (R, S), stride, pad, dilation
CASES = {
    "straddle8": (2, 4, 8, 8, 5, 7, (3, 3), (1, 1), (1, 1), (1, 1)),     # every 16-column block straddles two groups
    "cout24": (1, 3, 16, 24, 6, 6, (3, 3), (1, 1), (1, 1), (1, 1)),      # straddling at alternating offsets
    "red360": (3, 2, 40, 16, 10, 11, (3, 3), (1, 1), (1, 1), (1, 1)),    # stages straddle taps; 330 rows: tiles + tail
    "cout80": (1, 2, 32, 80, 4, 4, (3, 3), (1, 1), (1, 1), (1, 1)),      # a group spans two column tiles; column tail
    "stride2": (2, 2, 16, 16, 9, 6, (3, 3), (2, 2), (1, 1), (1, 1)),     # data-gradient phases; odd / even extents
    "1x1s2": (1, 2, 8, 16, 7, 7, (1, 1), (2, 2), (0, 0), (1, 1)),        # phases no tap reaches: zeros
    "dil2": (1, 2, 8, 8, 9, 9, (3, 3), (1, 1), (2, 2), (2, 2)),
    "5x3": (2, 2, 24, 8, 6, 5, (5, 3), (1, 2), (2, 1), (1, 1)),
    "split": None,   # straddle8 enlarged until the weight gradient splits its pixels (resolved in the test)
}


def _draw(shape, exact, lim, g):
    if exact:
        return torch.randint(-lim, lim + 1, shape, generator=g).double()
    return torch.randn(shape, generator=g).bfloat16().double()


def _check(name, got, ref, S, n, exact, extra=0.0):
    got = got.cpu().double()
    assert not got.isnan().any(), f"{name}: unwritten elements"
    if exact and extra == 0.0:   # fp32 results of integer data
        assert torch.equal(got, ref), f"{name}: {(got - ref).abs().max().item()}"
        return
    bound = (n + 8) * 2.0 ** -23 * S + extra * ref.abs() + 1e-30
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"{name}: max err / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: {ratio}"


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("case", list(CASES))
def test_gconv_mfma_launches_match_fp64(case, exact, bias):
    """Exact: integer data, fp32 results equal fp64 bit for bit. Gaussian: |err| <= (n + 8) 2^-23 S per element, n the
    reduction length and S the same sum over absolute values (plus |b|, plus the value accumulated into for the weight
    gradient); bf16 results add 2^-8 |ref|. The weight gradient accumulates into non-zero dw / db."""
    from bigdl_amd.ops import conv_fn, native

    C_ = native.get()
    tag = f"{case} {'exact' if exact else 'gauss'} {'bias' if bias else 'nobias'}"
    if case == "split":
        N, G, cin_g, cout_g, H, W, k, st, pd, dl = CASES["straddle8"]
        N = 4
        H = -(-C_.gconv_mfma_wgrad_split_min() // (N * W))
    else:
        N, G, cin_g, cout_g, H, W, k, st, pd, dl = CASES[case]
    C, K = G * cin_g, G * cout_g
    g = torch.Generator().manual_seed(7)
    x = _draw((N, C, H, W), exact, 2, g).requires_grad_(True)
    w = _draw((K, cin_g, *k), exact, 2, g).requires_grad_(True)
    b = _draw((K,), exact, 4, g) if bias else None
    y64 = F.conv2d(x, w, b, st, pd, dl, G)
    dy = _draw(tuple(y64.shape), exact, 2, g)
    gx64, gw64 = torch.autograd.grad(y64, (x, w), dy)
    xa, wa = x.detach().abs().requires_grad_(True), w.detach().abs().requires_grad_(True)
    Sy = F.conv2d(xa, wa, b.abs() if bias else None, st, pd, dl, G)
    Sgx, Sgw = torch.autograd.grad(Sy, (xa, wa), dy.abs())
    y64, Sy = y64.detach(), Sy.detach()
    dw0, db0 = _draw(tuple(w.shape), exact, 3, g), _draw((K,), exact, 3, g)

    geo = [st[0], st[1], pd[0], pd[1], dl[0], dl[1], G]
    x16 = x.detach().to(BF16).cuda().contiguous(memory_format=CL)
    w16 = w.detach().to(BF16).cuda().contiguous(memory_format=CL)
    dy16 = dy.to(BF16).cuda().contiguous(memory_format=CL)
    bg = b.float().cuda() if bias else None

    def nan(shape, dtype):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda").contiguous(memory_format=CL)

    nf, nd, npix = cin_g * k[0] * k[1], cout_g * k[0] * k[1], N * y64.shape[2] * y64.shape[3]
    for dtype, relu, extra in ((torch.float32, False, 0.0), (BF16, True, 2.0 ** -8)):
        y = nan(tuple(y64.shape), dtype)
        C_.gconv_mfma_fwd(x16, w16, bg, y, relu, geo)
        _check(f"{tag} fwd {dtype}", y, y64.relu() if relu else y64, Sy, nf, exact, extra)
        dx = nan(tuple(x.shape), dtype)
        C_.gconv_mfma_dgrad(dy16, conv_fn.group_transpose_w(w16, G), dx, geo)
        _check(f"{tag} dgrad {dtype}", dx, gx64, Sgx, nd, exact, extra)

    results = []
    for _ in range(2):
        dw = dw0.float().cuda().contiguous(memory_format=CL)
        db = db0.float().cuda() if bias else None
        splits = C_.gconv_mfma_wgrad_splits(dy16, x16, dw, geo)
        assert splits >= (2 if case == "split" else 1)
        ws = torch.full((splits * (dw.numel() + K),), float("nan"), device="cuda")
        C_.gconv_mfma_wgrad(dy16, x16, dw, db, ws, geo)
        results.append((dw, db))
    assert torch.equal(results[0][0], results[1][0]) and (not bias or torch.equal(results[0][1], results[1][1]))
    _check(f"{tag} wgrad", dw, dw0 + gw64, Sgw + dw0.abs(), npix, exact)
    if bias:
        _check(f"{tag} bgrad", db, db0 + dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)) + db0.abs(), npix, exact)


@pytest.mark.parametrize("C,K,G,pad", [(8, 16, 2, 1), (16, 24, 2, 1), (8, 8, 1, 1), (16, 16, 2, 3)],
                         ids=["cin_g4", "cout_g12", "G1", "pad3"])
def test_gconv_mfma_predicate(C, K, G, pad):
    from bigdl_amd.ops import native

    geo = [1, 1, pad, pad, 1, 1, G]
    assert not native.get().gconv_mfma_supported(1, C, 6, 6, K, 3, 3, geo)
    assert native.get().gconv_mfma_supported(1, 16, 6, 6, 16, 3, 3, [1, 1, 1, 1, 1, 1, 2])
    x = torch.zeros(1, C, 6, 6, dtype=BF16, device="cuda").contiguous(memory_format=CL)
    w = torch.zeros(K, C // G, 3, 3, dtype=BF16, device="cuda").contiguous(memory_format=CL)
    y = torch.zeros(1, K, 4 + 2 * pad, 4 + 2 * pad, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(RuntimeError):
        native.get().gconv_mfma_fwd(x, w, None, y, False, geo)


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _run_module(cpu, shape, switch):
    from bigdl_amd.ops import conv_fn

    gpu = copy.deepcopy(cpu).to("cuda")
    x = torch.randn(*shape).to(BF16).float()
    yc = cpu.forward(x)
    gy = torch.randn_like(yc)
    gc = cpu.backward(x, gy)
    conv_fn.set_gconv_mfma(switch)
    try:
        yg = gpu.forward(x.cuda())
        gg = gpu.backward(x.cuda(), gy.cuda())
        torch.cuda.synchronize()
    finally:
        conv_fn.set_gconv_mfma(None)
    assert _rel(yg, yc) < 1e-2, _rel(yg, yc)
    assert _rel(gg, gc) < 2e-2, _rel(gg, gc)
    for a, b in zip(gpu.parameters()[1], cpu.parameters()[1]):
        assert _rel(a, b) < 2e-2, (a.shape, _rel(a, b))
    return conv_fn.last_group_route()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("args,shape", [((64, 64, 3, 3, 1, 1, 1, 1, 2), (2, 64, 8, 8)),
                                        ((32, 64, 3, 3, 2, 2, 1, 1, 4), (2, 32, 9, 9))])
def test_grouped_module_on_mfma_matches_cpu_engine(args, shape, bias):
    from bigdl_amd import nn
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(5)
    assert _run_module(nn.SpatialConvolution(*args[:8], nGroup=args[8], withBias=bias), shape, True) == "mfma"


def test_grouped_module_other_routes():
    from bigdl_amd import nn
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(5)
    assert _run_module(nn.SpatialConvolution(16, 16, 3, 3, 1, 1, 1, 1, nGroup=16), (2, 16, 8, 8), True) == "direct"
    assert _run_module(nn.SpatialConvolution(64, 64, 3, 3, 1, 1, 1, 1, nGroup=2), (2, 64, 8, 8), False) == "loop"


def test_group_conv2d_function_on_mfma_matches_fp64():
    """bf16-representable inputs and fp32 results: only fp32 accumulation over at most 72 terms separates the function
    from fp64, (72 + 8) 2^-23 < 1e-5 per element relative to the sum of absolute values, so 1e-5 in relative norm."""
    from bigdl_amd.ops import conv_fn

    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 32, 9, 9, generator=g).bfloat16().float().requires_grad_(True)
    w = (torch.randn(64, 8, 3, 3, generator=g) / 8).bfloat16().float().requires_grad_(True)
    b = torch.randn(64, generator=g).requires_grad_(True)
    gy = torch.randn(2, 64, 5, 5, generator=g).bfloat16().float()
    ref = torch.autograd.grad(F.conv2d(x.double(), w.double(), b.double(), 2, 1, 1, 4), (x, w, b), gy.double())
    xg, wg, bg = (t.detach().cuda().requires_grad_(True) for t in (x, w, b))
    conv_fn.set_gconv_mfma(True)
    try:
        y = conv_fn.group_conv2d(xg, wg, bg, (2, 2), (1, 1), (1, 1), 4)
        got = torch.autograd.grad(y, (xg, wg, bg), gy.cuda())
    finally:
        conv_fn.set_gconv_mfma(None)
    assert conv_fn.last_group_route() == "mfma"
    assert _rel(y, F.conv2d(x, w, b, 2, 1, 1, 4).detach()) < 1e-5
    for a, r in zip(got, ref):
        assert _rel(a, r) < 1e-5, (a.shape, _rel(a, r))
