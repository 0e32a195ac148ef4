"""Fused depthwise-separable convolution (csrc/sepconv.hip): the launch itself against an fp64 reference, element by
element, and nn.SpatialSeparableConvolution / keras.SeparableConvolution2D on the fused route against the CPU engine."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# N, Cin, dm, Cout, H, W, (kH, kW), (sH, sW), (pH, pW), bias, mid16
FWD_CASES = [
    (1, 3, 1, 24, 9, 17, (3, 3), (1, 1), (1, 1), True, True),       # 9 x 17 output: both tile edges; Cmid 3 < one chunk
    (3, 20, 2, 136, 10, 10, (3, 3), (1, 1), (1, 1), True, True),    # Cmid 40: K tail; Cout 128 + 8: two Cout blocks
    (1, 8, 5, 24, 2, 3, (3, 3), (1, 1), (1, 1), False, False),      # map smaller than the halo; 16 x 8 tile; dm 5
    (1, 7, 3, 40, 11, 12, (5, 5), (2, 2), (2, 0), True, True),      # dm 3 (not a divisor of 32), stride 2, pad (2, 0)
    (1, 5, 1, 16, 6, 20, (1, 1), (1, 2), (0, 0), False, True),      # 1 x 1, stride (1, 2)
    (1, 4, 1, 8, 9, 9, (3, 1), (1, 1), (1, 0), True, False),        # 3 x 1
    (2, 6, 2, 24, 8, 21, (1, 5), (1, 2), (0, 2), False, True),      # 1 x 5
    (1, 70, 1, 24, 10, 10, (3, 3), (1, 1), (1, 1), True, True),     # 3 chunks: a stage buffer is reused; > 64 KiB LDS
    (8, 3, 1, 136, 64, 128, (3, 3), (1, 1), (1, 1), True, False),   # 512 tiles and Cout > 128: 256-channel blocks
]


@pytest.mark.parametrize("case", FWD_CASES)
def test_sepconv_fwd_matches_fp64(case):
    """|y - y64| <= (2^-9 + (Cmid + kH kW + 8) 2^-23) S per element, S = |wp| . (|wd| conv |x|) + |b| in fp64: the one
    bf16 rounding of mid (the point weight is bf16 already) plus fp32 accumulation over kH kW taps and Cmid channels.
    mid16 is the bf16 rounding of the fp32 depthwise sum: within one bf16 ulp (2^-7 relative) of the fp64 value.

    One bf16 rounding of mid would cost up to 2^-8 |mid| (8 significant bits), over the 2^-9 term, so the kernel feeds
    the GEMM bf16(mid) + bf16(mid - bf16(mid)); mid16 holds the first term."""
    from bigdl_amd.ops import native

    N, Cin, dm, Cout, H, W, (kH, kW), stride, pad, bias, want_mid = case
    Cmid, C8, C32, K8 = Cin * dm, -(-Cin * dm // 8) * 8, -(-Cin * dm // 32) * 32, -(-Cout // 8) * 8
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, Cin, H, W, generator=g)
    wd = torch.randn(Cmid, 1, kH, kW, generator=g) / (kH * kW) ** 0.5
    wp = (torch.randn(Cout, Cmid, generator=g) / Cmid ** 0.5).bfloat16()
    b = torch.randn(Cout, generator=g) if bias else None
    mid64 = F.conv2d(x.double(), wd.double(), None, stride, pad, 1, Cin)
    y64 = F.conv2d(mid64, wp.double().view(Cout, Cmid, 1, 1), b.double() if bias else None)
    smid = F.conv2d(x.double().abs(), wd.double().abs(), None, stride, pad, 1, Cin)
    S = F.conv2d(smid, wp.double().abs().view(Cout, Cmid, 1, 1), b.double().abs() if bias else None)
    OH, OW = y64.shape[2:]

    wp32 = torch.zeros(K8, C32, dtype=torch.bfloat16)
    wp32[:Cout, :Cmid] = wp
    y = torch.full((N, Cout, OH, OW), float("nan"), device="cuda")
    mid16 = torch.full((N, OH, OW, C8), float("nan"), dtype=torch.bfloat16, device="cuda") if want_mid else None
    native.get().sepconv_fwd(x.cuda(), wd.cuda(), wp32.cuda(), b.cuda() if bias else None, y, mid16,
                             [stride[0], stride[1], pad[0], pad[1]])
    if want_mid:
        m = mid16.cpu().double().permute(0, 3, 1, 2)
        assert bool((m[:, Cmid:] == 0).all())
        merr = (m[:, :Cmid] - mid64).abs()
        assert bool((merr <= 2.0 ** -7 * mid64.abs() + kH * kW * 2.0 ** -23 * smid + 1e-30).all()), merr.max().item()
    err = (y.cpu().double() - y64).abs()
    bound = (2.0 ** -9 + (Cmid + kH * kW + 8) * 2.0 ** -23) * S + 1e-30
    print(f"max |y - y64| / bound = {(err / bound).max().item():.4f}, NaN outputs: {int(y.isnan().sum())}")
    assert bool((err <= bound).all()), (err / bound).max().item()


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _module(name):
    from bigdl_amd import keras as K
    from bigdl_amd import nn

    if name == "nchw":
        return nn.SpatialSeparableConvolution(8, 24, 2, 3, 3, 1, 1, 1, 1), (2, 8, 10, 10)
    if name == "nhwc":
        return nn.SpatialSeparableConvolution(6, 20, 1, 3, 5, 2, 1, 1, 2, dataFormat="NHWC"), (2, 11, 9, 6)
    if name == "keras":
        return K.Sequential().add(K.SeparableConvolution2D(12, 3, 3, depthMultiplier=2, inputShape=(5, 9, 9))), (2, 5, 9, 9)
    return nn.SpatialSeparableConvolution(4, 8, 1, 9, 9, 1, 1, 4, 4), (2, 4, 12, 12)       # kernel 9: not taken


@pytest.mark.parametrize("name,route", [("nchw", "fused"), ("nhwc", "fused"), ("keras", "fused"), ("k9", "split")])
def test_separable_module_fused_matches_cpu_engine(name, route):
    from bigdl_amd.ops import conv_fn
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(5)
    cpu, shape = _module(name)
    gpu = copy.deepcopy(cpu).to("cuda")
    x = torch.randn(*shape).to(torch.bfloat16).float()
    yc = cpu.forward(x)
    gy = torch.randn_like(yc)
    gc = cpu.backward(x, gy)
    conv_fn.set_sepconv_fused(True)
    try:
        yg = gpu.forward(x.cuda())
        gg = gpu.backward(x.cuda(), gy.cuda())
    finally:
        conv_fn.set_sepconv_fused(None)
    assert conv_fn.last_separable_route() == route
    assert yg.shape == yc.shape
    assert _rel(yg, yc) < 1e-2, _rel(yg, yc)
    assert _rel(gg, gc) < 2e-2, _rel(gg, gc)
    grads_g, grads_c = gpu.parameters()[1], cpu.parameters()[1]
    assert len(grads_g) == 3
    for a, b in zip(grads_g, grads_c):
        assert _rel(a, b) < 2e-2, (a.shape, _rel(a, b))
