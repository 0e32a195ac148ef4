"""Compact gradient of a 1x1 / stride-2 projection shortcut (ops/conv.py conv2d_dgrad ``compact``) and the subsampled
addend of the consumer's data-gradient epilogue (csrc/kernels.h ConvArgs::add_sh): the streaming 1x1 kernel (K 128 /
256) and the multi-stage tile kernel (K 512) given the compact addend must produce bit for bit what they produce from
the materialised one (zeros between the addend's pixels: the same fp32 additions)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16


def _rel(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _randn(shape, seed, dev):
    return torch.randn(shape, device=dev, generator=torch.Generator(dev).manual_seed(seed))


def _pack_mask(z):
    """(N, C, H, W) bool -> [P][C / 8] uint8 sign mask, bit e of byte g = channel 8 g + e (bigdl_bn_apply zm)."""
    N, C, H, W = z.shape
    bits = z.permute(0, 2, 3, 1).reshape(N * H * W, C // 8, 8).to(torch.int32)
    wts = (2 ** torch.arange(8, device=z.device, dtype=torch.int32)).view(1, 1, 8)
    return (bits * wts).sum(-1).to(torch.uint8).contiguous()


@pytest.mark.parametrize("bnmode", ["none", "zm", "aff"])
@pytest.mark.parametrize("K", [128, 256, 512])
@pytest.mark.parametrize("N,H", [(2, 8), (3, 10)])       # M = 128; M = 300: a row tail in every kernel's tile
def test_strided_addend_equals_materialised(N, H, K, bnmode):
    from bigdl_amd.ops import bn as bnops
    from bigdl_amd.ops import conv as cv

    dev = torch.device("cuda:0")
    C = 256
    assert cv.addend_stride_applies(N, K, H, H, C, (2, 2), 0 if bnmode == "none" else 1)
    w = (_randn((K, C, 1, 1), 1, dev) * (1.0 / K ** 0.5)).to(BF, memory_format=CL)      # the consumer's weight
    wt = cv.transpose_w(w)
    gy = _randn((N, K, H, H), 2, dev).to(BF, memory_format=CL)
    Hc = (H + 1) // 2
    compact = _randn((N, C, Hc, Hc), 3, dev).to(BF, memory_format=CL)
    full = torch.zeros((N, C, H, H), dtype=BF, device=dev).contiguous(memory_format=CL)
    full[:, :, ::2, ::2] = compact
    compact._compact_stride = (2, 2)
    bx = _randn((N, C, H, H), 4, dev).to(BF, memory_format=CL)
    zpos = _randn((N, C, H, H), 5, dev) > 0
    mean = torch.linspace(-0.1, 0.1, C, device=dev)
    aff = torch.cat([torch.linspace(0.5, 1.5, C, device=dev), torch.linspace(-0.2, 0.2, C, device=dev)])

    def run(addend):
        bn = None
        if bnmode != "none":
            bn = {"x": bx, "z": None, "zm": _pack_mask(zpos) if bnmode == "zm" else None, "mean": mean, "aff": aff,
                  "red": bnops.new_stats(C, dev)}
        dx = cv.conv2d_dgrad(gy, wt, (N, C, H, H), (1, 1), (0, 0), addend=addend, bn=bn)
        torch.cuda.synchronize()
        return dx, bn

    dx_c, bn_c = run(compact)
    dx_f, bn_f = run(full)
    assert torch.equal(dx_c, dx_f)
    # and both are the data gradient plus the addend (bf16 data-gradient tolerance of tests/test_kernels_gpu.py)
    ref = torch.nn.grad.conv2d_input((N, C, H, H), w.float().cpu(), gy.float().cpu()) + full.float().cpu()
    assert _rel(dx_c.cpu(), ref) < 1e-2
    if bnmode != "none":
        # the consumer-BN sums see the gradient including the addend: fp32 sums of the kernel's own rounded output
        assert bn_c["done"] and bn_f["done"]
        d = dx_c.float()
        xf = bx.float()
        mask = zpos if bnmode == "zm" else (xf * aff[:C].view(1, C, 1, 1) + aff[C:].view(1, C, 1, 1)) > 0
        dm = d * mask
        want = (dm.sum(dim=(0, 2, 3)), (dm * (xf - mean.view(1, C, 1, 1))).sum(dim=(0, 2, 3)))
        for bn in (bn_c, bn_f):
            r2 = bn["red"].view(bnops.stat_slots(), 2, C).sum(0)
            assert _rel(r2[0], want[0]) < 1e-3
            assert _rel(r2[1], want[1]) < 1e-3


def test_compact_dgrad_is_the_strided_quarter():
    """conv2d_dgrad ``compact``: the 1x1 / stride-2 data gradient at the output resolution equals the stride's pixels
    of the full one, whose other pixels are zero; any other convolution ignores the flag."""
    from bigdl_amd.ops import conv as cv

    dev = torch.device("cuda:0")
    N, C, H, K = 2, 128, 10, 256
    w = (_randn((K, C, 1, 1), 1, dev) * (1.0 / K ** 0.5)).to(BF, memory_format=CL)
    wt = cv.transpose_w(w)
    gy = _randn((N, K, 5, 5), 2, dev).to(BF, memory_format=CL)
    full = cv.conv2d_dgrad(gy, wt, (N, C, H, H), (2, 2), (0, 0))
    comp = cv.conv2d_dgrad(gy, wt, (N, C, H, H), (2, 2), (0, 0), compact=True)
    assert tuple(comp.shape) == (N, C, 5, 5) and cv.compact_stride(comp) == (2, 2)
    assert torch.equal(cv.expand_compact(comp, H, H), full)
    ref = torch.nn.grad.conv2d_input((N, C, H, H), w.float().cpu(), gy.float().cpu(), stride=2)
    assert _rel(full.cpu(), ref) < 1e-2
    gy1 = _randn((N, K, H, H), 3, dev).to(BF, memory_format=CL)
    plain = cv.conv2d_dgrad(gy1, wt, (N, C, H, H), (1, 1), (0, 0), compact=True)
    assert tuple(plain.shape) == (N, C, H, H) and cv.compact_stride(plain) is None


def _grads(m):
    return [g.detach().float().clone() for g in m.parameters()[1]]


@pytest.mark.parametrize("det", [False, True])
def test_downsampling_block_switch_on_off(det, monkeypatch):
    """One ResNet downsampling bottleneck at stage-2 widths (256 -> 128 -> 512, stride 2; N = 2, 16 x 16): forward and
    backward with BIGDL_COMPACT_SHORTCUT's switch on and off. The compact path must actually run; gradInput and every
    parameter gradient agree, bit for bit in deterministic mode (no kernel but the addend path differs: the shortcut's
    GEMM computes the same fp32 sums either way; otherwise the BN reductions' atomic order flips isolated roundings)."""
    from bigdl_amd.models.resnet import _Builder
    from bigdl_amd.nn import BatchNormalization
    from bigdl_amd.nn.fusion import fuse_for_training
    from bigdl_amd.ops import conv as cv
    from bigdl_amd.ops import native

    b = _Builder("B", True)
    b.iChannels = 256
    blk = b.bottleneck(128, 2)
    g = torch.Generator().manual_seed(3)
    for m in blk.flattened_layers():
        if isinstance(m, BatchNormalization) and m.affine:
            m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    seen = []
    orig = cv.conv2d_dgrad

    def spy(*a, **k):
        seen.append((bool(k.get("compact")), cv.compact_stride(k.get("addend")) is not None))
        return orig(*a, **k)

    monkeypatch.setattr(cv, "conv2d_dgrad", spy)
    torch.manual_seed(1)
    x = torch.randn(2, 256, 16, 16).cuda().to(BF).contiguous(memory_format=CL)
    gy = torch.randn(2, 512, 8, 8).cuda().to(BF).contiguous(memory_format=CL)
    res = {}
    saved, saved_det = cv.COMPACT_SHORTCUT[0], native.deterministic()
    native.set_deterministic(det)
    try:
        for on in (True, False):
            m = copy.deepcopy(blk).to("cuda")
            fuse_for_training(m)
            assert m._residual_plan is not None
            cv.set_compact_shortcut(on)
            del seen[:]
            m.forward(x)
            gi = m.backward(x, gy)
            torch.cuda.synchronize()
            assert tuple(gi.shape) == tuple(x.shape)
            # on: the shortcut convolution gives a compact gradient and the branch's first convolution adds it
            assert ((True, False) in seen and (False, True) in seen) == on
            res[on] = (gi.float().clone(), _grads(m))
    finally:
        cv.set_compact_shortcut(saved)
        native.set_deterministic(saved_det)
    assert _rel(res[True][0], res[False][0]) < 1e-2
    for a, r in zip(res[True][1], res[False][1]):
        assert _rel(a, r) < 1e-2
    if det:
        assert torch.equal(res[True][0], res[False][0])
        for a, r in zip(res[True][1], res[False][1]):
            assert torch.equal(a, r)
