"""One-pass 3x3 / stride-2 / pad-1 data gradient (csrc/conv_halo.hip conv_halo_kernel S2: all four stride phases in one
launch from halo tiles of dy) vs torch.nn.grad.conv2d_input in fp32 on the CPU, with the consumer-BN backward reduction
under both ReLU-mask forms, run-to-run bit equality, the four-phase path behind the switch, and the declined calls."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16

CASES = [
    # N, C, H, K (conv C -> K, 3x3 / 2 / pad 1 over H x H; the data gradient is K -> C)
    (2, 32, 14, 32),       # dy 7 x 7, one 32-channel chunk
    (4, 64, 14, 128),      # dy 7 x 7, four chunks
    (3, 128, 28, 64),      # dy 14 x 14, two channel tiles
    (1, 64, 56, 32),       # dy 28 x 28, seven row segments per image
    (5, 160, 28, 96),      # Cs = 96 (three chunks), Ncol = 160: the last channel tile runs past Ncol
]


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


@functools.lru_cache(maxsize=None)
def _problem(N, C, H, K):
    """Operands and the fp32 CPU reference of one case (computed once, shared, never modified)."""
    dev = torch.device("cuda:0")
    w = (_randn((K, C, 3, 3), 1, dev) * (1.0 / (K * 9) ** 0.5)).to(BF, memory_format=CL)
    OH = (H + 2 - 3) // 2 + 1
    gy = _randn((N, K, OH, OH), 2, dev).to(BF, memory_format=CL)
    ref = torch.nn.grad.conv2d_input((N, C, H, H), w.float().cpu(), gy.float().cpu(), stride=2, padding=1)
    return w, gy, ref


@pytest.mark.parametrize("case", CASES)
def test_dgrad_s2_one_pass(case):
    from bigdl_amd.ops import bn as bnops
    from bigdl_amd.ops import conv as cv
    from bigdl_amd.ops import native

    C_ = native.get()
    N, C, H, K = case
    dev = torch.device("cuda:0")
    w, gy, ref = _problem(N, C, H, K)
    wt = cv.transpose_w(w)
    shape = (N, C, H, H)
    # the kernel takes the call, and conv2d_dgrad routes to it: same bits (no atomics on dx)
    direct = torch.empty(shape, dtype=BF, device=dev).contiguous(memory_format=CL)
    assert C_.dgrad_s2(gy, wt, direct)
    dx = cv.conv2d_dgrad(gy, wt, shape, (2, 2), (1, 1))
    dx2 = cv.conv2d_dgrad(gy, wt, shape, (2, 2), (1, 1))
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2) and torch.equal(dx, direct)
    assert _rel(dx.cpu(), ref) < 1e-2
    # consumer-BN backward reduction under the sign mask and under the affine mask: fp32 sums of the rounded output
    bx = _randn(shape, 4, dev).to(BF, memory_format=CL)
    zpos = _randn(shape, 5, dev) > 0
    mean = torch.linspace(-0.1, 0.1, C, device=dev)
    aff = torch.cat([torch.linspace(0.5, 1.5, C, device=dev), torch.linspace(-0.2, 0.2, C, device=dev)])
    xf = bx.float()
    for mode in ("zm", "aff"):
        bn = {"x": bx, "z": None, "zm": _pack_mask(zpos) if mode == "zm" else None, "mean": mean, "aff": aff,
              "red": bnops.new_stats(C, dev)}
        dxb = cv.conv2d_dgrad(gy, wt, shape, (2, 2), (1, 1), bn=bn)
        torch.cuda.synchronize()
        assert bn["done"] and torch.equal(dxb, dx)
        mask = zpos if mode == "zm" else (xf * aff[:C].view(1, C, 1, 1) + aff[C:].view(1, C, 1, 1)) > 0
        dm = dxb.float() * mask
        r2 = bn["red"].view(bnops.stat_slots(), 2, C).sum(0)
        assert _rel(r2[0], dm.sum(dim=(0, 2, 3))) < 1e-3
        assert _rel(r2[1], (dm * (xf - mean.view(1, C, 1, 1))).sum(dim=(0, 2, 3))) < 1e-3
    # the four-phase path behind the switch: same reference
    C_.set_dgrad_s2(0)
    try:
        assert not C_.dgrad_s2(gy, wt, direct)
        old = cv.conv2d_dgrad(gy, wt, shape, (2, 2), (1, 1))
        torch.cuda.synchronize()
    finally:
        C_.set_dgrad_s2(1)
    assert _rel(old.cpu(), ref) < 1e-2
    assert _rel(dx, old) < 1e-2


def test_dgrad_s2_declined_calls_take_the_phase_path():
    """A call with an addend, and one outside the supported geometry (H = 13), still give the right gradient."""
    from bigdl_amd.ops import conv as cv
    from bigdl_amd.ops import native

    C_ = native.get()
    dev = torch.device("cuda:0")
    N, C, H, K = 2, 64, 14, 64
    w, gy, ref = _problem(N, C, H, K)
    wt = cv.transpose_w(w)
    add = _randn((N, C, H, H), 7, dev).to(BF, memory_format=CL)
    dx = cv.conv2d_dgrad(gy, wt, (N, C, H, H), (2, 2), (1, 1), addend=add)
    assert _rel(dx.cpu(), ref + add.float().cpu()) < 1e-2
    H = 13
    w, gy, ref = _problem(N, C, H, K)
    out = torch.empty((N, C, H, H), dtype=BF, device=dev).contiguous(memory_format=CL)
    assert not C_.dgrad_s2(gy, wt, out)
    dx = cv.conv2d_dgrad(gy, wt, (N, C, H, H), (2, 2), (1, 1))
    assert _rel(dx.cpu(), ref) < 1e-2
