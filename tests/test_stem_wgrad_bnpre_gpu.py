"""The stem BN's backward applied on load inside the pair-view stem weight gradient (csrc/stem_fwd.hip stem_wgrad_kernel
PRE): dW' and dbias from (dz, x, coefficients) must equal, bit for bit, what the same kernel computes from the input
gradient that bn_bwd_apply materialises (both reduce their per-workgroup partials in a fixed order), and an
integer-valued case must equal an fp64 CPU result exactly."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
DEV = "cuda:0"
K, R, S2 = 64, 7, 4


def _randn(shape, seed):
    return torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _geometry(N, H):
    from bigdl_amd.ops import conv as cv

    OH, OW, s2, _, _ = cv.pair_geometry(H, 224, 7, 7, 2, 3, 3)
    assert OW == 112 and s2 == S2
    return OH, OW


def _unpair(dwp):
    """pair layout back to (K, C, R, S): w'[k][r][j][e * 4 + c] = w[k][c][r][2 j + e]"""
    wpv = dwp.view(K, R, S2, 2, 4)
    got = torch.zeros(K, 3, 7, 7, dtype=dwp.dtype, device=dwp.device)
    for j in range(S2):
        for e in range(2):
            if 2 * j + e < 7:
                got[:, :, :, 2 * j + e] = wpv[:, :, j, e, :3].permute(0, 2, 1)
    return got


# N = 1, OH = 2: one tile and a grid of one; N = 3, OH = 4: 6 tiles; N = 5, OH = 112: 280 tiles, more than the chip has
# CUs, so workgroups loop over two tiles and use both LDS buffers
@pytest.mark.parametrize("N,H", [(1, 4), (3, 8), (5, 224)])
def test_on_load_equals_materialised(N, H):
    from bigdl_amd.ops import bn as bnops
    from bigdl_amd.ops import conv as cv
    from bigdl_amd.ops import native

    C_ = native.get()
    OH, OW = _geometry(N, H)
    if (N, H) == (5, 224):
        assert N * OH // 2 > torch.cuda.get_device_properties(0).multi_processor_count
    P = N * OH * OW
    img = _randn((N, 3, H, 224), 1)
    xp = cv.to_pairs_bf16(img, 7, 7, 2, 3, 3)
    assert cv.pairs_wgrad_takes_bn_pre(xp, K, OH, OW, R, S2, 2, True)
    y = _randn((N, K, OH, OW), 2).to(BF).contiguous(memory_format=CL)          # the stem BN's input
    dz = _randn((N, K, OH, OW), 3).to(BF).contiguous(memory_format=CL)
    # ReLU mask y * scale + shift > 0: about half of the bits clear
    aff = torch.cat([torch.linspace(0.5, 1.5, K, device=DEV), torch.linspace(-0.2, 0.2, K, device=DEV)])
    frac = ((y.float() * aff[:K].view(1, K, 1, 1) + aff[K:].view(1, K, 1, 1)) > 0).float().mean().item()
    assert 0.4 < frac < 0.6
    # slot sums chosen so that B and D are of A's order: a dropped term cannot hide below the bf16 rounding
    mean, invstd = torch.linspace(-0.3, 0.3, K, device=DEV), torch.linspace(0.7, 1.3, K, device=DEV)
    gamma = torch.linspace(1.2, 0.8, K, device=DEV)
    red = torch.zeros(bnops.stat_slots(), 2, K, device=DEV)
    red[0, 0] = P * torch.linspace(0.2, 0.4, K, device=DEV)
    red[0, 1] = P * torch.linspace(-0.5, -0.3, K, device=DEV)
    red = red.reshape(-1)
    coef = torch.empty(3 * K, device=DEV)
    dx = torch.empty_like(y)
    C_.bn_bwd_apply(dz, None, y, mean, invstd, gamma, red, bnops.stat_slots(), coef, dx, None, None, None, P, K, aff)
    assert coef[K:2 * K].abs().min().item() > 0.05 and coef[2 * K:].abs().min().item() > 0.05
    out = []
    for gy, pre in ((dx, None), (dz, (y, coef, aff))):
        dwp, db = torch.zeros(K, R * S2 * 8, device=DEV), torch.zeros(K, device=DEV)
        cv.conv2d_pairs_wgrad(gy, xp, R, S2, 2, dwp, db, bn_pre=pre)
        torch.cuda.synchronize()
        out.append((dwp, db))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    assert out[0][0].abs().sum().item() > 0 and out[0][1].abs().sum().item() > 0
    # the materialised path is the convolution weight gradient of dx (bf16 operands, fp32 sums)
    ref = torch.nn.grad.conv2d_weight(img.to(BF).float(), (K, 3, 7, 7), dx.float(), stride=2, padding=3)
    rel = ((_unpair(out[1][0]) - ref).norm() / ref.norm()).item()
    assert rel < 1e-3, rel


def test_on_load_integer_inputs_exact():
    """Small integers everywhere: every product and sum is exact in bf16 / fp32, so the result equals fp64."""
    from bigdl_amd.ops import conv as cv

    N, H = 3, 8
    OH, OW = _geometry(N, H)
    g = torch.Generator().manual_seed(4)
    img = torch.randint(-2, 3, (N, 3, H, 224), generator=g).float()
    y = torch.randint(-3, 4, (N, K, OH, OW), generator=g).float()
    dz = torch.randint(-2, 3, (N, K, OH, OW), generator=g).float()
    A = torch.randint(1, 4, (K,), generator=g).float()
    B = torch.randint(1, 3, (K,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (K,), generator=g).float())
    D = torch.randint(1, 4, (K,), generator=g).float()
    scale, shift = torch.ones(K), torch.full((K,), -0.5)           # mask: y >= 1
    v = lambda t: t.double().view(1, K, 1, 1)
    mask = (y.double() * v(scale) + v(shift)) > 0
    assert 0.3 < mask.double().mean().item() < 0.6
    dy = v(A) * torch.where(mask, dz.double(), torch.zeros((), dtype=torch.float64)) + v(B) * y.double() + v(D)
    ref_w = torch.nn.grad.conv2d_weight(img.double(), (K, 3, 7, 7), dy, stride=2, padding=3)
    ref_b = dy.sum(dim=(0, 2, 3))
    xp = cv.to_pairs_bf16(img.to(DEV), 7, 7, 2, 3, 3)
    dwp, db = torch.zeros(K, R * S2 * 8, device=DEV), torch.zeros(K, device=DEV)
    cv.conv2d_pairs_wgrad(dz.to(DEV).to(BF).contiguous(memory_format=CL), xp, R, S2, 2, dwp, db,
                          bn_pre=(y.to(DEV).to(BF).contiguous(memory_format=CL), torch.cat([A, B, D]).to(DEV),
                                  torch.cat([scale, shift]).to(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(_unpair(dwp).double().cpu(), ref_w)
    assert torch.equal(db.double().cpu(), ref_b)


def test_stem_bn_hands_coefficients_to_the_stem():
    """The ImageNet stem (conv 7x7/2 -> BN -> ReLU -> max pool) after fuse_for_training: the BN's backward runs no
    apply pass (BIGDL_STEM_BNPRE's switch on; off: it does), and all four parameter gradients agree between the two. The
    kernels are bit-equal (above), but the BN's reduction comes from the pool backward's float atomics, whose order
    differs from run to run: the BN's own gradients (fp32 sums, only the order differs) agree to 1e-5, and the
    convolution's to 1e-3 (isolated bf16 roundings of dx flip, 2^-8 each, under sums over thousands of pixels; a
    dropped term or a wrong operand is an error of order one)."""
    import copy

    from bigdl_amd import nn
    from bigdl_amd.nn import normalization as nz
    from bigdl_amd.nn.fusion import fuse_for_training
    from bigdl_amd.models.resnet import Convolution, Sbn
    from bigdl_amd.ops import bn as bnops
    from bigdl_amd.ops import native

    stem = (nn.Sequential().add(Convolution(3, 64, 7, 7, 2, 2, 3, 3, propagateBack=False)).add(Sbn(64))
            .add(nn.ReLU(True)).add(nn.SpatialMaxPooling(3, 3, 2, 2, 1, 1)))
    torch.manual_seed(5)
    x = torch.randn(2, 3, 32, 224, device=DEV)
    gy = torch.randn(2, 64, 8, 56, device=DEV).to(BF).contiguous(memory_format=CL)
    calls = []
    orig = bnops.bn_backward_gpu

    def spy(*a, **k):
        calls.append(k.get("need_dx", True))
        return orig(*a, **k)

    res = {}
    saved, saved_det = nz._STEM_BNPRE, native.deterministic()
    bnops.bn_backward_gpu = spy
    native.set_deterministic(False)      # (deterministic mode has no pool-side reduction and keeps the apply pass)
    try:
        for on in (False, True):
            nz._STEM_BNPRE = on
            m = copy.deepcopy(stem).to(DEV)
            fuse_for_training(m)
            del calls[:]
            m.forward(x)
            m.backward(x, gy)
            from bigdl_amd.ops import side_stream

            side_stream.join()
            torch.cuda.synchronize()
            assert calls == [not on]
            res[on] = [g.detach().clone() for g in m.parameters()[1]]
    finally:
        nz._STEM_BNPRE = saved
        bnops.bn_backward_gpu = orig
        native.set_deterministic(saved_det)
    assert len(res[True]) == 4              # conv weight, conv bias, BN weight, BN bias
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        a, b = a.float(), b.float()
        assert b.abs().sum().item() > 0
        rel = ((a - b).norm() / b.norm()).item()
        assert rel < (1e-3 if i < 2 else 1e-5), (i, rel)
