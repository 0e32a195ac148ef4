"""Exact checks of the LDS-DMA weight-gradient pipelines (conv_wgrad_glds_kernel, conv_wgrad_g3_kernel,
conv_wgrad_p8_kernel, conv_wgrad_halo_kernel).

What can go wrong in these kernels is a stage read before its DMA has landed, or overwritten before every wave has
read it. So the inputs are integer-valued bf16 from -3..3, different in every stage: every product is an integer of
magnitude <= 9 and every partial sum over at most 4096 pixels an integer below 2^24, which fp32 holds exactly in any
summation order. The result must EQUAL the integer reference computed on the CPU in fp64. Every case runs with 5
seeds (a race need not show on the first try), and checks through the plan which kernel it reaches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
SEEDS = range(5)


def _dev():
    return torch.device("cuda:0")


def _C():
    from bigdl_amd.ops import native

    return native.get()


def _geo(N, C, H, W, K, R, st, pd):
    OH, OW = (H + 2 * pd - R) // st + 1, (W + 2 * pd - R) // st + 1
    return [N, H, W, C, OH, OW, R, R, st, st, pd, pd, 1, 1, N * OH * OW, K, R * R * C, K], OH, OW


def _ints(shape, gen):
    return torch.randint(-3, 4, shape, generator=gen).to(torch.float64)


def _run_exact(case, bias, seed):
    """One exact run: integer inputs -> conv_wgrad -> compare with the fp64 CPU reference."""
    N, C, H, W, K, R, st, pd = case
    geo, OH, OW = _geo(*case)
    assert geo[14] * 9 < 2 ** 24
    gen = torch.Generator().manual_seed(1000 + seed)
    x64 = _ints((N, C, H, W), gen)
    dy64 = _ints((N, K, OH, OW), gen)
    ref = torch.nn.grad.conv2d_weight(x64, (K, C, R, R), dy64, stride=st, padding=pd)
    refb = dy64.sum(dim=(0, 2, 3))
    dev = _dev()
    x = x64.to(dev).to(BF).contiguous(memory_format=CL)
    dy = dy64.to(dev).to(BF).contiguous(memory_format=CL)
    dw = torch.zeros(K, C, R, R, device=dev).contiguous(memory_format=CL)
    db = torch.zeros(K, device=dev) if bias else None
    _C().conv_wgrad(dy, x, dw, db, geo)
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu().double(), ref), f"dW differs from the integer reference (seed {seed})"
    if bias:
        assert torch.equal(db.cpu().double(), refb), f"dbias differs from the integer reference (seed {seed})"


def _assert_128_tile_dma_kernel(case, bias):
    """The case is left to the 128 x 128 LDS-DMA kernels (2-stage, or 3-stage under set_wgrad_g3)."""
    geo, _, _ = _geo(*case)
    splits, wsn, halo, p8, reg = _C().conv_wgrad_plan_info(geo, bias)
    assert halo == 0 and p8 == 0 and reg == 0 and splits >= 0, (splits, wsn, halo, p8, reg)
    return splits, wsn


# (N, H, W) -> pixel count M = N * H * W for stride 1 ("same" output size)
RING = {
    64: (1, 8, 8),         # one stage, no steady state
    65: (5, 13, 1),        # a one-row tail stage
    128: (2, 8, 8),        # two stages
    129: (3, 43, 1),
    327: (3, 109, 1),      # 64 * 5 + 7
    513: (27, 19, 1),      # 2 pixel splits of 320 (not a multiple of the 19-pixel image): 5 stages and 3 stages + 1 row
    1025: (25, 41, 1),     # 3 pixel splits of 384: 6 stages, 6 stages, 4 stages + 1 row
}
RING_SPLITS = {513: 2, 1025: 3}


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("form", ["1x1", "im2col"])
@pytest.mark.parametrize("kernel", ["glds", "g3"])
@pytest.mark.parametrize("M", sorted(RING))
def test_ring_edges(M, kernel, form, bias):
    """Stage-ring edges of the 2-stage kernel (and the 3-stage one): 1 x 1 / stride 1 (GEMM-shaped) and 3 x 3 / pad 1
    (taps outside the image, Kdim = 144: a second kk tile of two granules)."""
    N, H, W = RING[M]
    case = (N, 16, H, W, 128, 3, 1, 1) if form == "im2col" else (N, 128, H, W, 128, 1, 1, 0)
    C_ = _C()
    old = C_.get_wgrad_g3()
    C_.set_wgrad_g3(1 if kernel == "g3" else 0)
    try:
        splits, wsn = _assert_128_tile_dma_kernel(case, bias)
        if M in RING_SPLITS:
            assert splits == RING_SPLITS[M] and wsn > 0, (splits, wsn)
        else:
            assert wsn == 0            # one workspace split: the kernel adds into dW itself
        for seed in SEEDS:
            _run_exact(case, bias, seed)
    finally:
        C_.set_wgrad_g3(old)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("ch", [8, 128, 136])
def test_granule_edges(ch, bias):
    """Ncol = Kdim = 8 (one valid granule, fifteen zero-granule DMAs), 128, 136 (a second tile with one granule)."""
    case = (3, ch, 43, 1, ch, 1, 1, 0)
    _assert_128_tile_dma_kernel(case, bias)
    for seed in SEEDS:
        _run_exact(case, bias, seed)


IM2COL = [
    (3, 16, 5, 5, 16, 3, 1, 1),      # 3 x 3 / pad 1 on 5 x 5: taps outside the image on every border
    (3, 64, 7, 7, 128, 1, 2, 0),     # 1 x 1 / stride 2 on 7 x 7
    (3, 16, 6, 6, 32, 3, 2, 1),      # 3 x 3 / stride 2 / pad 1 on 6 x 6
]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", IM2COL)
def test_im2col_edges(case, bias):
    _assert_128_tile_dma_kernel(case, bias)
    for seed in SEEDS:
        _run_exact(case, bias, seed)


# N, C, H, K, more than one split? The smallest batch of each width the halo plan takes. A 56 / 28 / 14-wide image is
# 56 / 14 / 7 row stages, which the plan always spreads over several splits at these channel counts; one 7 x 7 image is
# one stage, so one split.
HALO = [
    (1, 64, 56, 64, True),
    (1, 64, 28, 128, True),
    (1, 128, 14, 128, True),
    (1, 64, 7, 64, False),
    (2, 64, 7, 128, True),
]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", HALO)
def test_halo_kernel(case, bias):
    N, C, H, K, multi = case
    full = (N, C, H, H, K, 3, 1, 1)
    geo, _, _ = _geo(*full)
    splits, wsn, halo, p8, reg = _C().conv_wgrad_plan_info(geo, bias)
    assert halo > 0 and splits == halo, (splits, halo)
    assert (halo > 1) == multi, halo
    for seed in SEEDS:
        _run_exact(full, bias, seed)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M", [512, 513])
@pytest.mark.parametrize("K", [256, 264])
def test_p8_kernel(K, M, bias):
    """conv_wgrad_p8_kernel under BIGDL_WGRAD_P8=2: Ncol x Kdim = 256 x 256 and 264 x 256, M = 64 * 8 and 64 * 8 + 1."""
    N, H, W = (8, 8, 8) if M == 512 else (27, 19, 1)
    case = (N, 256, H, W, K, 1, 1, 0)
    geo, _, _ = _geo(*case)
    C_ = _C()
    C_.set_wgrad_p8(2)
    try:
        assert C_.conv_wgrad_uses_p8(geo, bias)
        assert C_.conv_wgrad_plan_info(geo, bias)[3] == 1
        for seed in SEEDS:
            _run_exact(case, bias, seed)
    finally:
        C_.set_wgrad_p8(1)


BITEQ = [
    ("glds", (27, 128, 19, 1, 128, 1, 1, 0)),     # 1 x 1, 2 workspace splits
    ("glds", (25, 16, 41, 1, 128, 3, 1, 1)),      # 3 x 3 / pad 1, 3 workspace splits, kk tail tile
    ("glds", (25, 136, 41, 1, 136, 1, 1, 0)),     # Ncol / Kdim tail tiles, 3 workspace splits
    ("g3", (25, 16, 41, 1, 128, 3, 1, 1)),
    ("p8", (27, 256, 19, 1, 264, 1, 1, 0)),
]


@pytest.mark.parametrize("kernel,case", BITEQ)
def test_tr_asm_switch_is_bit_identical(kernel, case):
    """BIGDL_WGRAD_TR_ASM=1 (inline-assembly transposing reads, hand-placed waits) and =0 (compiler intrinsic) run
    the same MFMAs in the same order: on the workspace path without the bias gradient (no fp32 atomics) the results
    are identical bits for random non-integer inputs."""
    N, C, H, W, K, R, st, pd = case
    geo, OH, OW = _geo(*case)
    C_ = _C()
    old_g3, old_tr = C_.get_wgrad_g3(), C_.get_wgrad_tr_asm()
    C_.set_wgrad_g3(1 if kernel == "g3" else 0)
    C_.set_wgrad_p8(2 if kernel == "p8" else 1)
    try:
        splits, wsn, halo, p8, reg = C_.conv_wgrad_plan_info(geo, False)
        if kernel == "p8":
            assert p8 == 1
        else:
            assert halo == 0 and p8 == 0 and reg == 0 and splits > 1 and wsn > 0
        dev = _dev()
        for seed in SEEDS:
            gen = torch.Generator().manual_seed(2000 + seed)
            x = torch.randn(N, C, H, W, generator=gen).to(dev).to(BF).contiguous(memory_format=CL)
            dy = torch.randn(N, K, OH, OW, generator=gen).to(dev).to(BF).contiguous(memory_format=CL)
            outs = []
            for tr in (1, 0):
                C_.set_wgrad_tr_asm(tr)
                dw = torch.zeros(K, C, R, R, device=dev).contiguous(memory_format=CL)
                C_.conv_wgrad(dy, x, dw, None, geo)
                torch.cuda.synchronize()
                outs.append(dw)
            assert torch.equal(outs[0], outs[1]), f"TR_ASM=1 and =0 differ (seed {seed})"
            assert outs[0].abs().sum().item() > 0
    finally:
        C_.set_wgrad_tr_asm(old_tr)
        C_.set_wgrad_g3(old_g3)
        C_.set_wgrad_p8(1)
