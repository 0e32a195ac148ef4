"""Native 3-D convolution (csrc/conv3d.hip through ops/conv_fn.py) against torch's fp64 CPU convolution and its
autograd. Inputs, weights and gy sit on the bf16 grid, so operand rounding is no part of the error.

exact leg: integer data, every partial sum below 2^24 (checked on the reference), so products and fp32 sums are
exact and the results must equal the fp64 reference cast to fp32. The per-temporal-tap path the kernels replace
rounds each tap's partial output to bf16 and fails this leg.
gauss leg: every element within 2^-23 |ref| + Kdim 2^-24 S, S the same convolution of the absolute values: the
first-order fp32 summation bound for any accumulation order with exact products."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _split_n():
    """Batch size at which a 4x4x4-voxel output reaches the launcher's smallest split voxel count."""
    from bigdl_amd.ops import native

    return native.get().conv3d_wgrad_split_min() // 64


# name: (transposed, N, C, K, (T, H, W), kernel, stride, pad, adj); N None = read from the launcher
CASES = {
    "off_granule_C6_K10": (False, 1, 6, 10, (3, 4, 5), (2, 2, 2), (1, 1, 1), (0, 0, 0), None),
    "stage_straddles_taps_C72": (False, 1, 72, 8, (3, 3, 4), (2, 2, 2), (1, 1, 1), (1, 0, 1), None),
    "two_m_tiles_two_n_tiles": (False, 2, 8, 80, (5, 7, 9), (1, 3, 3), (1, 1, 1), (0, 1, 1), None),
    "pad_cut_kernel_longer_than_axis": (False, 2, 8, 8, (1, 2, 3), (3, 3, 3), (1, 1, 1), (1, 1, 1), None),
    "stride_122_odd_extents": (False, 1, 8, 16, (3, 5, 7), (3, 3, 3), (1, 2, 2), (1, 1, 1), None),
    "stride_212_odd_extents": (False, 1, 8, 16, (5, 3, 7), (3, 3, 3), (2, 1, 2), (1, 1, 1), None),
    "dgrad_phase_without_taps": (False, 1, 16, 8, (3, 4, 5), (1, 1, 1), (2, 2, 2), (0, 0, 0), None),
    "anisotropic_1x3x5": (False, 1, 8, 8, (2, 5, 7), (1, 3, 5), (1, 1, 1), (0, 1, 2), None),
    "one_output_voxel": (False, 1, 8, 8, (3, 3, 3), (3, 3, 3), (1, 1, 1), (0, 0, 0), None),
    "transposed_s2_p1_adj100": (True, 2, 6, 10, (3, 4, 3), (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 0, 0)),
    "transposed_s1": (True, 1, 8, 12, (3, 3, 4), (2, 3, 2), (1, 1, 1), (0, 1, 0), (0, 0, 0)),
    "wgrad_split": (False, None, 8, 8, (4, 4, 4), (3, 3, 3), (1, 1, 1), (1, 1, 1), None),
    "wgrad_unsplit": (False, 1, 8, 8, (4, 4, 4), (3, 3, 3), (1, 1, 1), (1, 1, 1), None),
    # 256 tiles of 128 voxels: the smallest M at which forward and data gradient leave the 64-row tile
    "tile_128_rows": (False, 8, 8, 8, (16, 16, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), None),
}


def _reference(transposed, x, w, b, gy, stride, pad, adj):
    """(y, gx, gw, gb) of torch's CPU convolution in the dtype of the inputs (fp64)."""
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.conv_transpose3d(x, w, b, stride, pad, adj) if transposed else F.conv3d(x, w, b, stride, pad)
    return (y.detach(),) + torch.autograd.grad(y, (x, w, b), gy)


def _inputs(case, leg):
    from bigdl_amd.ops import conv_fn

    transposed, N, C, K, ext, k, stride, pad, adj = CASES[case]
    N = _split_n() if N is None else N
    wshape = (C, K, *k) if transposed else (K, C, *k)
    oext = [(e - 1) * s - 2 * p + kk + a for e, kk, s, p, a in zip(ext, k, stride, pad, adj)] if transposed else \
        [conv_fn._out_size(e, kk, s, p, 1) for e, kk, s, p in zip(ext, k, stride, pad)]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    shapes = ((N, C, *ext), wshape, (K,), (N, K, *oext))
    if leg == "exact":
        return [torch.randint(-8, 9, s, generator=g).double() for s in shapes]
    return [torch.randn(s, generator=g).bfloat16().double() for s in shapes]


@pytest.mark.parametrize("leg", ["exact", "gauss"])
@pytest.mark.parametrize("case", list(CASES))
def test_conv3d_against_fp64(case, leg):
    from bigdl_amd.ops import conv_fn

    transposed, _, C, K, _, k, stride, pad, adj = CASES[case]
    x, w, b, gy = _inputs(case, leg)
    ref = _reference(transposed, x, w, b, gy, stride, pad, adj)
    mag = _reference(transposed, x.abs(), w.abs(), b.abs(), gy.abs(), stride, pad, adj)   # S = sum |a||b| per element
    if leg == "exact":
        assert max(m.max().item() for m in mag) < 2 ** 24
    dev = [t.float().cuda().requires_grad_(True) for t in (x, w, b)]
    if transposed:
        y = conv_fn.conv_transpose3d(*dev, stride, pad, adj)
    else:
        y = conv_fn.conv3d(*dev, stride, pad)
    got = (y.detach(),) + torch.autograd.grad(y, dev, gy.float().cuda())
    taps = k[0] * k[1] * k[2]
    # reduction length of each GEMM; the weight gradient sums over the voxels of the underlying convolution's output
    # grid, which is x's grid for a transposed convolution
    kdims = (taps * C, taps * K, (x.numel() // C) if transposed else (gy.numel() // K), gy.numel() // K)
    for name, a, r, s, kdim in zip(("y", "gx", "gw", "gb"), got, ref, mag, kdims):
        a = a.cpu()
        assert a.shape == r.shape and a.dtype == torch.float32, name
        if leg == "exact":
            assert torch.equal(a, r.float()), (name, (a.double() - r).abs().max().item())
        else:
            excess = (a.double() - r).abs() - (2.0 ** -23 * r.abs() + kdim * 2.0 ** -24 * s)
            assert excess.max().item() <= 0, (name, excess.max().item())


def test_conv3d_wgrad_split_threshold_and_determinism():
    """The split case really splits (and one batch entry less does not); in deterministic mode, as outside it, two
    runs of it are bit-identical."""
    from bigdl_amd.ops import conv_fn, native


    x, w, b, gy = (t.float().cuda() for t in _inputs("wgrad_split", "gauss"))
    x16, gy16, geo = conv_fn._ndhwc16(x, 8), conv_fn._ndhwc16(gy, 8), [1, 1, 1, 1, 1, 1]
    dw = torch.zeros(8, 3, 3, 3, 8, device="cuda")
    assert native.get().conv3d_wgrad_splits(gy16, x16, dw, geo) > 1
    assert native.get().conv3d_wgrad_splits(gy16[:-1], x16[:-1], dw, geo) == 1
    was = native.deterministic()
    try:
        for mode in (True, False):
            native.set_deterministic(mode)
            runs = []
            for _ in range(2):
                dev = [t.clone().requires_grad_(True) for t in (x, w, b)]
                runs.append(torch.autograd.grad(conv_fn.conv3d(*dev, (1, 1, 1), (1, 1, 1)), dev, gy))
            assert all(torch.equal(p, q) for p, q in zip(*runs)), mode
    finally:
        native.set_deterministic(was)


@pytest.mark.parametrize("layer", ["VolumetricConvolution", "VolumetricFullConvolution"])
def test_volumetric_layers_take_the_native_kernels(layer, monkeypatch):
    """Through the layers, forward and backward: the depth gather / scatter of the per-tap path is gone."""
    from bigdl_amd import nn

    def boom(*a, **k):
        raise AssertionError("per-tap 3-D path taken on the GPU")

    monkeypatch.setattr(torch, "index_select", boom)
    monkeypatch.setattr(torch.Tensor, "index_select", boom)
    monkeypatch.setattr(torch.Tensor, "index_add", boom)
    m = getattr(nn, layer)(6, 10, 3, 3, 3, 2, 2, 2, 1, 1, 1).to("cuda")
    x = torch.randn(2, 6, 4, 5, 5, device="cuda")
    y = m.forward(x)
    gx = m.backward(x, torch.ones_like(y))
    assert gx.shape == x.shape and torch.isfinite(gx).all() and torch.isfinite(y).all()
