"""Projection-shortcut passes folded into their neighbours (csrc/batchnorm.hip, nn/fusion.py):

  a. bn_apply with a residual affine (the shortcut BN's apply folded into the block's last BN apply) against the two-pass
     form: the output and the sign mask bit for bit;
  b. bn_bwd_apply's second-BN reduction (R2) with and without the residual gradient dres written;
  c. the shortcut BN's backward from (output gradient, sign mask) against the one from a materialised dres;
  d. whole projection bottlenecks through residual_forward / residual_backward with the switches on and off, against
     each other and against the fp32 CPU engine.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
DEV = "cuda:0"


def _randn(shape, seed):
    return torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _act(shape, seed, scale=1.0):
    return (_randn(shape, seed) * scale).to(BF).contiguous(memory_format=CL)


def _chan(C, lo, hi):
    return torch.linspace(lo, hi, C, device=DEV)


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# (N2, C64, 5x7): P = 70 is no multiple of the row unroll (4) or of rows per iteration (32); (N1, C8, 3x3): one channel
# group; (N1, C2056, 1x3): 257 channel groups = a second blockIdx.y chunk holding one group
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,C,H,W", [(2, 64, 5, 7), (1, 8, 3, 3), (1, 2056, 1, 3)])
def test_apply_with_residual_affine_equals_two_passes(N, C, H, W, relu):
    from bigdl_amd.ops import native

    C_ = native.get()
    P = N * H * W
    x, xs = _act((N, C, H, W), 1), _act((N, C, H, W), 2, 2.0)
    sc, sh = _chan(C, 0.5, 1.5), _chan(C, -0.3, 0.3)
    rsc, rsh = _chan(C, 1.7, 0.4), _chan(C, 0.25, -0.25)
    # two passes: the shortcut BN's apply (no ReLU), then the block BN's apply with the plain residual
    res = torch.empty_like(xs)
    C_.bn_apply(xs, rsc, rsh, None, res, P, C, False)
    y2, zm2 = torch.empty_like(x), torch.zeros(P * C // 8, dtype=torch.uint8, device=DEV)
    C_.bn_apply(x, sc, sh, res, y2, P, C, relu, zm2)
    # one pass
    y1, zm1 = torch.empty_like(x), torch.zeros(P * C // 8, dtype=torch.uint8, device=DEV)
    C_.bn_apply(x, sc, sh, xs, y1, P, C, relu, zm1, rsc, rsh)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(zm1, zm2)
    # and both are the fused expression: fp32 reference with the residual rounded to bf16 (one final bf16 rounding)
    v = lambda t: t.view(1, C, 1, 1)
    want = x.float() * v(sc) + v(sh) + (xs.float() * v(rsc) + v(rsh)).to(BF).float()
    if relu:
        want = torch.relu(want)
    assert (y1.float() - want).abs().max().item() <= 2.0 ** -7 * want.abs().max().item()


def _pack_mask(z):
    N, C, H, W = z.shape
    bits = z.permute(0, 2, 3, 1).reshape(N * H * W, C // 8, 8).to(torch.int32)
    wts = (2 ** torch.arange(8, device=z.device, dtype=torch.int32)).view(1, 1, 8)
    return (bits * wts).sum(-1).to(torch.uint8).reshape(-1).contiguous()


def _bwd_inputs(N, C, H, W):
    from bigdl_amd.ops import bn as bnops
    from bigdl_amd.ops import native

    C_ = native.get()
    P = N * H * W
    dz, x, x2 = _act((N, C, H, W), 3), _act((N, C, H, W), 4), _act((N, C, H, W), 5)
    zm = _pack_mask(_randn((N, C, H, W), 6) > 0)
    mean, invstd, gamma = _chan(C, -0.2, 0.2), _chan(C, 0.6, 1.4), _chan(C, 1.3, 0.7)
    mean2 = _chan(C, 0.1, -0.1)
    red = torch.zeros(bnops.stat_slots() * 2 * C, device=DEV)
    C_.bn_bwd_reduce(dz, None, x, mean, red, P, C, None, zm)
    return C_, P, dz, x, x2, zm, mean, invstd, gamma, mean2, red


# row blocks of the apply grid: C 64 -> 256 rows each, P = 429 -> 2; C 2056 -> 8 rows each, P = 21 -> 3; both far below
# STAT_SLOTS, so every slot word of red2 receives one add onto zero and the sums compare exactly
@pytest.mark.parametrize("N,C,H,W", [(3, 64, 11, 13), (1, 2056, 3, 7)])
def test_second_bn_reduction_without_dres(N, C, H, W):
    from bigdl_amd.ops import bn as bnops

    C_, P, dz, x, x2, zm, mean, invstd, gamma, mean2, red = _bwd_inputs(N, C, H, W)
    assert P % 2 == 1
    out = {}
    for with_dres in (True, False):
        coef = torch.empty(3 * C, device=DEV)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if with_dres else None
        red2 = torch.zeros(bnops.stat_slots() * 2 * C, device=DEV)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        C_.bn_bwd_apply(dz, None, x, mean, invstd, gamma, red, bnops.stat_slots(), coef, dx, dres, dg, db, P, C, None,
                        zm, x2=x2, mean2=mean2, red2=red2)
        torch.cuda.synchronize()
        out[with_dres] = (dx, red2, dg, db, dres)
    for a, b in zip(out[True][:4], out[False][:4]):
        assert torch.equal(a, b)
    # the sums are those of the stored bf16 dres
    dres = out[True][4].float()
    r2 = out[False][1].view(bnops.stat_slots(), 2, C).sum(0)
    assert _rel(r2[0], dres.sum(dim=(0, 2, 3))) < 1e-5
    assert _rel(r2[1], (dres * (x2.float() - mean2.view(1, C, 1, 1))).sum(dim=(0, 2, 3))) < 1e-5
    assert r2.abs().sum().item() > 0


@pytest.mark.parametrize("N,C,H,W", [(3, 64, 11, 13), (1, 2056, 3, 7)])
def test_shortcut_bn_backward_from_masked_gradient(N, C, H, W):
    """The shortcut BN's backward given (block output gradient, block BN sign mask) and the reduction handed over from
    the block BN's pass, against the same from the materialised dres: dx, dgamma, dbeta bit for bit."""
    from bigdl_amd.ops import bn as bnops

    C_, P, dz, x, x2, zm, mean, invstd, gamma, mean2, red = _bwd_inputs(N, C, H, W)
    coef = torch.empty(3 * C, device=DEV)
    dres = torch.empty_like(x)
    red2 = torch.zeros(bnops.stat_slots() * 2 * C, device=DEV)
    C_.bn_bwd_apply(dz, None, x, mean, invstd, gamma, red, bnops.stat_slots(), coef, torch.empty_like(x), dres, None,
                    None, P, C, None, zm, x2=x2, mean2=mean2, red2=red2)
    inv2, g2 = _chan(C, 0.8, 1.2), _chan(C, 0.9, 1.1)
    out = []
    for gy, mask in ((dres, None), (dz, zm)):
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dx2, _ = bnops.bn_backward_gpu(gy, None, x2, mean2, inv2, g2, dg, db, red=red2, zm=mask)
        torch.cuda.synchronize()
        out.append((dx2, dg, db))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert out[0][1].abs().sum().item() > 0 and out[0][0].float().abs().sum().item() > 0


# ---------------------------------------------------------------------------------------------------------------------
def _block(n_in, n, stride):
    from bigdl_amd.models.resnet import _Builder
    from bigdl_amd.nn import BatchNormalization

    b = _Builder("B", True)
    b.iChannels = n_in
    blk = b.bottleneck(n, stride)
    g = torch.Generator().manual_seed(3)
    for m in blk.flattened_layers():
        if isinstance(m, BatchNormalization) and m.affine:
            m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return blk


def _run_block(blk, x, gy, fuse):
    m = copy.deepcopy(blk).to(x.device)
    if fuse:
        from bigdl_amd.nn.fusion import fuse_for_training

        fuse_for_training(m)
        assert m._residual_plan is not None
    m.zeroGradParameters()
    out = m.forward(x)
    out = out.detach().clone()
    gi = m.backward(x, gy)
    if x.is_cuda:
        torch.cuda.synchronize()
    return [out.float().cpu(), gi.detach().float().cpu()] + [g.detach().float().cpu().clone() for g in m.parameters()[1]]


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("n_in,n,stride", [(64, 64, 1), (256, 128, 2)])
def test_projection_block_switches_on_off(n_in, n, stride, det, monkeypatch, capsys):
    """One projection bottleneck (64 -> 256 / stride 1 and 256 -> 512 / stride 2, 8 x 8, N = 2) with the shortcut fold
    (forward) and the dres-free backward on and off. The forward output is bit-equal (the fold rounds as the two passes
    do); in deterministic mode so is every gradient. Against the fp32 CPU engine each tensor's error with the switches
    on is at most 1.1 x its error with them off (the 1.1 covers the atomic order of the default mode)."""
    from bigdl_amd.nn import fusion
    from bigdl_amd.ops import bn as bnops
    from bigdl_amd.ops import native

    blk = _block(n_in, n, stride)
    torch.manual_seed(1)
    xc = torch.randn(2, n_in, 8, 8).to(BF).float()
    gyc = torch.randn(2, 4 * n, 8 // stride, 8 // stride).to(BF).float()
    ref = _run_block(blk, xc, gyc, fuse=False)                       # fp32 CPU engine
    x = xc.to(DEV).to(BF).contiguous(memory_format=CL)
    gy = gyc.to(DEV).to(BF).contiguous(memory_format=CL)
    seen = {"lin": 0, "nodres": 0}
    orig_def, orig_bwd = bnops.deferred, bnops.bn_backward_gpu

    def spy_def(t, aff, relu=True):
        seen["lin"] += not relu
        return orig_def(t, aff, relu)

    def spy_bwd(*a, **k):
        seen["nodres"] += k.get("sec") is not None and not k.get("need_dres")
        return orig_bwd(*a, **k)

    monkeypatch.setattr(bnops, "deferred", spy_def)
    monkeypatch.setattr(bnops, "bn_backward_gpu", spy_bwd)
    saved_det, saved_sw = native.deterministic(), (fusion.SHORTCUT_FOLD[0], fusion.SHORTCUT_NODRES[0])
    native.set_deterministic(det)
    res = {}
    try:
        for on in (False, True):
            fusion.SHORTCUT_FOLD[0] = fusion.SHORTCUT_NODRES[0] = on
            seen.update(lin=0, nodres=0)
            res[on] = _run_block(blk, x, gy, fuse=True)
            # on: both paths actually ran (the dres-free backward needs the second-BN reduction: not in deterministic mode)
            assert seen["lin"] == (1 if on else 0)
            assert seen["nodres"] == (1 if on and not det else 0)
    finally:
        native.set_deterministic(saved_det)
        fusion.SHORTCUT_FOLD[0], fusion.SHORTCUT_NODRES[0] = saved_sw
    assert torch.equal(res[True][0], res[False][0])
    if det:
        for a, b in zip(res[True], res[False]):
            assert torch.equal(a, b)
    names = ["output", "gradInput"] + [f"grad[{i}]" for i in range(len(ref) - 2)]
    bad = []
    for name, r, off, on in zip(names, ref, res[False], res[True]):
        e_off, e_on = _rel(off, r), _rel(on, r)
        ratio = e_on / e_off if e_off > 0 else (1.0 if e_on == 0 else float("inf"))
        with capsys.disabled():
            print(f"  fold n_in={n_in} stride={stride} det={int(det)} {name}: err off {e_off:.3e} on {e_on:.3e} "
                  f"ratio {ratio:.4f}")
        if not e_on <= 1.1 * e_off:
            bad.append((name, e_off, e_on))
    assert not bad, bad


def test_folded_shortcut_output_materialises():
    """A reader of the shortcut's output outside the plan gets real values through ops.bn.materialize."""
    from bigdl_amd.nn import fusion
    from bigdl_amd.nn.fusion import fuse_for_training
    from bigdl_amd.ops import bn as bnops

    blk = _block(64, 64, 1)
    torch.manual_seed(2)
    x = torch.randn(2, 64, 8, 8).to(DEV).to(BF).contiguous(memory_format=CL)
    outs = {}
    saved = fusion.SHORTCUT_FOLD[0]
    try:
        for on in (False, True):
            fusion.SHORTCUT_FOLD[0] = on
            m = copy.deepcopy(blk).to(DEV)
            fuse_for_training(m)
            m.forward(x)
            short = m.modules[0].modules[1]
            assert (getattr(short.output, "_bn_lin", None) is not None) == on
            outs[on] = bnops.materialize(short.output).clone()
    finally:
        fusion.SHORTCUT_FOLD[0] = saved
    torch.cuda.synchronize()
    assert torch.equal(outs[True].view(torch.int16), outs[False].view(torch.int16))
