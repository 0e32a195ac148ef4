"""csrc/layernorm.hip element by element against fp64 F.layer_norm and its autograd gradients.

Yardstick: the error of fp32 CPU F.layer_norm (forward and autograd) against fp64 on the same inputs, per tensor;
the kernels are held to |kernel - fp64| <= 4 x that + 1e-7 max|fp64| for y, dx, dg, db. The largest ratios seen on
an MI355X are recorded in profiles/attention_layernorm_edge_errors.txt.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-6
NAMES = ("y", "dx", "dg", "db")


def _cpu(x, g, b, dy, dtype, need_dx=True):
    """F.layer_norm + autograd on the CPU in ``dtype``; absent tensors stay None."""
    xs = x.detach().to(dtype).requires_grad_(need_dx)
    gs = g.detach().to(dtype).requires_grad_(True) if g is not None else None
    bs = b.detach().to(dtype).requires_grad_(True) if b is not None else None
    y = F.layer_norm(xs, (x.shape[-1],), gs, bs, EPS)
    if xs.requires_grad or gs is not None or bs is not None:
        y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": xs.grad, "dg": gs.grad if gs is not None else None,
            "db": bs.grad if bs is not None else None}


def _check(tag, got, x, g, b, dy, names=NAMES, low=torch.float32):
    """got: dict of device results. Reference fp64, yardstick ``low`` (fp32) on the CPU, same inputs."""
    need_dx = "dx" in names
    hi = _cpu(x, g, b, dy, torch.float64, need_dx)
    lo = _cpu(x, g, b, dy, low, need_dx)
    failures = []
    for n in names:
        if hi[n] is None:
            assert got[n] is None, n
            continue
        yard = (lo[n].double() - hi[n]).abs().max().item()
        err = (got[n].detach().cpu().double().reshape(hi[n].shape) - hi[n]).abs()
        bound = 4 * yard + 1e-7 * hi[n].abs().max().item()
        worst = err.max().item()
        print(f"EDGE_RATIO layernorm {tag} {n} err={worst:.3e} yard={yard:.3e} "
              f"ratio={worst / yard if yard > 0 else float(worst > 0):.3f}")
        if not (err <= bound).all():                    # 4 x the fp32 CPU error: not to be raised
            failures.append((n, worst, bound))
    assert not failures, failures


def _run(x, g, b, dy, fn=None):
    """layer_norm on the GPU. x / g / b / dy are CPU tensors or ready-made device tensors (views)."""
    from bigdl_amd.ops.norm import layer_norm

    def leaf(t):
        if t is None:
            return None
        return (t if t.is_cuda else t.cuda()).detach().requires_grad_(True)

    xd, gd, bd = leaf(x), leaf(g), leaf(b)
    y = (fn or layer_norm)(xd, gd, bd, EPS)
    y.backward(dy if dy.is_cuda else dy.cuda())
    torch.cuda.synchronize()
    return {"y": y, "dx": xd.grad, "dg": gd.grad if gd is not None else None,
            "db": bd.grad if bd is not None else None}


def _data(rows, D, seed=0, has_g=True, has_b=True):
    gen = torch.Generator().manual_seed(seed * 100003 + rows * 8191 + D)
    x = torch.randn(rows, D, generator=gen) * 3 + 1
    dy = torch.randn(rows, D, generator=gen)
    g = torch.randn(D, generator=gen) if has_g else None
    b = torch.randn(D, generator=gen) if has_b else None
    return x, g, b, dy


@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("D", [1, 2, 3, 5, 63, 255, 256, 257, 1023, 4095, 4096])
def test_hidden_sizes(rows, D):
    """D not a multiple of 4, below / at / above the 256-thread block, up to the 16-values-per-thread limit."""
    x, g, b, dy = _data(rows, D)
    got = _run(x, g, b, dy)
    _check(f"{rows}x{D}", got, x, g, b, dy)
    if D == 1:
        # a single element is its own mean: y == b exactly, and dx is finite (it is 0, not 0 * inf)
        assert torch.equal(got["y"].cpu(), b.expand(rows, 1))
        assert torch.isfinite(got["dx"]).all()


@pytest.mark.parametrize("has_g,has_b", [(True, True), (True, False), (False, True), (False, False)])
def test_affine_parameters_present_or_absent(has_g, has_b):
    """layer_norm(x, None, None, eps) is supported (plain normalisation, no parameter gradients)."""
    x, g, b, dy = _data(65, 257, 1, has_g, has_b)
    got = _run(x, g, b, dy)
    _check(f"65x257-g{int(has_g)}b{int(has_b)}", got, x, g, b, dy)


@pytest.mark.parametrize("rows,D", [(8200, 4096), (26300, 1025)])
def test_parameter_gradients_past_the_block_cap(rows, D):
    """bx * by > 2048 in bigdl_layernorm_bwd (16 x 129 and 5 x 411 blocks of 64 rows): the row chunks are re-cut."""
    assert ((D + 255) // 256) * ((rows + 63) // 64) > 2048
    x, g, b, dy = _data(rows, D, 2)
    got = _run(x, g, b, dy)
    _check(f"{rows}x{D}", got, x, g, b, dy, names=("dg", "db"))


def test_large_common_offset():
    """x = 1000 + 0.01 randn: a one-pass E[x^2] - E[x]^2 variance would lose every digit; the kernel's two-pass
    variance does not. The fp32 error inherent in such inputs is in the yardstick already."""
    gen = torch.Generator().manual_seed(3)
    rows, D = 65, 1024
    x = 1000 + 0.01 * torch.randn(rows, D, generator=gen)
    dy = torch.randn(rows, D, generator=gen)
    g, b = torch.randn(D, generator=gen), torch.randn(D, generator=gen)
    _check("offset-65x1024", _run(x, g, b, dy), x, g, b, dy)


def test_strided_arguments():
    """x and dy as transposed views, gamma and beta as [::2] slices of a 2 D buffer. (Before the contiguous gamma
    was saved for the backward, dx read every other gamma from the wrong place.)"""
    gen = torch.Generator().manual_seed(4)
    rows, D = 65, 257
    xt = (torch.randn(D, rows, generator=gen) * 3 + 1).cuda()
    dyt = torch.randn(D, rows, generator=gen).cuda()
    g2, b2 = torch.randn(2 * D, generator=gen).cuda(), torch.randn(2 * D, generator=gen).cuda()
    x, dy, g, b = xt.t(), dyt.t(), g2[::2], b2[::2]
    for t in (x, dy, g, b):
        assert not t.is_contiguous()
    got = _run(x, g, b, dy)
    _check("strided-65x257", got, x.cpu(), g.cpu(), b.cpu(), dy.cpu())


def test_native_backward_rejects_strided_gamma():
    from bigdl_amd.ops import native

    rows, D = 4, 8
    x = torch.randn(rows, D, device="cuda")
    g2 = torch.randn(2 * D, device="cuda")
    y, mean, rstd = torch.empty_like(x), x.new_empty(rows), x.new_empty(rows)
    native.get().layernorm_fwd(x, g2[::2].contiguous(), None, y, mean, rstd, EPS)
    with pytest.raises(RuntimeError, match="gamma"):
        native.get().layernorm_bwd(torch.ones_like(x), x, g2[::2], mean, rstd, torch.empty_like(x), None, None)


@pytest.mark.parametrize("kind", ["D4097", "bf16"])
def test_fallback_route(kind, monkeypatch):
    """Hidden sizes above 4096 and non-fp32 inputs take F.layer_norm, not the native kernels, and still match."""
    from bigdl_amd.ops import norm

    def boom(*a, **kw):
        raise AssertionError("native LayerNorm on the fallback route")

    monkeypatch.setattr(norm._LayerNorm, "apply", boom)
    if kind == "D4097":
        x, g, b, dy = _data(3, 4097, 5)
        _check("fallback-3x4097", _run(x, g, b, dy, norm.layer_norm), x, g, b, dy)
    else:
        x, g, b, dy = (t.bfloat16() for t in _data(65, 256, 6))
        # same rule one format down: the yardstick is the CPU's bf16 F.layer_norm against fp64 on the bf16 values
        _check("fallback-bf16-65x256", _run(x, g, b, dy, norm.layer_norm), x, g, b, dy, low=torch.bfloat16)
